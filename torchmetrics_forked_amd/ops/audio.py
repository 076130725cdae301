"""Thin wrappers of the signal-pair ops of ``csrc/signal_pairs.hip`` (SNR, SI-SDR, SA-SDR and the PIT pair matrix)."""
from typing import Tuple

import torch
from torch import Tensor

PAIR_DIAGONAL, PAIR_ALL, PAIR_AGGREGATED = 0, 1, 2


def signal_pair_ratios(preds: Tensor, target: Tensor, scale_invariant: bool, zero_mean: bool, pairing: int, eps: float) -> Tensor:
    """``tmx::signal_pair_ratios``: fp64 ratios in dB of ``preds`` / ``target`` ``[G, S, T]`` (fp32 / bf16 / fp16, made contiguous and read
    in place; no expanded copy).  Per pair, in fp64 on the up-cast samples: ``p~ = p − mean(p)``, ``t~ = t − mean(t)`` when ``zero_mean``;
    ``α = (Σ p~ t~ + eps) / (Σ t~² + eps)`` when ``scale_invariant``, else 1; ``10 log10((α² Σ t~² + eps) / (Σ (α t~ − p~)² + eps))``.
    ``pairing`` 0: ``[G, S]``, the pairs ``(p_s, t_s)``; 1: ``[G, S, S]`` with ``out[g, j, i]`` the ratio of ``(preds[g, i], target[g, j])``; 2: ``[G]``, one
    ``α`` and one ratio over the ``S`` pairs ``(p_s, t_s)`` of a group.  ``eps`` is the caller's ``torch.finfo(dtype).eps``: silent targets,
    ``p == t`` and ``T == 1`` give the composition's finite values.  One fp64 partial per workgroup added in a fixed order (no atomics:
    two runs are bit-equal).  No host read.  No autograd."""
    return torch.ops.tmx.signal_pair_ratios(preds, target, bool(scale_invariant), bool(zero_mean), int(pairing), float(eps))


def signal_chunks(g: int, s: int, t: int, pairing: int) -> int:
    """How many chunks the pair passes of ``signal_pair_ratios`` split every signal of a ``[g, s, t]`` call into: a function of the
    shape and the pairing alone, unless ``TMX_SIGNAL_CHUNK`` (samples per chunk, read per call, rounded up to the alignment of
    ``signal_tile``) overrides it.  Only the last chunk may be short."""
    return int(torch.ops.tmx.signal_chunks(int(g), int(s), int(t), int(pairing)))


def signal_tile() -> Tuple[int, int, int, int]:
    """``(threads per workgroup, fp32 samples per 16-byte load, largest pair-tile extent, chunk alignment in samples)``; 16-bit inputs
    take twice the samples per load."""
    threads, width, tile, align = torch.ops.tmx.signal_tile()
    return int(threads), int(width), int(tile), int(align)
