"""Thin wrappers of the ops of ``csrc/infolm.hip``: InfoLM's sentence distributions and the row-pair measures (the nine InfoLM
information measures, KL divergence and cosine similarity)."""
import os
from typing import NamedTuple

import torch
from torch import Tensor

from torchmetrics_forked_amd import ops

(KIND_KL, KIND_ALPHA, KIND_AB, KIND_RENYI, KIND_L1, KIND_L2, KIND_LINF, KIND_FISHER_RAO,
 KIND_KL_PROB, KIND_KL_LOG_PROB, KIND_COSINE) = range(11)

_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
# A/B switches for whole processes, read once
_INFOLM_NATIVE = os.environ.get("TMX_INFOLM_NATIVE", "1") != "0"
_ROWPAIR_NATIVE = os.environ.get("TMX_ROWPAIR_NATIVE", "1") != "0"


class InfolmTile(NamedTuple):
    """``acc_tile``: vocabulary columns a workgroup of the accumulate kernel owns; ``threads``: per workgroup; ``small_limit`` / ``wave_limit``:
    largest row length of the 8-lane and of the wave-per-row split of ``row_pair_measure``; ``block_tile``: elements a workgroup of its
    workgroup-per-row split covers per step."""

    acc_tile: int
    threads: int
    small_limit: int
    wave_limit: int
    block_tile: int


def infolm_tile() -> InfolmTile:
    """The geometry of the kernels (see ``InfolmTile``)."""
    return InfolmTile(*[int(x) for x in torch.ops.tmx.infolm_tile()])


def infolm_native(logits: Tensor, temperature: float) -> bool:
    """True when ``infolm_accumulate`` serves these logits: GPU, fp32 / bf16 / fp16, ``[R, S, V]`` with a contiguous vocabulary."""
    return (
        _INFOLM_NATIVE
        and temperature > 0
        and logits.dim() == 3
        and logits.dtype in _DTYPES
        and (logits.shape[2] == 1 or logits.stride(2) == 1)
        and not (logits.requires_grad and torch.is_grad_enabled())
        and ops.use_native(logits)
    )


def infolm_accumulate(logits: Tensor, pos: Tensor, owner: Tensor, weight: Tensor, temperature: float, acc: Tensor) -> None:
    """``tmx::infolm_accumulate``: ``acc[owner[r]] += weight[r] * softmax(logits[r, pos[r]] / temperature)`` for every row ``r``.

    ``logits`` ``[R, S, V]`` (fp32 / bf16 / fp16, any row and sequence strides) is read in place; ``pos`` / ``owner`` int64 ``[R]`` with
    ``owner`` non-decreasing; ``weight`` fp32 ``[R]``; ``acc`` contiguous fp32 ``[B, V]``.  The softmax is computed in fp32 whatever the
    dtype of the logits.  No atomics: two calls give the same bits, and a sentence without rows keeps its ``acc`` row as it was."""
    torch.ops.tmx.infolm_accumulate(logits, pos, owner, weight, float(temperature), acc)


def row_pair_native(p: Tensor, t: Tensor) -> bool:
    """True when ``row_pair_measure`` serves this pair: GPU, one of fp32 / bf16 / fp16 for both, no autograd."""
    return (
        _ROWPAIR_NATIVE
        and p.dtype in _DTYPES
        and t.dtype == p.dtype
        and p.dim() >= 1
        and p.shape == t.shape
        and p.shape[-1] > 0
        and not ((p.requires_grad or t.requires_grad) and torch.is_grad_enabled())
        and ops.use_native(p, t)
    )


def row_pair_measure(p: Tensor, t: Tensor, kind: int, alpha: float = 0.0, beta: float = 0.0) -> Tensor:
    """``tmx::row_pair_measure``: fp32 ``[N]``, one number per row pair of ``p`` / ``t`` ``[N, V]`` (``kind``: a ``KIND_*``).

    Element terms in fp32 as the compositions write them, sums and epilogue in fp64.  The eight InfoLM kinds apply ``nan_to_num``
    (NaN -> 0, +-inf -> +-``FLT_MAX``); ``KIND_KL_PROB`` normalises both rows by their sums (fp64 element terms), ``KIND_KL_LOG_PROB`` takes log-probabilities,
    ``KIND_COSINE`` is ``dot / (|p| |t|)``; those three return NaN / inf as they arise."""
    return torch.ops.tmx.row_pair_measure(p, t, int(kind), float(alpha), float(beta))
