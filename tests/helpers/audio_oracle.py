"""CPU oracles of SNR, SI-SDR and SA-SDR, written from the formulas (nothing imported from the package).

Every function takes ``(..., T)`` signals (SA-SDR ``(..., S, T)``) and evaluates in ``dtype``: fp64 as the oracle, fp32 as the measure of
what the fp32 composition itself loses.  ``eps`` defaults to ``torch.finfo(preds.dtype).eps`` of the tensors handed in, which is what
the functionals add: it is the constant of the INPUT dtype whatever ``dtype`` the evaluation runs in.

``speakers(shape, seed, ...)`` draws ``(preds, target)`` ``[..., S, T]``: every speaker's target is a shared component plus its own, preds
is the target plus noise whose level differs per speaker, so ``ratio(preds_i, target_j) != ratio(preds_j, target_i)`` and a transposed
pair matrix fails.
"""
from typing import Callable, Optional, Tuple

import torch
from torch import Tensor


def _prep(preds: Tensor, target: Tensor, dtype: torch.dtype, eps: Optional[float], zero_mean: bool) -> Tuple[Tensor, Tensor, float]:
    eps = float(torch.finfo(preds.dtype).eps) if eps is None else float(eps)
    p, t = preds.detach().cpu().to(dtype), target.detach().cpu().to(dtype)
    if zero_mean:
        p, t = p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True)
    return p, t, eps


def snr(preds: Tensor, target: Tensor, zero_mean: bool = False, dtype: torch.dtype = torch.float64, eps: Optional[float] = None) -> Tensor:
    """``10 log10((Σ t² + eps) / (Σ (t − p)² + eps))``."""
    p, t, eps = _prep(preds, target, dtype, eps, zero_mean)
    return 10 * torch.log10(((t * t).sum(-1) + eps) / (((t - p) ** 2).sum(-1) + eps))


def si_sdr(preds: Tensor, target: Tensor, zero_mean: bool = False, dtype: torch.dtype = torch.float64, eps: Optional[float] = None) -> Tensor:
    """``α = (Σ p t + eps) / (Σ t² + eps)``; ``10 log10((Σ (α t)² + eps) / (Σ (α t − p)² + eps))``."""
    p, t, eps = _prep(preds, target, dtype, eps, zero_mean)
    alpha = ((p * t).sum(-1, keepdim=True) + eps) / ((t * t).sum(-1, keepdim=True) + eps)
    scaled = alpha * t
    return 10 * torch.log10(((scaled * scaled).sum(-1) + eps) / (((scaled - p) ** 2).sum(-1) + eps))


def sa_sdr(preds: Tensor, target: Tensor, scale_invariant: bool = True, zero_mean: bool = False, dtype: torch.dtype = torch.float64,
           eps: Optional[float] = None) -> Tensor:
    """One ``α`` and one ratio over the speakers and samples of ``(..., S, T)``."""
    p, t, eps = _prep(preds, target, dtype, eps, zero_mean)
    if scale_invariant:
        alpha = ((p * t).sum((-1, -2), keepdim=True) + eps) / ((t * t).sum((-1, -2), keepdim=True) + eps)
        t = alpha * t
    return 10 * torch.log10(((t * t).sum((-1, -2)) + eps) / (((t - p) ** 2).sum((-1, -2)) + eps))


def pair_matrix(preds: Tensor, target: Tensor, fn: Callable[..., Tensor], **kwargs) -> Tensor:
    """``out[b, j, i] = fn(preds[b, i], target[b, j])`` for ``[B, S, T]`` inputs, one pair at a time."""
    b, s = preds.shape[:2]
    first = fn(preds[:, 0], target[:, 0], **kwargs)
    out = torch.empty(b, s, s, dtype=first.dtype)
    for j in range(s):
        for i in range(s):
            out[:, j, i] = fn(preds[:, i], target[:, j], **kwargs)
    return out


def speakers(shape: Tuple[int, ...], seed: int, scale: float = 1.0, offset: float = 0.0, noise: float = 0.2) -> Tuple[Tensor, Tensor]:
    """fp32 ``(preds, target)`` of ``[..., S, T]``.  ``target_s = scale · (0.6 shared + 0.8 own_s) + offset`` (unit variance before the scale),
    ``preds_s = target_s + scale · noise · (1 + s / 2) · n_s``: 14 dB at ``noise = 0.2`` for the first speaker, lower for the later ones."""
    g = torch.Generator().manual_seed(seed)
    s = shape[-2]
    shared = torch.randn(*shape[:-2], 1, shape[-1], generator=g, dtype=torch.float64)
    own = torch.randn(*shape, generator=g, dtype=torch.float64)
    level = noise * (1 + 0.5 * torch.arange(s, dtype=torch.float64))[:, None]
    t = scale * (0.6 * shared + 0.8 * own) + offset
    p = t + scale * level * torch.randn(*shape, generator=g, dtype=torch.float64)
    return p.float(), t.float()
