"""CPU oracles of the spectral angle mapper and ERGAS, written from the definitions with plain dense torch.

``sam_angles`` returns what ``tmx::sam_map`` returns and ``ergas_scores`` what ``tmx::ergas_scores`` returns, in fp64 as the oracle or
in fp32 as the measure of what the fp32 composition itself loses (the ``comp32`` of ``vif_oracle.value_rule``).
"""
import torch
from torch import Tensor


def sam_angles(p: Tensor, t: Tensor, dtype: torch.dtype = torch.float64) -> Tensor:
    """``[B, C, H, W]`` -> ``[B, H, W]`` in ``dtype``: ``acos(clamp(<p,t> / (|p| |t|), −1, 1))`` over the band vector of every pixel."""
    p, t = p.detach().cpu().to(dtype), t.detach().cpu().to(dtype)
    dot = (p * t).sum(1)
    norms = (p * p).sum(1).sqrt() * (t * t).sum(1).sqrt()
    return torch.acos((dot / norms).clamp(-1, 1))


def ergas_scores(p: Tensor, t: Tensor, ratio: float, dtype: torch.dtype = torch.float64) -> Tensor:
    """``[B, C, H, W]`` -> ``[B]`` in ``dtype``: ``100 · ratio · sqrt(mean_c((SSE_bc / HW) / mean_t_bc²))``."""
    p, t = p.detach().cpu().to(dtype), t.detach().cpu().to(dtype)
    hw = p.shape[2] * p.shape[3]
    d = p - t
    mse = (d * d).sum((2, 3)) / hw
    mean_t = t.sum((2, 3)) / hw
    return 100 * ratio * torch.sqrt((mse / (mean_t * mean_t)).sum(1) / p.shape[1])
