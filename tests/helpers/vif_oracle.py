"""CPU oracle of pixel-domain visual information fidelity, written from the definition with the dense 2-D window.

``vif_scale_sums`` returns what ``tmx::vif_sums`` returns (per scale and per plane the numerator and denominator sums), in
fp64 as the oracle or in fp32 as the measure of what the fp32 composition itself loses.  ``value_rule`` is the bound every
native result is held to: ``|native − oracle64| <= 4 |comp32 − oracle64| + 1e-6 max|oracle64|`` (the factor 4 is the project's
bound for the SSIM gradient), per scale, for ``num`` and ``den`` separately, as a maximum over planes.
"""
import json
from typing import Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

WINDOWS = (17, 9, 5, 3)
EPS = 1e-10


def window_2d(n: int, dtype: torch.dtype) -> Tensor:
    """``exp(−(di² + dj²) / (2 (n / 5)²))`` normalised to sum 1, ``[n, n]``."""
    d = torch.arange(n, dtype=dtype) - (n - 1) / 2
    g = torch.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * (n / 5) ** 2))
    return g / g.sum()


def vif_scale_sums(p: Tensor, t: Tensor, sigma_n_sq: float, dtype: torch.dtype = torch.float64) -> Tensor:
    """``p`` / ``t`` ``[P, H, W]`` -> ``[4, 2, P]`` in ``dtype``: ``out[s, 0]`` = sum over the valid windows of scale ``s`` of
    ``log10(1 + g² σt² / (σv² + σn²))``, ``out[s, 1]`` = sum of ``log10(1 + σt² / σn²)``."""
    p, t = p.detach().cpu().to(dtype)[:, None], t.detach().cpu().to(dtype)[:, None]
    eps = torch.tensor(EPS, dtype=dtype)
    sn = torch.tensor(sigma_n_sq, dtype=dtype)
    zero = torch.zeros((), dtype=dtype)
    out = torch.zeros(4, 2, p.shape[0], dtype=dtype)
    for s, n in enumerate(WINDOWS):
        k = window_2d(n, dtype)[None, None]
        if s > 0:  # the next level: filter with this scale's window, keep every second row and column
            p, t = F.conv2d(p, k)[:, :, ::2, ::2], F.conv2d(t, k)[:, :, ::2, ::2]
        mu_p, mu_t = F.conv2d(p, k), F.conv2d(t, k)
        s_pp = (F.conv2d(p * p, k) - mu_p * mu_p).clamp(min=0.0)
        s_tt = (F.conv2d(t * t, k) - mu_t * mu_t).clamp(min=0.0)
        s_tp = F.conv2d(p * t, k) - mu_p * mu_t
        g = s_tp / (s_tt + eps)
        s_v = s_pp - g * s_tp
        m = s_tt < eps  # no signal in the target window
        g, s_v, s_tt = torch.where(m, zero, g), torch.where(m, s_pp, s_v), torch.where(m, zero, s_tt)
        m = s_pp < eps  # no signal in the preds window
        g, s_v = torch.where(m, zero, g), torch.where(m, zero, s_v)
        m = g < 0  # anti-correlated
        s_v, g = torch.where(m, s_pp, s_v), torch.where(m, zero, g)
        s_v = s_v.clamp(min=eps)
        out[s, 0] = torch.log10(1.0 + g * g * s_tt / (s_v + sn)).sum((1, 2, 3))
        out[s, 1] = torch.log10(1.0 + s_tt / sn).sum((1, 2, 3))
    return out


def scores(sums: Tensor) -> Tensor:
    """``[4, 2, P]`` sums -> ``[P]`` VIF."""
    tot = sums.sum(0)
    return tot[0] / tot[1]


def noisy_pair(shape: Tuple[int, ...], seed: int, scale: float = 1.0) -> Tuple[Tensor, Tensor]:
    """fp32 ``(preds, target)`` of ``[..., H, W]``: target = a smooth field plus uniform noise, preds = target plus Gaussian
    noise, scaled to ``[0, scale]``.  Every window has a variance far above the 1e-10 mask threshold."""
    g = torch.Generator().manual_seed(seed)
    h, w = shape[-2:]
    yy = torch.linspace(0, 3.0, h, dtype=torch.float64)[:, None]
    xx = torch.linspace(0, 2.0, w, dtype=torch.float64)[None, :]
    smooth = 0.5 + 0.25 * torch.sin(2.1 * yy + 0.7) * torch.cos(3.3 * xx + 0.2)
    t = (smooth + 0.25 * (torch.rand(*shape, generator=g, dtype=torch.float64) - 0.5)).clamp(0, 1)
    p = (t + 0.05 * torch.randn(*shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    return (p * scale).float(), (t * scale).float()


def value_rule(label: str, native: Tensor, oracle64: Tensor, comp32: Tensor) -> float:
    """Assert the value rule on ``[..., P]`` tensors (the maximum runs over the last axis); prints and returns the worst
    ratio error / bound."""
    native, oracle64, comp32 = (x.detach().double().cpu() for x in (native, oracle64, comp32))
    assert native.shape == oracle64.shape == comp32.shape, (label, native.shape, oracle64.shape, comp32.shape)
    if native.dim() == 0:
        native, oracle64, comp32 = native[None], oracle64[None], comp32[None]
    err = (native - oracle64).abs().amax(-1)
    bound = 4 * (comp32 - oracle64).abs().amax(-1) + 1e-6 * oracle64.abs().amax(-1)
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))  # (0 <= 0 holds: both exact)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("vif_err " + json.dumps({"case": label, "ratio": worst, "err": float(err.max()), "bound": float(bound.max())}))
    assert torch.isfinite(native).all(), label
    assert bool((err <= bound).all()), (label, err.tolist(), bound.tolist())
    return worst
