"""CPU oracle of the 2-D structural similarity sums, written from the definition with dense valid windows.

``valid_window_sums`` returns what ``tmx::ssim_sums`` returns with ``with_sse=True`` (per plane the sums of SSIM, of the contrast
sensitivity and of ``(p − t)²``): ``oracle64`` with everything in fp64, and ``comp32`` with the same arithmetic in fp32 and the
per-window values added in fp64 -- the measure of what fp32 window arithmetic itself loses.  The windows are passed as the fp32
tensors the op consumes and converted exactly, so both sides compute the same operation.  The bound every native result is held
to is ``tests.helpers.vif_oracle.value_rule``.

Per window, with the five moments ``μp, μt, E[p²], E[t²], E[pt]`` (``σp² = E[p²] − μp²``, ``σpt = E[pt] − μp μt``):
``cs = (2 σpt + c2) / (σp² + σt² + c2)`` and ``ssim = (2 μp μt + c1) / (μp² + μt² + c1) · cs``.
"""
import json
from typing import Tuple

import torch
from torch import Tensor

from tests.helpers.vif_oracle import noisy_pair

K1, K2 = 0.01, 0.03


def gaussian(kernel_size: int, sigma: float) -> Tensor:
    """Normalised 1-D Gaussian ``[kernel_size]``, fp32 (what the op takes)."""
    d = torch.arange(kernel_size, dtype=torch.float64) - (kernel_size - 1) / 2
    g = torch.exp(-((d / sigma) ** 2) / 2)
    return (g / g.sum()).float()


def uniform(kernel_size: int) -> Tensor:
    """``1 / kernel_size`` in every tap, fp32."""
    return torch.full((kernel_size,), 1.0 / kernel_size, dtype=torch.float32)


def consts(data_range: float) -> Tuple[float, float]:
    """``(c1, c2)`` of a data range, as the fp32 values the op reads."""
    c = torch.tensor([(K1 * data_range) ** 2, (K2 * data_range) ** 2], dtype=torch.float32)
    return float(c[0]), float(c[1])


def valid_window_sums(p: Tensor, t: Tensor, wy: Tensor, wx: Tensor, c1: float, c2: float, dtype: torch.dtype = torch.float64) -> Tensor:
    """``p`` / ``t`` ``[P, H, W]``, ``wy`` / ``wx`` the 1-D windows of the H / W axis -> fp64 ``[3, P]``: the sums over all valid windows of SSIM
    and of the contrast sensitivity, computed in ``dtype`` and added in fp64, and the sum over all pixels of ``(p − t)²`` in ``dtype``."""
    p, t = p.detach().cpu().to(dtype), t.detach().cpu().to(dtype)
    wy, wx = wy.detach().cpu().to(dtype), wx.detach().cpu().to(dtype)
    c1, c2 = torch.tensor(c1, dtype=dtype), torch.tensor(c2, dtype=dtype)

    def filt(x: Tensor) -> Tensor:  # out[y, x] = sum_k sum_l wy[k] wx[l] in[y + k, x + l] over the windows inside the plane
        return (x.unfold(1, wy.numel(), 1) @ wy).unfold(2, wx.numel(), 1) @ wx

    mu_p, mu_t, e_pp, e_tt, e_pt = filt(p), filt(t), filt(p * p), filt(t * t), filt(p * t)
    upper = 2 * (e_pt - mu_p * mu_t) + c2
    lower = (e_pp - mu_p * mu_p) + (e_tt - mu_t * mu_t) + c2
    cs = upper / lower
    sim = (2 * mu_p * mu_t + c1) / (mu_p * mu_p + mu_t * mu_t + c1) * cs
    d = p - t
    return torch.stack([sim.double().sum((1, 2)), cs.double().sum((1, 2)), (d * d).double().sum((1, 2))])


def planes(shape: Tuple[int, ...], seed: int, kind: str = "unit") -> Tuple[Tensor, Tensor, float]:
    """Seeded fp32 ``(preds, target, data_range)`` of ``[..., H, W]`` from ``noisy_pair``: ``"unit"`` in ``[0, 1]``, ``"255"`` in ``[0, 255]``,
    ``"negative"`` in ``[−0.5, 0.5]``, ``"shifted"`` in ``[0.2, 1.2]`` and ``"shifted_low"`` in ``[0.2, 0.95]``, the last three with data range 1."""
    if kind == "255":
        return (*noisy_pair(shape, seed, 255.0), 255.0)
    p, t = noisy_pair(shape, seed, 1.0)
    shift, scale = {"unit": (0.0, 1.0), "negative": (-0.5, 1.0), "shifted": (0.2, 1.0), "shifted_low": (0.2, 0.75)}[kind]
    return (scale * p.double() + shift).float(), (scale * t.double() + shift).float(), 1.0


def print_err(label: str, ratio: float, err: float, bound: float) -> None:
    print("ssim2d_err " + json.dumps({"case": label, "ratio": ratio, "err": err, "bound": bound}))
