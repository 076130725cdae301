"""PSNR with blocking-effect factor (API parity: reference ``functional/image/psnrb.py:22-130``).

GPU path (4-D fp32 / bf16 / fp16 ``[B, 1, H, W]`` inputs of equal shape and dtype, ``H >= 2`` and ``W >= 2``, no autograd): ``tmx::psnrb_sums``
(``csrc/neighbour_diff.hip``) -- one streaming kernel that reads ``preds`` and ``target`` in place, once, and returns ``Σ(p − t)²``, the boundary
and non-boundary sums of squared neighbour differences and the minimum and maximum of ``target`` in fp64; no difference map, mask
gather or second pass over ``target``.  The blocking-effect factor is then formed on the device in fp64 with ``torch.where`` in place of
the composition's ``if d_b > d_bc``: no host read in ``update``.  Kept on the composition below (strided slices of the boundary /
non-boundary column and row differences instead of host-built index lists): integer and fp64 images, gradients, the CPU, planes
with a single row or column, more than one channel (it raises there) and ``TMX_GRADIENT_NATIVE=0`` (the A/B knob of
``tools/gradient_bench.py``, read once per process)."""
import math
import os
from typing import Tuple, Union

import torch
from torch import Tensor, tensor

from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.ops.image import psnrb_sums as _psnrb_sums

_GRADIENT_NATIVE = os.environ.get("TMX_GRADIENT_NATIVE", "1") != "0"


def _native_psnrb_ok(preds: Tensor, target: Tensor) -> bool:
    """Route to ``tmx::psnrb_sums``; everything else keeps the composition.

    No shape class is routed back: the native route is the faster one on every shape of ``tools/gradient_bench.py``
    (``profiles/gradient_bench.json``)."""
    if not (preds.is_cuda and target.is_cuda) or preds.shape != target.shape:
        return False
    if preds.dtype != target.dtype or preds.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    if preds.ndim != 4 or preds.numel() == 0 or preds.size(1) != 1 or preds.size(2) < 2 or preds.size(3) < 2:
        return False
    if torch.is_grad_enabled() and (preds.requires_grad or target.requires_grad):
        return False
    return _GRADIENT_NATIVE and ops.use_native(preds, target)


def _psnrb_native_update(preds: Tensor, target: Tensor, block_size: int) -> Tuple[Tensor, Tensor, int, Tensor]:
    """``(sse, bef, num_obs, max − min of target)`` from one ``tmx::psnrb_sums`` call; ``bef`` in fp64 on the device, the counts as in
    ``_compute_bef``; ``sse`` and ``bef`` cast once to the input dtype.  No host read."""
    height, width = preds.shape[2:]
    sums = _psnrb_sums(preds, target, block_size)
    n_hb = height * (width / block_size) - 1
    n_hbc = height * (width - 1) - n_hb
    n_vb = width * (height / block_size) - 1
    n_vbc = width * (height - 1) - n_vb
    d_b = sums[1] / (n_hb + n_vb)
    d_bc = sums[2] / (n_hbc + n_vbc)
    t = math.log2(block_size) / math.log2(min(height, width))
    diff = d_b - d_bc
    bef = torch.where(d_b > d_bc, t * diff, 0 * diff)  # ``t * (d_b − d_bc)`` with ``t = 0`` on the other branch, as the composition forms it
    low_high = sums[3:5].to(preds.dtype)
    return sums[0].to(preds.dtype), bef.to(preds.dtype), target.numel(), low_high[1] - low_high[0]


def _compute_bef(x: Tensor, block_size: int = 8) -> Tensor:
    _, channels, height, width = x.shape
    if channels > 1:
        raise ValueError(f"`psnrb` metric expects grayscale images, but got images with {channels} channels.")
    dh = (x[..., :, :-1] - x[..., :, 1:]).pow(2.0)  # [.., H, W-1]: difference at column boundary j|j+1
    dv = (x[..., :-1, :] - x[..., 1:, :]).pow(2.0)
    hb = torch.zeros(width - 1, dtype=torch.bool, device=x.device)
    hb[block_size - 1 :: block_size] = True
    vb = torch.zeros(height - 1, dtype=torch.bool, device=x.device)
    vb[block_size - 1 :: block_size] = True
    d_b = dh[..., hb].sum() + dv[..., vb, :].sum()
    d_bc = dh[..., ~hb].sum() + dv[..., ~vb, :].sum()
    n_hb = height * (width / block_size) - 1
    n_hbc = height * (width - 1) - n_hb
    n_vb = width * (height / block_size) - 1
    n_vbc = width * (height - 1) - n_vb
    d_b = d_b / (n_hb + n_vb)
    d_bc = d_bc / (n_hbc + n_vbc)
    t = math.log2(block_size) / math.log2(min(height, width)) if d_b > d_bc else 0
    return t * (d_b - d_bc)


def _psnrb_compute(sum_squared_error: Tensor, bef: Tensor, num_obs: Tensor, data_range: Tensor) -> Tensor:
    mse = sum_squared_error / num_obs + bef
    if data_range > 2:
        return 10 * torch.log10(data_range**2 / mse)
    return 10 * torch.log10(1.0 / mse)


def _psnrb_update(preds: Tensor, target: Tensor, block_size: int = 8) -> Tuple[Tensor, Tensor, Union[Tensor, int]]:
    if _native_psnrb_ok(preds, target):
        return _psnrb_native_update(preds, target, block_size)[:3]
    sse = torch.sum(torch.pow(preds - target, 2))
    return sse, _compute_bef(preds, block_size=block_size), tensor(target.numel(), device=target.device)


def _psnrb_update_with_range(preds: Tensor, target: Tensor, block_size: int = 8) -> Tuple[Tensor, Tensor, Union[Tensor, int], Tensor]:
    """``_psnrb_update`` and ``target.max() − target.min()``: on the native route from the same read of ``target``."""
    if _native_psnrb_ok(preds, target):
        return _psnrb_native_update(preds, target, block_size)
    sse, bef, n = _psnrb_update(preds, target, block_size=block_size)
    return sse, bef, n, torch.max(target) - torch.min(target)


def peak_signal_noise_ratio_with_blocked_effect(preds: Tensor, target: Tensor, block_size: int = 8) -> Tensor:
    if _native_psnrb_ok(preds, target):
        sse, bef, n, data_range = _psnrb_native_update(preds, target, block_size)
        return _psnrb_compute(sse, bef, n, data_range)
    data_range = target.max() - target.min()
    sse, bef, n = _psnrb_update(preds, target, block_size=block_size)
    return _psnrb_compute(sse, bef, n, data_range)
