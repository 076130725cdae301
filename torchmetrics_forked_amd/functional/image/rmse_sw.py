"""RMSE with a sliding window (API parity: reference ``functional/image/rmse_sw.py:22-140``).

GPU path (4-D fp32 / bf16 / fp16 inputs of equal shape and dtype, no autograd, ``2 <= window_size <= 16``, ``H`` and ``W`` above
``2 round(window_size / 2)``): ``tmx::box_rmse_maps`` (``csrc/box_window.hip``) -- one fused box-window kernel that reads the
``[B, C, H, W]`` inputs in place and returns the batch sum of the per-image RMSE map in fp32 and its cropped sum per channel in
fp64; no padded copy, squared error or per-image map is written.  ``relative_average_spectral_error`` reaches the same kernel
with ``with_target_mean=True``.  Kept on the composition below: ``window_size`` 1 or above 16, planes with an empty crop (the
result is NaN, as in the reference), fp64, gradients, the CPU and ``TMX_BOX_NATIVE=0`` (the A/B knob of
``tools/box_bench.py``, read once per process)."""
import os
from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.functional.image.helper import _uniform_filter
from torchmetrics_forked_amd.ops.image import box_rmse_maps as _box_rmse_maps
from torchmetrics_forked_amd.utilities.checks import _check_same_shape

_BOX_NATIVE = os.environ.get("TMX_BOX_NATIVE", "1") != "0"


def _native_rmse_sw_ok(preds: Tensor, target: Tensor, window_size: int) -> bool:
    """Route to ``tmx::box_rmse_maps``; everything else keeps the composition.

    No shape class is routed back: on every shape of ``tools/box_bench.py`` the native route is the faster one, from 2.5x at
    32 x 1 x 41 x 41 to 14x (RMSE-SW) and 15x (RASE) at 1024 x 1024 with window 8 and 31x / 38x with window 15
    (``profiles/box_bench.json``)."""
    if not (preds.is_cuda and target.is_cuda) or preds.ndim != 4 or preds.shape != target.shape:
        return False
    if preds.dtype != target.dtype or preds.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    if torch.is_grad_enabled() and (preds.requires_grad or target.requires_grad):
        return False
    if not 2 <= window_size <= 16:
        return False
    crop = round(window_size / 2)
    if preds.numel() == 0 or preds.size(-2) <= 2 * crop or preds.size(-1) <= 2 * crop:
        return False
    return _BOX_NATIVE and ops.use_native(preds, target)


def _rmse_sw_validate(preds: Tensor, target: Tensor, window_size: int) -> None:
    if preds.dtype != target.dtype:
        raise TypeError(
            f"Expected `preds` and `target` to have the same data type. But got {preds.dtype} and {target.dtype}."
        )
    _check_same_shape(preds, target)
    if len(preds.shape) != 4:
        raise ValueError(f"Expected `preds` and `target` to have BxCxHxW shape. But got {preds.shape}.")
    if round(window_size / 2) >= target.shape[2] or round(window_size / 2) >= target.shape[3]:
        raise ValueError(
            f"Parameter `round(window_size / 2)` is expected to be smaller than {min(target.shape[2], target.shape[3])}"
            f" but got {round(window_size / 2)}."
        )


def _count_images(total_images: Optional[Tensor], target: Tensor) -> Tensor:
    if total_images is not None:
        total_images += target.shape[0]
        return total_images
    # (torch.full, not torch.tensor: the same 0-d int64 tensor without the blocking host-to-device copy)
    return torch.full((), target.shape[0], dtype=torch.int64, device=target.device)


def _native_rmse_sw_batch(
    preds: Tensor, target: Tensor, window_size: int, with_target_mean: bool
) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """``(val, rmse_map, target_mean)`` of one batch from ``tmx::box_rmse_maps``, cast to the input dtype as the composition's are."""
    crop = round(window_size / 2)
    c, h, w = preds.shape[1:]
    rmse_map, crop_sums, target_mean = _box_rmse_maps(preds, target, window_size, crop, with_target_mean)
    val = (crop_sums.sum() / (c * (h - 2 * crop) * (w - 2 * crop))).to(preds.dtype)
    return val, rmse_map.to(preds.dtype), target_mean.to(preds.dtype) if with_target_mean else None


def _rmse_sw_update(
    preds: Tensor,
    target: Tensor,
    window_size: int,
    rmse_val_sum: Optional[Tensor],
    rmse_map: Optional[Tensor],
    total_images: Optional[Tensor],
) -> Tuple[Tensor, Tensor, Tensor]:
    _rmse_sw_validate(preds, target, window_size)
    total_images = _count_images(total_images, target)
    if _native_rmse_sw_ok(preds, target, window_size):
        val, batch_map, _ = _native_rmse_sw_batch(preds, target, window_size, False)
    else:
        _rmse_map = torch.sqrt(_uniform_filter((target - preds) ** 2, window_size))
        crop = round(window_size / 2)
        val = _rmse_map[:, :, crop:-crop, crop:-crop].sum(0).mean()
        batch_map = _rmse_map.sum(0)
    rmse_val_sum = rmse_val_sum + val if rmse_val_sum is not None else val
    rmse_map = rmse_map + batch_map if rmse_map is not None else batch_map
    return rmse_val_sum, rmse_map, total_images


def _rmse_sw_compute(rmse_val_sum: Optional[Tensor], rmse_map: Tensor, total_images: Tensor) -> Tuple[Optional[Tensor], Tensor]:
    rmse = rmse_val_sum / total_images if rmse_val_sum is not None else None
    if rmse_map is not None:
        rmse_map = rmse_map / total_images
    return rmse, rmse_map


def root_mean_squared_error_using_sliding_window(
    preds: Tensor, target: Tensor, window_size: int = 8, return_rmse_map: bool = False
) -> Union[Optional[Tensor], Tuple[Optional[Tensor], Tensor]]:
    if not isinstance(window_size, int) or window_size < 1:
        raise ValueError("Argument `window_size` is expected to be a positive integer.")
    val_sum, rmse_map, total = _rmse_sw_update(preds, target, window_size, None, None, None)
    rmse, rmse_map = _rmse_sw_compute(val_sum, rmse_map, total)
    return (rmse, rmse_map) if return_rmse_map else rmse
