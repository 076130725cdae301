"""ERGAS (API parity: reference ``functional/image/ergas.py:22-100``).

GPU path (4-D fp32 / bf16 / fp16 inputs of equal shape and dtype, no autograd): ``tmx::ergas_scores`` (``csrc/spectral.hip``) -- one
streaming kernel that reads the ``[B, C, H, W]`` inputs in place, once, and writes fp64 partial sums of ``(p − t)²`` and ``t`` per plane
chunk, and a fold kernel that forms the per-image score in fp64; no difference or squared tensor is written.  16-bit inputs are
up-cast on load (the composition rounds the difference to the input dtype).  Kept on the composition below: fp64, gradients, the
CPU and ``TMX_SPECTRAL_NATIVE=0`` (the A/B knob of ``tools/spectral_bench.py``, read once per process)."""
from typing import Tuple

import torch
from torch import Tensor
from typing_extensions import Literal

from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.functional.image.sam import _SPECTRAL_NATIVE
from torchmetrics_forked_amd.ops.image import ergas_scores as _ergas_scores
from torchmetrics_forked_amd.utilities.checks import _check_same_shape
from torchmetrics_forked_amd.utilities.distributed import reduce


def _native_ergas_ok(preds: Tensor, target: Tensor) -> bool:
    """Route to ``tmx::ergas_scores``; everything else keeps the composition.

    No shape class is routed back: the native route is the faster one on every shape of ``tools/spectral_bench.py``
    (``profiles/spectral_bench.json``)."""
    if not (preds.is_cuda and target.is_cuda) or preds.shape != target.shape:
        return False
    if preds.dtype != target.dtype or preds.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    if preds.ndim != 4 or preds.numel() == 0:
        return False
    if torch.is_grad_enabled() and (preds.requires_grad or target.requires_grad):
        return False
    return _SPECTRAL_NATIVE and ops.use_native(preds, target)


def _ergas_update(preds: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    if preds.dtype != target.dtype:
        raise TypeError(
            "Expected `preds` and `target` to have the same data type."
            f" Got preds: {preds.dtype} and target: {target.dtype}."
        )
    _check_same_shape(preds, target)
    if len(preds.shape) != 4:
        raise ValueError(
            f"Expected `preds` and `target` to have BxCxHxW shape. Got preds: {preds.shape} and target: {target.shape}."
        )
    return preds, target


def _ergas_compute(
    preds: Tensor, target: Tensor, ratio: float = 4, reduction: Literal["elementwise_mean", "sum", "none", None] = "elementwise_mean"
) -> Tensor:
    if _native_ergas_ok(preds, target):
        return reduce(_ergas_scores(preds, target, ratio).to(preds.dtype), reduction)
    b, c, h, w = preds.shape
    preds, target = preds.reshape(b, c, h * w), target.reshape(b, c, h * w)
    diff = preds - target
    rmse_per_band = torch.sqrt(torch.sum(diff * diff, dim=2) / (h * w))
    mean_target = torch.mean(target, dim=2)
    score = 100 * ratio * torch.sqrt(torch.sum((rmse_per_band / mean_target) ** 2, dim=1) / c)
    return reduce(score, reduction)


def error_relative_global_dimensionless_synthesis(
    preds: Tensor, target: Tensor, ratio: float = 4, reduction: Literal["elementwise_mean", "sum", "none", None] = "elementwise_mean"
) -> Tensor:
    preds, target = _ergas_update(preds, target)
    return _ergas_compute(preds, target, ratio, reduction)
