"""Spectral angle mapper (API parity: reference ``functional/image/sam.py:22-100``).

GPU path (4-D fp32 / bf16 / fp16 inputs of equal shape and dtype, at least two bands, no autograd): ``tmx::sam_map`` for ``"none"`` /
``None`` and ``tmx::sam_sums`` for ``"sum"`` / ``"elementwise_mean"`` (``csrc/spectral.hip``) -- one streaming kernel that reads the
``[B, C, H, W]`` inputs in place, once, and keeps the three band sums of a pixel in registers; no product tensor, norm or cosine map
is written, and the reduced forms write no angle map either.  The sums and the cosine are formed in fp64, so identical
non-zero vectors give exactly 0 where the composition gives up to 7e-4.  Kept on the composition below: fp64, gradients, the CPU,
an unknown ``reduction`` (it raises there) and ``TMX_SPECTRAL_NATIVE=0`` (the A/B knob of ``tools/spectral_bench.py``, read once per
process); mismatched dtypes or shapes, inputs that are not 4-D and single-band inputs raise in ``_sam_update`` before the gate."""
import os
from typing import Tuple

import torch
from torch import Tensor
from typing_extensions import Literal

from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.ops.image import sam_map as _sam_map
from torchmetrics_forked_amd.ops.image import sam_sums as _sam_sums
from torchmetrics_forked_amd.utilities.checks import _check_same_shape
from torchmetrics_forked_amd.utilities.distributed import reduce

_SPECTRAL_NATIVE = os.environ.get("TMX_SPECTRAL_NATIVE", "1") != "0"


def _native_sam_ok(preds: Tensor, target: Tensor) -> bool:
    """Route to ``tmx::sam_map`` / ``tmx::sam_sums``; everything else keeps the composition.

    No shape class is routed back: the native route is the faster one on every shape of ``tools/spectral_bench.py``
    (``profiles/spectral_bench.json``)."""
    if not (preds.is_cuda and target.is_cuda) or preds.shape != target.shape:
        return False
    if preds.dtype != target.dtype or preds.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    if preds.ndim != 4 or preds.size(1) < 2 or preds.numel() == 0:
        return False
    if torch.is_grad_enabled() and (preds.requires_grad or target.requires_grad):
        return False
    return _SPECTRAL_NATIVE and ops.use_native(preds, target)


def _sam_update(preds: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
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
    if preds.shape[1] <= 1 or target.shape[1] <= 1:
        raise ValueError(
            "Expected channel dimension of `preds` and `target` to be larger than 1."
            f" Got preds: {preds.shape[1]} and target: {target.shape[1]}."
        )
    return preds, target


def _sam_compute(preds: Tensor, target: Tensor, reduction: Literal["elementwise_mean", "sum", "none", None] = "elementwise_mean") -> Tensor:
    if reduction in ("elementwise_mean", "sum", "none", None) and _native_sam_ok(preds, target):
        if reduction == "none" or reduction is None:
            return _sam_map(preds, target).to(preds.dtype)
        total = _sam_sums(preds, target).sum()
        if reduction == "elementwise_mean":
            total = total / (preds.size(0) * preds.size(2) * preds.size(3))
        return total.to(preds.dtype)
    dot = (preds * target).sum(dim=1)
    score = torch.clamp(dot / (preds.norm(dim=1) * target.norm(dim=1)), -1, 1).acos()
    return reduce(score, reduction)


def spectral_angle_mapper(
    preds: Tensor, target: Tensor, reduction: Literal["elementwise_mean", "sum", "none", None] = "elementwise_mean"
) -> Tensor:
    preds, target = _sam_update(preds, target)
    return _sam_compute(preds, target, reduction)
