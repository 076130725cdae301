"""Total variation (API parity: reference ``functional/image/tv.py:20-80``).

GPU path (4-D fp32 / bf16 / fp16 input, no autograd): ``tmx::tv_sums`` (``csrc/neighbour_diff.hip``) -- one streaming kernel that reads the
``[B, C, H, W]`` input in place, once, and adds the absolute row and column differences per image in fp64; no difference or
absolute-value map is written.  Kept on the composition below: integer and fp64 images, gradients (there is no native backward),
the CPU and ``TMX_GRADIENT_NATIVE=0`` (the A/B knob of ``tools/gradient_bench.py``, read once per process); inputs that are not 4-D raise
before the gate."""
import os
from typing import Optional, Tuple, Union

import torch
from torch import Tensor
from typing_extensions import Literal

from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.ops.image import tv_sums as _tv_sums

_GRADIENT_NATIVE = os.environ.get("TMX_GRADIENT_NATIVE", "1") != "0"


def _native_tv_ok(img: Tensor) -> bool:
    """Route to ``tmx::tv_sums``; everything else keeps the composition.

    No shape class is routed back: the native route is the faster one on every shape of ``tools/gradient_bench.py``
    (``profiles/gradient_bench.json``)."""
    if not img.is_cuda or img.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    if img.ndim != 4 or img.numel() == 0:
        return False
    if torch.is_grad_enabled() and img.requires_grad:
        return False
    return _GRADIENT_NATIVE and ops.use_native(img)


def _total_variation_update(img: Tensor) -> Tuple[Tensor, int]:
    if img.ndim != 4:
        raise RuntimeError(f"Expected input `img` to be an 4D tensor, but got {img.shape}")
    if _native_tv_ok(img):
        return _tv_sums(img).to(img.dtype), img.shape[0]
    res1 = (img[..., 1:, :] - img[..., :-1, :]).abs().sum([1, 2, 3])
    res2 = (img[..., :, 1:] - img[..., :, :-1]).abs().sum([1, 2, 3])
    return res1 + res2, img.shape[0]


def _total_variation_compute(score: Tensor, num_elements: Union[int, Tensor], reduction: Optional[Literal["mean", "sum", "none"]]) -> Tensor:
    if reduction == "mean":
        return score.sum() / num_elements
    if reduction == "sum":
        return score.sum()
    if reduction is None or reduction == "none":
        return score
    raise ValueError("Expected argument `reduction` to either be 'sum', 'mean', 'none' or None")


def total_variation(img: Tensor, reduction: Optional[Literal["mean", "sum", "none"]] = "sum") -> Tensor:
    score, n = _total_variation_update(img)
    return _total_variation_compute(score, n, reduction)
