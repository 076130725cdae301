"""Shared plumbing of the segmentation functionals: argument checks, the native gate, the class-overlap counts and their scores.

All three metrics are functions of the per-(sample, class) counts ``I`` (pixels in the class on both sides), ``P`` (in ``preds``) and ``T``
(in ``target``), an int64 ``[B, C, 3]`` tensor.  On the GPU the counts come from one read of the inputs by ``tmx::segment_overlap_index`` /
``tmx::segment_overlap_onehot`` (``csrc/segment_overlap.hip``) and the scores from one launch of ``tmx::segment_scores``.  Kept on the
composition (``_overlap_composition`` / ``_scores_composition``, the same semantics): CPU tensors, dtypes outside the op's set, index form
with more classes than the op's LDS arrays hold (``_SEGMENT_MAX_CLASSES``) and ``TMX_SEGMENT_NATIVE=0`` (the A/B knob of
``tools/segmentation_bench.py``, read once per process)."""
import os
from typing import Optional, Tuple

import torch
from torch import Tensor

from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.ops import segmentation as _ops_seg

_SEGMENT_NATIVE = os.environ.get("TMX_SEGMENT_NATIVE", "1") != "0"
_SEGMENT_MAX_CLASSES = 4096  # ``ops.segmentation.segment_overlap_tile()[2]`` (the library is not asked on every call; the GPU tests hold the two together)
_INDEX_DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64)
_ONEHOT_DTYPES = (torch.bool, torch.uint8, torch.int32, torch.int64)


def _check_arguments(num_classes: int, include_background: bool, input_format: str) -> None:
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 1:
        raise ValueError(f"Expected argument `num_classes` to be a positive integer, but got {num_classes}.")
    if not isinstance(include_background, bool):
        raise ValueError(f"Expected argument `include_background` to be a bool, but got {include_background}.")
    if input_format not in ("one-hot", "index"):
        raise ValueError(f"Expected argument `input_format` to be one of 'one-hot', 'index', but got {input_format}.")
    if not include_background and num_classes == 1:
        raise ValueError("`include_background=False` leaves no class when `num_classes` is 1.")


def _check_inputs(preds: Tensor, target: Tensor, num_classes: int, include_background: bool, input_format: str) -> None:
    """Everything that raises does so here, before any launch."""
    _check_arguments(num_classes, include_background, input_format)
    for name, x in (("preds", preds), ("target", target)):
        if x.is_floating_point() or x.is_complex():
            raise ValueError(f"Expected `{name}` to hold integer labels or boolean / integer masks, but got dtype {x.dtype}.")
    if preds.shape != target.shape:
        raise ValueError(f"Expected `preds` and `target` to have the same shape, but got {tuple(preds.shape)} and {tuple(target.shape)}.")
    if input_format == "index":
        if preds.ndim < 2:
            raise ValueError(f"Expected label maps of shape [B, *spatial] with at least one spatial dim, but got {tuple(preds.shape)}.")
    else:
        if preds.ndim < 3:
            raise ValueError(f"Expected one-hot masks of shape [B, C, *spatial] with at least one spatial dim, but got {tuple(preds.shape)}.")
        if preds.shape[1] != num_classes:
            raise ValueError(f"Expected one-hot masks with {num_classes} channels, but got {preds.shape[1]}.")


def _native_segment_ok(preds: Tensor, target: Tensor, num_classes: int, input_format: str) -> bool:
    """Route to the ops of ``csrc/segment_overlap.hip``; everything else keeps the composition."""
    if not (preds.is_cuda and target.is_cuda):
        return False
    dtypes = _INDEX_DTYPES if input_format == "index" else _ONEHOT_DTYPES
    if preds.dtype not in dtypes or target.dtype not in dtypes:
        return False
    if input_format == "index" and num_classes > _SEGMENT_MAX_CLASSES:
        return False
    return _SEGMENT_NATIVE and ops.use_native(preds, target)


def _overlap_composition(preds: Tensor, target: Tensor, num_classes: int, input_format: str) -> Tensor:
    """The counts by comparison and sum.  Membership of a label map is ``label == class`` (never ``one_hot``): a label outside ``[0, C)``
    matches no class and nothing raises, on the CPU and the GPU alike."""
    if input_format == "index":
        classes = torch.arange(num_classes, device=preds.device).view(1, num_classes, *([1] * (preds.ndim - 1)))
        pm, tm = preds.unsqueeze(1) == classes, target.unsqueeze(1) == classes
    else:
        pm, tm = preds != 0, target != 0
    pm, tm = pm.flatten(2), tm.flatten(2)
    return torch.stack([(pm & tm).sum(-1), pm.sum(-1), tm.sum(-1)], dim=-1)


def _overlap_counts(preds: Tensor, target: Tensor, num_classes: int, input_format: str) -> Tuple[Tensor, bool]:
    """``(int64 [B, C, 3] counts, whether the native op made them)``."""
    if _native_segment_ok(preds, target, num_classes, input_format):
        if input_format == "index":
            return _ops_seg.segment_overlap_index(preds, target, num_classes), True
        return _ops_seg.segment_overlap_onehot(preds, target), True
    return _overlap_composition(preds, target, num_classes, input_format), False


def _sdiv(a: Tensor, b: Tensor) -> Tensor:
    ok = b != 0
    return torch.where(ok, a / torch.where(ok, b, torch.ones_like(b)), torch.zeros_like(a))


def _scores_composition(counts: Tensor, metric: int, option: int, include_background: bool) -> Tensor:
    """fp64 scores of the counts, the arithmetic of ``segment_scores_kernel`` as tensor expressions."""
    k = counts[:, (0 if include_background else 1):].double()
    i, p, t = k[..., 0], k[..., 1], k[..., 2]
    if metric == _ops_seg.METRIC_IOU:
        iou = _sdiv(i, p + t - i)
        return iou if option == 1 else iou.mean(dim=1)
    if metric == _ops_seg.METRIC_DICE:
        d = _sdiv(2 * i, p + t)
        if option == 0:
            return _sdiv((2 * i).sum(dim=1), (p + t).sum(dim=1))
        if option == 1:
            return d.mean(dim=1)
        if option == 2:
            return (_sdiv(t, t.sum(dim=1, keepdim=True).expand_as(t)) * d).sum(dim=1)
        return d
    weight, per_class = option % 3, option >= 3
    if weight == 2:
        w = torch.ones_like(t)
    else:
        present = t != 0
        safe = torch.where(present, t, torch.ones_like(t))
        w = torch.where(present, 1.0 / (safe * safe if weight == 0 else safe), torch.zeros_like(t))
        # an absent class takes the largest finite weight of its own sample (0 when the sample has none)
        w = torch.where(present, w, w.max(dim=1, keepdim=True).values.expand_as(w))
    if per_class:
        return _sdiv(2 * i * w, (p + t) * w)
    return _sdiv((2 * i * w).sum(dim=1), ((p + t) * w).sum(dim=1))


def _segment_values(preds: Tensor, target: Tensor, num_classes: int, include_background: bool, input_format: str, metric: int,
                    option: int) -> Tensor:
    """fp64 per-sample values ``[B]`` or ``[B, C']``: one overlap call, then one score call on the same route."""
    _check_inputs(preds, target, num_classes, include_background, input_format)
    counts, native = _overlap_counts(preds, target, num_classes, input_format)
    if native:
        return _ops_seg.segment_scores(counts, metric, option, include_background)
    return _scores_composition(counts, metric, option, include_background)


def _kept_classes(num_classes: int, include_background: bool) -> int:
    return num_classes if include_background else num_classes - 1


def _check_flag(name: str, value: Optional[bool]) -> None:
    if not isinstance(value, bool):
        raise ValueError(f"Expected argument `{name}` to be a bool, but got {value}.")
