"""Thin wrappers of the class-overlap ops of ``csrc/segment_overlap.hip`` behind the segmentation metrics (mean IoU, Dice, generalized Dice)."""
from typing import Tuple

import torch
from torch import Tensor

METRIC_IOU, METRIC_DICE, METRIC_GENERALIZED_DICE = 0, 1, 2
DICE_OPTIONS = {"micro": 0, "macro": 1, "weighted": 2, "none": 3}
WEIGHT_OPTIONS = {"square": 0, "simple": 1, "linear": 2}


def segment_overlap_index(preds: Tensor, target: Tensor, num_classes: int) -> Tensor:
    """``tmx::segment_overlap_index``: int64 ``[B, C, 3]`` counts ``(I, P, T)`` of the label maps ``preds`` / ``target`` ``[B, *spatial]``
    (uint8 / int16 / int32 / int64, the two may differ, read in place): pixels in class ``c`` on both sides, in ``preds`` and in ``target``.
    A label outside ``[0, C)`` is in no class on its side.  ``C`` at most ``segment_overlap_tile()[2]``.  Integer atomics: two runs are
    bit-equal.  No host read, no autograd."""
    return torch.ops.tmx.segment_overlap_index(preds, target, int(num_classes))


def segment_overlap_onehot(preds: Tensor, target: Tensor) -> Tensor:
    """``tmx::segment_overlap_onehot``: the same counts from masks ``[B, C, *spatial]`` (bool / uint8 / int32 / int64, the two may differ),
    nonzero meaning member."""
    return torch.ops.tmx.segment_overlap_onehot(preds, target)


def segment_scores(counts: Tensor, metric: int, option: int, include_background: bool) -> Tensor:
    """``tmx::segment_scores``: fp64 scores of int64 counts ``[B, C, 3]`` in one launch, ``[B]`` or ``[B, C']`` for the per-class forms.
    ``metric``: ``METRIC_IOU`` (``option`` 0 mean over classes, 1 per class), ``METRIC_DICE`` (``DICE_OPTIONS``) or
    ``METRIC_GENERALIZED_DICE`` (``WEIGHT_OPTIONS[weight_type] + 3 * per_class``)."""
    return torch.ops.tmx.segment_scores(counts, int(metric), int(option), bool(include_background))


def segment_overlap_tile() -> Tuple[int, int, int, int]:
    """``(threads per workgroup, pixels per lane per step, class cap of the index form, chunk alignment in pixels)``."""
    return tuple(int(v) for v in torch.ops.tmx.segment_overlap_tile())  # type: ignore[return-value]


def segment_overlap_chunks(B: int, n: int, C: int, onehot: bool) -> int:
    """Chunks the overlap kernels split every row of ``n`` pixels into (index form: ``B`` rows; one-hot form: ``B * C``): a function of the
    shape alone, and of ``TMX_SEGMENT_CHUNK`` where a test sets it."""
    return int(torch.ops.tmx.segment_overlap_chunks(int(B), int(n), int(C), bool(onehot)))
