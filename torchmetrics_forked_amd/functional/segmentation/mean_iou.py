"""Per-sample mean intersection over union of segmentation maps (beyond the reference's API; named as upstream's later ``segmentation``
package).

``iou[b, c] = I / (P + T - I)`` from the class-overlap counts of sample ``b`` (0 where the class is absent from both sides), averaged over
the classes kept.  On the GPU the counts are one read of the inputs by the kernels of ``csrc/segment_overlap.hip`` and the scores one
launch (see ``utils.py`` for what keeps the composition); score arithmetic is fp64, results are fp32.

This is a per-image score.  Dataset-level mIoU from one confusion matrix over the whole dataset stays ``MulticlassJaccardIndex``."""
from torch import Tensor

from torchmetrics_forked_amd.functional.segmentation.utils import _check_flag, _segment_values
from torchmetrics_forked_amd.ops.segmentation import METRIC_IOU


def _mean_iou_values(preds: Tensor, target: Tensor, num_classes: int, include_background: bool, per_class: bool, input_format: str) -> Tensor:
    _check_flag("per_class", per_class)
    return _segment_values(preds, target, num_classes, include_background, input_format, METRIC_IOU, 1 if per_class else 0)


def mean_iou(preds: Tensor, target: Tensor, num_classes: int, include_background: bool = True, per_class: bool = False,
             input_format: str = "one-hot") -> Tensor:
    """``[B]`` mean IoU of every sample, or ``[B, C']`` IoU per class with ``per_class``.

    ``input_format="one-hot"``: ``preds`` / ``target`` ``[B, C, *spatial]`` masks (bool / integer, nonzero = member);
    ``"index"``: ``[B, *spatial]`` integer label maps, where a label outside ``[0, num_classes)`` (a void label) belongs to no class.

    Example:
        >>> import torch
        >>> from torchmetrics_forked_amd.functional.segmentation import mean_iou
        >>> preds = torch.tensor([[[0, 1], [1, 2]]])
        >>> target = torch.tensor([[[0, 1], [2, 2]]])
        >>> mean_iou(preds, target, num_classes=3, input_format="index")
        tensor([0.6667])
    """
    return _mean_iou_values(preds, target, num_classes, include_background, per_class, input_format).float()
