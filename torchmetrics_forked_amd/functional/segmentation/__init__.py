"""Segmentation functionals: per-sample scores of label maps and masks (beyond the reference's API)."""
from torchmetrics_forked_amd.functional.segmentation.dice import dice_score
from torchmetrics_forked_amd.functional.segmentation.generalized_dice import generalized_dice_score
from torchmetrics_forked_amd.functional.segmentation.mean_iou import mean_iou

__all__ = ["dice_score", "generalized_dice_score", "mean_iou"]
