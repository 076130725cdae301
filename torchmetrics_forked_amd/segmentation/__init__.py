"""Segmentation metrics: means over samples of per-sample scores of label maps and masks (beyond the reference's API)."""
from torchmetrics_forked_amd.segmentation.dice import DiceScore
from torchmetrics_forked_amd.segmentation.generalized_dice import GeneralizedDiceScore
from torchmetrics_forked_amd.segmentation.mean_iou import MeanIoU

__all__ = ["DiceScore", "GeneralizedDiceScore", "MeanIoU"]
