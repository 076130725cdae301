"""Adjusted Rand score (API parity: reference ``functional/clustering/adjusted_rand_score.py``)."""
import torch
from torch import Tensor

from torchmetrics_forked_amd.functional.clustering.utils import (
    _native_extrinsic,
    calculate_contingency_matrix,
    calculate_pair_cluster_confusion_matrix,
    check_cluster_labels,
)


def _adjusted_rand_score_update(preds: Tensor, target: Tensor) -> Tensor:
    check_cluster_labels(preds, target)
    return calculate_contingency_matrix(preds, target)


def _adjusted_rand_score_compute(contingency: Tensor) -> Tensor:
    (tn, fp), (fn, tp) = calculate_pair_cluster_confusion_matrix(contingency=contingency)
    if fn == 0 and fp == 0:
        return torch.ones_like(tn, dtype=torch.float32)
    tn, fp, fn, tp = (x.double() for x in (tn, fp, fn, tp))
    return (2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))).float()


def adjusted_rand_score(preds: Tensor, target: Tensor) -> Tensor:
    check_cluster_labels(preds, target)
    native = _native_extrinsic(preds, target, "adjusted_rand")
    if native is not None:
        return native
    return _adjusted_rand_score_compute(_adjusted_rand_score_update(preds, target))
