"""Rand score (API parity: reference ``functional/clustering/rand_score.py``)."""
import torch
from torch import Tensor

from torchmetrics_forked_amd.functional.clustering.utils import (
    _native_extrinsic,
    calculate_contingency_matrix,
    calculate_pair_cluster_confusion_matrix,
    check_cluster_labels,
)


def _rand_score_update(preds: Tensor, target: Tensor) -> Tensor:
    check_cluster_labels(preds, target)
    return calculate_contingency_matrix(preds, target)


def _rand_score_compute(contingency: Tensor) -> Tensor:
    pair = calculate_pair_cluster_confusion_matrix(contingency=contingency)
    num, den = pair.diagonal().sum(), pair.sum()
    if num == den or den == 0:
        return torch.ones_like(num, dtype=torch.float32)
    return num / den


def rand_score(preds: Tensor, target: Tensor) -> Tensor:
    check_cluster_labels(preds, target)
    native = _native_extrinsic(preds, target, "rand")
    if native is not None:
        return native
    return _rand_score_compute(_rand_score_update(preds, target))
