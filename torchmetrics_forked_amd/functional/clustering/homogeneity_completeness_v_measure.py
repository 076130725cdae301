"""Homogeneity / completeness / V-measure (API parity: reference
``functional/clustering/homogeneity_completeness_v_measure.py``)."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from torchmetrics_forked_amd.functional.clustering.mutual_info_score import mutual_info_score
from torchmetrics_forked_amd.functional.clustering.utils import _native_extrinsic, calculate_entropy, check_cluster_labels


def _homogeneity_score_compute(preds: Tensor, target: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    check_cluster_labels(preds, target)
    if len(target) == 0:
        zero = torch.tensor(0.0, dtype=torch.float32, device=preds.device)
        return zero.clone(), zero.clone(), zero.clone(), zero.clone()
    h_t, h_p = calculate_entropy(target), calculate_entropy(preds)
    mi = mutual_info_score(preds, target)
    homogeneity = mi / h_t if h_t else torch.ones_like(h_t)
    return homogeneity, mi, h_p, h_t


def _completeness_score_compute(preds: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    homogeneity, mi, h_p, _ = _homogeneity_score_compute(preds, target)
    completeness = mi / h_p if h_p else torch.ones_like(h_p)
    return completeness, homogeneity


def _native_score(preds: Tensor, target: Tensor, metric: str, beta: float = 1.0) -> Optional[Tensor]:
    check_cluster_labels(preds, target)
    return _native_extrinsic(preds, target, metric, beta=beta)


def homogeneity_score(preds: Tensor, target: Tensor) -> Tensor:
    native = _native_score(preds, target, "homogeneity")
    if native is not None:
        return native
    return _homogeneity_score_compute(preds, target)[0]


def completeness_score(preds: Tensor, target: Tensor) -> Tensor:
    native = _native_score(preds, target, "completeness")
    if native is not None:
        return native
    return _completeness_score_compute(preds, target)[0]


def v_measure_score(preds: Tensor, target: Tensor, beta: float = 1.0) -> Tensor:
    native = _native_score(preds, target, "v_measure", beta)
    if native is not None:
        return native
    completeness, homogeneity = _completeness_score_compute(preds, target)
    if homogeneity + completeness == 0.0:
        return torch.ones_like(homogeneity)
    return (1 + beta) * homogeneity * completeness / (beta * homogeneity + completeness)
