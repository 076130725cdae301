"""Normalized mutual information (API parity: reference ``functional/clustering/normalized_mutual_info_score.py``)."""
import torch
from torch import Tensor
from typing_extensions import Literal

from torchmetrics_forked_amd.functional.clustering.mutual_info_score import mutual_info_score
from torchmetrics_forked_amd.functional.clustering.utils import (
    _native_extrinsic,
    _validate_average_method_arg,
    calculate_entropy,
    calculate_generalized_mean,
    check_cluster_labels,
)


def normalized_mutual_info_score(
    preds: Tensor, target: Tensor, average_method: Literal["min", "geometric", "arithmetic", "max"] = "arithmetic"
) -> Tensor:
    check_cluster_labels(preds, target)
    _validate_average_method_arg(average_method)
    native = _native_extrinsic(preds, target, "normalized_mutual_info", average_method)
    if native is not None:
        return native
    mutual_info = mutual_info_score(preds, target)
    if torch.allclose(mutual_info, torch.tensor(0.0, device=mutual_info.device), atol=torch.finfo().eps):
        return mutual_info
    normalizer = calculate_generalized_mean(torch.stack([calculate_entropy(preds), calculate_entropy(target)]), average_method)
    return mutual_info / normalizer
