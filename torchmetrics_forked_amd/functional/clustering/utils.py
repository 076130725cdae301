"""Clustering helpers (behavioural parity: reference ``functional/clustering/utils.py:20-284``).

Contingency tables are built with one dense bincount over ``target_idx * K_pred + pred_idx`` (the framework's
LDS histogram kernel on the GPU) instead of a sparse COO tensor densified afterwards."""
import math
import os
from typing import Optional, Union

import torch
from torch import Tensor, tensor
from typing_extensions import Literal

from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.utilities.checks import _check_same_shape
from torchmetrics_forked_amd.utilities.data import _bincount


def is_nonnegative(x: Tensor, atol: float = 1e-5) -> Tensor:
    return torch.logical_or(x > 0.0, torch.abs(x) < atol).all()


def _validate_average_method_arg(average_method: str = "arithmetic") -> None:
    if average_method not in ("min", "geometric", "arithmetic", "max"):
        raise ValueError(
            "Expected argument `average_method` to be one of  `min`, `geometric`, `arithmetic`, `max`,"
            f"but got {average_method}"
        )


def calculate_entropy(x: Tensor) -> Tensor:
    """Shannon entropy (nats) of a label vector."""
    if len(x) == 0:
        return tensor(1.0, device=x.device)
    p = torch.bincount(torch.unique(x, return_inverse=True)[1])
    p = p[p > 0]
    n = p.sum()
    return -torch.sum(p / n * (torch.log(p) - torch.log(n)))


def calculate_generalized_mean(x: Tensor, p: Union[int, Literal["min", "geometric", "arithmetic", "max"]]) -> Tensor:
    if torch.is_complex(x) or not is_nonnegative(x):
        raise ValueError("`x` must contain positive real numbers")
    if isinstance(p, str):
        if p == "min":
            return x.min()
        if p == "geometric":
            return torch.exp(torch.mean(x.log()))
        if p == "arithmetic":
            return x.mean()
        if p == "max":
            return x.max()
        raise ValueError("'method' must be 'min', 'geometric', 'arirthmetic', or 'max'")
    return torch.mean(torch.pow(x, p)) ** (1.0 / p)


def calculate_contingency_matrix(preds: Tensor, target: Tensor, eps: Optional[float] = None, sparse: bool = False) -> Tensor:
    """``[n_target_clusters, n_pred_clusters]`` co-occurrence counts."""
    if eps is not None and sparse is True:
        raise ValueError("Cannot specify `eps` and return sparse tensor.")
    if preds.ndim != 1 or target.ndim != 1:
        raise ValueError(f"Expected 1d `preds` and `target` but got {preds.ndim} and {target.dim}.")
    contingency = None
    if _native_extrinsic_ok(preds, target):
        from torchmetrics_forked_amd.ops import clustering as native

        contingency = native.cluster_pair_table(preds, target)  # None above the cluster cap
    if contingency is None:
        contingency = _composed_contingency_matrix(preds, target)
    if sparse:
        return contingency.to_sparse()
    if eps:
        contingency = contingency + eps
    return contingency


def _composed_contingency_matrix(preds: Tensor, target: Tensor) -> Tensor:
    _, p_idx = torch.unique(preds, return_inverse=True)
    _, t_idx = torch.unique(target, return_inverse=True)
    kp = int(p_idx.max()) + 1 if p_idx.numel() else 0
    kt = int(t_idx.max()) + 1 if t_idx.numel() else 0
    return _bincount(t_idx * kp + p_idx, minlength=kt * kp).reshape(kt, kp)


def _is_real_discrete_label(x: Tensor) -> bool:
    if x.ndim != 1:
        raise ValueError(f"Expected arguments to be 1-d tensors but got {x.ndim}-d tensors.")
    return not (torch.is_floating_point(x) or torch.is_complex(x))


def check_cluster_labels(preds: Tensor, target: Tensor) -> None:
    _check_same_shape(preds, target)
    if not (_is_real_discrete_label(preds) and _is_real_discrete_label(target)):
        raise ValueError(f"Expected real, discrete values for x but received {preds.dtype} and {target.dtype}.")


def _validate_intrinsic_cluster_data(data: Tensor, labels: Tensor) -> None:
    if data.ndim != 2:
        raise ValueError(f"Expected 2D data, got {data.ndim}D data instead")
    if not data.is_floating_point():
        raise ValueError(f"Expected floating point data, got {data.dtype} data instead")
    if labels.ndim != 1:
        raise ValueError(f"Expected 1D labels, got {labels.ndim}D labels instead")


def _validate_intrinsic_labels_to_samples(num_labels: int, num_samples: int) -> None:
    if not 1 < num_labels < num_samples:
        raise ValueError(
            "Number of detected clusters must be greater than one and less than the number of samples."
            f"Got {num_labels} clusters and {num_samples} samples."
        )


def calculate_pair_cluster_confusion_matrix(
    preds: Optional[Tensor] = None, target: Optional[Tensor] = None, contingency: Optional[Tensor] = None
) -> Tensor:
    """2x2 pair confusion matrix (pairs of samples clustered together / apart in preds vs target)."""
    if preds is None and target is None and contingency is None:
        raise ValueError("Must provide either `preds` and `target` or `contingency`.")
    if preds is not None and target is not None and contingency is not None:
        raise ValueError("Must provide either `preds` and `target` or `contingency`, not both.")
    if preds is not None and target is not None:
        contingency = calculate_contingency_matrix(preds, target)
    if contingency is None:
        raise ValueError("Must provide `contingency` if `preds` and `target` are not provided.")
    n = contingency.sum()
    sum_c, sum_k = contingency.sum(dim=1), contingency.sum(dim=0)
    sq = (contingency**2).sum()
    out = torch.zeros(2, 2, dtype=contingency.dtype, device=contingency.device)
    out[1, 1] = sq - n
    out[1, 0] = (contingency * sum_k).sum() - sq
    out[0, 1] = (contingency.T * sum_c).sum() - sq
    out[0, 0] = n**2 - out[0, 1] - out[1, 0] - sq
    return out


def _cluster_means(data: Tensor, labels: Tensor, k: int) -> "tuple[Tensor, Tensor]":
    """Per-cluster sizes ``[K]`` and centroids ``[K, D]`` with one segmented sum."""
    counts = torch.bincount(labels, minlength=k).to(data.dtype)
    sums = torch.zeros(k, data.shape[1], dtype=data.dtype, device=data.device).index_add_(0, labels, data)
    return counts, sums / counts.unsqueeze(1)


_NATIVE_FLOATS = (torch.float32, torch.bfloat16, torch.float16)
_NATIVE_LABELS = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def _native_intrinsic_ok(data: Tensor, labels: Tensor, p: float = 2) -> bool:
    """True when an intrinsic clustering score of (``data``, ``labels``) can run on ``csrc/cluster_scatter.hip``: 2-D
    fp32 / bf16 / fp16 data on the GPU with at least one row and column, integer labels of the same length on the same
    device, no gradient wanted, a finite norm ``p >= 1`` and ``TMX_CLUSTER_NATIVE`` not ``0``.  Everything else (fp64,
    CPU tensors, float labels, ``p = inf``, ``p < 1``) keeps the torch composition; so does a call with more clusters
    than ``ops.clustering.cluster_tile()["cap"]`` or than ``_native_wins`` admits (``_native_intrinsic``)."""
    if not (isinstance(data, Tensor) and isinstance(labels, Tensor) and data.is_cuda and labels.is_cuda):
        return False
    if data.ndim != 2 or labels.ndim != 1 or data.dtype not in _NATIVE_FLOATS or labels.dtype not in _NATIVE_LABELS:
        return False
    if data.shape[0] < 1 or data.shape[1] < 1 or labels.shape[0] != data.shape[0] or data.shape[0] >= 2**31 - 1:
        return False
    if data.requires_grad and torch.is_grad_enabled():
        return False
    if not isinstance(p, (int, float)) or not (math.isfinite(p) and p >= 1):
        return False
    return os.environ.get("TMX_CLUSTER_NATIVE", "1") != "0" and ops.use_native(data, labels)


def _native_extrinsic_ok(preds: Tensor, target: Tensor) -> bool:
    """True when the contingency table of (``preds``, ``target``) can be built by ``csrc/cluster_pairs.hip``: two 1-D label
    vectors of equal, non-zero length on the GPU, each of an integer dtype (the sides may differ), the default dtype fp32
    (the composition's result dtype follows it) and ``TMX_CLUSTER_NATIVE`` not ``0``.  Everything else (CPU tensors, empty
    inputs, float or bool labels) keeps the torch composition; so does a call with more clusters on a side than
    ``ops.clustering.cluster_pair_tile()["cap"]`` (``_native_extrinsic``)."""
    if not (isinstance(preds, Tensor) and isinstance(target, Tensor) and preds.is_cuda and target.is_cuda):
        return False
    if preds.ndim != 1 or target.ndim != 1 or preds.dtype not in _NATIVE_LABELS or target.dtype not in _NATIVE_LABELS:
        return False
    if preds.shape[0] < 1 or preds.shape[0] != target.shape[0] or preds.shape[0] >= 2**31 - 1:
        return False
    if torch.get_default_dtype() != torch.float32:
        return False
    return os.environ.get("TMX_CLUSTER_NATIVE", "1") != "0" and ops.use_native(preds, target)


def _native_extrinsic(preds: Tensor, target: Tensor, metric: str, average_method: str = "arithmetic", beta: float = 1.0) -> Optional[Tensor]:
    """The native score of two validated label vectors, or None when the call keeps the composition."""
    if not isinstance(beta, (int, float)) or not _native_extrinsic_ok(preds, target):
        return None
    from torchmetrics_forked_amd.ops import clustering as native

    return native.cluster_extrinsic_score(preds, target, metric, average_method, beta)


def _native_wins(n: int, d: int, k: int) -> bool:
    """Measured routing (``tools/cluster_bench.py``, ``profiles/cluster_bench.json``; whole call, fp32).  The native route
    wins for all three metrics at 1M x 128 with K = 16 (1.8-15.9x), 262 144 x 32 with K = 100 (1.3-3.8x), 65 536 x 2 with
    K = 8 (2.1-6.8x) and 4096 x 512 with K = 10 (1.2-1.8x).  At 1M x 16 with K = 1000 it loses (0.13-0.69x): the sums pass
    walks 63 cluster windows and the one-workgroup score kernel forms a million centroid pairs.  No shape between K = 100
    and K = 1000 was measured, so the route ends at 128 clusters, just above the largest K measured to win."""
    return k <= 128


def _native_intrinsic(data: Tensor, labels: Tensor, metric: str, p: float = 2, validate: bool = True) -> Optional[Tensor]:
    """The native score of an admitted call, or None when the number of clusters keeps it on the composition."""
    from torchmetrics_forked_amd.ops import clustering as native

    inv, k = native.cluster_label_ranks(labels)
    if validate:
        _validate_intrinsic_labels_to_samples(k, data.shape[0])
    if k < 2 or k > native.cluster_tile()["cap"] or not _native_wins(data.shape[0], data.shape[1], k):
        return None
    return native.cluster_intrinsic_score(data, inv, k, metric, p)
