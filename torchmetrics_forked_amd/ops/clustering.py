"""Python entry points for ``csrc/clustering.hip`` (expected mutual information on the GPU) and
``csrc/cluster_scatter.hip`` (label ranks, segmented sums, scatter and score of the intrinsic clustering metrics)."""
from typing import Dict, Tuple

from torch import Tensor
import torch

CLUSTER_METRICS = {"calinski_harabasz": 0, "davies_bouldin": 1, "dunn": 2}


def expected_mutual_info(a: Tensor, b: Tensor, n_samples: int) -> Tensor:
    """fp64 EMI of the row / column marginals ``a`` [R] and ``b`` [K] (one wave per cluster pair)."""
    return torch.ops.tmx.expected_mutual_info(a.double().contiguous(), b.double().contiguous(), float(n_samples))


def _require() -> None:
    from torchmetrics_forked_amd import ops

    ops.require()


def cluster_tile() -> Dict[str, int]:
    """Constants of the cluster kernels: workgroup threads, columns per sums tile (``td``), clusters per sums window
    (``kw``), the narrowest row group (``min_dp``), the presence bitmap's span and the largest ``K`` the route takes."""
    _require()
    return dict(zip(("threads", "td", "kw", "min_dp", "bitmap_span", "cap"), (int(v) for v in torch.ops.tmx.cluster_tile())))


def cluster_rows_per_chunk(n: int, d: int, k: int, which: int = 0) -> int:
    """Rows one workgroup of the sums pass (``which=0``), the CH / Dunn scatter (1) or the DB scatter (2) walks for a
    ``[n, d]`` call with ``k`` clusters (a function of the shape alone)."""
    _require()
    return int(torch.ops.tmx.cluster_rows_per_chunk(int(n), int(d), int(k), int(which)))


def cluster_label_ranks(labels: Tensor) -> Tuple[Tensor, int]:
    """int32 ranks of integer ``labels`` among their distinct values, and the number of distinct values ``K``.

    One host read: the pair (K, wide flag).  Labels spanning 2^20 or more take ``torch.unique``'s inverse."""
    inv, info = torch.ops.tmx.cluster_label_ranks(labels)
    k, wide = info.tolist()
    if wide:
        uniq, inv = torch.unique(labels, return_inverse=True)
        return inv.to(torch.int32), len(uniq)
    return inv, k


def cluster_intrinsic_score(data: Tensor, inv: Tensor, k: int, metric: str, p: float = 2.0) -> Tensor:
    """Score of ``data`` [N, D] under the int32 ranks ``inv`` in ``[0, k)``, in the dtype the composition returns.

    fp32 data never reads the host.  For 16-bit data the composition's dtype depends on the value (its ``within == 0``
    and ``allclose`` rules return fp32 constants), so Calinski-Harabasz and Davies-Bouldin read the kernel's edge flag."""
    res, resf = torch.ops.tmx.cluster_intrinsic_score(data, inv, int(k), CLUSTER_METRICS[metric], float(p))
    if data.dtype == torch.float32 or (metric != "dunn" and bool(res[1])):
        return resf.reshape(())
    return res[0].to(data.dtype)
