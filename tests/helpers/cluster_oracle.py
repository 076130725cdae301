"""Plain numpy fp64 oracle of the intrinsic clustering scores (labels compacted with ``numpy.unique``), with the
composition's edge rules: CH is 1 when the within-cluster scatter is 0, DB is 0 when every intra-cluster mean distance or
every centroid distance is within 1e-8 of 0 and treats a zero centroid distance as +inf."""
import numpy as np


def cluster_oracle(data, labels, metric, p=2.0):
    x = np.asarray(data, dtype=np.float64)
    _, inv = np.unique(np.asarray(labels), return_inverse=True)
    k, n = int(inv.max()) + 1, x.shape[0]
    counts = np.bincount(inv, minlength=k).astype(np.float64)
    mu = np.stack([x[inv == c].mean(axis=0) for c in range(k)])
    diff = x - mu[inv]
    with np.errstate(all="ignore"):
        if metric == "calinski_harabasz":
            within = (diff**2).sum()
            between = (counts * ((mu - x.mean(axis=0)) ** 2).sum(axis=1)).sum()
            return 1.0 if within == 0 else between * (n - k) / (within * (k - 1.0))
        pair = mu[:, None, :] - mu[None, :, :]
        if metric == "davies_bouldin":
            dist = np.sqrt((diff**2).sum(axis=1))
            s = np.array([dist[inv == c].mean() for c in range(k)])
            d = np.sqrt((pair**2).sum(axis=2))
            if np.all(np.abs(s) <= 1e-8) or np.all(np.abs(d) <= 1e-8):
                return 0.0
            d[d == 0] = np.inf
            ratio = (s[:, None] + s[None, :]) / d
            return float(np.where(np.isnan(ratio).any(axis=1), np.nan, ratio.max(axis=1)).mean())
        inter = (np.abs(pair) ** p).sum(axis=2) ** (1.0 / p)
        radius = (np.abs(diff) ** p).sum(axis=1) ** (1.0 / p)
        inter = inter[np.triu_indices(k, 1)]
        if np.isnan(inter).any() or np.isnan(radius).any():
            return float("nan")
        return float(inter.min() / radius.max())
