"""Brute-force Hausdorff distance of two boolean planes in plain NumPy fp64: edges by four shifted copies with zero padding, then the minimum
over all edge pairs.  Imports nothing from the package."""
import numpy as np


def edges(mask):
    """The pixels of ``mask`` [H, W] that are not interior (interior: the pixel and its four neighbours are members; outside is not)."""
    m = np.asarray(mask, dtype=bool)
    p = np.pad(m, 1)
    return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def directed(a, b, metric="euclidean", spacing=(1.0, 1.0), squared=False):
    """``h(A -> B)`` over the edge sets: max over nothing 0, min over nothing inf.  ``squared``: the euclidean distance squared (an exact
    integer without spacing)."""
    ea, eb = np.argwhere(edges(a)), np.argwhere(edges(b))
    if len(ea) == 0:
        return 0.0
    if len(eb) == 0:
        return np.inf
    off = np.abs(ea[:, None, :].astype(np.float64) - eb[None, :, :]) * np.asarray(spacing, dtype=np.float64)
    if metric == "euclidean":
        d = (off ** 2).sum(-1)
        d = d if squared else np.sqrt(d)
    elif metric == "chessboard":
        d = off.max(-1)
    else:
        d = off.sum(-1)
    return float(d.min(axis=1).max())


def hausdorff(a, b, metric="euclidean", spacing=(1.0, 1.0), is_directed=False, squared=False):
    h = directed(a, b, metric, spacing, squared)
    return h if is_directed else max(h, directed(b, a, metric, spacing, squared))


def planes(preds, target, metric="euclidean", spacing=(1.0, 1.0), is_directed=False, squared=False):
    """fp64 [B, C'] of boolean [B, C', H, W] arrays."""
    return np.array([[hausdorff(p, t, metric, spacing, is_directed, squared) for p, t in zip(ps, ts)] for ps, ts in zip(preds, target)], dtype=np.float64)


def blobs(shape, seed, discs=3):
    """Boolean ``shape`` (..., H, W): a few random discs per plane."""
    rng = np.random.default_rng(seed)
    h, w = shape[-2:]
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros((int(np.prod(shape[:-2], dtype=np.int64)), h, w), dtype=bool)
    for m in out:
        for _ in range(discs):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1, max(2.0, min(h, w) / 3))
            m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return out.reshape(shape)
