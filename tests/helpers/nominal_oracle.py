"""Plain oracle of the nominal association metrics, written from the formulas; imports nothing from the package.

Labels follow the metrics' rule: NaN is replaced (``"replace"``) or the row is left out of every pair it takes part in (``"drop"``), then the
value is truncated toward zero.  A pair's contingency table is one ``numpy.bincount``; its rows are the second series' (``target``) categories,
its columns the first series' (``preds``).  The four scores are evaluated in a given dtype from the exact integer table: ``torch.float64`` is
the oracle, ``torch.float32`` (``comp32``) measures what an fp32 evaluation of the same formulas loses.

    χ² = Σ (n_ab - e_ab)² / e_ab,  e_ab = n_a. n_.b / n   over the r non-empty rows and c non-empty columns; 0 when (r - 1)(c - 1) == 0;
         with bias correction and (r - 1)(c - 1) == 1 every count first moves half a count toward its expectation
    φ² = χ² / n;  bias-corrected: φ²c = max(φ² - (r - 1)(c - 1) / (n - 1), 0), rc = r - (r - 1)² / (n - 1), cc alike; NaN when min(rc, cc) == 1
    Cramér's V = sqrt(φ² / min(r - 1, c - 1)),  Tschuprow's T = sqrt(φ² / sqrt((r - 1)(c - 1))),  Pearson's C = sqrt(φ² / (1 + φ²)), clamped to [0, 1]
    Theil's U = (H(preds) - H(preds | target)) / H(preds), 0 when H(preds) == 0
"""
from typing import Optional, Tuple

import numpy as np
import torch

CRAMERS, TSCHUPROWS, PEARSON, THEILS = 0, 1, 2, 3
KINDS = (CRAMERS, TSCHUPROWS, PEARSON, THEILS)
DROP = -1  # the label of a dropped element


def labels(matrix, nan_strategy: str = "replace", nan_replace: Optional[float] = 0.0) -> np.ndarray:
    """int64 labels of a ``[N, V]`` (or ``[N]``) array or tensor; ``DROP`` where a NaN is dropped."""
    a = matrix.detach().cpu().numpy() if isinstance(matrix, torch.Tensor) else np.asarray(matrix)
    if a.dtype.kind != "f":
        return a.astype(np.int64)
    bad = np.isnan(a)
    if nan_strategy == "replace":
        a = np.where(bad, a.dtype.type(nan_replace), a)
        return np.trunc(a).astype(np.int64)
    return np.where(bad, DROP, np.trunc(np.where(bad, 0, a))).astype(np.int64)


def table(preds_lab: np.ndarray, target_lab: np.ndarray, k: int) -> np.ndarray:
    """int64 ``[k, k]``: entry ``[a, b]`` counts the rows with ``target == a`` and ``preds == b``; rows with a dropped label are left out."""
    keep = (preds_lab != DROP) & (target_lab != DROP)
    p, t = preds_lab[keep], target_lab[keep]
    assert p.size == 0 or (p.min() >= 0 and t.min() >= 0 and p.max() < k and t.max() < k)
    return np.bincount(t * k + p, minlength=k * k).reshape(k, k)


def pair_tables(lab: np.ndarray, k: int) -> np.ndarray:
    """int64 ``[V, V, k, k]`` with ``[i, j] = table(preds=col_i, target=col_j)`` for ``i < j``, zeros elsewhere."""
    v = lab.shape[1]
    out = np.zeros((v, v, k, k), dtype=np.int64)
    for i in range(v):
        for j in range(i + 1, v):
            out[i, j] = table(lab[:, i], lab[:, j], k)
    return out


def _shape(tab) -> Tuple[torch.Tensor, int, int]:
    t = torch.as_tensor(np.asarray(tab)).to(torch.float64)
    t = t[t.sum(1) != 0]
    t = t[:, t.sum(0) != 0]
    return t, t.shape[0], t.shape[1]


def unable(tab) -> bool:
    """True where the bias correction cannot be applied: ``min(rc, cc) == 1``, that is one non-empty row or column, or as many as samples
    (a single sample gives 0 / 0 and compares unequal)."""
    t, r, c = _shape(tab)
    n = np.float64(t.sum())
    with np.errstate(all="ignore"):
        rc = np.float64(r) - np.float64((r - 1) ** 2) / (n - 1)
        cc = np.float64(c) - np.float64((c - 1) ** 2) / (n - 1)
    return bool(np.minimum(rc, cc) == 1)


def score(tab, kind: int, bias_correction: bool = False, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """The score of one table, every operation in ``dtype``; 0-dim tensor of ``dtype``."""
    t, r, c = _shape(tab)
    t = t.to(dtype)
    n = t.sum()
    nan = torch.tensor(float("nan"), dtype=dtype)
    if kind == THEILS:
        if r == 0:
            return torch.zeros((), dtype=dtype)
        p_x = t.sum(0) / n
        s_x = -(p_x * torch.log(p_x)).sum()
        if s_x == 0:
            return torch.zeros((), dtype=dtype)
        p_xy = t / n
        p_y = (t.sum(1) / n)[:, None].expand_as(p_xy)
        nz = t != 0
        s_xy = (p_xy[nz] * torch.log(p_y[nz] / p_xy[nz])).sum()
        return (s_x - s_xy) / s_x
    if r == 0:
        return nan
    df = (r - 1) * (c - 1)
    correct = bias_correction and kind != PEARSON
    expected = torch.outer(t.sum(1), t.sum(0)) / n
    if df == 0:
        chi = torch.zeros((), dtype=dtype)
    else:
        if df == 1 and correct:
            t = t + 0.5 * torch.sign(expected - t)
        chi = ((t - expected) ** 2 / expected).sum()
    phi = chi / n
    if kind == PEARSON:
        return torch.sqrt(phi / (1 + phi)).clamp(0.0, 1.0)
    if correct:
        phi = torch.clamp(phi - df / (n - 1), min=0.0)
        rc = r - (r - 1) ** 2 / (n - 1)
        cc = c - (c - 1) ** 2 / (n - 1)
        if torch.minimum(rc, cc) == 1:
            return nan
        rm, cm = rc - 1, cc - 1
    else:
        rm, cm = torch.tensor(r - 1, dtype=dtype), torch.tensor(c - 1, dtype=dtype)
    value = torch.sqrt(phi / torch.minimum(rm, cm)) if kind == CRAMERS else torch.sqrt(phi / torch.sqrt(rm * cm))
    return value.clamp(0.0, 1.0)


def scores(tabs, kind: int, bias_correction: bool = False, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """``score`` of every table of ``[P, k, k]``: ``[P]`` of ``dtype``."""
    return torch.stack([score(t, kind, bias_correction, dtype) for t in np.asarray(tabs)])


def pair_score(preds, target, kind: int, bias_correction: bool = False, nan_strategy: str = "replace", nan_replace: Optional[float] = 0.0,
               dtype: torch.dtype = torch.float64) -> torch.Tensor:
    p, t = labels(preds, nan_strategy, nan_replace), labels(target, nan_strategy, nan_replace)
    k = int(max(p.max(initial=0), t.max(initial=0))) + 1
    return score(table(p, t, k), kind, bias_correction, dtype)


def pair_matrix(matrix, kind: int, bias_correction: bool = False, nan_strategy: str = "replace", nan_replace: Optional[float] = 0.0,
                dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """The ``[V, V]`` matrix of all column pairs, diagonal 1: ``out[i, j]`` scores ``(preds=col_i, target=col_j)``.  The symmetric kinds are
    evaluated once per pair (``i < j``) and mirrored; Theil's U is evaluated for both orders."""
    lab = labels(matrix, nan_strategy, nan_replace)
    v = lab.shape[1]
    k = int(lab.max(initial=0)) + 1
    out = torch.ones(v, v, dtype=dtype)
    for i in range(v):
        for j in range(i + 1, v):
            tab = table(lab[:, i], lab[:, j], k)
            out[i, j] = score(tab, kind, bias_correction, dtype)
            out[j, i] = score(tab.T, kind, bias_correction, dtype) if kind == THEILS else out[i, j]
    return out


def any_unable(matrix, nan_strategy: str = "replace", nan_replace: Optional[float] = 0.0) -> bool:
    lab = labels(matrix, nan_strategy, nan_replace)
    v = lab.shape[1]
    k = int(lab.max(initial=0)) + 1
    return any(unable(table(lab[:, i], lab[:, j], k)) for i in range(v) for j in range(i + 1, v))


def upper(m: torch.Tensor) -> torch.Tensor:
    """The entries above the diagonal as one vector (the comparison vector of the value rule)."""
    i, j = torch.triu_indices(m.shape[0], m.shape[1], 1)
    return m[i, j]


def off_diagonal(m: torch.Tensor) -> torch.Tensor:
    v = m.shape[0]
    return m[~torch.eye(v, dtype=torch.bool)]
