"""Independent oracles of the register-resident row kernels (csrc/rowwise.hip) and the rank kernels (csrc/rank.hip).

Plain torch-on-CPU / numpy / Python loops; imports nothing from the package under test.  Every oracle takes the *stored*
inputs, i.e. scores already rounded to the kernel's input dtype, and widens them exactly (every bf16 / fp16 / fp32 value is
an fp64 value).

Notation of the bounds: ``u`` is the unit roundoff of the input dtype (``finfo(dtype).eps / 2``), ``u32 = 2^-24``.  The
kernels compute in fp32 and round an intermediate to the input dtype wherever the reference's tensor expression stores one;
such a step is one fp32 operation followed by one rounding, ``ur = u + u32`` for the 16-bit types and ``u32`` for fp32.
Compounded roundings are covered by ``g(x) = x / (1 - 4 x)`` (at most four (1 + delta) factors meet in any term below).
"""
import math
from typing import List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

U32 = 2.0**-24


def unit_roundoff(dtype: torch.dtype) -> float:
    return float(torch.finfo(dtype).eps) / 2


def _ur(dtype: torch.dtype) -> float:
    """One fp32 operation stored in ``dtype``, compounded up to four times."""
    x = U32 if dtype in (torch.float32, torch.float64) else unit_roundoff(dtype) + U32
    return x / (1 - 4 * x)


def _sub(dtype: torch.dtype) -> float:
    """Half the spacing of the subnormals of ``dtype``: the absolute error of a rounding that underflows."""
    fi = torch.finfo(dtype)
    return float(fi.tiny) * float(fi.eps) / 2


# ------------------------------------------------------------------------------------------------------ top-k stats
def topk_order(scores: Tensor) -> List[List[int]]:
    """Per row, the class indices in the kernel's stated order: NaN first (by index), then value descending, index
    ascending among equals.  A Python sort on the key ``(not isnan, -value, index)``; a NaN's ``-value`` is replaced by 0
    so that the key is totally ordered."""
    out = []
    for row in scores.detach().cpu().double().tolist():
        out.append(sorted(range(len(row)), key=lambda i, row=row: (True, -row[i], i) if row[i] == row[i] else (False, 0.0, i)))
    return out


def topk_stats_oracle(
    scores: Optional[Tensor],
    target: Tensor,
    C: int,
    k: int,
    ignore_index: Optional[int],
    X: int,
    samplewise: bool,
    labels: Optional[Tensor] = None,
    order: Optional[List[List[int]]] = None,
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """int64 ``tp, fp, tn, fn`` (``[C]``, or ``[M / X, C]`` samplewise: rows ``s X .. (s + 1) X - 1`` form sample ``s``)
    of the top-``k`` picks of ``scores`` ``[M, C]`` against ``target`` ``[M]``, and a bool ``[M]`` flag per row.

    A row whose target equals ``ignore_index`` or lies outside ``[0, C)`` counts nowhere.  For every other row the picked
    classes are the first ``k`` of :func:`topk_order`; class ``c`` counts tp (picked and target), fp (picked, not target),
    fn (target, not picked) or tn (neither).  With ``labels`` ``[M]`` (``k == 1``) the single pick is the label; a label
    outside ``[0, C)`` picks nothing.  ``order`` may carry a precomputed :func:`topk_order` of the same scores.

    The flag is set where the k-th and (k+1)-th entries of the order compare equal or are both NaN: only there does the
    order *inside* a tie decide the result, so only there may another correct top-k (``torch.topk`` leaves its tie
    order unspecified) differ from the kernel's contract."""
    t = target.detach().cpu().reshape(-1).tolist()
    M = len(t)
    assert M % X == 0
    S = M // X if samplewise else 1
    out = np.zeros((4, S, C), dtype=np.int64)
    flag = np.zeros(M, dtype=bool)
    rows = None
    if labels is None:
        assert scores is not None and tuple(scores.shape) == (M, C) and 1 <= k <= C
        rows = scores.detach().cpu().double().numpy()
        order = topk_order(scores) if order is None else order
    else:
        assert k == 1
        lab = labels.detach().cpu().reshape(-1).tolist()
    for r in range(M):
        if labels is None and k < C:
            a, b = rows[r, order[r][k - 1]], rows[r, order[r][k]]
            flag[r] = bool(a == b or (a != a and b != b))
        if (ignore_index is not None and t[r] == ignore_index) or not 0 <= t[r] < C:
            continue
        picked = np.zeros(C, dtype=bool)
        if labels is None:
            picked[order[r][:k]] = True
        elif 0 <= lab[r] < C:
            picked[lab[r]] = True
        is_t = np.zeros(C, dtype=bool)
        is_t[t[r]] = True
        s = r // X if samplewise else 0
        out[0, s] += picked & is_t
        out[1, s] += picked & ~is_t
        out[2, s] += ~picked & ~is_t
        out[3, s] += ~picked & is_t
    res = [torch.from_numpy(out[i] if samplewise else out[i, 0]) for i in range(4)]
    return res[0], res[1], res[2], res[3], torch.from_numpy(flag)


# ------------------------------------------------------------------------------------------------------------ hinge
def hinge_oracle(preds: Tensor, target: Tensor, squared: bool, one_vs_all: bool, softmax: Optional[bool] = None) -> Tuple[Tensor, Tensor]:
    """fp64 sums over the rows of the multiclass hinge measures, ``[]`` (crammer-singer) or ``[C]`` (one-vs-all), and a
    bound of the same shape on ``|kernel - oracle|``.  NaN / inf sums carry no bound; compare them as classes.

    ``softmax=None`` applies the reference's rule: the rows go through a softmax iff any value of the batch is outside
    [0, 1] or is NaN.  Measures: crammer-singer ``max(0, 1 - (p_t - max_{c != t} p_c))`` (0 when there is no other
    class: the maximum of nothing is -inf); one-vs-all, per class, ``max(0, 1 - p_c)`` for the target and
    ``max(0, 1 + p_c)`` otherwise; squared afterwards when asked.

    Bound, first order terms with the compounding constant of the module docstring (``ur``).  N rows, C classes.

    * Probabilities.  Without softmax the kernel reads p exactly: ``dp_c = 0``.  With softmax it evaluates
      ``e_c = expf(x_c - m)`` (m the exact row maximum), ``s = sum e_c``, ``p_c = store(e_c / s)``.  The subtraction rounds
      once (relative error of ``e_c``: ``|x_c - m| u32``), expf is allowed 2 ulp (4 u32; HIP documents 1), so the sum
      inherits at most the p-weighted mean of those, ``(4 + sum_c p_c (m - x_c)) u32 <= (4 + ln C) u32`` (the mean is the
      entropy minus ``ln s``, ``s >= 1``), a C-term fp32 sum in any order adds ``(C - 1) u32``, the divide ``u32``.  With
      ``p_c (m - x_c) <= 1 / e`` that is ``p_c (C + ln C + 8) u32 + u32 / e``, rounded up to
      ``dp_c = p_c (C + ln C + 10) u32 + u32 / 2``, plus the store ``ur p_c`` and its underflow.
    * crammer-singer: ``d = store(p_t - mo)`` errs by ``E_d = dp_t + max_c dp_c + ur |d|`` (a maximum moves by at most
      the largest move of its arguments), ``a = store(1 - d)`` by ``E_a = E_d + ur (|1 - d| + E_d)``; the clamp is
      1-Lipschitz.  one-vs-all: ``E_a = dp_c + ur (|1 -+ p_c| + dp_c)`` (the negation is exact).
    * squared: ``store(a^2)`` errs by ``E_a (2 a + E_a) + ur (a + E_a)^2``.
    * every store may underflow: ``+ tiny * eps / 2`` of the dtype each (three at most).
    * the N measures are summed in fp32 in an order that is no contract: ``(N - 1) u32 sum_r (m_r + E_r)``.
    """
    dtype = preds.dtype
    x = preds.detach().cpu().double()
    t = target.detach().cpu().reshape(-1).long()
    N, C = x.shape
    if softmax is None:
        softmax = bool((~((x >= 0) & (x <= 1))).any())
    ur, sub = _ur(dtype), 3 * _sub(dtype)
    if softmax:
        p = torch.softmax(x, dim=1)
        dp = p * ((C + math.log(C) + 10) * U32 + ur) + U32 / 2 + _sub(dtype)
    else:
        p, dp = x, torch.zeros_like(x)
    onehot = torch.zeros(N, C, dtype=torch.bool)
    onehot[torch.arange(N), t] = True
    if one_vs_all:
        a = 1 - torch.where(onehot, p, -p)
        e_a = dp + ur * (a.abs() + dp)
    else:
        pt = p[onehot]
        if C == 1:  # no other class: 1 - (p_t + inf) clamps to exactly 0 in any arithmetic (NaN p_t aside)
            zero = torch.where(torch.isnan(pt), pt, torch.zeros_like(pt))
            return zero.sum(), torch.zeros((), dtype=torch.float64)
        mo = p.masked_fill(onehot, -math.inf).max(dim=1).values
        d = pt - mo
        e_d = dp[onehot] + dp.max(dim=1).values + ur * d.abs()
        a = 1 - d
        e_a = e_d + ur * (a.abs() + e_d)
    m = torch.where(torch.isnan(a), a, a.clamp(min=0))
    if squared:
        e_a = e_a * (2 * m + e_a) + ur * (m + e_a) ** 2
        m = m * m
    e = e_a + sub
    total, bound = m.sum(0), e.sum(0) + (N - 1) * U32 * (m + e).sum(0)
    return total, bound


# ---------------------------------------------------------------------------------------------- multilabel ranking
def coverage_oracle(preds: Tensor, target: Tensor) -> Tensor:
    """Per-row coverage counts (fp32 ``[N]``), the reference's arithmetic step by step, so the comparison is exact.

    ``shift = |min(batch)| + 10`` evaluated in the input dtype (NaN when any score is NaN: ``min`` propagates it);
    ``mod = v`` on relevant labels, ``store(v + shift)`` elsewhere, one IEEE fp32 add and one rounding to the dtype, which
    is what torch does for a 16-bit add and what the kernel does; a NaN-propagating row minimum; the count of
    ``v >= min`` (no score compares ``>=`` a NaN, so such a row counts 0)."""
    v = preds.detach().cpu()
    rel = target.detach().cpu() == 1
    shift = v.min().abs() + 10  # a 0-dim tensor of the input dtype
    mod = torch.where(rel, v.float(), (v.float() + shift.float()).to(v.dtype).float())
    row_min = torch.full((v.shape[0],), math.inf)
    for c in range(v.shape[1]):  # NaN-propagating fold, written out
        col = mod[:, c]
        row_min = torch.where(torch.isnan(row_min) | (row_min < col), row_min, col)
    return (v.float() >= row_min[:, None]).sum(1).float()


def _row_chunks(n: int, width: int):
    step = max(1, (1 << 23) // max(1, width * width))
    for s in range(0, n, step):
        yield slice(s, min(n, s + step))


def lrap_oracle(preds: Tensor, target: Tensor, strict: bool = False, drop_one_relevant: bool = False) -> Tuple[Tensor, Tensor]:
    """Per-row label-ranking average precision in fp64 and its bound, from the definition: the mean over the relevant
    labels j of ``#{relevant i : p_i >= p_j} / #{i : p_i >= p_j}``; 1 for a row with no or only relevant labels.

    Bound: the counts are exact integers below 2^24, so each of the ``n`` fp32 quotients (each <= 1) errs by ``u32`` times
    itself (IEEE divide), their serial fp32 sum S by ``(n - 1) u32 S``, the final divide by ``u32 S / n``: in all
    ``(n + 1) u32`` times the row's value, taken with the compounding constant ``g``.

    ``strict`` / ``drop_one_relevant`` build the deliberately wrong variants of the discrimination test (``>`` for ``>=``;
    the first relevant label of every row treated as not relevant)."""
    v = preds.detach().cpu().double()
    rel = target.detach().cpu() == 1
    if drop_one_relevant:
        rel = rel.clone()
        first = rel.int().argmax(1)
        rel[torch.arange(rel.shape[0]), first] = False
    N, L = v.shape
    out = torch.ones(N, dtype=torch.float64)
    n = rel.sum(1)
    for sl in _row_chunks(N, L):
        ge = (v[sl, :, None] > v[sl, None, :]) if strict else (v[sl, :, None] >= v[sl, None, :])  # [n, i, j]
        all_rank = ge.sum(1)
        rel_rank = (ge & rel[sl, :, None]).sum(1)
        ratio = torch.where(rel[sl], rel_rank.double() / all_rank.double().clamp(min=1), torch.zeros((), dtype=torch.float64))
        out[sl] = ratio.sum(1) / n[sl].clamp(min=1)
    out = torch.where((n == 0) | (n == L), torch.ones_like(out), out)
    g = U32 / (1 - 4 * U32)
    return out, (n + 1).double() * g * out


def ranking_loss_oracle(preds: Tensor, target: Tensor, drop_one_relevant: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """Per-row ranking loss in fp64, its bound, and the bool "row is not degenerate".

    With n relevant labels of L: ``(sum_{j relevant} #{i : p_i > p_j or (p_i == p_j and i >= j)} - n (n + 1) / 2) /
    (n (L - n))`` in exact integers, one fp64 divide; 0 for a row with no or only relevant labels.  The kernel's
    numerator and denominator are integers below 2^24, exact in fp32, so its one IEEE divide errs by ``u32`` times the
    value."""
    v = preds.detach().cpu().double()
    rel = target.detach().cpu() == 1
    if drop_one_relevant:
        rel = rel.clone()
        first = rel.int().argmax(1)
        rel[torch.arange(rel.shape[0]), first] = False
    N, L = v.shape
    n = rel.sum(1)
    tot = torch.zeros(N, dtype=torch.int64)
    idx = torch.arange(L)
    for sl in _row_chunks(N, L):
        a, b = v[sl, :, None], v[sl, None, :]  # a: p_i, b: p_j
        cnt = ((a > b) | ((a == b) & (idx[:, None] >= idx[None, :]))).sum(1)  # [n, j]
        tot[sl] = (cnt * rel[sl]).sum(1)
    valid = (n > 0) & (n < L)
    num = 2 * tot - n * (n + 1)  # twice the numerator, an exact integer
    den = (2 * n * (L - n)).clamp(min=1)
    out = torch.where(valid, num.double() / den.double(), torch.zeros((), dtype=torch.float64))
    return out, U32 / (1 - 4 * U32) * out.abs(), valid


# ------------------------------------------------------------------------------------------------------------ ranks
def average_ranks_oracle(x: Tensor) -> Tensor:
    """Tie-averaged 1-based ranks of every row of ``x`` (``[n]`` or ``[D, n]``), O(n^2) with IEEE comparisons:
    ``#less + (#equal + 1) / 2`` (a half-integer, exact in fp32 below 2^23)."""
    a = x.detach().cpu().double().numpy()
    rows = a.reshape(1, -1) if a.ndim == 1 else a
    out = np.empty_like(rows)
    for d, row in enumerate(rows):
        less = (row[None, :] < row[:, None]).sum(1)
        equal = (row[None, :] == row[:, None]).sum(1)
        out[d] = less + (equal + 1) / 2
    return torch.from_numpy(out.reshape(a.shape)).to(x.dtype)


def inversions_oracle(y: Tensor) -> int:
    """``#{i < j : y_i > y_j}`` by brute force with IEEE comparisons (-0.0 == +0.0, +-inf ordered)."""
    a = y.detach().cpu().double().numpy()
    total = 0
    for i in range(len(a) - 1):
        total += int((a[i] > a[i + 1 :]).sum())
    return total
