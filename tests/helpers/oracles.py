"""Independent statements of the small native ops, written from each operation's definition in exact integer or fp64
arithmetic.  Nothing here calls this library's implementation of the same operation: the GPU tests compare the HIP
kernels with these, and tests/unittests/misc/test_oracles.py checks each of them against the library's CPU path."""
import functools
import math
from typing import List, Optional, Sequence

import numpy as np
import torch

# ------------------------------------------------------------------------------------------- regression

REG_NONE, REG_APE, REG_SAPE, REG_SLE, REG_LOGCOSH, REG_MINKOWSKI, REG_ABS_T, REG_TWEEDIE = range(8)
REG_EPS = 1.17e-06
_U64 = 2.0 ** -53


def reg_unit_roundoff(dtype: torch.dtype) -> float:
    """Unit roundoff of the type the elementwise math runs in: fp32 for inputs of up to 32 bits, fp64 for fp64."""
    return _U64 if dtype == torch.float64 else 2.0 ** -24


def _reg_op_formula(op: int, p: torch.Tensor, t: torch.Tensor, param: float) -> torch.Tensor:
    """Channel 7's elementwise error, from its definition, in the dtype of ``p`` / ``t``:
    APE |p−t| / max(|t|, eps);  SAPE 2 |p−t| / max(|t|+|p|, eps);  SLE (log1p p − log1p t)²;
    log-cosh log((e^d + e^−d) / 2), d = p − t;  Minkowski |p−t|^param;  |t|;
    Tweedie deviance of power ``param``: 0 → (t−p)²;  1 → 2 (t·log(t/p) + p − t) with 0·log 0 = 0;
    2 → 2 (log(p/t) + t/p − 1);  else 2 (max(t,0)^(2−a) / ((1−a)(2−a)) − t·p^(1−a) / (1−a) + p^(2−a) / (2−a))."""
    d = p - t
    if op == REG_NONE:
        return torch.zeros_like(p)
    if op == REG_APE:
        return d.abs() / torch.clamp(t.abs(), min=REG_EPS)
    if op == REG_SAPE:
        return 2 * (d.abs() / torch.clamp(t.abs() + p.abs(), min=REG_EPS))
    if op == REG_SLE:
        e = torch.log1p(p) - torch.log1p(t)
        return e * e
    if op == REG_LOGCOSH:
        return torch.log((torch.exp(d) + torch.exp(-d)) / 2)
    if op == REG_MINKOWSKI:
        return d.abs() ** param
    if op == REG_ABS_T:
        return t.abs()
    if op != REG_TWEEDIE:
        raise ValueError(f"unknown op {op}")
    a = float(param)
    if a == 0:
        return (t - p) * (t - p)
    if a == 1:
        tlog = torch.where(t == 0, torch.zeros_like(t), t * torch.log(t / p))
        return 2 * (tlog + p - t)
    if a == 2:
        return 2 * (torch.log(p / t) + t / p - 1)
    term1 = torch.clamp(t, min=0) ** (2 - a) / ((1 - a) * (2 - a))
    term2 = t * p ** (1 - a) / (1 - a)
    term3 = p ** (2 - a) / (2 - a)
    return 2 * (term1 - term2 + term3)


def regression_table_exact(p: torch.Tensor, t: torch.Tensor, op: int = REG_NONE, param: float = 0.0):
    """``(table, budget)``, both fp64 ``[8, D]``, of the sums (Σp, Σt, Σp², Σt², Σpt, Σ(p−t)², Σ|p−t|, Σ op(p, t)) over
    the rows of ``p`` / ``t`` ``[N, D]``, from the values as stored upcast to fp64, and what a correct one-pass
    implementation may differ from them by.

    Budgets (N rows, u = unit roundoff of the compute type, fp64 accumulation in any order):
      ch 0, 1     (N+2)·2⁻⁵³·Σ|x|: N−1 fp64 additions, each off by at most 2⁻⁵³ of a partial sum ≤ Σ|x|;
      ch 2, 3, 4  (N+2)·2⁻⁵³·Σ|x·y|: the same, the products of two values of ≤ 24 bits being exact in fp64 (and the
                  one rounding of an fp64 product taking one of the two spare units);
      ch 5        (4u + N·2⁻⁵³)·Σd²: d and d·d are each rounded once in the compute type, (1+u)³ − 1 < 4u;
      ch 6        (u + N·2⁻⁵³)·Σ|d|;
      ch 7        4·Σ|eager − exact| + (4u + N·2⁻⁵³)·Σ|exact|, where ``eager`` is the same formula evaluated by the CPU
                  in the compute type: the formula's own rounding (cancellation included) with a 4x margin, over a
                  floor of 4u for a device libm that is good to 2 ulp."""
    dt = torch.promote_types(p.dtype, t.dtype)
    u = reg_unit_roundoff(dt)
    cdt = torch.float64 if dt == torch.float64 else torch.float32
    pc, tc = p.to(dt).to(cdt), t.to(dt).to(cdt)
    x, y = pc.double(), tc.double()
    n = x.shape[0]
    d = x - y
    exact7 = _reg_op_formula(op, x, y, param)
    eager7 = _reg_op_formula(op, pc, tc, param).double()
    chans = [x, y, x * x, y * y, x * y, d * d, d.abs(), exact7]
    table = torch.stack([_fsum_cols(c) for c in chans])
    mag = torch.stack([_fsum_cols(c.abs()) for c in chans])
    nu = n * _U64
    budget = torch.empty_like(table)
    budget[:5] = (n + 2) * _U64 * mag[:5]
    budget[5] = (4 * u + nu) * mag[5]
    budget[6] = (u + nu) * mag[6]
    budget[7] = 4 * _fsum_cols((eager7 - exact7).abs()) + (4 * u + nu) * mag[7]
    return table, budget


def _fsum_cols(v: torch.Tensor) -> torch.Tensor:
    """Column sums of an fp64 ``[N, D]`` tensor: correctly rounded (``math.fsum``) up to 4096 elements; beyond, summed
    row by row in the 64-bit significand of ``numpy.longdouble`` (error ≤ N·2⁻⁶⁴·Σ|v|, 2⁻¹¹ of the budgets above), which
    keeps the cost of the oracle in numpy."""
    a = v.numpy()
    if a.size <= 4096 or np.finfo(np.longdouble).eps > 2.0 ** -60:
        return torch.tensor([math.fsum(a[:, c]) for c in range(a.shape[1])], dtype=torch.float64)
    return torch.from_numpy(np.sum(a.astype(np.longdouble), axis=0).astype(np.float64))


def pearson_states_exact(batches: Sequence, state_dtype: torch.dtype = torch.float64):
    """``(states, budget)`` of the streaming Pearson states after the ``(p, t)`` ``[N_b, D]`` batches: every batch's
    centred two-pass moments in fp64, merged with Chan's formula in fp64.  ``states`` maps mean_x, mean_y, var_x, var_y,
    corr_xy, n_total to fp64 ``[D]``; ``budget`` maps var_x, var_y, corr_xy to what an implementation that reads fp64
    raw moments Σx, Σy, Σx², Σy², Σxy of each batch, merges in fp64 and stores the states in ``state_dtype`` may be off by:

      every batch     4(N_b+2)·2⁻⁵³·Σ_b|x·y|: centring the raw moments, s2 − s0·s0/N.  s2 carries (N+2)·2⁻⁵³·Σx²
                      (``regression_table_exact``), s0·s0/N twice the relative error of s0 on a value ≤ Σx²
                      (Cauchy-Schwarz), and one more unit covers the roundings of the expression itself;
      fp32 states     w_b(2|dx_b|ε_b + ε_b²) + 2⁻²³·|state| per batch, w_b = n0·N_b/(n0+N_b), dx_b = batch mean − prior
                      mean: the merge term w·dx² sees the stored prior mean, which is off by ε_b; ε grows by 2⁻²⁴·|mean|
                      with every stored update and shrinks by n0/n in the merge; storing the state rounds it by
                      2⁻²⁴·|state|, taken twice.  (For corr_xy: w_b(|dx|ε_y + |dy|ε_x + ε_x·ε_y).)
    ``budget`` also holds ε of the stored means after the last batch as mean_x, mean_y.  An empty batch changes nothing."""
    d_cols = batches[0][0].shape[1]
    z = lambda: torch.zeros(d_cols, dtype=torch.float64)  # noqa: E731
    mx, my, vx, vy, cxy, n0 = z(), z(), z(), z(), z(), 0.0
    bud = {"var_x": z(), "var_y": z(), "corr_xy": z()}
    ex, ey = z(), z()
    fp32 = state_dtype == torch.float32
    u_state = 2.0 ** -24 if fp32 else _U64
    for p, t in batches:
        nb = p.shape[0]
        if nb == 0:
            continue
        x, y = p.double(), t.double()
        mxb, myb = _fsum_cols(x) / nb, _fsum_cols(y) / nb
        xc, yc = x - mxb, y - myb
        # corrected two-pass: the second term removes what the rounding of the batch mean leaves behind
        sxc, syc = _fsum_cols(xc), _fsum_cols(yc)
        m2x = _fsum_cols(xc * xc) - sxc ** 2 / nb
        m2y = _fsum_cols(yc * yc) - syc ** 2 / nb
        cb = _fsum_cols(xc * yc) - sxc * syc / nb
        n = n0 + nb
        dx, dy = mxb - mx, myb - my
        w = n0 * nb / n
        vx = vx + m2x + w * dx * dx
        vy = vy + m2y + w * dy * dy
        cxy = cxy + cb + w * dx * dy
        mx = mx + dx * (nb / n)
        my = my + dy * (nb / n)
        raw = 4 * (nb + 2) * _U64
        bud["var_x"] += raw * _fsum_cols(x * x)
        bud["var_y"] += raw * _fsum_cols(y * y)
        bud["corr_xy"] += raw * _fsum_cols((x * y).abs())
        if fp32:
            bud["var_x"] += w * (2 * dx.abs() * ex + ex * ex) + 2.0 ** -23 * vx.abs()
            bud["var_y"] += w * (2 * dy.abs() * ey + ey * ey) + 2.0 ** -23 * vy.abs()
            bud["corr_xy"] += w * (dx.abs() * ey + dy.abs() * ex + ex * ey) + 2.0 ** -23 * cxy.abs()
        ex = ex * (n0 / n) + u_state * mx.abs()
        ey = ey * (n0 / n) + u_state * my.abs()
        n0 = n
    bud["mean_x"], bud["mean_y"] = ex, ey
    states = {"mean_x": mx, "mean_y": my, "var_x": vx, "var_y": vy, "corr_xy": cxy,
              "n_total": torch.full((d_cols,), n0, dtype=torch.float64)}
    return states, bud


def pearson_from_states(st) -> torch.Tensor:
    """Pearson's r ``corr_xy / sqrt(var_x · var_y)`` (the 1/(n−1) factors cancel) in fp64."""
    return st["corr_xy"] / torch.sqrt(st["var_x"] * st["var_y"])


def concordance_from_states(st) -> torch.Tensor:
    """Lin's concordance ``2 s_xy / (s_x² + s_y² + (mean_x − mean_y)²)`` with the 1/(n−1) sample moments, in fp64."""
    n1 = st["n_total"] - 1
    return 2 * st["corr_xy"] / n1 / (st["var_x"] / n1 + st["var_y"] / n1 + (st["mean_x"] - st["mean_y"]) ** 2)


def concordance_mean_slack(st, bud) -> torch.Tensor:
    """What the rounding of the stored means may move the concordance coefficient by, relative to it: the means enter
    through (mean_x − mean_y)² in the denominator, so (2|δ|ε + ε²) / denominator with δ = mean_x − mean_y and
    ε = ε_x + ε_y.  It matters for a small batch with fp32 states, where the moment budgets are a few 2⁻²⁴."""
    n1 = st["n_total"] - 1
    delta, e = (st["mean_x"] - st["mean_y"]).abs(), bud["mean_x"] + bud["mean_y"]
    return (2 * delta * e + e * e) / (st["var_x"] / n1 + st["var_y"] / n1 + delta * delta)


def relative_state_budget(st, bud) -> float:
    """Largest budget / |state| over var_x, var_y, corr_xy and the columns."""
    return max(float((bud[k] / st[k].abs()).max()) for k in ("var_x", "var_y", "corr_xy"))


def offset_batches(sizes: Sequence[int], d_cols: int, mean: float, std: float, dtype: torch.dtype = torch.float32, seed: int = 0,
                   rho: float = 0.5):
    """Batches ``(p, t)`` ``[N_b, D]`` of data that sits far from zero: both around ``mean`` with spread ``std`` and
    correlation ``rho``; the columns differ a little in spread so that a column mix-up shows."""
    g = torch.Generator().manual_seed(seed)
    scale = std * (1 + torch.arange(d_cols, dtype=torch.float64) / 8)
    out = []
    for nb in sizes:
        z1 = torch.randn(nb, d_cols, generator=g, dtype=torch.float64)
        z2 = torch.randn(nb, d_cols, generator=g, dtype=torch.float64)
        p = mean + scale * z1
        t = mean + scale * (rho * z1 + math.sqrt(1 - rho * rho) * z2)
        out.append((p.to(dtype), t.to(dtype)))
    return out


# ------------------------------------------------------------------------------------------------- text


def nll_fp64(logits: torch.Tensor, target: torch.Tensor, ignore_index: Optional[int] = None) -> torch.Tensor:
    """``logsumexp(x[r]) - x[r, t[r]]`` in fp64 on the (already quantised) logits ``[N, V]``; 0 for ignored rows,
    NaN for rows whose target is outside ``[0, V)``."""
    x = logits.double()
    n, v = x.shape
    t = target.long()
    ignored = torch.zeros(n, dtype=torch.bool) if ignore_index is None else t == ignore_index
    bad = ((t < 0) | (t >= v)) & ~ignored
    safe = torch.where(ignored | bad, torch.zeros_like(t), t)
    out = torch.logsumexp(x, dim=1) - x.gather(1, safe.view(-1, 1)).squeeze(1)
    out = torch.where(bad, torch.full_like(out, float("nan")), out)
    return torch.where(ignored, torch.zeros_like(out), out)


def greedy_match_fp64(p: torch.Tensor, r: torch.Tensor):
    """Row and column maxima of ``P_b R_b^T`` in fp64 (NaN propagates as in ``torch.max``)."""
    sim = torch.bmm(p.double(), r.double().transpose(1, 2))
    return sim.max(2).values, sim.max(1).values


# ------------------------------------------------------------------------------------------- clustering


def _product(vals: List[int]) -> int:
    while len(vals) > 1:  # balanced tree: the big multiplications are few and between equal sizes
        vals = [vals[i] * vals[i + 1] if i + 1 < len(vals) else vals[i] for i in range(0, len(vals), 2)]
    return vals[0] if vals else 1


@functools.lru_cache(maxsize=64)
def comb_exact(n: int, k: int) -> int:
    """``math.comb(n, k)``; above a few thousand it is assembled from its prime factorisation (Legendre: the exponent
    of p in m! is sum_i floor(m / p^i)), which takes milliseconds where the running product takes seconds."""
    if k < 0 or k > n:
        return 0
    if n < 4096:
        return math.comb(n, k)
    sieve = bytearray([1]) * (n + 1)
    sieve[0:2] = b"\0\0"
    for p in range(2, int(n ** 0.5) + 1):
        if sieve[p]:
            sieve[p * p::p] = bytes(len(range(p * p, n + 1, p)))
    factors = []
    for p in range(2, n + 1):
        if sieve[p]:
            e, q = 0, p
            while q <= n:
                e += n // q - k // q - (n - k) // q
                q *= p
            if e:
                factors.append(p ** e)
    return _product(factors)


def emi_exact(a: Sequence[int], b: Sequence[int], N: int) -> float:
    """Expected mutual information of two clusterings with marginals ``a`` / ``b`` over ``N`` samples:
    sum over i, j, n in [max(1, a_i + b_j - N), min(a_i, b_j)] of
    ``n / N * log(N n / (a_i b_j)) * C(a_i, n) C(N - a_i, b_j - n) / C(N, b_j)``.
    The hypergeometric weight is one exact integer ratio rounded once to a float; along n its numerator is advanced
    by the exact recurrence ``C(a, n+1) C(N-a, b-n-1) = C(a, n) C(N-a, b-n) (a-n)(b-n) / ((n+1)(N-a-b+n+1))``
    (an integer at every step), which gives the same integers as two ``math.comb`` calls per term.
    Terms whose weight is below 2^-1200 are left out without being formed: they round to 0.0 (the smallest double is
    2^-1074) and the lgamma estimate that finds them is good to a fraction of a bit, so the sum is unchanged; this only
    keeps a range of 10^5 values of n (numbers of 10^5 bits) affordable."""
    N = int(N)
    lg = math.lgamma
    terms: List[float] = []
    for ai in (int(v) for v in a):
        for bj in (int(v) for v in b):
            lo, hi = max(1, ai + bj - N), min(ai, bj)
            if lo > hi:
                continue

            def log2_weight(n: int) -> float:
                return (lg(ai + 1) - lg(n + 1) - lg(ai - n + 1) + lg(N - ai + 1) - lg(bj - n + 1) - lg(N - ai - bj + n + 1)
                        - lg(N + 1) + lg(bj + 1) + lg(N - bj + 1)) / math.log(2.0)

            while lo <= hi and log2_weight(lo) < -1200.0:  # the weights are unimodal in n: trim both tails
                lo += 1
            while hi >= lo and log2_weight(hi) < -1200.0:
                hi -= 1
            if lo > hi:
                continue
            den = comb_exact(N, bj)
            num = comb_exact(ai, lo) * comb_exact(N - ai, bj - lo)
            for n in range(lo, hi + 1):
                w = num / den  # correctly rounded big-integer division
                if w != 0.0:
                    terms.append(n / N * math.log(N * n / (ai * bj)) * w)
                if n < hi:
                    num = num * ((ai - n) * (bj - n)) // ((n + 1) * (N - ai - bj + n + 1))
    return math.fsum(terms)


# -------------------------------------------------------------------------------------------- retrieval


def retrieval_stats_fp64(scores_sorted, target, k: Optional[int], adaptive: bool = False) -> List[float]:
    """The ten per-query columns of ``tmx::retrieval_segments`` for ONE query whose documents are already ordered by
    descending score: (rel_total, neg_total, rel_in_k, neg_in_k, ap_sum, first_rel or -1, rel_in_R, dcg, idcg, k).
    Relevant means target > 0.  ``ap_sum`` is the sum over relevant documents in the top k of (relevant so far) / rank.
    DCG is tie averaged: the documents of a run of equal scores share equally the discounts ``1 / log2(pos + 2)`` of
    the positions the run covers inside the top k.  The ideal DCG takes the targets in descending order."""
    s = np.asarray(scores_sorted, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    n = len(s)
    kq = n if k is None else (min(int(k), n) if adaptive else int(k))
    kk = min(kq, n)
    rel = t > 0
    rel_total = int(rel.sum())
    rel_k = neg_k = rel_r = 0
    first = -1
    ap = 0.0
    seen = 0
    for i in range(n):
        if rel[i]:
            seen += 1
        if i < kq:
            if rel[i]:
                rel_k += 1
                ap += seen / (i + 1)
                if first < 0:
                    first = i
            else:
                neg_k += 1
        if i < rel_total and rel[i]:
            rel_r += 1
    disc = [1.0 / math.log2(pos + 2.0) for pos in range(n)]
    dcg = 0.0
    i = 0
    while i < n:
        e = i + 1
        while e < n and s[e] == s[i]:
            e += 1
        share = math.fsum(disc[i:min(e, kk)]) / (e - i) if i < kk else 0.0
        dcg += float(t[i:e].sum()) * share
        i = e
    ideal = np.sort(t)[::-1]
    idcg = math.fsum(float(ideal[pos]) * disc[pos] for pos in range(kk))
    return [float(rel_total), float(n - rel_total), float(rel_k), float(neg_k), ap, float(first), float(rel_r), dcg, idcg,
            float(kq)]


# ----------------------------------------------------------------------------------------------- interp


def macro_interp_fp64(x, xps: Sequence, fps: Sequence) -> np.ndarray:
    """Sum over the classes of the piecewise-linear interpolation of ``(xps[c], fps[c])`` at ``x`` in fp64: segment
    ``j = #(xp <= x) - 1`` clamped to ``[0, L - 2]`` (so queries outside the range extrapolate the end segments), a zero
    denominator counts as 1, a class of length 1 adds ``fp[0]`` and an empty class adds nothing."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    for xp, fp in zip(xps, fps):
        xp, fp = np.asarray(xp, dtype=np.float64), np.asarray(fp, dtype=np.float64)
        if len(xp) == 0:
            continue
        if len(xp) == 1:
            out += fp[0]
            continue
        j = np.clip(np.searchsorted(np.sort(xp), x, "right") - 1, 0, len(xp) - 2)
        dx = xp[j + 1] - xp[j]
        dx = np.where(dx == 0, 1.0, dx)
        slope = (fp[j + 1] - fp[j]) / dx
        out += slope * x + (fp[j] - slope * xp[j])
    return out


# -------------------------------------------------------------------------------------------------- RLE


def coco_counts_string(runs: Sequence[int]) -> bytes:
    """COCO's ``rleToString``: run i > 2 is stored as its difference to run i - 2; every value goes out in 5-bit groups,
    least significant first, each group + 48 with bit 0x20 set while more groups follow; the last group carries the
    sign in bit 0x10."""
    out = bytearray()
    for i, c in enumerate(runs):
        x = int(c) - (int(runs[i - 2]) if i > 2 else 0)
        while True:
            g = x & 0x1F
            x >>= 5
            done = (x == -1) if (g & 0x10) else (x == 0)
            out.append((g if done else g | 0x20) + 48)
            if done:
                break
    return bytes(out)


def mask_from_runs(runs: Sequence[int], H: int, W: int) -> np.ndarray:
    """``[H, W]`` uint8 mask whose column-major pixel sequence is ``runs[0]`` background pixels, ``runs[1]`` foreground
    pixels, ... (COCO's run order; the runs must add up to ``H * W``)."""
    assert sum(int(c) for c in runs) == H * W, "runs must cover the mask"
    flat = np.repeat(np.arange(len(runs)) & 1, np.asarray(runs, dtype=np.int64)).astype(np.uint8)
    return np.ascontiguousarray(flat.reshape(W, H).T)
