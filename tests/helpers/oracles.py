"""Independent statements of the small native ops, written from each operation's definition in exact integer or fp64
arithmetic.  Nothing here calls this library's implementation of the same operation: the GPU tests compare the HIP
kernels with these, and tests/unittests/misc/test_oracles.py checks each of them against the library's CPU path."""
import functools
import math
from typing import List, Optional, Sequence

import numpy as np
import torch

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
