"""Planted inputs for the row kernels of csrc/rowwise.hip, shared by the CPU test of the oracles and the GPU edge tests.

A row of width W sits in registers as ``c = lane + 64 j`` (64 lanes, slot j), so the interesting places are lane 0, lane 63,
the first lane of a middle slot and the last valid lane of the last slot.  Top-k rows are built in *rank space*: a
strictly descending ladder of representable values (consecutive bit patterns, so distinct in every dtype), ties planted on
chosen ranks, then scattered to classes by a permutation.  That keeps the k | k + 1 boundary free of accidental ties, which
16-bit random scores have all the time; only the handful of random rows and the rows that plant a boundary tie on purpose
are flagged by the oracle.
"""
import math
from typing import List, Optional, Tuple

import torch
from torch import Tensor

WIDTHS = [1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047, 2048]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TOPK_ROWS = 42  # 37 planted + 5 random; a multiple of X = 3 and no multiple of the 4 waves of a block
NAN, INF = math.nan, math.inf


def topk_ks(C: int) -> List[int]:
    return sorted({k for k in (1, 2, 5, 63, 64, 65, min(C, 130), C) if k <= C})


def slot_positions(W: int) -> List[int]:
    """Lane 0, lane 63, the first lane of a middle slot, the last valid lane of the last slot (clipped to the row)."""
    slots = (W + 63) // 64
    return [0, min(63, W - 1), min(W - 1, 64 * (slots // 2)), W - 1]


def ladder(dtype: torch.dtype, n: int) -> Tensor:
    """``n`` distinct finite values of ``dtype`` in (0, 1], strictly descending: the bit patterns below that of 1.0."""
    if dtype == torch.float32:
        return (0x3F800000 - torch.arange(n, dtype=torch.int32)).view(torch.float32)
    one = 0x3F80 if dtype == torch.bfloat16 else 0x3C00
    return (one - torch.arange(n, dtype=torch.int16)).view(dtype)


def _tied(vals: Tensor, lo: int, hi: int) -> Tensor:
    """``vals`` with ranks ``[lo, hi)`` (clipped) sharing one value."""
    lo, hi = max(0, lo), min(vals.numel(), hi)
    if hi - lo >= 2:
        vals = vals.clone()
        vals[lo:hi] = vals[lo]
    return vals


def topk_rows(C: int, k: int, dtype: torch.dtype, seed: int) -> Tuple[Tensor, Tensor]:
    """``scores [42, C]`` of ``dtype`` and ``target [42]`` for top-``k``: the planted rows of the module docstring."""
    g = torch.Generator().manual_seed(seed)
    rows, tgt = [], []
    lad = ladder(dtype, C)
    kk = min(k, C - 1)  # rank of the first entry not picked (the last entry when everything is picked)

    def scatter(vals: Tensor, perm: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        perm = torch.randperm(C, generator=g) if perm is None else perm
        row = torch.empty(C, dtype=dtype)
        row[perm] = vals
        return row, perm

    def perm_with(rank: int, cls: int) -> Tensor:
        """A random permutation rank -> class that sends ``rank`` to ``cls``."""
        perm = torch.randperm(C, generator=g)
        j = int((perm == cls).nonzero())
        perm[j], perm[rank] = perm[rank].clone(), perm[j].clone()
        return perm

    def add(row: Tensor, t: int) -> None:
        rows.append(row)
        tgt.append(int(t))

    for _ in range(3):  # the target is the last pick / the first entry not picked
        row, perm = scatter(lad)
        add(row, perm[k - 1])
        row, perm = scatter(lad)
        add(row, perm[kk])
    for pos in slot_positions(C):  # the same two, with the target in a chosen lane and slot
        add(scatter(lad, perm_with(k - 1, pos))[0], pos)
        add(scatter(lad, perm_with(kk, pos))[0], pos)
    row, perm = scatter(_tied(lad, k - 3, k))  # a tie group wholly inside the top k
    add(row, perm[k - 1])
    row, perm = scatter(_tied(lad, k, k + 3))  # wholly outside
    add(row, perm[kk])
    # straddling the boundary: ranks k-1 .. k+1 tie, one of them is picked, by contract the lowest class index
    row, perm = scatter(_tied(lad, k - 1, k + 2))
    group = perm[max(0, k - 1) : min(C, k + 2)]
    add(row, group.min())
    add(row.clone(), group.max())
    add(torch.full((C,), 0.5, dtype=dtype), k - 1)  # all equal: classes 0 .. k-1 are picked
    add(torch.full((C,), -INF, dtype=dtype), kk)  # all -inf: the same
    row, perm = scatter(lad)  # a +inf entry is the first pick
    row[perm[C - 1]] = INF
    add(row, perm[C - 1])
    row, perm = scatter(lad)  # one NaN: picked before +inf and every number
    row[perm[C - 1]] = NAN
    row[perm[0]] = INF
    add(row, perm[C - 1])
    # several NaNs, picked in index order; for small k one more than fits, so the index order decides (flagged)
    nn = min(C, k + 1) if k < 8 else min(C, 3)
    row, perm = scatter(lad)
    where = perm[C - nn :]
    row[where] = NAN
    add(row, where.max())
    row, perm = scatter(_tied(lad, 1, k) if k >= 3 else _tied(lad, k + 1, k + 4))  # a NaN together with ties
    row[perm[0]] = NAN
    add(row, perm[k - 1])
    while len(rows) < TOPK_ROWS - 5:  # plain ladder rows, the target on a random rank
        row, perm = scatter(lad)
        add(row, perm[int(torch.randint(0, C, (1,), generator=g))])
    for _ in range(5):  # random scores rounded to the dtype: natural ties in 16 bits
        add(torch.randn(C, generator=g).to(dtype), int(torch.randint(0, C, (1,), generator=g)))
    assert len(rows) == TOPK_ROWS
    return torch.stack(rows), torch.tensor(tgt, dtype=torch.long)


def topk_targets(target: Tensor, ignore_index: Optional[int]) -> Tensor:
    """The targets with ``ignore_index`` planted on one scattered row and on the whole last sample of three rows."""
    if ignore_index is None:
        return target
    t = target.clone()
    t[1] = ignore_index
    t[-3:] = ignore_index
    return t


def hinge_rows(C: int, dtype: torch.dtype, kind: str, seed: int) -> Tuple[Tensor, Tensor]:
    """``preds [N, C]`` of ``dtype`` and ``target [N]`` (N = 41) for the hinge kernel.

    ``kind``: "probs" values in [0, 1] (no softmax), "logits" (softmax branch), "raw" scores outside [0, 1] meant for a
    forced no-softmax call, where margins beyond 1 exist.  Planted values are small dyadic numbers, exact in every dtype."""
    g = torch.Generator().manual_seed(seed)
    rows, tgt = [], []

    def base() -> Tensor:
        if kind == "probs":
            return torch.randint(0, 25, (C,), generator=g).float() / 64  # <= 0.375
        if kind == "logits":
            return (torch.randn(C, generator=g) * 3).clamp(-12, 7)
        return torch.randint(-16, 9, (C,), generator=g).float() / 4  # [-4, 2]

    hi = {"probs": 0.5, "logits": 8.0, "raw": 2.5}[kind]  # above every base value
    step = {"probs": 0.125, "logits": 1.0, "raw": 0.25}[kind]

    def add(row: Tensor, t: int) -> None:
        rows.append(row)
        tgt.append(int(t))

    pos = slot_positions(C)
    for t in pos:
        for other in ((t + 1) % C, (t - 1) % C, (t + 64) % C, (t + C // 2) % C):  # adjacent lanes, another slot
            row = base()
            if other != t:
                row[other] = hi  # the largest other score, above the target or below it
            row[t] = hi + step * (1 if (t + other) % 2 else -1)
            add(row, t)
    t, o = pos[1], pos[2]
    row = base(); row[t] = row[o] = hi; add(row, t)  # the target ties the best other score: margin 0  # noqa: E702
    row = base(); row[:] = hi; add(row, pos[3])  # everything ties  # noqa: E702
    if kind == "logits":
        row = torch.full((C,), -INF); row[t] = 2.0; add(row, t)  # one-hot after the softmax: margin exactly 1, measure 0  # noqa: E702
        row = base(); row[::2] = -INF; row[t] = 1.0; add(row, t)  # masked logits: zero probabilities  # noqa: E702
        row = base(); row[t] = 60.0; add(row, t)  # a dominant logit: the others underflow in 16 bits  # noqa: E702
    else:
        lo = 0.0 if kind == "probs" else -4.0
        row = torch.full((C,), lo); row[t] = lo + 1.0; add(row, t)  # margin exactly 1: the measure is exactly 0  # noqa: E702
        row = torch.full((C,), lo); row[t] = lo + (1.0 if kind == "probs" else 3.5); add(row, t)  # margin > 1 (raw): clamped to 0  # noqa: E702
        row = base(); row[t] = hi + 1.0 if kind == "raw" else 1.0; add(row, t)  # noqa: E702
    while len(rows) < 41:
        row = base() if kind != "probs" else torch.rand(C, generator=g)
        add(row, int(torch.randint(0, C, (1,), generator=g)))
    return torch.stack(rows).to(dtype), torch.tensor(tgt, dtype=torch.long)


def hinge_batches(n: int) -> List[slice]:
    """The whole batch and its rows five at a time: the kernel returns sums, and a sum over few rows keeps a wrong row
    from drowning in the bound of forty right ones."""
    return [slice(0, n)] + [slice(i, min(n, i + 5)) for i in range(0, n, 5)]


def ranking_rows(L: int, dtype: torch.dtype, seed: int) -> Tuple[Tensor, Tensor]:
    """``preds [N, L]`` of ``dtype`` and 0/1 ``target [N, L]`` (N = 41) for the multilabel ranking kernel; no NaN."""
    g = torch.Generator().manual_seed(seed)
    rows, tgt = [], []

    def rnd() -> Tensor:
        return torch.randn(L, generator=g)

    def labels(p: float = 0.5) -> Tensor:
        return (torch.rand(L, generator=g) < p).long()

    def only(*where: int) -> Tensor:
        t = torch.zeros(L, dtype=torch.long)
        t[list(where)] = 1
        return t

    def add(row: Tensor, t: Tensor) -> None:
        rows.append(row)
        tgt.append(t)

    pos = slot_positions(L)
    add(rnd(), torch.zeros(L, dtype=torch.long))  # nrel = 0
    add(rnd(), torch.ones(L, dtype=torch.long))  # nrel = L
    for p in pos:
        add(rnd(), only(p))  # nrel = 1 in each slot position
        add(rnd(), 1 - only(p))  # nrel = L - 1
        row = rnd(); row[p] = row.min() - 1; add(row, only(p))  # the relevant label ranked last  # noqa: E702
        row = rnd(); row[p] = row.max() + 1; add(row, only(p))  # ranked first  # noqa: E702
    add(torch.full((L,), 0.25), labels())  # all scores equal
    add(torch.full((L,), 0.25), only(pos[1]))
    for hi in (2, 4, 50):  # integer-valued tie-heavy scores
        add(torch.randint(0, hi, (L,), generator=g).float(), labels())
    row, t = rnd(), labels()  # a relevant label tied with a non-relevant one
    t[pos[0]], t[pos[3]] = 1, 0
    row[pos[0]] = row[pos[3]]
    add(row, t)
    # scores of very different magnitude; the -1000 makes the coverage shift 1010 (1008 once stored in bf16)
    row = torch.tensor([3e4, 1e-3, -1000.0, 7.0] * ((L + 3) // 4))[:L].clone()
    add(row, labels())
    for p in (0.05, 0.95):
        add(rnd() * 100, labels(p))
    while len(rows) < 39:
        add(rnd(), labels())
    x = torch.stack(rows).to(dtype)
    t = torch.stack(tgt)
    # the minimum relevant score equals a shifted non-relevant one after the rounding of v + shift to the dtype
    shift = x.min().abs() + 10
    for nonrel in (-0.3, 0.3):
        row = torch.full((L,), 3e4, dtype=dtype)
        lab = torch.ones(L, dtype=torch.long)
        row[pos[3]] = nonrel
        lab[pos[3]] = 0
        if L > 1:
            row[pos[0]] = (row[pos[3]].float() + shift.float()).to(dtype)
        x = torch.cat([x, row[None]])
        t = torch.cat([t, lab[None]])
    return x, t
