"""Plain oracles and planted cases for the GPU string kernels (csrc/text_gpu.hip, csrc/text_dp.hip, csrc/ter.hip).

Everything here is Python / numpy written from the definition of each operation; nothing is imported from the
package's native ops, so the host ops and the device ops are both held against it.

Oracles
* ``levenshtein_full(a, b, ins, dele, sub)``: the textbook full-table DP that rewrites ``a`` into ``b`` (row 0 is
  ``j * ins``, column 0 is ``i * dele``).  ``levenshtein_unit_np`` is the unit-cost form with numpy rows: a row is
  ``c = minimum(prev[:-1] + neq, prev[1:] + 1)`` and the insertion chain ``cur[j] = min(c[j], cur[j-1] + 1)`` is
  ``minimum.accumulate(c - arange) + arange``; all int64, so it stays exact.
* ``levenshtein_band(a, b, ins, dele, sub)``: Tercom's band rule.  ``ratio = m / n`` (1 for ``n = 0``), ``beam =
  ceil(ratio / 2 + 25)`` if ``ratio / 2 > 25`` else 25; row ``i`` fills ``[max(0, floor(i ratio) - beam), min(m + 1,
  floor(i ratio) + beam))``, the last row is filled whole, every other cell is 1e16 and a cell never exceeds 1e16.
* ``lcs_full(a, b)``: textbook LCS table; ``lcs_np`` the same with numpy rows (``maximum.accumulate``).
* ``ngram_overlap_counts`` / ``bleu_counts``: ``collections.Counter`` over token tuples.

The n-gram plants (``ngram_plants``) are six n-grams over one core: a pair that differs only in the top bit of the first
token's field, which lies in the high word of the 128-bit key whenever the key is wider than 64 bits, a pair that
differs only in the last token and a pair that differs only in the first token, both on the two largest legal ids.

Planted cases (shared by the CPU tests of the oracles and the GPU tests of the kernels; every generator is seeded, so
both see the same data): ``lev_cases``, ``beam_cases``, ``ngram_cases``, ``bleu_cases``, ``eed_cases`` and the TER plants
(``ter_block_move`` ... ``ter_short_batch``), each TER plant with its known edit count.
"""
import math
import random
from collections import Counter
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

INF = 10 ** 16
BEAM = 25
Seq = List[int]


# ---------------------------------------------------------------------------------------------------------- oracles
def levenshtein_full(a: Sequence, b: Sequence, ins: int = 1, dele: int = 1, sub: int = 1) -> int:
    n, m = len(a), len(b)
    prev = [j * ins for j in range(m + 1)]
    for i in range(1, n + 1):
        cur = [i * dele] + [0] * m
        x = a[i - 1]
        for j in range(1, m + 1):
            cur[j] = min(prev[j - 1] + (0 if x == b[j - 1] else sub), prev[j] + dele, cur[j - 1] + ins)
        prev = cur
    return prev[m]


def levenshtein_unit_np(a: Sequence[int], b: Sequence[int]) -> int:
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return n + m
    bb = np.asarray(b, dtype=np.int64)
    ar = np.arange(m + 1, dtype=np.int64)
    prev = ar.copy()
    for i in range(1, n + 1):
        c = np.empty(m + 1, dtype=np.int64)
        c[0] = i
        c[1:] = np.minimum(prev[:-1] + (bb != a[i - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(c - ar) + ar
    return int(prev[m])


def levenshtein_band(a: Sequence, b: Sequence, ins: int = 1, dele: int = 1, sub: int = 1) -> int:
    n, m = len(a), len(b)
    ratio = m / n if n else 1.0
    beam = math.ceil(ratio / 2 + BEAM) if ratio / 2 > BEAM else BEAM
    prev = [j * ins for j in range(m + 1)]
    for i in range(1, n + 1):
        diag = math.floor(i * ratio)
        lo = max(0, diag - beam)
        hi = m + 1 if i == n else min(m + 1, diag + beam)
        cur = [INF] * (m + 1)
        x = a[i - 1]
        for j in range(lo, hi):
            if j == 0:
                cur[0] = prev[0] + dele
            else:
                cur[j] = min(INF, prev[j - 1] + (0 if x == b[j - 1] else sub), prev[j] + dele, cur[j - 1] + ins)
        prev = cur
    return prev[m]


def lcs_full(a: Sequence, b: Sequence) -> int:
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0] * (len(b) + 1)
        for j, y in enumerate(b, 1):
            cur[j] = prev[j - 1] + 1 if x == y else max(prev[j], cur[j - 1])
        prev = cur
    return prev[-1]


def lcs_np(a: Sequence[int], b: Sequence[int]) -> int:
    """``cur[j] = max(prev[j], cur[j-1], prev[j-1] + [a_i = b_j])`` (the same table as ``lcs_full``: a row never decreases)."""
    m = len(b)
    if not len(a) or not m:
        return 0
    bb = np.asarray(b, dtype=np.int64)
    prev = np.zeros(m + 1, dtype=np.int64)
    for x in a:
        cur = np.zeros(m + 1, dtype=np.int64)
        cur[1:] = np.maximum.accumulate(np.maximum(prev[1:], prev[:-1] + (bb == x)))
        prev = cur
    return int(prev[m])


def _grams(t: Sequence[int], n: int) -> Counter:
    return Counter(tuple(t[j:j + n]) for j in range(len(t) - n + 1))


def ngram_overlap_counts(hyps: Sequence[Seq], refs: Sequence[Seq], groups: Sequence[int], n_order: int):
    """``match[r][n-1]`` = sum over n-grams of min(count in the hypothesis that owns r, count in r); ``hyp_tot[i][n-1]`` /
    ``ref_tot[r][n-1]`` = number of n-grams (0 when shorter than n).  ``groups[i]:groups[i+1]`` are hypothesis i's references."""
    match = [[0] * n_order for _ in refs]
    htot = [[max(len(h) - n + 1, 0) for n in range(1, n_order + 1)] for h in hyps]
    rtot = [[max(len(r) - n + 1, 0) for n in range(1, n_order + 1)] for r in refs]
    for i, h in enumerate(hyps):
        for n in range(1, n_order + 1):
            hc = _grams(h, n)
            for r in range(groups[i], groups[i + 1]):
                rc = _grams(refs[r], n)
                match[r][n - 1] = sum(min(c, rc[g]) for g, c in hc.items())
    return match, htot, rtot


def bleu_counts(hyps: Sequence[Seq], refs: Sequence[Seq], groups: Sequence[int], n_gram: int):
    """Per hypothesis: clipped matches against the maximum count over its references, n-gram totals, and
    (hypothesis length, closest reference length: the first minimum of |hl - rl|, 0 without references)."""
    num = [[0.0] * n_gram for _ in hyps]
    den = [[float(max(len(h) - n + 1, 0)) for n in range(1, n_gram + 1)] for h in hyps]
    lens = []
    for i, h in enumerate(hyps):
        mine = refs[groups[i]:groups[i + 1]]
        best = 0
        for k, r in enumerate(mine):
            if k == 0 or abs(len(h) - len(r)) < abs(len(h) - best):
                best = len(r)
        lens.append([float(len(h)), float(best)])
        for n in range(1, n_gram + 1):
            top: Dict[tuple, int] = {}
            for r in mine:
                for g, c in _grams(r, n).items():
                    top[g] = max(top.get(g, 0), c)
            num[i][n - 1] = float(sum(min(c, top.get(g, 0)) for g, c in _grams(h, n).items()))
    return num, den, lens


# ---------------------------------------------------------------------------------------------------------- packing
def pack(seqs: Sequence[Sequence[int]], dtype=torch.long) -> Tuple[torch.Tensor, torch.Tensor]:
    """Flat ids + int64 offsets, the layout every text op takes."""
    flat = [x for s in seqs for x in s]
    off = [0]
    for s in seqs:
        off.append(off[-1] + len(s))
    return torch.tensor(flat, dtype=dtype).reshape(-1), torch.tensor(off, dtype=torch.long)


def group_offsets(counts: Sequence[int]) -> List[int]:
    out = [0]
    for c in counts:
        out.append(out[-1] + c)
    return out


# ------------------------------------------------------------------------------------- Levenshtein / LCS planted cases
LEV_REF_LENS = [1, 63, 64, 65, 127, 128, 129, 1023, 1024]
LEV_PRED_LENS = [1, 64, 65, 200]
LEV_EQUAL_LENS = [63, 64, 65, 127, 128, 129]  # n = m: the only lengths at which b = a[1:] + [x] exists
LEV_BIG = 100_000  # pairs with more cells than this are few (see lev_cases)
LEV_NP_ABOVE = 20_000  # the oracle of a pair with more cells than this is the numpy form


def lev_cases() -> List[Tuple[str, Seq, Seq, object, object]]:
    """``(label, a, b, distance, lcs)`` with a the prediction (n tokens) and b the reference (m tokens); distance / lcs are
    the values the plant fixes by construction, None for the random pairs.  Distinct tokens everywhere but in the random
    pairs, so the planted values hold exactly."""
    rng = random.Random(20240)
    new = 10_000  # a token no base sequence holds
    out = []
    pairs = [(m, n) for m in LEV_REF_LENS for n in LEV_PRED_LENS] + [(64, 1100), (1024, 1100)] + [(k, k) for k in LEV_EQUAL_LENS]
    for m, n in dict.fromkeys(pairs):
        big = m * n > LEV_BIG
        lo, hi = min(n, m), max(n, m)
        base = list(range(1, hi + 1))  # distinct
        a, b = base[:n], base[:m]
        tag = f"m{m}-n{n}"
        out.append((f"{tag}-prefix", a, b, hi - lo, lo))
        if not big:
            out.append((f"{tag}-disjoint", a, [x + 5000 for x in b], hi, 0))
        if n == m and n >= 2:
            out.append((f"{tag}-rotate", a, a[1:] + [new], 2, n - 1))
        spots = [63, 64, m - 1] + ([] if big else [0])
        for p in sorted({p for p in spots if 0 <= p < lo}):
            a2 = list(a)
            a2[p] = new
            out.append((f"{tag}-mismatch{p}", a2, b, hi - lo + 1, lo - 1))
        out.append((f"{tag}-random", [rng.randrange(3) for _ in range(n)], [rng.randrange(3) for _ in range(m)], None, None))
    assert sum(len(a) * len(b) > LEV_BIG for _, a, b, _, _ in out) <= 13
    return out


def lev_calls(chunk: int = 68) -> List[List[Tuple[str, Seq, Seq, object, object]]]:
    """The cases in calls of about 70 pairs: an empty prediction first, an empty reference last, and a pair count that
    is no multiple of the 4 waves of a block (so the last block is partial)."""
    cases = lev_cases()
    calls = []
    for s in range(0, len(cases), chunk):
        call = [("empty-pred", [], [7, 8, 9], 3, 0)] + cases[s:s + chunk] + [("empty-ref", [7, 8], [], 2, 0)]
        if len(call) % 4 == 0:
            call.insert(1, ("both-empty", [], [], 0, 0))
        calls.append(call)
    return calls


def lev_oracle(a: Seq, b: Seq) -> Tuple[int, int]:
    if len(a) * len(b) > LEV_NP_ABOVE:
        return levenshtein_unit_np(a, b), lcs_np(a, b)
    return levenshtein_full(a, b), lcs_full(a, b)


# ------------------------------------------------------------------------------------------------- beam planted cases
BEAM_COSTS = [(1, 1, 1), (2, 3, 1), (3, 2, 5), (1, 1, 2)]
BEAM_LENS = [0, 1, 2, 20, 26, 49, 50, 51, 100, 300]


def beam_cases() -> List[Tuple[Seq, Seq]]:
    """257 (prediction, reference) pairs: every length pair of BEAM_LENS twice (random over 3 symbols; the reference a
    noisy resampling of the prediction) and 57 more short pairs over 2 symbols."""
    rng = random.Random(77)
    out = []
    for n in BEAM_LENS:
        for m in BEAM_LENS:
            a = [rng.randrange(3) for _ in range(n)]
            out.append((a, [rng.randrange(3) for _ in range(m)]))
            a = [rng.randrange(40) for _ in range(n)]
            b = [a[min(n - 1, j * n // m)] if n and rng.random() < 0.8 else 50 + rng.randrange(5) for j in range(m)]
            out.append((a, b))
    for _ in range(57):
        out.append(([rng.randrange(2) for _ in range(rng.choice([0, 1, 2, 20, 26]))],
                    [rng.randrange(2) for _ in range(rng.choice([0, 1, 2, 20, 26]))]))
    assert len(out) == 257
    return out


# ------------------------------------------------------------------------------------------------ n-gram planted cases
NGRAM_CONFIGS = [(2, 64), (8, 16), (3, 33), (2, 43), (6, 11), (4, 17), (9, 5)]
NGRAM_SLOT_SPOTS = [5, 64 + 5, 448 + 5]  # one repeated n-gram in slots 0, 1 and 7


def ngram_ids(bits: int, rng: random.Random) -> List[int]:
    """0, 1, the two largest legal ids (id + 1 <= 2^bits - 1) and three random ones.  At 64 bits the ids are int64: the
    largest that keep id + 1 in int64, and -3 / -2, whose bit patterns are 2^64 - 3 and 2^64 - 2 (id + 1 fills the
    unsigned field to its last bit)."""
    if bits >= 64:
        return [0, 1, -3, -2, 2 ** 63 - 3, 2 ** 63 - 2] + [rng.randrange(2, 2 ** 63 - 3) for _ in range(3)]
    top = 2 ** bits
    ids = [0, 1, top - 3, top - 2]
    return ids + [rng.randrange(2, max(3, top - 3)) for _ in range(3)]


def high_twin(bits: int) -> int:
    """The id whose field (id + 1) differs from that of id 1 in the top bit of the field alone.  In an n-gram of more than
    64 bits the first token's top bit lies in the high word of the key, so two n-grams that differ only by this swap at
    their first token have equal low words.  At 64 bits it is the int64 with the bit pattern 2^63 + 1."""
    return 2 ** (bits - 1) + 1 if bits < 64 else -(2 ** 63) + 1


def ngram_plants(n: int, ids: List[int], bits: int) -> List[Seq]:
    """Six n-grams over one core of n - 1 tokens: two that differ only in the top bit of their first token, two that
    differ only in their last token and two that differ only in their first token (the extreme ids on the differing token)."""
    core = [ids[(3 * j + 1) % 4] for j in range(n - 1)]
    return [[high_twin(bits)] + core, [1] + core, core + [ids[3]], core + [ids[2]], [ids[3]] + core, [ids[2]] + core]


def _plant_into(seq: Seq, n: int, plants: List[Seq], spots: Sequence[int]) -> None:
    """Plant 0 at every spot with another plant right behind it and a third a little further on: each only where it fits."""
    for k, p in enumerate(spots):
        for q, g in ((p, plants[0]), (p + n, plants[1 + k % 5]), (p + 2 * n + 3, plants[1 + (k + 2) % 5])):
            if q + n <= len(seq):
                seq[q:q + n] = g


def ngram_cases(n: int, top_ids: List[int], hyp_lens: Sequence[int], seed: int, long_ref: int = 600, bits: int = 16):
    """``(hyps, refs, groups)``: hypotheses of the given lengths with the plants at NGRAM_SLOT_SPOTS and two more
    spots; groups of 0, 1 and 3 references; among the references one shorter than n and one of ``long_ref``
    tokens, each holding the plants in other multiplicities than the hypothesis."""
    rng = random.Random(seed)
    plants = ngram_plants(n, top_ids, bits)
    hyps, refs, counts = [], [], []
    pool = top_ids + [high_twin(bits)]
    for k, hl in enumerate(hyp_lens):
        h = [rng.choice(pool) for _ in range(hl)]
        _plant_into(h, n, plants, NGRAM_SLOT_SPOTS + [128 + 17, 256 + 40])
        hyps.append(h)
        c = 0 if k in (2, 6) else (3 if k % 2 else 1)
        for t in range(c):
            rl = (max(hl, 2 * n + 7), n - 1, long_ref)[t] if c == 3 else (hl + 3 if hl else 0)
            r = [rng.choice(pool) for _ in range(rl)]
            _plant_into(r, n, plants, [2, 2 + 3 * n + 9, 300, 520][:1 + (k + t) % 4])
            refs.append(r)
        counts.append(c)
    return hyps, refs, group_offsets(counts)


def ngram_hyp_lens(n: int) -> List[int]:
    return [0, 1, n - 1, n, 63, 64, 65, 191, 192, 193, 448, 511, 512]


BLEU_IDS = [0, 1, 65533, 65534]
BLEU_HYP_LENS = [0, 1, 3, 4, 64, 65, 255, 256]


def bleu_cases():
    """As ``ngram_cases`` at order 4 with ids at the 16-bit field limit, then: a hypothesis of 64 tokens whose references
    have 60 and 68 tokens and one of 65 with references of 70 and 60 (equal distance: the first wins both times), and a
    hypothesis without references."""
    hyps, refs, groups = ngram_cases(4, BLEU_IDS, BLEU_HYP_LENS, seed=4, long_ref=300)
    rng = random.Random(5)
    counts = [groups[i + 1] - groups[i] for i in range(len(hyps))]
    for hl, rls in ((64, (60, 68)), (65, (70, 60)), (7, ())):
        hyps.append([rng.choice(BLEU_IDS) for _ in range(hl)])
        refs.extend([rng.choice(BLEU_IDS) for _ in range(rl)] for rl in rls)
        counts.append(len(rls))
    return hyps, refs, group_offsets(counts)


# --------------------------------------------------------------------------------------------------- EED planted cases
EED_ARGS = (ord(" "), 2.0, 0.3, 0.2, 1.0)  # space, alpha, rho, deletion, insertion


def eed_cases() -> Tuple[List[str], List[str]]:
    """257 (hypothesis, reference) strings: an empty hypothesis, an empty reference, both empty, a reference of spaces
    only (every row jumps), then random sentences."""
    rng = random.Random(9)
    words = "the a cat sat on mat dog ran far away".split()
    sent = lambda: " " + " ".join(rng.choice(words) for _ in range(rng.randint(1, 12))) + " "  # noqa: E731
    hyps = ["", sent(), "", sent(), " "] + [sent() for _ in range(252)]
    refs = [sent(), "", "", " " * 9, " " * 4] + [sent() for _ in range(252)]
    return hyps, refs


# ---------------------------------------------------------------------------------------------------------- TER plants
def _words(k: int, base: int = 0) -> Seq:
    return list(range(base, base + k))  # k distinct words


def ter_block_move(k: int, length: int, start: int, target: int) -> Tuple[Seq, Seq, int]:
    """Reference of k distinct words; hypothesis = the reference with the block [start, start + length) taken out and
    put back in front of position ``target`` of the remainder (target != start, |target - start| <= 50): 1 edit."""
    assert 1 <= length <= 9 and 0 <= start <= k - length and 0 <= target <= k - length and 0 < abs(target - start) <= 50
    ref = _words(k)
    rest = ref[:start] + ref[start + length:]
    return ref, rest[:target] + ref[start:start + length] + rest[target:], 1


def ter_two_moves(k: int, length: int) -> Tuple[Seq, Seq, int]:
    """Two block moves in disjoint halves of the sentence (k >= 4 length + 8): 2 edits."""
    half = k // 2
    assert half >= 2 * length + 4
    ref = _words(k)
    _, h1, _ = ter_block_move(half, length, 1, length + 2)
    _, h2, _ = ter_block_move(k - half, length, 0, length + 3)
    return ref, h1 + [x + half for x in h2], 2


def ter_substitution(k: int, at: int) -> Tuple[Seq, Seq, int]:
    ref = _words(k)
    return ref, ref[:at] + [100_000] + ref[at + 1:], 1


def ter_drop(k: int, at: int) -> Tuple[Seq, Seq, int]:
    ref = _words(k)
    return ref, ref[:at] + ref[at + 1:], 1


def ter_append(k: int) -> Tuple[Seq, Seq, int]:
    ref = _words(k)
    return ref, ref + [100_000], 1


def ter_identical(k: int) -> Tuple[Seq, Seq, int]:
    return _words(k), _words(k), 0


TER_KS = [6, 30, 64, 65, 100]
TER_BLOCKS = [1, 5, 9]


def ter_plants() -> List[Tuple[Seq, Seq, int]]:
    """About 200 (reference, hypothesis, edits) plants, longest sentences first, the degenerate pairs last: block moves
    for every k of TER_KS and block length of TER_BLOCKS (left and right, short and long distances), the one-edit and
    zero-edit plants, two-move plants, then an empty hypothesis (0 edits), an empty reference (one insertion per
    hypothesis word) and 2-word pairs."""
    rng = random.Random(31)
    out = []
    for k in TER_KS:
        for length in TER_BLOCKS:
            if length >= k:
                continue
            top = k - length
            legal = [(s, t) for s in range(top + 1) for t in range(top + 1) if 0 < abs(s - t) <= 50]
            far = min(top, 50)
            moves = {(0, far), (far, 0), (0, 1), (top, top - 1), (top, top - far)}
            moves |= set(rng.sample(legal, min(len(legal), 10)))
            moves = sorted(moves)[:10] if len(moves) > 10 else sorted(moves)
            out += [ter_block_move(k, length, s, t) for s, t in moves]
        out += [ter_substitution(k, 0), ter_substitution(k, k - 1), ter_substitution(k, k // 2), ter_drop(k, 0), ter_drop(k, k - 1),
                ter_drop(k, k // 3), ter_append(k), ter_identical(k)]
        out += [ter_two_moves(k, length) for length in (1, 5, 9) if k // 2 >= 2 * length + 4]
    out.sort(key=lambda c: -max(len(c[0]), len(c[1])))
    out += [([3, 4, 5], [], 0), ([], [3, 4], 2), ([1, 2], [1, 2], 0), ([1, 2], [2, 1], 1), ([1, 2], [1, 9], 1), ([], [], 0)]
    return out


def ter_short_batch(count: int = 1100) -> List[Tuple[Seq, Seq, int]]:
    """``count`` plants of 3 to 12 words."""
    rng = random.Random(47)
    out = []
    while len(out) < count:
        k = rng.randint(3, 12)
        kind = rng.randrange(6)
        if kind <= 1:
            length = rng.randint(1, min(9, k - 1))
            top = k - length
            s, t = rng.randint(0, top), rng.randint(0, top)
            if s == t:
                continue
            out.append(ter_block_move(k, length, s, t))
        elif kind == 2:
            out.append(ter_substitution(k, rng.randrange(k)))
        elif kind == 3:
            out.append(ter_drop(k, rng.randrange(k)))
        elif kind == 4:
            out.append(ter_append(k))
        else:
            out.append(ter_identical(k))
    return out


def ter_long_pair(k: int = 400) -> Tuple[Seq, Seq, int]:
    """One long pair for the module-level case: a 400-word sentence and its copy with one block of 7 words moved 30 on."""
    return ter_block_move(k, 7, 200, 230)
