"""gfx950 segmented retrieval kernel (csrc/retrieval.hip, one wave per query) vs the eager CPU engine of the same
functions: every module and functional metric, with top-k / adaptive-k, tie-heavy scores (tie-averaged nDCG),
graded relevance, queries with no positives, and queries longer than a wave; then the kernel's ten-column table against
plain per-query fp64 loops (tests/helpers/oracles.py) for every score / target dtype and more queries than the grid has waves."""
import importlib

import pytest
import torch

import torchmetrics_forked_amd.retrieval as M
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


FN = [
    ("retrieval_average_precision", {}), ("retrieval_average_precision", {"top_k": 3}),
    ("retrieval_reciprocal_rank", {}), ("retrieval_reciprocal_rank", {"top_k": 70}),
    ("retrieval_precision", {}), ("retrieval_precision", {"top_k": 4}), ("retrieval_precision", {"top_k": 300, "adaptive_k": True}),
    ("retrieval_precision", {"top_k": 300}), ("retrieval_recall", {"top_k": 65}), ("retrieval_fall_out", {"top_k": 5}),
    ("retrieval_hit_rate", {"top_k": 2}), ("retrieval_r_precision", {}), ("retrieval_normalized_dcg", {}),
    ("retrieval_normalized_dcg", {"top_k": 3}), ("retrieval_normalized_dcg", {"top_k": 100}),
]


@pytest.mark.parametrize("fn,kw", FN)
@pytest.mark.parametrize("n", [1, 17, 64, 200])
@pytest.mark.parametrize("ties", [False, True])
def test_functional_gpu_vs_cpu(fn, kw, n, ties):
    f = getattr(importlib.import_module("torchmetrics_forked_amd.functional.retrieval"), fn)
    g = torch.Generator().manual_seed(n + 7 * ties)
    p = torch.rand(n, generator=g)
    if ties:
        p = (p * 5).round() / 5
    t = torch.randint(0, 4 if "dcg" in fn else 2, (n,), generator=g)
    cpu = f(p, t, **kw)
    gpu = f(p.cuda(), t.cuda(), **kw).cpu()
    torch.testing.assert_close(gpu, cpu, rtol=1e-5, atol=1e-6)


MODULES = [
    ("RetrievalMAP", {}), ("RetrievalMAP", {"top_k": 2}), ("RetrievalMRR", {}), ("RetrievalPrecision", {"top_k": 3}),
    ("RetrievalPrecision", {"top_k": 8, "adaptive_k": True}), ("RetrievalRecall", {"top_k": 3}), ("RetrievalFallOut", {"top_k": 3}),
    ("RetrievalHitRate", {"top_k": 2}), ("RetrievalRPrecision", {}), ("RetrievalNormalizedDCG", {}),
    ("RetrievalNormalizedDCG", {"top_k": 2}),
]


@pytest.mark.parametrize("action", ["neg", "pos", "skip"])
@pytest.mark.parametrize("cls,kw", MODULES)
def test_modules_gpu_vs_cpu(cls, kw, action):
    g = torch.Generator().manual_seed(3)
    mc, mg = getattr(M, cls)(empty_target_action=action, **kw), getattr(M, cls)(empty_target_action=action, **kw).cuda()
    for _ in range(3):
        n = 5000
        idx = torch.randint(0, 300, (n,), generator=g)
        p = (torch.rand(n, generator=g) * 20).round() / 20
        t = torch.randint(0, 4 if "DCG" in cls else 2, (n,), generator=g)
        t[idx % 17 == 0] = 0  # queries without positives
        mc.update(p, t, indexes=idx)
        mg.update(p.cuda(), t.cuda(), indexes=idx.cuda())
    torch.testing.assert_close(mg.compute().cpu(), mc.compute(), rtol=1e-5, atol=1e-6)


def test_segments_stats_table():
    from torchmetrics_forked_amd.functional.retrieval._grouped import Grouped

    p = torch.tensor([0.9, 0.5, 0.5, 0.1, 0.7, 0.7]).cuda()
    t = torch.tensor([0, 1, 1, 0, 1, 0]).cuda()
    idx = torch.tensor([0, 0, 0, 0, 1, 1]).cuda()
    st = Grouped(p, t, idx).stats(2).cpu()
    # query 0 sorted: 0.9(0) 0.5(1) 0.5(1) 0.1(0): rel 2, neg 2, rel@2 1, neg@2 1, AP num 1/2, first 1, rel@R(2) 1
    assert st[0, :7].tolist() == [2.0, 2.0, 1.0, 1.0, 0.5, 1.0, 1.0]
    assert st[1, 0].item() == 1.0 and st[1, 9].item() == 2.0


# ------------------------------------------------------------------------------------------------------------------
# tmx::retrieval_segments against the plain per-query fp64 loops of tests/helpers/oracles.py.
from tests.helpers import oracles as O  # noqa: E402

_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 200]


def _stepped_scores(n):
    """Sorted scores whose tie runs cover positions [0, 3), [3, 60), [60, 70), [70, 126), [126, 131), [131, ...): runs
    that cross the 64-document chunk edges 63|64 and 127|128 and every cut-off k in {1, 3, 64, 65}."""
    pos = torch.arange(n)
    s = torch.full((n,), 0.1)
    for end, v in ((131, 0.2), (126, 0.3), (70, 0.5), (60, 0.7), (3, 0.9)):
        s[pos < end] = v
    return s


def _segment_inputs(seed):
    """Two queries of every size: one with the stepped scores above, one with three random score values; graded
    targets 0..3, one query without a positive and one with nothing else; documents of all queries interleaved."""
    g = torch.Generator().manual_seed(seed)
    p, t, idx = [], [], []
    for q, n in enumerate(_SIZES + _SIZES):
        p.append(_stepped_scores(n) if q < len(_SIZES) else torch.randint(0, 3, (n,), generator=g).float() / 4)
        t.append(torch.randint(0, 4, (n,), generator=g))
        idx.append(torch.full((n,), q))
    t[5][:] = 0
    t[6][:] = torch.randint(1, 4, (_SIZES[6],), generator=g)
    p, t, idx = torch.cat(p), torch.cat(t), torch.cat(idx)
    perm = torch.randperm(p.numel(), generator=g)
    return p[perm], t[perm], idx[perm]


def _ideal_layout(t, idx, q_count):
    """Targets in descending order inside each query, queries in ascending id order (the layout of Grouped)."""
    return torch.cat([t[idx == q].sort(descending=True).values for q in range(q_count)])


def _check_stats(st, grouped, k, adaptive, what):
    st = st.cpu()
    sizes, ps, ts = grouped.sizes.cpu().tolist(), grouped.preds.cpu().double(), grouped.target.cpu().double()
    assert st.shape == (len(sizes), 10) and st.dtype == torch.float64
    s0, worst = 0, 0.0
    for q, n in enumerate(sizes):
        scores, targets = ps[s0:s0 + n].tolist(), ts[s0:s0 + n].tolist()
        assert all(a >= b for a, b in zip(scores, scores[1:])), "layout: scores must descend inside a query"
        ref = O.retrieval_stats_fp64(scores, targets, k, adaptive)
        got = st[q].tolist()
        for c in (0, 1, 2, 3, 5, 6, 9):
            assert got[c] == ref[c], f"{what} query {q} (n={n}) column {c}: {got[c]} != {ref[c]}"
        for c in (4, 7, 8):  # fp32 sums of non-negative terms: n * 2^-23 * sum |terms|
            tol = n * 2.0 ** -23 * abs(ref[c])
            if tol:
                worst = max(worst, abs(got[c] - ref[c]) / tol)
            assert abs(got[c] - ref[c]) <= tol, f"{what} query {q} (n={n}) column {c}: {got[c]} vs {ref[c]} (bound {tol:.3e})"
        s0 += n
    return worst


@pytest.mark.parametrize("score_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("target_dtype", [torch.int64, torch.int32, torch.float32])
def test_segments_stats_vs_fp64_oracle(score_dtype, target_dtype):
    """All ten columns for queries of 1 .. 200 documents (shorter than, equal to and longer than a 64-lane chunk) with tie
    runs across the chunk edges and the cut-off, k in {None, 1, 3, 64, 65, 300} adaptive or not, fp32 / fp64 scores and
    int64 / int32 / float graded targets."""
    from torchmetrics_forked_amd.functional.retrieval._grouped import Grouped

    p, t, idx = _segment_inputs(11)
    grouped = Grouped(p.to(score_dtype).cuda(), t.to(target_dtype).cuda(), idx.cuda())
    assert grouped.target.dtype == target_dtype and grouped.sizes.cpu().tolist() == _SIZES + _SIZES
    ideal = _ideal_layout(t, idx, 2 * len(_SIZES)).to(target_dtype).cuda()
    worst = 0.0
    for k in (None, 1, 3, 64, 65, 300):
        for adaptive in (False, True):
            st = grouped.stats(k, adaptive=adaptive, ideal=ideal)
            worst = max(worst, _check_stats(st, grouped, k, adaptive, f"k={k} adaptive={adaptive}"))
    print(f"retrieval_segments scores={score_dtype} targets={target_dtype}: max err/bound over ap_sum, dcg, idcg {worst:.3f}")


def test_segments_stats_more_queries_than_waves():
    """16,500 queries of 1 .. 3 documents in one launch: more than the 4096 blocks x 4 waves of the capped grid, so the
    last queries are reached only by the grid-stride loop."""
    from torchmetrics_forked_amd.functional.retrieval._grouped import Grouped

    g = torch.Generator().manual_seed(5)
    q_count = 16500
    sizes = torch.randint(1, 4, (q_count,), generator=g)
    idx = torch.repeat_interleave(torch.arange(q_count), sizes)
    p = torch.randint(0, 2, (idx.numel(),), generator=g).float() / 2
    t = torch.randint(0, 3, (idx.numel(),), generator=g)
    perm = torch.randperm(idx.numel(), generator=g)
    p, t, idx = p[perm], t[perm], idx[perm]
    grouped = Grouped(p.cuda(), t.cuda(), idx.cuda())
    st = grouped.stats(2, ideal=torch.cat([v.sort(descending=True).values for v in torch.split(t[idx.argsort(stable=True)], sizes.tolist())]).cuda())
    worst = _check_stats(st, grouped, 2, False, "16,500 queries")
    print(f"retrieval_segments 16,500 queries: max err/bound {worst:.3f}")
