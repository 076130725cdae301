"""gfx950 row kernels (csrc/rowwise.hip) against the plain oracles of tests/helpers/rowwise_oracle.py, per row / per class.

The ops are called directly (``torch.ops.tmx.*`` or the thin wrappers of ``ops/classification.py``), so no mean hides a
row.  Widths sit on every edge of the registers-per-lane dispatch (64 | 65 ... 2048), rows are planted (``rowwise_cases``)
and few: about forty, no multiple of the four waves of a block, plus one long narrow case per kernel that reaches its
grid-stride loop.

* ``topk_stats``: exact.  Ties are pinned to the kernel's contract (value descending, index ascending, NaN first by
  index); on the rows the oracle does not flag as decided inside a tie the eager CPU function is a second witness.
* ``mc_hinge``: ``err / bound <= 1`` with the bound of ``hinge_oracle`` (printed per case); NaN / inf by class.
* ``ml_ranking``: coverage exact in all three dtypes, LRAP and the ranking loss within their bounds row by row.
"""
import math

import pytest
import torch

import torchmetrics_forked_amd.functional as F
from tests.helpers import rowwise_cases as cases
from tests.helpers import rowwise_oracle as O
from tests.helpers.routes import assert_route, kernels_run
from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.ops import classification as cls_ops

pytestmark = pytest.mark.gpu

NAMES = ("tp", "fp", "tn", "fn")


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _ratio(err, bound):
    """max err / bound; a zero bound asks for a zero error."""
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------ top-k
def _assert_counts(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        a = a.cpu()
        assert a.shape == b.shape and torch.equal(a, b), f"{what}: {name} differs in {int((a != b).sum())} places, kernel {a.flatten()[(a != b).flatten()][:8].tolist()} oracle {b.flatten()[(a != b).flatten()][:8].tolist()}"


def _eager_counts(scores, target, C, k, ignore_index):
    out = F.multiclass_stat_scores(scores, target, num_classes=C, top_k=k, average=None, ignore_index=ignore_index, validate_args=False)
    return [out[:, i] for i in range(4)]


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("C", cases.WIDTHS)
def test_topk_stats_planted_rows_vs_oracle(C, dtype):
    M = cases.TOPK_ROWS
    for k in cases.topk_ks(C):
        scores, target = cases.topk_rows(C, k, dtype, 100 * C + k)
        order = O.topk_order(scores)
        dev = scores.cuda()
        for ii in dict.fromkeys((None, 0, -1, C - 1)):
            t = cases.topk_targets(target, ii)
            for samplewise, X in ((False, 1), (True, 1), (True, 3)):
                *want, flag = O.topk_stats_oracle(scores, t, C, k, ii, X, samplewise, order=order)
                got = cls_ops.topk_stats(dev, None, t.cuda(), C, k, ii, M // X, samplewise)
                _assert_counts(got, want, f"C={C} k={k} {dtype} ignore_index={ii} samplewise={samplewise} X={X}")
            assert 4 * int(flag.sum()) <= M
            if C >= 2:  # second witness where no tie order decides: the eager CPU function
                keep = (~flag).nonzero().flatten().tolist()
                *want, _ = O.topk_stats_oracle(scores[keep], t[keep], C, k, ii, 1, False, order=[order[r] for r in keep])
                for name, a, b in zip(NAMES, _eager_counts(scores[keep], t[keep], C, k, ii), want):
                    assert torch.equal(a, b), f"eager vs oracle C={C} k={k} {dtype} ignore_index={ii}: {name}"


@pytest.mark.parametrize("C", cases.WIDTHS + [5000])
def test_topk_stats_label_predictions_vs_oracle(C):
    """The label path (k = 1, one pick per row, any class count) on the targets of the planted rows."""
    M = cases.TOPK_ROWS
    _, target = cases.topk_rows(min(C, 2048), 1, torch.float32, C)
    g = torch.Generator().manual_seed(C)
    labels = torch.where(torch.rand(M, generator=g) < 0.5, target, torch.randint(0, C, (M,), generator=g))
    for ii in dict.fromkeys((None, 0, -1, C - 1)):
        t = cases.topk_targets(target, ii)
        for samplewise, X in ((False, 1), (True, 1), (True, 3)):
            *want, _ = O.topk_stats_oracle(None, t, C, 1, ii, X, samplewise, labels=labels)
            got = cls_ops.topk_stats(None, labels.cuda(), t.cuda(), C, 1, ii, M // X, samplewise)
            _assert_counts(got, want, f"labels C={C} ignore_index={ii} samplewise={samplewise} X={X}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_topk_stats_grid_stride_rows(dtype):
    """16384 + 5 rows of 5: one more than the capped grid's waves, so the row loop runs again for the last rows."""
    M, C = 16384 + 5, 5
    g = torch.Generator().manual_seed(1)
    scores = torch.randn(M, C, generator=g).to(dtype)
    target = torch.randint(0, C, (M,), generator=g)
    order = O.topk_order(scores)
    for k, ii, samplewise, X in ((2, None, False, 1), (5, 1, False, 1), (2, 1, True, 3)):
        *want, _ = O.topk_stats_oracle(scores, target, C, k, ii, X, samplewise, order=order)
        got = cls_ops.topk_stats(scores.cuda(), None, target.cuda(), C, k, ii, M // X, samplewise)
        _assert_counts(got, want, f"M={M} k={k} ignore_index={ii} samplewise={samplewise}")
    labels = torch.randint(0, C, (M,), generator=g)
    *want, _ = O.topk_stats_oracle(None, target, C, 1, None, 1, False, labels=labels)
    _assert_counts(cls_ops.topk_stats(None, labels.cuda(), target.cuda(), C, 1, None, M, False), want, "labels")


def test_topk_70_of_100_runs_the_row_kernel():
    """More picks than a wave has lanes, through the functional API, with the kernel shown to have run."""
    C, k = 100, 70
    scores, target = cases.topk_rows(C, k, torch.float32, 7)
    *want, _ = O.topk_stats_oracle(scores, target, C, k, None, 1, False)
    p, t = scores.cuda(), target.cuda()
    out = F.multiclass_stat_scores(p, t, num_classes=C, top_k=k, average=None).cpu()
    for i, name in enumerate(NAMES):
        assert torch.equal(out[:, i], want[i]), f"{name}: kernel total {int(out[:, i].sum())} oracle {int(want[i].sum())}"
    assert_route(kernels_run(lambda: F.multiclass_stat_scores(p, t, num_classes=C, top_k=k, average=None)), present=["topk_stats_kernel"])


def test_topk_stats_refuses_k_it_cannot_serve():
    p, t = torch.rand(4, 8).cuda(), torch.zeros(4, dtype=torch.long).cuda()
    for k in (0, 9):
        with pytest.raises(RuntimeError, match="k out of range"):
            cls_ops.topk_stats(p, None, t, 8, k, None, 4, False)
    with pytest.raises(RuntimeError, match="k == 1"):  # label predictions carry one pick
        cls_ops.topk_stats(None, t, t, 8, 2, None, 4, False)


# ------------------------------------------------------------------------------------------------------------ hinge
def _hinge_flag(softmax):
    return torch.tensor([int(softmax)], dtype=torch.int32, device="cuda")


def _hinge_check(x, t, xd, td, flag, softmax, squared, ova, sl):
    ref, bound = O.hinge_oracle(x[sl], t[sl], squared, ova, softmax=softmax)
    got = torch.ops.tmx.mc_hinge(xd[sl].contiguous(), td[sl].contiguous(), flag, squared, ova).cpu().double()
    assert got.shape == ref.shape and torch.isfinite(ref).all() and torch.isfinite(got).all(), (got, ref)
    return _ratio((got - ref).abs().reshape(-1), bound.reshape(-1))


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("C", cases.WIDTHS)
def test_mc_hinge_planted_rows_vs_fp64_oracle(C, dtype):
    """Both modes, squared or not; probabilities, logits (softmax) and raw scores with the softmax forced off (the only
    way to a margin beyond 1).  The whole batch and its rows five at a time; every class of the one-vs-all sums."""
    for kind in ("probs", "logits", "raw"):
        x, t = cases.hinge_rows(C, dtype, kind, C)
        softmax = kind == "logits"
        xd, td, flag = x.cuda(), t.cuda(), _hinge_flag(softmax)
        for ova in (False, True):
            for squared in (False, True):
                worst = max(_hinge_check(x, t, xd, td, flag, softmax, squared, ova, sl) for sl in cases.hinge_batches(len(t)))
                print(f"mc_hinge C={C} {dtype} {kind} one_vs_all={ova} squared={squared}: max err/bound {worst:.3f}")
                assert worst <= 1.0
                if kind != "raw":  # the wrapper reads the same decision from the device range flag
                    whole = torch.ops.tmx.mc_hinge(xd, td, flag, squared, ova)
                    assert torch.equal(cls_ops.mc_hinge(xd, td, squared, ova), whole)
        if kind == "raw":  # rows 18 and 19: margin exactly 1 and margin beyond 1, the measure is exactly 0
            for r in (18, 19):
                assert float(x[r].float().sum()) == -4.0 * (C - 1) + float(x[r, t[r]])
                for squared in (False, True):
                    assert float(torch.ops.tmx.mc_hinge(xd[r : r + 1].contiguous(), td[r : r + 1], flag, squared, False)) == 0.0


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("C", [3, 65, 2048])
def test_mc_hinge_nan_and_inf_rows_by_class(C, dtype):
    """A NaN, a +inf or a row of -inf sends the batch through the softmax (the range rule) and poisons its row as
    torch's softmax does; a row with some -inf stays finite.  Compared with the oracle as classes, finite sums by bound."""
    base, t = cases.hinge_rows(C, dtype, "probs", C)
    base, t = base[:9], t[:9]
    nan, inf = math.nan, math.inf
    specials = {"nan": [(4, 1, nan)], "+inf": [(4, 2, inf)], "all -inf": [(4, slice(None), -inf)], "some -inf": [(4, slice(0, None, 2), -inf), (4, int(t[4]), 0.5)],
                "nan in the last lane": [(8, C - 1, nan)]}
    for name, edits in specials.items():
        x = base.clone()
        for r, c, v in edits:
            x[r, c] = v
        for ova in (False, True):
            for squared in (False, True):
                ref, bound = O.hinge_oracle(x, t, squared, ova)
                got = cls_ops.mc_hinge(x.cuda(), t.cuda(), squared, ova).cpu().double()
                assert torch.equal(torch.isnan(got), torch.isnan(ref)), (name, ova, squared, got, ref)
                assert torch.equal(torch.isposinf(got), torch.isposinf(ref)) and not torch.isneginf(got).any(), (name, got, ref)
                assert bool(torch.isnan(ref).all()) == (name != "some -inf")
                fin = torch.isfinite(ref)
                if fin.any():
                    assert _ratio((got - ref).abs()[fin].reshape(-1), bound[fin].reshape(-1)) <= 1.0, (name, ova, squared)


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_mc_hinge_grid_stride_rows(dtype):
    """4096 + 5 rows of 3: the grid is capped at 1024 blocks of 4 waves, the last rows take the loop's second turn."""
    N, C = 4096 + 5, 3
    g = torch.Generator().manual_seed(2)
    t = torch.randint(0, C, (N,), generator=g)
    for kind in ("probs", "logits"):
        x = torch.randn(N, C, generator=g)
        x = (x.softmax(1) if kind == "probs" else x * 3).to(dtype)
        xd, td, flag = x.cuda(), t.cuda(), _hinge_flag(kind == "logits")
        for ova in (False, True):
            for squared in (False, True):
                worst = _hinge_check(x, t, xd, td, flag, kind == "logits", squared, ova, slice(0, N))
                print(f"mc_hinge N={N} C={C} {dtype} {kind} one_vs_all={ova} squared={squared}: max err/bound {worst:.3f}")
                assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------- ranking
def _ranking_check(x, t, what):
    xd, td = x.cuda(), t.cuda()
    cov, _ = cls_ops.ml_ranking(xd, td, 0)
    want = O.coverage_oracle(x, t)
    assert torch.equal(cov.cpu(), want), f"coverage {what}: rows {(cov.cpu() != want).nonzero().flatten()[:8].tolist()} differ"
    got, _ = cls_ops.ml_ranking(xd, td, 1)
    ref, bound = O.lrap_oracle(x, t)
    r1 = _ratio((got.cpu().double() - ref).abs(), bound)
    got, flag = cls_ops.ml_ranking(xd, td, 2)
    ref, bound, valid = O.ranking_loss_oracle(x, t)
    r2 = _ratio((got.cpu().double() - ref).abs(), bound)
    print(f"ml_ranking {what}: max err/bound LRAP {r1:.3f} ranking loss {r2:.3f}")
    assert r1 <= 1.0 and r2 <= 1.0
    assert int(flag) == int(valid.any())


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("L", cases.WIDTHS)
def test_ml_ranking_planted_rows_vs_oracle(L, dtype):
    x, t = cases.ranking_rows(L, dtype, L)
    assert len(x) % 4
    _ranking_check(x, t, f"L={L} {dtype}")
    # the coverage shift |min| + 10 is NaN once any score is: every row with a non-relevant label counts 0
    pos = cases.slot_positions(L)
    for r, c in ((5, pos[3]), (1, pos[1])):  # a mixed row; row 1, where every label is relevant
        y = x.clone()
        y[r, c] = math.nan
        cov, _ = cls_ops.ml_ranking(y.cuda(), t.cuda(), 0)
        want = O.coverage_oracle(y, t)
        assert int(want[0]) == 0 and int(want[1]) == (0 if r == 1 else L)  # row 0 has no relevant label, row 1 no other
        assert torch.equal(cov.cpu(), want), f"coverage with a NaN in row {r}: kernel {cov.cpu().tolist()} oracle {want.tolist()}"


def test_ml_ranking_any_valid_flag():
    x = torch.randn(10, 70).cuda()
    t = torch.zeros(10, 70, dtype=torch.long)
    t[::2] = 1  # every row has no or only relevant labels
    out, flag = cls_ops.ml_ranking(x, t.cuda(), 2)
    assert int(flag) == 0 and float(out.abs().sum()) == 0.0
    t[9, 69] = 1
    assert int(cls_ops.ml_ranking(x, t.cuda(), 2)[1]) == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ml_ranking_grid_stride_rows(dtype):
    N, L = 16384 + 5, 5
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(0, 8, (N, L), generator=g).float() / 4 + torch.where(torch.rand(N, L, generator=g) < 0.5, 0.0, 0.001)).to(dtype)
    t = torch.randint(0, 2, (N, L), generator=g)
    _ranking_check(x, t, f"N={N} L={L} {dtype}")


# ----------------------------------------------------------------------------------------------------------- routes
def _functional_calls(p, t, scores, labels, W):
    return {
        "topk_stats_kernel": lambda: F.multiclass_stat_scores(p, t, num_classes=W, top_k=2, average=None),
        "mc_hinge_kernel": lambda: F.multiclass_hinge_loss(p, t, W, squared=True, multiclass_mode="one-vs-all"),
        "ml_ranking_kernel": lambda: (F.multilabel_coverage_error(scores, labels, num_labels=W),
                                      F.multilabel_ranking_average_precision(scores, labels, num_labels=W),
                                      F.multilabel_ranking_loss(scores, labels, num_labels=W)),
    }


@pytest.mark.parametrize("W,dtype,native", [(65, torch.float32, True), (2048, torch.bfloat16, True), (65, torch.float16, True),
                                            (2049, torch.float32, False), (65, torch.float64, False)])
def test_row_kernel_routes_and_eager_fallback(W, dtype, native):
    """Widths up to 2048 in the three dtypes launch the row kernels through the functional API; width 2049 and fp64 do
    not (the eager tensor expressions on the GPU), and still match the oracles."""
    g = torch.Generator().manual_seed(W)
    N = 21
    # a permutation of W dyadic values per row: tie-free in fp32 / fp64, so torch.topk's tie order plays no part where the
    # fallback is compared with the oracle, and fp64 values that fp32 holds (the eager LRAP ranks in fp32)
    x = (torch.rand(N, W, generator=g).argsort(1).float() / 4096).to(dtype)  # in [0, 0.5]: the format step applies no sigmoid
    tgt = torch.randint(0, W, (N,), generator=g)
    lab = torch.randint(0, 2, (N, W), generator=g)
    p, t, labd = x.cuda(), tgt.cuda(), lab.cuda()
    for kernel, fn in _functional_calls(p, t, p, labd, W).items():
        assert_route(kernels_run(fn), present=[kernel] if native else [], absent=[] if native else [kernel])
    if native:
        return
    *want, _ = O.topk_stats_oracle(x, tgt, W, 2, None, 1, False)
    out = F.multiclass_stat_scores(p, t, num_classes=W, top_k=2, average=None).cpu()
    assert all(torch.equal(out[:, i], want[i]) for i in range(4))
    for ova in (False, True):
        ref, bound = O.hinge_oracle(x * 64 - 16, tgt, True, ova)  # logits: the softmax branch
        got = F.multiclass_hinge_loss(p * 64 - 16, t, W, squared=True, multiclass_mode="one-vs-all" if ova else "crammer-singer").cpu().double()
        assert _ratio((got - ref / N).abs().reshape(-1), (bound / N + 2.0**-24 * ref.abs() / N).reshape(-1)) <= 1.0  # + the fp32 divide by N
    u = 2.0**-24  # the functional API returns the fp32 mean of the rows: their sum in any order, one divide
    cov = O.coverage_oracle(x, lab).double()
    assert float(F.multilabel_coverage_error(p, labd, num_labels=W)) == pytest.approx(float(cov.mean()), rel=2 * u)
    ref, bound = O.lrap_oracle(x, lab)
    got = float(F.multilabel_ranking_average_precision(p, labd, num_labels=W))
    assert abs(got - float(ref.mean())) <= float(bound.sum() + (N + 1) * u * ref.sum()) / N
    ref, bound, _ = O.ranking_loss_oracle(x, lab)
    got = float(F.multilabel_ranking_loss(p, labd, num_labels=W))
    assert abs(got - float(ref.mean())) <= float(bound.sum() + (N + 1) * u * ref.sum()) / N
