"""The oracles of tests/helpers/rowwise_oracle.py, checked without a GPU.

* Agreement: on tie-free random data every oracle agrees with this package's eager CPU functions, integers exactly and
  floats within the oracle's own bound (the eager hinge path included).
* Discrimination: a deliberately wrong variant of each float measure lands more than 10x the bound away on the planted
  inputs, so a loose bound cannot hide a real failure.
* The planted top-k inputs keep the rows whose result hangs on the order inside a tie to a quarter of every case.
"""
import math

import pytest
import torch

import torchmetrics_forked_amd.functional as F
from tests.helpers import rowwise_cases as cases
from tests.helpers import rowwise_oracle as O
from torchmetrics_forked_amd.functional.classification import hinge as H
from torchmetrics_forked_amd.functional.classification import ranking as R


# ------------------------------------------------------------------------------------------------------------ top-k
def test_topk_order_and_flag_by_hand():
    nan = math.nan
    x = torch.tensor([[0.5, 2.0, 0.5, nan, 2.0, nan, -math.inf, 0.5]])
    assert O.topk_order(x) == [[3, 5, 1, 4, 0, 2, 7, 6]]
    t = torch.tensor([2])
    # k = 5: picks {3, 5, 1, 4, 0}; classes 0, 2 and 7 tie across the boundary and the lowest index is inside
    tp, fp, tn, fn, flag = O.topk_stats_oracle(x, t, 8, 5, None, 1, False)
    assert tp.tolist() == [0] * 8 and fn.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    assert fp.tolist() == [1, 1, 0, 1, 1, 1, 0, 0] and tn.tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    assert flag.tolist() == [True]
    for k, want in [(1, True), (2, False), (3, True), (4, False), (6, True), (7, False), (8, False)]:
        assert O.topk_stats_oracle(x, t, 8, k, None, 1, False)[4].tolist() == [want], k
    # ignored and out-of-range targets count nowhere; a sample of ignored rows stays all zero
    x3 = x.repeat(3, 1)
    out = O.topk_stats_oracle(x3, torch.tensor([2, -1, 8]), 8, 5, None, 1, False)
    assert all(torch.equal(a, b) for a, b in zip(out[:4], (tp, fp, tn, fn)))
    out = O.topk_stats_oracle(x3, torch.tensor([7, 7, 7]), 8, 5, 7, 3, True)
    assert all(int(a.sum()) == 0 and a.shape == (1, 8) for a in out[:4])
    # label predictions: one pick, nothing picked for a label outside [0, C)
    tp, fp, tn, fn, _ = O.topk_stats_oracle(None, torch.tensor([1, 1, 1]), 3, 1, None, 1, False, labels=torch.tensor([1, 2, 5]))
    assert (tp.tolist(), fp.tolist(), tn.tolist(), fn.tolist()) == ([0, 1, 0], [0, 0, 1], [3, 0, 2], [0, 2, 0])


def _eager_stats(p, t, C, k, ignore_index, samplewise):
    out = F.multiclass_stat_scores(p, t, num_classes=C, top_k=k, average=None, ignore_index=ignore_index,
                                   multidim_average="samplewise" if samplewise else "global", validate_args=False)
    return [out[..., i] for i in range(4)]


@pytest.mark.parametrize("C,ks", [(5, (1, 2, 5)), (70, (1, 65, 70)), (131, (64, 130))])
@pytest.mark.parametrize("ignore_index", [None, 0, -1])
def test_topk_oracle_agrees_with_eager(C, ks, ignore_index):
    g = torch.Generator().manual_seed(C)
    n, x = 12, 3
    p = torch.randn(n, C, x, generator=g)  # tie-free
    t = torch.randint(0, C, (n, x), generator=g)
    if ignore_index is not None:
        t[::4, 1] = ignore_index
        t[5] = ignore_index  # a whole sample
    rows = p.movedim(1, -1).reshape(n * x, C)
    for k in ks:
        for samplewise in (False, True):
            *mine, flag = O.topk_stats_oracle(rows, t.reshape(-1), C, k, ignore_index, x, samplewise)
            assert not flag.any()
            for a, b in zip(mine, _eager_stats(p, t, C, k, ignore_index, samplewise)):
                assert torch.equal(a, b), (k, samplewise)


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("C", cases.WIDTHS)
def test_topk_cases_flag_at_most_a_quarter(C, dtype):
    for k in cases.topk_ks(C):
        scores, target = cases.topk_rows(C, k, dtype, 100 * C + k)
        flag = O.topk_stats_oracle(scores, target, C, k, None, 1, False)[4]
        assert scores.shape == (cases.TOPK_ROWS, C) and cases.TOPK_ROWS % 4 and cases.TOPK_ROWS % 3 == 0
        assert 4 * int(flag.sum()) <= cases.TOPK_ROWS, (k, int(flag.sum()))
        if k < C:  # the straddling tie is there and flagged
            assert int(flag.sum()) >= 2


# ------------------------------------------------------------------------------------------------------------ hinge
def _eager_hinge_sums(x, t, squared, ova):
    measures, n = H._multiclass_hinge_loss_update(x, t, squared, "one-vs-all" if ova else "crammer-singer")
    return measures.double()


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("kind", ["probs", "logits"])
@pytest.mark.parametrize("C", [2, 3, 65, 300])
def test_hinge_oracle_agrees_with_eager(C, kind, dtype):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(50, C, generator=g) * 2
    x = (x.softmax(1) if kind == "probs" else x).to(dtype)
    t = torch.randint(0, C, (50,), generator=g)
    for squared in (False, True):
        for ova in (False, True):
            ref, bound = O.hinge_oracle(x, t, squared, ova)
            got = _eager_hinge_sums(x, t, squared, ova)
            # the eager path stores its sum in the input dtype: one more rounding of the result, absent from the kernel
            store = 0.0 if dtype == torch.float32 else O.unit_roundoff(dtype) * ref.abs()
            ratio = float(((got - ref).abs() / (bound + store)).max())
            assert ratio <= 1.0, (squared, ova, ratio)


@pytest.mark.parametrize("dtype", cases.DTYPES)
@pytest.mark.parametrize("kind", ["probs", "logits", "raw"])
@pytest.mark.parametrize("C", [2, 65, 2048])
def test_hinge_bound_discriminates(C, kind, dtype):
    """Wrong variants on the planted rows: the target shifted by one class, and (crammer-singer) the maximum taken over
    all classes, the target included."""
    x, t = cases.hinge_rows(C, dtype, kind, C)
    softmax = {"probs": False, "logits": True, "raw": False}[kind]
    rows = torch.arange(len(t))
    for squared in (False, True):
        for ova in (False, True):
            shifted = all_max = False
            for sl in cases.hinge_batches(len(t)):
                ref, bound = O.hinge_oracle(x[sl], t[sl], squared, ova, softmax=softmax)
                assert torch.isfinite(ref).all() and torch.isfinite(bound).all()
                wrong, _ = O.hinge_oracle(x[sl], (t[sl] + 1) % C, squared, ova, softmax=softmax)
                shifted |= bool(((wrong - ref).abs() > 10 * bound).any())
                if not ova:
                    p = x[sl].double().softmax(1) if softmax else x[sl].double()
                    meas = (1 - (p[rows[sl] - rows[sl][0], t[sl]] - p.max(1).values)).clamp(min=0)  # max over every class
                    wrong = (meas * meas if squared else meas).sum()
                    all_max |= bool((wrong - ref).abs() > 10 * bound)
            assert shifted and (ova or all_max), (squared, ova, shifted, all_max)


def test_hinge_oracle_special_values():
    nan, inf = math.nan, math.inf
    x = torch.tensor([[0.2, 0.5, 0.3], [0.1, nan, 0.2]])
    t = torch.tensor([1, 0])
    assert torch.isnan(O.hinge_oracle(x, t, False, False)[0])  # a NaN forces the softmax and poisons its row
    assert torch.isnan(O.hinge_oracle(x, t, False, True)[0]).all()
    for bad in ([0.1, inf, 0.2], [-inf, -inf, -inf]):  # inf - inf inside the softmax
        assert torch.isnan(O.hinge_oracle(torch.tensor([[0.2, 0.5, 0.3], bad]), t, False, False)[0])
    ref, bound = O.hinge_oracle(torch.tensor([[3.0, 1.0, -2.0], [0.0, 1.0, 0.0]]), t, False, False, softmax=False)
    assert float(ref) == 5.0 and float(bound) < 1e-5  # margins -2 and -1: measures 3 and 2
    ref, _ = O.hinge_oracle(torch.tensor([[0.0, 3.0, 1.0], [1.0, 0.0, 0.0]]), t, True, False, softmax=False)
    assert float(ref) == 0.0  # margin 2 is clamped, margin exactly 1 gives exactly 0


# ---------------------------------------------------------------------------------------------------------- ranking
def test_coverage_oracle_equals_eager_also_with_nan():
    x = torch.tensor([[0.1, 0.7, 0.3, 0.5], [0.9, 0.2, 0.4, 0.6], [0.3, 0.8, 0.1, 0.2]])
    t = torch.tensor([[1, 0, 0, 1], [1, 0, 0, 1], [1, 1, 1, 1]])
    assert O.coverage_oracle(x, t).tolist() == [4.0, 2.0, 4.0]
    assert float(F.multilabel_coverage_error(x, t, num_labels=4)) == pytest.approx(10 / 3)
    y = x.clone()
    y[1, 2] = math.nan  # the shift is NaN: every row with a non-relevant label counts 0, the all-relevant row keeps 4
    assert O.coverage_oracle(y, t).tolist() == [0.0, 0.0, 4.0]
    assert float(F.multilabel_coverage_error(y, t, num_labels=4)) == pytest.approx(4 / 3)
    y = x.clone()
    y[2, 0] = math.nan  # the NaN inside the all-relevant row: its own minimum is NaN as well
    assert O.coverage_oracle(y, t).tolist() == [0.0, 0.0, 0.0]
    assert float(F.multilabel_coverage_error(y, t, num_labels=4)) == 0.0
    for dtype in cases.DTYPES:
        for L in (2, 65, 257):
            p, lab = cases.ranking_rows(L, dtype, L)
            total, n = R._multilabel_coverage_error_update(p, lab)
            mine = O.coverage_oracle(p, lab)
            assert n == len(mine) and float(total) == float(mine.double().sum()), (dtype, L)


@pytest.mark.parametrize("L", [2, 5, 65, 257])
def test_lrap_and_loss_oracles_agree_with_eager(L):
    g = torch.Generator().manual_seed(L)
    x = torch.randn(24, L, generator=g)  # tie-free
    t = torch.randint(0, 2, (24, L), generator=g)
    t[0], t[1] = 0, 1
    lrap, lb = O.lrap_oracle(x, t)
    loss, sb, valid = O.ranking_loss_oracle(x, t)
    assert float(lrap[0]) == 1.0 and float(lrap[1]) == 1.0 and float(loss[0]) == 0.0 and float(loss[1]) == 0.0
    assert not valid[0] and not valid[1]
    for r in range(24):
        got = float(R._multilabel_ranking_average_precision_update(x[r : r + 1], t[r : r + 1])[0])
        assert abs(got - float(lrap[r])) <= float(lb[r]), r
        got = float(R._multilabel_ranking_loss_update(x[r : r + 1], t[r : r + 1])[0])
        assert abs(got - float(loss[r])) <= float(sb[r]), r
    # the planted rows hold ties: integers still match the definition the eager path implements
    p, lab = cases.ranking_rows(L, torch.float32, L)
    lrap, lb = O.lrap_oracle(p, lab)
    loss, sb, _ = O.ranking_loss_oracle(p, lab)
    for r in range(len(p)):
        got = float(R._multilabel_ranking_average_precision_update(p[r : r + 1], lab[r : r + 1])[0])
        assert abs(got - float(lrap[r])) <= float(lb[r]), r
        got = float(R._multilabel_ranking_loss_update(p[r : r + 1], lab[r : r + 1])[0])
        assert abs(got - float(loss[r])) <= float(sb[r]), r


@pytest.mark.parametrize("L", [5, 65, 2048])
def test_ranking_bounds_discriminate(L):
    """A relevant label dropped, and ``>=`` replaced by ``>`` (which shows only on ties)."""
    p, lab = cases.ranking_rows(L, torch.bfloat16, L)
    lrap, lb = O.lrap_oracle(p, lab)
    assert (lb <= (L + 1) * 2.0**-23).all()
    wrong, _ = O.lrap_oracle(p, lab, drop_one_relevant=True)
    assert ((wrong - lrap).abs() > 10 * lb).any()
    wrong, _ = O.lrap_oracle(p, lab, strict=True)
    assert ((wrong - lrap).abs() > 10 * lb).any()
    loss, sb, _ = O.ranking_loss_oracle(p, lab)
    wrong, _, _ = O.ranking_loss_oracle(p, lab, drop_one_relevant=True)
    assert ((wrong - loss).abs() > 10 * sb).any()


# ------------------------------------------------------------------------------------------------------------ ranks
def test_rank_and_inversion_oracles():
    from torchmetrics_forked_amd.functional.regression import kendall as K
    from torchmetrics_forked_amd.functional.regression.spearman import _rank_data

    inf = math.inf
    assert O.average_ranks_oracle(torch.tensor([3.0, 1.0, 3.0, -inf, inf, 3.0])).tolist() == [4.0, 2.0, 4.0, 1.0, 6.0, 4.0]
    assert O.average_ranks_oracle(torch.tensor([[2.0, 2.0], [1.0, 0.0]])).tolist() == [[1.5, 1.5], [2.0, 1.0]]
    assert O.inversions_oracle(torch.tensor([3.0, 1.0, 2.0])) == 2
    assert O.inversions_oracle(torch.tensor([0.0, -0.0, 0.0, -0.0])) == 0
    assert O.inversions_oracle(torch.tensor([inf, 1.0, -inf, inf])) == 3
    g = torch.Generator().manual_seed(0)
    for n in (2, 7, 300):
        for x in (torch.randn(n, generator=g, dtype=torch.float64), torch.randint(0, 5, (n,), generator=g).double()):
            assert torch.equal(O.average_ranks_oracle(x), _rank_data(x))
            assert O.inversions_oracle(x) == int(K._count_inversions(x))
    assert O.inversions_oracle(torch.arange(50, 0, -1).double()) == 50 * 49 // 2
