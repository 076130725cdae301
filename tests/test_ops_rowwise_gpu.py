"""gfx950 row kernels (csrc/rowwise.hip, csrc/clustering.hip) vs the eager CPU path of the same functions.

* top-k / samplewise multiclass stat scores: integer counts, exact (tie-free scores);
* multiclass hinge (crammer-singer / one-vs-all, squared, logits and probabilities): fp32 within float rounding,
  16-bit inputs within one rounding of the input dtype per row;
* multilabel coverage / LRAP / ranking loss: exact on integer-valued (tie-heavy) scores;
* expected mutual information (adjusted mutual info) in fp64, also against exact integer binomials;
* macro curve interpolation called directly, against an fp64 loop and bit for bit against the fp32 per-class loop.
"""
import pytest
import torch

import torchmetrics_forked_amd as tm
import torchmetrics_forked_amd.functional as F
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _scores(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    # a random permutation per row: no ties in any dtype that holds the integers exactly
    n, c = shape[0], shape[1]
    rest = shape[2:]
    x = torch.rand(n, c, *rest, generator=g).argsort(dim=1).to(torch.float32) / c
    return x.to(dtype)


@pytest.mark.parametrize("C", [5, 64, 100, 1000, 2000])
@pytest.mark.parametrize("top_k", [1, 2, 5])
@pytest.mark.parametrize("average", ["micro", "macro", None])
@pytest.mark.parametrize("mdim", ["global", "samplewise"])
def test_topk_stat_scores_vs_cpu(C, top_k, average, mdim):
    if top_k > C:
        pytest.skip("top_k > C")
    n, x = 257, (3 if mdim == "samplewise" else 1)
    p = _scores((n, C, x), C + top_k).squeeze(-1) if x == 1 else _scores((n, C, x), C + top_k)
    g = torch.Generator().manual_seed(7)
    t = torch.randint(0, C, (n, x) if x > 1 else (n,), generator=g)
    kw = dict(num_classes=C, top_k=top_k, average=average, multidim_average=mdim)
    cpu = F.multiclass_stat_scores(p, t, **kw)
    gpu = F.multiclass_stat_scores(p.cuda(), t.cuda(), **kw).cpu()
    _same(gpu, cpu)


def _same(gpu, cpu):
    if cpu.is_floating_point():  # macro / weighted means: float reduction order may differ
        torch.testing.assert_close(gpu, cpu, rtol=1e-6, atol=1e-6)
    else:
        assert torch.equal(gpu, cpu)


@pytest.mark.parametrize("ignore_index", [0, -1, 7])
@pytest.mark.parametrize("mdim", ["global", "samplewise"])
def test_topk_stat_scores_ignore_index(ignore_index, mdim):
    C, n = 10, 300
    p = _scores((n, C, 4), 3)
    g = torch.Generator().manual_seed(8)
    t = torch.randint(0, C, (n, 4), generator=g)
    t[::5, 1] = ignore_index
    for k in (1, 3):
        kw = dict(num_classes=C, top_k=k, average=None, multidim_average=mdim, ignore_index=ignore_index)
        cpu = F.multiclass_stat_scores(p, t, **kw)
        gpu = F.multiclass_stat_scores(p.cuda(), t.cuda(), **kw).cpu()
        _same(gpu, cpu)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_topk_accuracy_module_matches_cpu(dtype):
    C, n = 1000, 4096
    p = _scores((n, C), 11, dtype=torch.float32).to(dtype)
    t = torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(12))
    for cls in (tm.classification.MulticlassAccuracy, tm.classification.MulticlassF1Score, tm.classification.MulticlassRecall):
        mc, mg = cls(num_classes=C, top_k=5), cls(num_classes=C, top_k=5).cuda()
        for s in range(0, n, 1024):
            mc.update(p[s : s + 1024], t[s : s + 1024])
            mg.update(p[s : s + 1024].cuda(), t[s : s + 1024].cuda())
        torch.testing.assert_close(mg.compute().cpu(), mc.compute(), rtol=1e-6, atol=1e-7)


def test_topk_nan_rows_follow_topk_order():
    """NaN is ordered before every number (torch.topk): a NaN entry is always picked first."""
    C, n = 20, 64
    p = _scores((n, C), 5)
    p[::3, 4] = float("nan")
    t = torch.full((n,), 4, dtype=torch.long)
    out = F.multiclass_stat_scores(p.cuda(), t.cuda(), num_classes=C, top_k=2, average=None).cpu()
    assert int(out[4, 0]) >= (n + 2) // 3  # every NaN row is a tp for class 4


@pytest.mark.parametrize("mode", ["crammer-singer", "one-vs-all"])
@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("probs", [False, True])
@pytest.mark.parametrize("C", [3, 100, 1000])
def test_mc_hinge_vs_cpu_fp32(mode, squared, probs, C):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(2000, C, generator=g)
    if probs:
        x = x.softmax(1)
    t = torch.randint(0, C, (2000,), generator=g)
    cpu = F.multiclass_hinge_loss(x, t, C, squared=squared, multiclass_mode=mode)
    gpu = F.multiclass_hinge_loss(x.cuda(), t.cuda(), C, squared=squared, multiclass_mode=mode).cpu()
    torch.testing.assert_close(gpu, cpu, rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mode", ["crammer-singer", "one-vs-all"])
def test_mc_hinge_16bit(dtype, mode):
    C = 50
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1000, C, generator=g).to(dtype)
    t = torch.randint(0, C, (1000,), generator=g)
    m = tm.classification.MulticlassHingeLoss(num_classes=C, multiclass_mode=mode).cuda()
    m.update(x.cuda(), t.cuda())
    ref = F.multiclass_hinge_loss(x.float().cuda(), t.cuda(), C, multiclass_mode=mode).cpu()
    # per-element rounding to the input dtype: within a few units of its epsilon of the fp32 value
    tol = 4 * torch.finfo(dtype).eps
    torch.testing.assert_close(m.compute().cpu().float(), ref, rtol=tol, atol=tol)


@pytest.mark.parametrize("L", [5, 64, 300, 1500])
@pytest.mark.parametrize("metric", ["coverage", "lrap", "loss"])
@pytest.mark.parametrize("ties", [False, True])
def test_multilabel_ranking_vs_cpu(L, metric, ties):
    g = torch.Generator().manual_seed(L)
    n = 777
    x = torch.randint(0, 6, (n, L), generator=g).float() if ties else torch.randn(n, L, generator=g)
    t = torch.randint(0, 2, (n, L), generator=g)
    t[0] = 0  # degenerate rows: nothing relevant / everything relevant
    t[1] = 1
    fn = {"coverage": F.multilabel_coverage_error, "lrap": F.multilabel_ranking_average_precision,
          "loss": F.multilabel_ranking_loss}[metric]
    cpu = fn(x, t, num_labels=L)
    gpu = fn(x.cuda(), t.cuda(), num_labels=L).cpu()
    torch.testing.assert_close(gpu, cpu, rtol=1e-5, atol=1e-6)


def test_multilabel_ranking_loss_all_degenerate():
    x = torch.randn(10, 4).cuda()
    t = torch.zeros(10, 4, dtype=torch.long).cuda()
    assert float(F.multilabel_ranking_loss(x, t, num_labels=4)) == 0.0


@pytest.mark.parametrize("n,kp,kt", [(1000, 5, 7), (20000, 40, 30), (300, 300, 2)])
def test_adjusted_mutual_info_gpu_vs_cpu(n, kp, kt):
    g = torch.Generator().manual_seed(n)
    p = torch.randint(0, kp, (n,), generator=g)
    t = torch.randint(0, kt, (n,), generator=g)
    cpu = F.clustering.adjusted_mutual_info_score(p, t)
    gpu = F.clustering.adjusted_mutual_info_score(p.cuda(), t.cuda()).cpu()
    torch.testing.assert_close(gpu, cpu, rtol=1e-5, atol=1e-6)


def test_expected_mutual_info_kernel_vs_fp64_oracle():
    from torchmetrics_forked_amd.functional.clustering.adjusted_mutual_info_score import expected_mutual_info_score
    from torchmetrics_forked_amd.ops.clustering import expected_mutual_info

    g = torch.Generator().manual_seed(0)
    cont = torch.randint(0, 50, (9, 13), generator=g)
    n = int(cont.sum())
    ref = expected_mutual_info_score(cont, n).double()  # CPU: masked fp64 tensor expression
    got = expected_mutual_info(cont.sum(1).double().cuda(), cont.sum(0).double().cuda(), n).cpu()
    assert abs(float(got) - float(ref)) <= 1e-6 * max(1.0, abs(float(ref)))


@pytest.mark.parametrize("C", [3, 17, 200])
@pytest.mark.parametrize("kind", ["roc", "pr"])
def test_macro_curve_interp_gpu_vs_cpu(C, kind):
    """Macro-averaged ROC / PR curves: one csrc/interp.hip launch over all classes vs the per-class interp loop."""
    g = torch.Generator().manual_seed(C)
    x = torch.randn(3000, C, generator=g).softmax(1)
    x = (x * 50).round() / 50  # ties: repeated curve points and zero-width segments
    t = torch.randint(0, C, (3000,), generator=g)
    fn = F.multiclass_roc if kind == "roc" else F.multiclass_precision_recall_curve
    for thresholds in (None, 50):
        cpu = fn(x, t, num_classes=C, average="macro", thresholds=thresholds)
        gpu = fn(x.cuda(), t.cuda(), num_classes=C, average="macro", thresholds=thresholds)
        for a, b in zip(gpu, cpu):
            torch.testing.assert_close(a.cpu(), b, rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------
# Edge cases against the independent oracles of tests/helpers/oracles.py (exact integers / fp64 loops).
import functools  # noqa: E402
import math  # noqa: E402

import numpy as np  # noqa: E402

from tests.helpers import oracles as O  # noqa: E402


def _emi_case(name):
    if name == "table-9x13":  # the table of the test above
        cont = torch.randint(0, 50, (9, 13), generator=torch.Generator().manual_seed(0))
        return cont.sum(1).tolist(), cont.sum(0).tolist()
    if name == "130x130-grid-stride":  # 16,900 pairs: more than the 4096 blocks x 4 waves of the capped grid
        a = torch.randint(1, 20, (130,), generator=torch.Generator().manual_seed(1))
        return a.tolist(), a[torch.randperm(130, generator=torch.Generator().manual_seed(2))].tolist()
    return {
        "lo>1-long-ranges": ([150000, 50000], [120000, 80000]),  # a_i + b_j > N, ranges of 5 * 10^4 values of n_ij
        "zero-marginal": ([30, 0, 20], [25, 0, 25]),
        "one-row": ([50], [20, 30]),
        "marginal-equals-N": ([50, 0], [20, 30]),
    }[name]


@functools.lru_cache(maxsize=None)
def _emi_reference(name):
    a, b = _emi_case(name)
    return O.emi_exact(a, b, sum(a))


@pytest.mark.parametrize("name", ["table-9x13", "130x130-grid-stride", "lo>1-long-ranges", "zero-marginal", "one-row",
                                  "marginal-equals-N"])
def test_expected_mutual_info_kernel_vs_exact_oracle(name):
    """csrc/clustering.hip against exact integer binomials.  Relative bound 64 * 2^-53 * lgamma(N + 1) (floor 1e-12):
    every weight is exp() of a sum of lgamma terms of that size, each good to a few ulp, and the cancellation leaves
    their absolute error in the exponent."""
    from torchmetrics_forked_amd.ops.clustering import expected_mutual_info

    a, b = _emi_case(name)
    n = sum(a)
    assert n == sum(b)
    ref = _emi_reference(name)
    got = float(expected_mutual_info(torch.tensor(a, dtype=torch.float64).cuda(), torch.tensor(b, dtype=torch.float64).cuda(), n).cpu())
    rel = max(64 * 2.0 ** -53 * math.lgamma(n + 1), 1e-12)
    print(f"expected_mutual_info {name}: got {got!r} exact {ref!r} rel err {abs(got - ref) / abs(ref) if ref else abs(got):.3e} bound {rel:.3e}")
    assert abs(got - ref) <= rel * abs(ref), (got, ref)


def _interp_classes(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    xps, fps = [], []
    for n in lengths:
        xp = torch.rand(n, generator=g).sort().values
        if n >= 5:
            xp[2] = xp[1]  # repeated abscissa: zero denominator
        if n == 5:
            xp = xp[torch.tensor([0, 3, 1, 2, 4])]  # not monotone (macro PR curves): the segment is a count, not a place
        if n >= 300:
            xp[-3:] = xp[-3].clone()
        xps.append(xp)
        fps.append(torch.rand(n, generator=g) * 2 - 0.5)
    return xps, fps


def _interp_queries(m, xps, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(m, generator=g) * 3 - 1  # a third below 0, a third above 1: outside every class's range
    knots = torch.cat(xps) if xps else torch.zeros(0)
    k = min(m, knots.numel())
    x[:k] = knots[:k]  # exactly on the knots
    return x


@pytest.mark.parametrize("lengths,m", [([0, 1, 2, 5, 300], 1000), ([0, 1, 2, 5, 300], 0), ([0, 1, 2, 5, 300], 1), ([300], 777), ([1], 65),
                                       ([0], 65), ([2, 0, 300, 1, 5], 1048577 + 300)])
def test_macro_interp_kernel_direct(lengths, m):
    """tmx::macro_interp called directly: empty and one-point classes, zero-width segments, queries outside every
    class's range, no query at all and more queries than the capped grid has threads (4096 x 256).
    fp64 bound per query: C * 2^-22 * max_c(|slope x| + |intercept|); and the header's claim, the same roundings in
    the same order as the fp32 per-class loop over ``interp``, is checked bit for bit."""
    from torchmetrics_forked_amd.ops.sort import argsort as _argsort
    from torchmetrics_forked_amd.utilities.compute import interp

    xps, fps = _interp_classes(lengths, sum(lengths) + m % 7)
    x = _interp_queries(m, xps, m)
    # the sorted copy, built as utilities.compute.macro_interp_sum builds it
    lens = torch.tensor([0] + lengths, dtype=torch.long)
    off = torch.cumsum(lens, 0).cuda()
    xp, fp = torch.cat(xps).cuda(), torch.cat(fps).cuda()
    cls = torch.repeat_interleave(torch.arange(len(lengths), device="cuda"), lens[1:].cuda())
    o1 = _argsort(xp)
    o2 = _argsort(cls[o1])
    xs = xp[o1[o2]]
    got = torch.ops.tmx.macro_interp(x.cuda(), xp, fp, xs, off).cpu()
    assert got.shape == (m,) and got.dtype == torch.float32
    if m == 0:
        return
    ref = O.macro_interp_fp64(x.numpy(), [t.numpy() for t in xps], [t.numpy() for t in fps])
    scale = np.zeros(m)
    xd = x.double().numpy()
    for xpc, fpc in zip(xps, fps):
        a, f = xpc.double().numpy(), fpc.double().numpy()
        if len(a) == 1:
            scale = np.maximum(scale, abs(f[0]))
        if len(a) < 2:
            continue
        j = np.clip(np.searchsorted(np.sort(a), xd, "right") - 1, 0, len(a) - 2)
        dx = np.where(a[j + 1] - a[j] == 0, 1.0, a[j + 1] - a[j])
        slope = (f[j + 1] - f[j]) / dx
        scale = np.maximum(scale, np.abs(slope * xd) + np.abs(f[j] - slope * a[j]))
    tol = len(lengths) * 2.0 ** -22 * scale
    err = np.abs(got.double().numpy() - ref)
    ratio = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"macro_interp lengths={lengths} M={m}: max err {err.max():.3e}, err/bound {ratio:.3f}")
    assert ratio <= 1.0
    cpu = torch.zeros(m)
    for xpc, fpc in zip(xps, fps):
        if xpc.numel() >= 2:
            cpu = cpu + interp(x, xpc.clone(), fpc)
        elif xpc.numel() == 1:
            cpu = cpu + fpc[0]
    assert torch.equal(got, cpu), f"{int((got != cpu).sum())} of {m} queries differ from the fp32 per-class loop"
