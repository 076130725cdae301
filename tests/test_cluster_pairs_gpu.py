"""Native extrinsic clustering scores (``csrc/cluster_pairs.hip``) against the plain numpy fp64 oracle.

Tables are bit-equal to the oracle's.  Value rule for the scores (the project's, as in ``test_cluster_scatter_gpu.py``):
over seven seeded draws of a case ``max |native - oracle| <= 4 * max |fp32 composition - oracle| + 1e-6 * max |oracle|``,
the composition evaluated on the same inputs with ``TMX_CLUSTER_NATIVE=0``.  Every drawn case keeps the oracle's MI, AMI
denominator and entropies a factor 100 from fp32 eps (asserted), so both routes take the same rule branch."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers.cluster_pair_oracle import EPS32, ami_denominator, pair_score, pair_stats, pair_table
from tests.helpers.routes import assert_route, count_calls, kernels_run

pytestmark = pytest.mark.gpu

STEP, LDS_CELLS, SPAN, CAP = 1024, 16384, 1 << 20, 1024  # asserted against cluster_pair_tile() below: parametrised before the library loads
DRAWS = 7
AVERAGES = ("min", "geometric", "arithmetic", "max")
METRICS = ([(m, "arithmetic", 1.0) for m in ("mutual_info", "rand", "adjusted_rand", "fowlkes_mallows", "homogeneity", "completeness")]
           + [(m, a, 1.0) for m in ("normalized_mutual_info", "adjusted_mutual_info") for a in AVERAGES]
           + [("v_measure", "arithmetic", b) for b in (0.5, 1.0, 2.0)])


def _fn(metric, average, beta):
    import torchmetrics_forked_amd.functional.clustering as FC

    if metric == "v_measure":
        return lambda p, t: FC.v_measure_score(p, t, beta=beta)
    if metric in ("normalized_mutual_info", "adjusted_mutual_info"):
        return lambda p, t: getattr(FC, metric + "_score")(p, t, average)
    return FC.fowlkes_mallows_index if metric == "fowlkes_mallows" else getattr(FC, metric + "_score")


def _grid(n, kp, kt, order="shuffled", seed=0):
    """Every label of 0 .. kp-1 and 0 .. kt-1 occurs once n >= max(kp, kt); ``sorted``: both sides ascending, runs of
    about n / max(kp, kt) equal pairs (whole waves in one cell)."""
    i = torch.arange(n)
    if order == "sorted":
        return i * kp // n, i * kt // n
    g = torch.Generator().manual_seed(seed)
    return (i % kp)[torch.randperm(n, generator=g)], (i % kt)[torch.randperm(n, generator=g)]


@functools.lru_cache(maxsize=None)
def _draw(seed, n, k):
    """preds: k clusters; target: k + 3 labels, 70 % of them following preds.  Returns (preds, target, oracle stats)."""
    g = torch.Generator().manual_seed(seed)
    preds = (torch.arange(n) % k)[torch.randperm(n, generator=g)]
    noise = (torch.arange(n) % (k + 3))[torch.randperm(n, generator=g)]
    target = torch.where(torch.rand(n, generator=g) < 0.7, (preds + 2) % (k + 3), noise)
    stats = pair_stats(preds.numpy(), target.numpy(), emi=True)
    assert min(stats["mi"], stats["h_p"], stats["h_t"]) > 100 * EPS32
    assert all(abs(ami_denominator(stats, a)) > 100 * EPS32 for a in AVERAGES)  # AMI's denominator
    return preds.cuda(), target.cuda(), stats


def test_tile_constants():
    from torchmetrics_forked_amd.ops.clustering import cluster_pair_rows_per_chunk, cluster_pair_tile

    tile = cluster_pair_tile()
    assert (tile["threads"] * tile["per_lane"], tile["lds_cells"], tile["replica_cap"], tile["cell_cap"], tile["cap"]) == (STEP, LDS_CELLS, 32, SPAN, CAP)
    assert all(cluster_pair_rows_per_chunk(n, 15) == STEP for n in (1, STEP + 1, 2 * STEP + 1))  # 2 * STEP + 1 pairs: three workgroups
    assert cluster_pair_rows_per_chunk(1 << 24, 64) == 8192 and cluster_pair_rows_per_chunk(1 << 20, 8192) == 2 * 8192


TABLES = ([(f"N{n}", n, 2, 2, "shuffled") for n in (1, 2, 3)]
          + [(f"N{n}_{o}", n, 3, 5, o) for n in (STEP - 1, STEP, STEP + 1, 2 * STEP + 1) for o in ("shuffled", "sorted")]
          + [(f"cells{kp * kt}", kp * kt + 37, kp, kt, "shuffled")
             for kp, kt in ((16, 16), (257, 1), (16, 32), (27, 19), (32, 32), (25, 41), (64, 64), (17, 241), (128, 64), (129, 64), (128, 128), (129, 128))]
          + [("Kp1", 300, 1, 7, "shuffled"), ("Kt1", 300, 7, 1, "shuffled"), ("K1", 300, 1, 1, "shuffled"),
             ("1024x1", 2 * CAP + 5, 1, CAP, "shuffled"), ("1x1024", 2 * CAP + 5, CAP, 1, "shuffled"),
             ("1024x1024", 4 * CAP, CAP, CAP, "shuffled"), ("sorted_runs", 8 * STEP, 2, 2, "sorted"), ("sorted_global", 40 * STEP, 150, 150, "sorted")])


@pytest.mark.parametrize(("name", "n", "kp", "kt", "order"), TABLES, ids=[c[0] for c in TABLES])
def test_table(name, n, kp, kt, order):
    from torchmetrics_forked_amd.functional.clustering.utils import calculate_contingency_matrix
    from torchmetrics_forked_amd.ops.clustering import cluster_pair_table

    preds, target = _grid(n, kp, kt, order)
    want = torch.from_numpy(pair_table(preds.numpy(), target.numpy()))
    got = cluster_pair_table(preds.cuda(), target.cuda())
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    assert torch.equal(cluster_pair_table(preds.cuda(), target.cuda()), got)  # two runs
    assert torch.equal(calculate_contingency_matrix(preds.cuda(), target.cuda()).cpu(), want)


@pytest.mark.parametrize(("dp", "dt"), [(torch.int64, torch.uint8), (torch.int32, torch.int16), (torch.int8, torch.int64)])
@pytest.mark.parametrize("view", ["whole", "offset", "strided"])
def test_table_dtypes_and_views(dp, dt, view):
    from torchmetrics_forked_amd.ops.clustering import cluster_pair_table

    preds, target = _grid(2 * STEP + 7, 9, 11, seed=3)
    preds = (preds - 4).to(dp).cuda() if dp == torch.int8 else (preds * 3).to(dp).cuda()  # int8 with negatives
    target = target.to(dt).cuda()
    if view == "offset":  # one element into the storage: not 16-byte aligned
        preds, target = preds[1:], target[1:]
    if view == "strided":
        preds, target = preds[::2], target[::2]
        assert not preds.is_contiguous()
    assert torch.equal(cluster_pair_table(preds, target).cpu(), torch.from_numpy(pair_table(preds.cpu().numpy(), target.cpu().numpy())))


def test_generic_instantiation():
    """Ranks one element into their storage take the dword-load instantiation: the same table in both arms."""
    for kp, kt in ((9, 11), (150, 150)):
        preds, target = _grid(2 * STEP + 7, kp, kt, seed=4)
        inv_p, inv_t = torch.zeros(len(preds) + 1, dtype=torch.int32).cuda(), torch.zeros(len(preds) + 1, dtype=torch.int32).cuda()
        inv_p[1:], inv_t[1:] = preds.cuda(), target.cuda()
        assert inv_p[1:].data_ptr() % 16 != 0
        got = torch.ops.tmx.cluster_pair_table(inv_p[1:], inv_t[1:], kp, kt)
        assert torch.equal(got, torch.ops.tmx.cluster_pair_table(inv_p[1:].clone(), inv_t[1:].clone(), kp, kt))
        assert torch.equal(got.long().cpu(), torch.from_numpy(pair_table(preds.numpy(), target.numpy())))


@pytest.mark.parametrize(("top", "sorted_route"), [(SPAN - 8, False), (SPAN - 7, True)])
def test_label_span(top, sorted_route, monkeypatch):
    """A span of exactly 2^20 takes the bitmap, one wider torch.unique's inverse; both equal to labels 0..3."""
    from torchmetrics_forked_amd.ops.clustering import cluster_pair_table

    preds, target = _grid(97, 4, 3, seed=5)
    wide = torch.tensor((-7, 0, 3, top))[preds].cuda()
    calls = count_calls(monkeypatch, torch, "unique")
    assert torch.equal(cluster_pair_table(wide, target.cuda()), cluster_pair_table(preds.cuda(), target.cuda()))
    assert torch.equal(cluster_pair_table(target.cuda(), wide), cluster_pair_table(target.cuda(), preds.cuda()))
    assert bool(calls) == sorted_route


SHAPES = [("N97_K4", 97, 4)] + [(f"K{k}", 4 * k, k) for k in (15, 16, 17, 91)] + [("global_arm", 1200, 130)]


@pytest.mark.parametrize(("metric", "average", "beta"), METRICS, ids=[f"{m}-{a}-{b}" for m, a, b in METRICS])
@pytest.mark.parametrize(("name", "n", "k"), SHAPES, ids=[s[0] for s in SHAPES])
def test_scores(name, n, k, metric, average, beta, monkeypatch):
    fn, nat, comp, ora = _fn(metric, average, beta), [], [], []
    for seed in range(DRAWS):
        preds, target, stats = _draw(100 + seed, n, k)
        ora.append(pair_score(stats, metric, average, beta))
        out = fn(preds, target)
        assert out.shape == () and out.dtype == torch.float32 and out.device == preds.device
        nat.append(float(out))
        with monkeypatch.context() as m:
            m.setenv("TMX_CLUSTER_NATIVE", "0")
            comp.append(float(fn(preds, target)))
    nat, comp, ora = np.array(nat), np.array(comp), np.array(ora)
    err, ref, floor = np.abs(nat - ora).max(), np.abs(comp - ora).max(), 1e-6 * np.abs(ora).max()
    print(f"RATIO {metric} {average} {beta} {name}: native/floor {err / floor:.3e} native/composition {err / ref if ref else float('nan'):.3e}")
    assert err <= 4 * ref + floor, (nat, comp, ora)


EDGES = {
    "identical": lambda: (torch.arange(60) % 5, torch.arange(60) % 5),
    "singletons": lambda: (torch.arange(64), torch.arange(64).flip(0)),
    "one_pred_cluster": lambda: (torch.zeros(60, dtype=torch.long), torch.arange(60) % 5),
    "one_target_cluster": lambda: (torch.arange(60) % 5, torch.zeros(60, dtype=torch.long)),
    "one_cluster_each": lambda: (torch.zeros(60, dtype=torch.long), torch.full((60,), 3)),
    "independent": lambda: (torch.arange(120) % 4, (torch.arange(120) // 4) % 3),
}
EXACT = {"identical": {"rand": 1.0, "adjusted_rand": 1.0, "fowlkes_mallows": 1.0}, "singletons": {"fowlkes_mallows": 0.0},
         "one_pred_cluster": {"mutual_info": 0.0, "homogeneity": 0.0, "completeness": 1.0, "v_measure": 0.0},
         "one_target_cluster": {"mutual_info": 0.0, "homogeneity": 1.0, "completeness": 0.0, "v_measure": 0.0},
         "one_cluster_each": {"homogeneity": 1.0, "completeness": 1.0, "v_measure": 1.0, "rand": 1.0, "adjusted_rand": 1.0}, "independent": {}}


@pytest.mark.parametrize("edge", list(EDGES))
def test_planted_edges(edge):
    preds, target = EDGES[edge]()
    stats = pair_stats(preds.numpy(), target.numpy(), emi=True)
    if edge == "singletons":
        assert stats["tk"] == 0
    if edge.startswith("one_"):
        assert stats["emi"] == 0.0 and min(stats["h_p"], stats["h_t"]) == 0.0
    if edge == "independent":
        assert abs(stats["mi"]) <= EPS32  # NMI returns MI
    for metric, average, beta in METRICS:
        if metric == "adjusted_mutual_info" and stats["mi"] != stats["emi"] and abs(ami_denominator(stats, average)) < 100 * EPS32:
            continue  # all singletons: (MI - EMI) / eps is the numerator's rounding noise times 8e6 on every route
        got, want = float(_fn(metric, average, beta)(preds.cuda(), target.cuda())), pair_score(stats, metric, average, beta)
        if metric in EXACT[edge]:
            assert got == want == EXACT[edge][metric], (metric, got, want)
        else:
            assert abs(got - want) <= 1e-6 * max(abs(want), 1.0), (metric, average, got, want)


@pytest.mark.parametrize(("n", "k", "arm"), [(2 * STEP + 7, 9, "lds"), (2 * STEP + 7, 150, "global")])
def test_route(n, k, arm, monkeypatch):
    import torchmetrics_forked_amd.clustering as C
    import torchmetrics_forked_amd.functional.clustering as FC
    from torchmetrics_forked_amd.ops.clustering import cluster_pair_tile

    assert (k * k <= cluster_pair_tile()["lds_cells"]) == (arm == "lds")
    preds, target = (x.cuda() for x in _grid(n, k, k, seed=6))
    calls = count_calls(monkeypatch, torch, "unique")
    for fn in (FC.v_measure_score, FC.adjusted_mutual_info_score, FC.adjusted_rand_score):
        assert_route(kernels_run(lambda: fn(preds, target)), present=("cluster_pair_table_kernel", "cluster_pair_stats_kernel", "cluster_pair_score_kernel"))
    module = C.RandScore().cuda()
    module.update(preds[:1000], target[:1000])
    module.update(preds[1000:], target[1000:])
    scored = count_calls(monkeypatch, torch.ops.tmx, "cluster_pair_score")
    assert abs(float(module.compute()) - pair_score(pair_stats(preds.cpu().numpy(), target.cpu().numpy()), "rand")) <= 1e-6
    assert len(scored) == 1 and not calls


@pytest.mark.parametrize("kept", ["over_cap", "cpu", "float_labels", "env"])
def test_kept_routes(kept, monkeypatch):
    from torchmetrics_forked_amd.functional.clustering.utils import calculate_contingency_matrix

    preds, target = _grid(2 * (CAP + 1), CAP + 1 if kept == "over_cap" else 9, 11, seed=7)
    want = pair_stats(preds.numpy(), target.numpy())
    if kept == "float_labels":
        preds = preds.float()
    if kept != "cpu":
        preds, target = preds.cuda(), target.cuda()
    if kept == "env":
        monkeypatch.setenv("TMX_CLUSTER_NATIVE", "0")
    ran = [count_calls(monkeypatch, torch.ops.tmx, op) for op in ("cluster_pair_table", "cluster_pair_score")]
    assert torch.equal(calculate_contingency_matrix(preds, target).cpu(), torch.from_numpy(pair_table(preds.cpu().numpy(), target.cpu().numpy())))
    if kept != "float_labels":  # the functionals refuse float labels on every route
        for metric in ("mutual_info", "adjusted_rand", "v_measure"):
            got = float(_fn(metric, "arithmetic", 1.0)(preds, target))
            assert abs(got - pair_score(want, metric)) <= 1e-4 * abs(pair_score(want, metric)) + 1e-6, metric
    assert not ran[0] and not ran[1]
