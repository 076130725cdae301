"""The device COCO evaluators (csrc/coco_match.hip) against the loop oracle (tests/helpers/coco_oracle.py), not only
against their host sibling: tmx::coco_evaluate_gpu with fp64 scores (two stable sorts) and fp32 scores (composite-key
ordering), tmx::coco_evaluate_gpu_img with fp32 / bf16 / fp16 scores and both forms of its maxDets argument, and
MeanAveragePrecision on both routes, on the planted cases and the recall-threshold sweep of tests/helpers/coco_cases.py.
Every comparison is exact (the oracle, the host evaluator and the kernels do the same IEEE double operations); each
test prints one line per case and route with the number of differing table cells (``-s``)."""
import pytest
import torch

from tests.helpers import coco_cases as cc
from tests.helpers.coco_oracle import summarize
from tests.helpers.routes import count_calls
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu

_NAMES = ("precision", "recall", "scores")


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


@pytest.fixture(scope="module")
def want():
    """Oracle and host-evaluator results, computed once per (case, score values): ``want(name, case, dtype)`` ->
    (oracle (precision, recall, scores, ious), host (precision, recall, scores))."""
    memo = {}

    def get(name, case, dtype):
        key = (name, None if dtype == torch.float64 or cc.scores_exact_in(case, dtype) else dtype)
        if key not in memo:
            dt = torch.float64 if key[1] is None else dtype
            host = torch.ops.tmx.coco_evaluate(*cc.host_args(cc.flat(case, dt)))
            memo[key] = (cc.run_oracle(case, dt), host[:3])
        return memo[key]

    return get


@pytest.fixture(scope="module")
def sweeps():
    return {"linspace": cc.sweep(cc.REC_THRS), "adversarial": cc.sweep(cc.adversarial_rec_thrs())}


def _cells(got, ref):
    return sum(int((g.cpu() != r).sum()) for g, r in zip(got, ref))


def _check_routes(name, case, want, img_flag=0):
    """Every route of the two device ops on one case; returns the failures (all lines are printed first)."""
    failures = []
    x = cc.flat(case)
    rows = max(int(x["det_off"].diff().max()), int(x["gt_off"].diff().max()))  # the most rows of one image
    assert img_flag == int(rows > 256)

    def compare(route, got, dtype):
        oracle, host = want(name, case, dtype)
        vs_oracle, vs_host = _cells(got, oracle[:3]), _cells(got, host)
        print(f"{name} {route}: cells differing from the oracle {vs_oracle}, from the host evaluator {vs_host}")
        for n, g, o, h in zip(_NAMES, got, oracle[:3], host):
            if not torch.equal(g.cpu(), o):
                failures.append(f"{name} {route}: {n} differs from the oracle in {int((g.cpu() != o).sum())} cells")
            if not torch.equal(g.cpu(), h):
                failures.append(f"{name} {route}: {n} differs from the host evaluator")
        return oracle

    for dtype in (torch.float64, torch.float32):  # grid route: two stable sorts / composite-key ordering
        route = f"grid[{str(dtype).split('.')[-1]}]"
        out = torch.ops.tmx.coco_evaluate_gpu(*cc.grid_args(cc.flat(case, dtype), "cuda", export_iou=True))
        oracle = compare(route, out[:3], dtype)
        if int(out[5]) != 0:
            failures.append(f"{name} {route}: ground-truth limit flag {int(out[5])}")
        got, ref = cc.iou_blocks(out[3], out[4]), cc.oracle_iou_blocks(oracle[3])
        bad = [k for k in ref if k not in got or not torch.equal(got[k], ref[k])] + [k for k in got if k not in ref]
        print(f"{name} {route}: exported IoU blocks differing from the oracle {len(bad)} of {len(ref)}")
        if bad:
            failures.append(f"{name} {route}: IoU blocks {bad[:4]}")
    for dtype in cc.SCORE_DTYPES:  # per-image route
        for md_dev in (False, True):
            route = f"img[{str(dtype).split('.')[-1]}, max_dets_dev={'given' if md_dev else 'None'}]"
            out = torch.ops.tmx.coco_evaluate_gpu_img(*cc.img_args(cc.flat(case, dtype), "cuda", md_dev))
            flag = int(out[3])
            if flag != img_flag:
                failures.append(f"{name} {route}: row-limit flag {flag}, expected {img_flag}")
            if img_flag:
                print(f"{name} {route}: row-limit flag {flag} (tables invalid by contract)")
            else:
                compare(route, out[:3], dtype)
    return failures


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_device_routes_equal_oracle_on_planted_case(name, want):
    failures = _check_routes(name, cc.CASES[name], want, img_flag=int("_257_" in name))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("which", ["linspace", "adversarial"])
def test_device_routes_equal_oracle_on_recall_sweep(which, sweeps, want):
    """The accumulate kernel's table of TP counts per recall threshold (ceil + two correction loops), its bucketed
    envelope and its answer at count 0, at every npig of the sweep; 256 thresholds is the kernel's limit."""
    failures = _check_routes(f"sweep/{which}", sweeps[which], want)
    assert not failures, "\n".join(failures)


def _one_pair(n_gt):
    gts = [(0, 1, [2 * g, 0, 1, 1], 0, 0) for g in range(n_gt)]
    return cc.make_case(dets=[(0, 1, [2 * (n_gt - 1), 0, 1, 1], 0.5)], gts=gts, n_img=1)


def test_grid_route_ground_truth_limit_flag(want):
    """1024 ground truths in one (image, class) pair: the last bit of the last bitset word, flag 0, the oracle's
    tables.  1025: output 5 is set (no export, so nothing is read on the host and no error is raised)."""
    case = _one_pair(1024)
    out = torch.ops.tmx.coco_evaluate_gpu(*cc.grid_args(cc.flat(case, torch.float32), "cuda", export_iou=False))
    oracle, host = want("pair_1024", case, torch.float32)
    print(f"pair_1024 grid[float32]: cells differing from the oracle {_cells(out[:3], oracle[:3])}, flag {int(out[5])}")
    assert int(out[5]) == 0
    for n, g, o, h in zip(_NAMES, out[:3], oracle[:3], host):
        assert torch.equal(g.cpu(), o) and torch.equal(g.cpu(), h), n
    assert float(out[1][0, 0, 0, 2]) == 1 / 1024
    over = torch.ops.tmx.coco_evaluate_gpu(*cc.grid_args(cc.flat(_one_pair(1025), torch.float32), "cuda", export_iou=False))
    print(f"pair_1025 grid[float32]: flag {int(over[5])}")
    assert int(over[5]) == 1


_KEYS = ("map", "map_50", "map_75", "map_small", "map_medium", "map_large",
         "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium", "mar_large")


@pytest.mark.parametrize("img_route", [True, False])
@pytest.mark.parametrize("name", cc.MODULE_CASES + ("image_row_limits_256", "image_row_limits_257_dets", "image_row_limits_257_gts"))
def test_module_routes_equal_oracle_summary(name, img_route, want, monkeypatch):
    """MeanAveragePrecision on the device: the per-image op up to 256 rows per image, the grid op past that or with
    the per-image route off; the 12 statistics are the oracle's either way."""
    import torchmetrics_forked_amd.detection.mean_ap as mod
    from torchmetrics_forked_amd.detection import MeanAveragePrecision

    case = cc.CASES[name]
    monkeypatch.setattr(mod, "_IMG_ROUTE", img_route)
    img_calls = count_calls(monkeypatch, torch.ops.tmx, "coco_evaluate_gpu_img")
    grid_calls = count_calls(monkeypatch, torch.ops.tmx, "coco_evaluate_gpu")
    host_calls = count_calls(monkeypatch, torch.ops.tmx, "coco_evaluate")
    preds, target, kwargs = cc.module_inputs(case, "cuda")
    metric = MeanAveragePrecision(**kwargs).cuda()
    metric.warn_on_many_detections = False
    metric.update(preds, target)
    res = metric.compute()
    expect_img = img_route and "_257_" not in name
    assert (len(img_calls), len(grid_calls), len(host_calls)) == ((1, 0, 0) if expect_img else (0, 1, 0))
    oracle, _ = want(name, case, torch.float32)
    stats = summarize(oracle[0].numpy(), oracle[1].numpy(), case["iou_thrs"], case["max_dets"])
    worst = max(abs(float(res[k]) - v) for k, v in zip(_KEYS, stats))
    print(f"{name} module[{'img' if expect_img else 'grid'} op]: largest difference of the 12 statistics {worst:.3g}")
    for k, v in zip(_KEYS, stats):
        assert abs(float(res[k]) - v) < 1e-6, (name, k, float(res[k]), v)
