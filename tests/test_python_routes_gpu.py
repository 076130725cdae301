"""Python-level routes, observed by call counts (``tests/helpers/routes.py`` ``count_calls``): which native op a module
called, next to the result assertions of that module's own tests."""
import pytest
import torch

import torchmetrics_forked_amd as tm
from tests.helpers.routes import count_calls
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


# ------------------------------------------------------------------------------------------- MeanAveragePrecision
def _boxes(n, g):
    xy = torch.rand(n, 2, generator=g) * 400
    wh = torch.rand(n, 2, generator=g) * 100 + 2
    return torch.cat([xy, xy + wh], 1)


def _map_batch(det_counts, score_dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    preds, target = [], []
    for nd in det_counts:
        ng = 6
        gt = _boxes(ng, g)
        det = gt[torch.randint(0, ng, (nd,), generator=g)] + torch.randn(nd, 4, generator=g) * 8
        det[:, 2:] = torch.maximum(det[:, 2:], det[:, :2] + 1)
        scores = ((torch.rand(nd, generator=g) * 64).floor() / 64).to(score_dtype)  # (exact in fp16)
        preds.append({"boxes": det, "scores": scores, "labels": torch.randint(0, 4, (nd,), generator=g)})
        target.append({"boxes": gt, "labels": torch.randint(0, 4, (ng,), generator=g)})
    return preds, target


def _to(batch, dev):
    return [[{k: v.to(dev) for k, v in d.items()} for d in lst] for lst in batch]


MAP_CASES = [
    # (id, detections per image, metric arguments, score dtype, per-image route)
    ("small", [10, 9, 11, 10], {}, torch.float32, True),
    ("257-detections", [10, 257, 11, 10], {}, torch.float32, False),
    ("extended-summary", [10, 9, 11, 10], {"extended_summary": True}, torch.float32, False),
    ("fp16-scores", [10, 9, 11, 10], {}, torch.float16, True),  # 16-bit scores are exact in fp32: still per image
    ("fp64-scores", [10, 9, 11, 10], {}, torch.float64, False),
]


@pytest.mark.parametrize("counts,kw,score_dtype,img_route", [c[1:] for c in MAP_CASES], ids=[c[0] for c in MAP_CASES])
def test_map_bbox_route(monkeypatch, counts, kw, score_dtype, img_route):
    from torchmetrics_forked_amd.detection import MeanAveragePrecision

    img = count_calls(monkeypatch, torch.ops.tmx, "coco_evaluate_gpu_img")
    grid = count_calls(monkeypatch, torch.ops.tmx, "coco_evaluate_gpu")
    batch = _map_batch(counts, score_dtype)
    gpu, cpu = MeanAveragePrecision(**kw).cuda(), MeanAveragePrecision(**kw)
    gpu.warn_on_many_detections = cpu.warn_on_many_detections = False
    gpu.update(*_to(batch, "cuda"))
    cpu.update(*batch)
    a, c = gpu.compute(), cpu.compute()
    for k in c:
        if k not in ("ious", "precision", "recall", "scores"):
            torch.testing.assert_close(a[k].cpu(), c[k], atol=1e-6, rtol=0, msg=k)  # (test_map_gpu_states_match_cpu's)
    assert (len(img) > 0, len(grid) > 0) == (img_route, not img_route), (len(img), len(grid))


# --------------------------------------------------------------------------------------------------- regression
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("cls", [tm.MeanSquaredError, tm.MeanAbsoluteError])
def test_sum_state_modules_accumulate_in_one_native_call(monkeypatch, cls, dtype):
    calls = count_calls(monkeypatch, torch.ops.tmx, "regression_accumulate")
    g = torch.Generator().manual_seed(0)
    gpu, cpu = cls().cuda(), cls()
    for k in range(3):
        p, t = torch.randn(10_001, generator=g, dtype=dtype), torch.randn(10_001, generator=g, dtype=dtype)
        gpu.update(p.cuda(), t.cuda())
        cpu.update(p, t)
        assert len(calls) == k + 1
    torch.testing.assert_close(gpu.compute().cpu(), cpu.compute(), rtol=1e-6, atol=1e-7)  # (test_accumulate_matches_cpu's)


@pytest.mark.parametrize("cls", [tm.MeanSquaredError, tm.MeanAbsoluteError])
def test_sum_state_modules_16bit_and_autograd_take_the_eager_update(monkeypatch, cls):
    calls = count_calls(monkeypatch, torch.ops.tmx, "regression_accumulate")
    g = torch.Generator().manual_seed(1)
    p, t = torch.randn(5000, generator=g).cuda(), torch.randn(5000, generator=g).cuda()
    m = cls().cuda()
    m.update(p.bfloat16(), t.bfloat16())
    assert not calls
    pq, tq = p.bfloat16().double(), t.bfloat16().double()
    ref = ((pq - tq) ** 2).mean() if cls is tm.MeanSquaredError else (pq - tq).abs().mean()
    # bf16 arithmetic at worst: 2^-9 on each difference (doubled by the square), 2^-9 on each square, 2^-9 on the sum
    torch.testing.assert_close(m.compute().double(), ref, rtol=2.0**-7, atol=0)
    q = p.clone().requires_grad_(True)
    out = cls().cuda()(q, t)
    out.backward()
    assert not calls and q.grad is not None


def test_pearson_updates_in_one_native_call(monkeypatch):
    calls = count_calls(monkeypatch, torch.ops.tmx, "pearson_update")
    g = torch.Generator().manual_seed(7)
    for dtype in (torch.float32, torch.float64):
        calls.clear()
        gpu, cpu = tm.PearsonCorrCoef().cuda(), tm.PearsonCorrCoef()
        for k in range(3):
            p = (torch.randn(20_000, generator=g) * 3 + 1).to(dtype)
            t = (0.5 * p + torch.randn(20_000, generator=g, dtype=dtype)).to(dtype)
            gpu.update(p.cuda(), t.cuda())
            cpu.update(p, t)
            assert len(calls) == k + 1
        assert torch.allclose(gpu.compute().cpu().double(), cpu.compute().double(), rtol=1e-5)  # (test_pearson_inplace_update_gpu's)
    # 16-bit inputs stay on the native op (unlike the sum-state modules: the kernel widens them, the states are fp32)
    calls.clear()
    pq, tq = p.bfloat16(), t.bfloat16()
    m = tm.PearsonCorrCoef().cuda()
    m.update(pq.cuda(), tq.cuda())
    assert len(calls) == 1
    ref = torch.corrcoef(torch.stack([pq.double(), tq.double()]))[0, 1]
    print(f"pearson bf16 inputs: |r - fp64 r| = {abs(float(m.compute()) - float(ref)):.3e}")
    # the quantised inputs are the same on both sides; what remains is fp32 moment arithmetic: 1e-5, as for fp32 above
    torch.testing.assert_close(m.compute().cpu().double(), ref, rtol=1e-5, atol=1e-6)
    # forward on inputs that record autograd: the accumulation into the states runs without grad (one native call),
    # the batch value is recomputed by the eager update, which is differentiable
    calls.clear()
    q = p.float().cuda().requires_grad_(True)
    out = tm.PearsonCorrCoef().cuda()(q, t.float().cuda())
    out.backward()
    assert len(calls) == 1 and q.grad is not None and torch.isfinite(q.grad).all()


# ------------------------------------------------------------------------------------- MiFID memorization distance
@pytest.mark.parametrize("dtype,d,fused", [(torch.float32, 96, True), (torch.float32, 1025, False), (torch.float64, 256, True),
                                           (torch.float64, 257, False)])
def test_mifid_cosine_distance_route(monkeypatch, dtype, d, fused):
    """``_rowmax_fused_wins`` decides; here the op is seen called (or not) on either side of the fp32 and fp64 depth
    limits, and both sides equal the host composition."""
    from torchmetrics_forked_amd.image.generative import _compute_cosine_distance

    calls = count_calls(monkeypatch, torch.ops.tmx, "pairwise_abs_cos_rowmax")
    g = torch.Generator().manual_seed(d)
    a = torch.randn(300, d, generator=g, dtype=dtype)
    b = a[:200] + 0.05 * torch.randn(200, d, generator=g, dtype=dtype)  # near-duplicates: a small distance
    got = _compute_cosine_distance(a.cuda(), b.cuda(), 0.5).cpu()
    assert len(calls) == int(fused)
    torch.testing.assert_close(got, _compute_cosine_distance(a, b, 0.5), rtol=1e-5, atol=1e-6)  # (test_mifid_cosine_distance_fused_matches_cpu's)
