"""Native Hausdorff distance (``tmx::hausdorff_index`` / ``tmx::hausdorff_onehot``, ``csrc/hausdorff.hip``) against the brute-force fp64 oracle
of ``tests/helpers/hausdorff_oracle.py``.

Value rule.  Without spacing the kernels are integer up to the final root, so the result is bit-equal to ``float32(sqrt(float64(d²)))`` of
the oracle's integer ``d²`` (to the integer distance for chessboard and taxicab).  With spacing it is within ``4 · 2^-24`` relative of the
fp64 oracle: one fp32 rounding each for the two scaled offsets, their squares, the sum and the root, and the minimum of values with relative
error e has relative error e.  Shapes come from the constants ``hausdorff_tile()`` exports; routes are proven with ``tests/helpers/routes.py``.
"""
import importlib

import numpy as np
import pytest
import torch

from tests.helpers import hausdorff_oracle as ho
from tests.helpers.routes import assert_route, kernels_run

pytestmark = pytest.mark.gpu

COLS, STRIPS, BATCH, ROWS, MAX_W, MAX_H = 64, 8, 4, 4, 2048, 32767  # asserted against hausdorff_tile() below
_KERNELS = ("hausdorff_columns_kernel", "hausdorff_rows_kernel", "hausdorff_finish_kernel")
_METRICS = ("euclidean", "chessboard", "taxicab")


def _hd(p, t, **kw):
    """The functional on boolean [B, C', H, W] arrays (or tensors) as one-hot masks with every channel kept."""
    from torchmetrics_forked_amd.functional.segmentation import hausdorff_distance

    p, t = (torch.as_tensor(x).cuda() for x in (p, t))
    return hausdorff_distance(p, t, p.shape[1], include_background=True, **kw)


def _check(got, p, t, distance_metric="euclidean", spacing=None, directed=False):
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == p.shape[:2]
    got = got.cpu().numpy()
    if spacing is None:
        want = ho.planes(p, t, distance_metric, is_directed=directed, squared=True)
        want = (np.sqrt(want) if distance_metric == "euclidean" else want).astype(np.float32)
        assert np.array_equal(got, want), (got, want)
    else:
        want = ho.planes(p, t, distance_metric, spacing, directed)
        fin = np.isfinite(want)
        assert np.array_equal(got[~fin], want[~fin].astype(np.float32))
        assert np.all(np.abs(got[fin] - want[fin]) <= 4 * 2.0 ** -24 * want[fin]), (got, want)


def test_tile_is_what_the_shapes_assume():
    from torchmetrics_forked_amd import ops
    hd = importlib.import_module("torchmetrics_forked_amd.functional.segmentation.hausdorff_distance")  # (the package exports the function under this name)
    from torchmetrics_forked_amd.ops.segmentation import hausdorff_tile

    ops.require()
    assert hausdorff_tile() == (COLS, STRIPS, BATCH, ROWS, MAX_W, MAX_H)
    assert (hd._HAUSDORFF_MAX_W, hd._HAUSDORFF_MAX_H) == (MAX_W, MAX_H)


# H and W of 1, 2, 3; W around the column block and the wave; H around the strip split (one row per strip, then two), the rows in flight of
# a strip (BATCH - 2, BATCH - 1 rows per strip fill one batch with the two halo rows) and the row groups of kernel 2; several blocks both ways
_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 3), (3, 1), (5, COLS - 1), (5, COLS), (5, COLS + 1), (6, 2 * COLS + 1),
           (STRIPS - 1, 9), (STRIPS, 9), (STRIPS + 1, 9), (STRIPS * (BATCH - 2), 5), (STRIPS * (BATCH - 1), 5), (STRIPS * (BATCH - 1) + 1, 5),
           (STRIPS * 2 * BATCH + 3, COLS + 6)]
_ALL_METRICS_AT = ((3, 3), (5, COLS + 1), (STRIPS + 1, 9), (STRIPS * 2 * BATCH + 3, COLS + 6))


@pytest.mark.parametrize("shape,metric", [(s, m) for s in _SHAPES for m in _METRICS if m == "euclidean" or s in _ALL_METRICS_AT])
def test_blobs_with_planted_corners(shape, metric):
    h, w = shape
    p, t = ho.blobs((2, 2, h, w), 10 * h + w), ho.blobs((2, 2, h, w), 10 * h + w + 1)
    p[0, 0, 0, 0] = t[0, 0, h - 1, w - 1] = True
    _check(_hd(p, t, distance_metric=metric), p, t, metric)


def _planted():
    h, w = 37, 2 * COLS + 22  # not square; three column blocks, the last one partial
    ring, corner_a, corner_b, inner, line, far, small, big, near, one = (np.zeros((h, w), dtype=bool) for _ in range(10))
    ring[[0, -1], :] = ring[:, [0, -1]] = True
    corner_a[0, 0] = corner_b[-1, -1] = inner[5, 70] = True
    line[:, 2] = far[3:9, w - 3] = True
    small[10:14, 10:14] = big[4:30, 4:100] = True
    one[10, 10] = near[12, 10] = near[10, 13] = True  # from (10, 10): two rows away or three columns away
    blob = ho.blobs((h, w), 5)
    return {"corners": (corner_a, corner_b), "pixel_vs_full": (inner, np.ones((h, w), dtype=bool)), "line_vs_far_column": (line, far), "identical": (blob, blob.copy()),
            "subset": (small, big), "borders": (ring | ho.blobs((h, w), 6), ring | ho.blobs((h, w), 7)), "scaled": (one, near)}


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("name", ["corners", "pixel_vs_full", "line_vs_far_column", "identical", "subset", "borders"])
def test_planted_planes(name, directed):
    a, b = _planted()[name]
    p, t = np.stack([a, b])[None], np.stack([b, a])[None]  # both orders, as two planes
    got = _hd(p, t, directed=directed)
    _check(got, p, t, directed=directed)
    assert name != "identical" or not got.any()
    assert not (name == "subset" and directed) or float(got[0, 0]) != float(got[0, 1])


@pytest.mark.parametrize("metric", _METRICS)
@pytest.mark.parametrize("spacing", [(3.0, 1.0), (1.0, 3.0), (0.7, 1.3)])
def test_spacing(spacing, metric):
    a, b = _planted()["scaled"]
    blob_p, blob_t = ho.blobs((1, 2, 37, 2 * COLS + 22), 8), ho.blobs((1, 2, 37, 2 * COLS + 22), 9)
    p, t = np.concatenate([np.stack([a, b])[None], blob_p]), np.concatenate([np.stack([b, a])[None], blob_t])
    _check(_hd(p, t, distance_metric=metric, spacing=spacing), p, t, metric, spacing)
    assert ho.hausdorff(a, b, "euclidean", (3.0, 1.0), True) == 3.0 and ho.hausdorff(a, b, "euclidean", (1.0, 3.0), True) == 2.0  # the nearest changes


@pytest.mark.parametrize("directed", [False, True])
def test_empty_masks_within_a_batch(directed):
    blob, other, none = ho.blobs((1, 9, 70), 3), ho.blobs((1, 9, 70), 4), np.zeros((1, 9, 70), dtype=bool)
    p, t = np.stack([none, blob, none, blob, other]), np.stack([blob, none, none, other, blob])
    got = _hd(p, t, directed=directed)
    _check(got, p, t, directed=directed)
    assert got[:3, 0].tolist() == [float("inf") if not directed else 0.0, float("inf"), 0.0]
    _check(_hd(p, t, directed=directed, spacing=(2.0, 0.5)), p, t, spacing=(2.0, 0.5), directed=directed)


def _labels(dtype=torch.int64):
    """[3, 23, COLS + 9] label maps of three classes with void labels planted: 255, and -1 for the signed types."""
    m = ho.blobs((2, 2, 3, 23, COLS + 9), 12)
    lab = np.where(m[:, 1], 2, np.where(m[:, 0], 1, 0))
    lab[:, :, 4, 5:40] = 255
    lab = torch.from_numpy(lab)
    lab[:, :, 9, 3:30] = -1 if dtype != torch.uint8 else 200
    return lab[0].to(dtype), lab[1].to(dtype)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.int32, torch.int64, torch.bool])
def test_input_forms_and_dtypes(dtype):
    from torchmetrics_forked_amd.functional.segmentation import hausdorff_distance

    index = dtype != torch.bool
    other = {torch.uint8: torch.int64, torch.int16: torch.int32, torch.int32: torch.uint8, torch.int64: torch.int16, torch.bool: torch.int32}[dtype]
    lp, lt = _labels(torch.uint8 if torch.uint8 in (dtype, other) else torch.int64)
    p, t = (np.stack([(x == c).numpy() for c in (1, 2)], axis=1) for x in (lp, lt))  # the kept classes of include_background=False
    kw = {"input_format": "index"} if index else {}
    if index:
        a, b = lp.to(dtype).cuda(), lt.to(other).cuda()
    else:
        onehot = [torch.stack([x == c for c in (0, 1, 2)], dim=1) for x in (lp, lt)]
        a, b = onehot[0].cuda(), (onehot[1].to(other) * 7).cuda()
        _check(hausdorff_distance(a.to(torch.uint8) * 128, b.to(torch.int64) * -3, 3, **kw), p, t)
    _check(hausdorff_distance(a, b, 3, **kw), p, t)
    buf = torch.zeros(a.numel() + 1, dtype=a.dtype, device="cuda")
    buf[1:] = a.reshape(-1)
    wide = torch.zeros(*b.shape[:-1], 2 * b.shape[-1], dtype=b.dtype, device="cuda")
    wide[..., ::2] = b
    assert not wide[..., ::2].is_contiguous()
    _check(hausdorff_distance(buf[1:].view(a.shape), wide[..., ::2], 3, **kw), p, t)  # an offset view and a strided view


def test_more_planes_than_a_grid_axis():
    base_p, base_t = ho.blobs((500, 1, 3, 3), 1, discs=1), ho.blobs((500, 1, 3, 3), 2, discs=1)
    want = np.sqrt(ho.planes(base_p, base_t, squared=True)).astype(np.float32).reshape(250, 2)
    p, t = (np.tile(x.reshape(250, 2, 3, 3), (140, 1, 1, 1)) for x in (base_p, base_t))  # B · C' = 70 000
    got = _hd(p, t).cpu().numpy()
    assert got.shape == (35000, 2) and np.array_equal(got, np.tile(want, (140, 1)))


def test_plane_chunks_and_repeat_runs_are_bit_equal(monkeypatch):
    p, t = ho.blobs((3, 2, 256, 256), 1), ho.blobs((3, 2, 256, 256), 2)  # six planes of 256 KiB of scratch each
    one = _hd(p, t)
    assert sum(_KERNELS[0] in k for k in kernels_run(lambda: _hd(p, t))) == 1
    monkeypatch.setenv("TMX_HAUSDORFF_SCRATCH_MB", "1")
    names = kernels_run(lambda: _hd(p, t))
    assert sum(_KERNELS[0] in k for k in names) == 2 and sum(_KERNELS[1] in k for k in names) == 2
    assert torch.equal(_hd(p, t), one) and torch.equal(_hd(p, t), one) and bool(torch.isfinite(one).all()) and bool((one > 0).all())


def test_routes_and_no_host_read(monkeypatch):
    hd = importlib.import_module("torchmetrics_forked_amd.functional.segmentation.hausdorff_distance")  # (the package exports the function under this name)
    from torchmetrics_forked_amd.segmentation import HausdorffDistance

    p, t = ho.blobs((2, 2, 9, 70), 3), ho.blobs((2, 2, 9, 70), 4)
    assert_route(kernels_run(lambda: _hd(p, t)), present=_KERNELS)
    lp, lt = _labels()
    assert_route(kernels_run(lambda: hd.hausdorff_distance(lp.cuda(), lt.cuda(), 3, input_format="index")), present=_KERNELS, absent=("one_hot", "CompareEq"))
    wide_p, wide_t = np.zeros((1, 1, 2, MAX_W + 1), dtype=bool), np.zeros((1, 1, 2, MAX_W + 1), dtype=bool)
    wide_p[0, 0, 0, 3] = wide_t[0, 0, 1, MAX_W] = True
    assert_route(kernels_run(lambda: _hd(wide_p, wide_t)), absent=("hausdorff_",))  # wider than the LDS rows
    _check(_hd(wide_p, wide_t), wide_p, wide_t)
    module = HausdorffDistance(2, include_background=True).cuda()
    pd, td = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    want = _hd(pd, td)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _hd(pd, td, spacing=(1.0, 1.0)), _hd(pd, td)
        module.update(pd, td)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(got[0], want) and torch.equal(got[1], want)
    assert float(module.compute()) == pytest.approx(float(want.double().mean()), rel=1e-6)
    calls = []
    monkeypatch.setattr(torch.ops.tmx, "hausdorff_onehot", lambda *a: calls.append(a))
    assert torch.equal(hd.hausdorff_distance(torch.from_numpy(p), torch.from_numpy(t), 2, include_background=True), want.cpu()) and not calls  # CPU tensors
    monkeypatch.setattr(hd, "_HAUSDORFF_NATIVE", False)  # what TMX_HAUSDORFF_NATIVE=0 sets at import
    assert_route(kernels_run(lambda: _hd(p, t)), absent=("hausdorff_",))
    assert torch.equal(_hd(p, t), want) and not calls
