"""Native sliding-window RMSE and RASE (``tmx::box_rmse_maps`` / ``tmx::rase_fold``, ``csrc/box_window.hip``) against the dense fp64
oracle of ``tests/helpers/box_oracle.py``, and the routes of ``root_mean_squared_error_using_sliding_window`` and
``relative_average_spectral_error``.

Value rule (``vif_oracle.value_rule``): ``|native − oracle64| <= 4 |comp32 − oracle64| + 1e-6 max|oracle64|`` with ``comp32`` the same oracle
in fp32 on the CPU, taken as a maximum over all entries of a map and over the seven channels for ``crop_sums``.  Inputs are
``vif_oracle.noisy_pair``.  Every tolerance case has seven channels: with one scalar a single draw of the composition's error
is below a quarter of an equally distributed native one about one time in six for any correct fp32 kernel
(``tests/test_vif_gpu.py`` has the argument).  Scalars (the functionals' and modules' results) are held to the rule as a vector
over seven seeds; their own fp32 rounding (2^-24 relative) is inside the 1e-6 term.  Every comparison prints one ``vif_err``
line (``-s`` shows them).

``rase_fold`` computes in fp64 from fp32 maps, so it is held to 1e-6 relative (the rule's floor term) against the fp64 oracle
evaluated on the same fp32 maps.

What is held to more than the rule: two runs are bit-equal; a batch map is bit-equal to the fp32 sum of the one-image maps
taken in the op's documented order (images of a chunk in order, then the chunks in order, ``box_batch_chunks``); the
outputs shared by ``with_target_mean`` on and off are bit-equal; 16-bit inputs give the bits of their up-cast; identical images
give exact zeros; a NaN stays inside its channel and its window's reach.

Measured on MI355X, error / bound: RMSE maps 0.041 to 0.11 (median 0.058, 44 comparisons), cropped sums at most 0.048,
target-mean maps at most 0.16, the functionals' and modules' scalars at most 0.065, the returned and the module's maps 0.08
(an fp32 emulation of the specified arithmetic on the CPU gave at most 0.092 for the maps).

Mutants of the op, built one at a time outside the tree, and the tests that catch each (the unchanged source built the same
way passes in full):
* reflection ``−k -> k``: 44 tests, ``test_smallest_plane[2-1.0]`` first;
* window shifted back by one at even sizes (back pad one longer): 26, every case with window 2, 8 or 16;
* ``crop`` as ``ws // 2``: 18, every case with window 3, 7 or 15 (the banker's-rounding entries that differ);
* crop guard ``<=`` for ``<``: 44, ``test_smallest_plane[2-1.0]`` first;
* square root after the sum: 44, the same first;
* ``target_mean`` divided by ``ws²`` once: 43, every case that checks ``target_mean``;
* strip count floored: 19, ``test_tile_edges[ws8-2x7x33x11]`` first; column-block count floored: 7, ``test_tile_edges[ws8-2x7x9x129]`` first;
* batch-chunk remainder dropped: ``test_batch_chunks_on_the_grid`` and ``test_target_mean_on_and_off``.
"""
import functools

import pytest
import torch

from tests.helpers import box_oracle as bo
from tests.helpers import vif_oracle as vo
from tests.helpers.routes import assert_route, count_calls, kernels_run
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu

R, CW = 32, 128  # asserted against box_tile() below: parametrisation happens before the library is loaded
CH = 7


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _op(p, t, ws, tm=False):
    from torchmetrics_forked_amd.ops.image import box_rmse_maps

    return box_rmse_maps(p, t, ws, bo.crop_of(ws), tm)


@functools.lru_cache(maxsize=None)
def _case(shape, ws, scale=1.0, seed=None):
    """(preds, target, oracle64, comp32) of one noisy ``[B, C, H, W]`` case, computed once."""
    seed = 1000 * shape[0] + 7 * shape[2] + shape[3] + 31 * ws if seed is None else seed
    p, t = vo.noisy_pair(shape, seed, scale)
    return p, t, bo.box_outputs(p, t, ws), bo.box_outputs(p, t, ws, torch.float32)


def _check(label, got, o64, c32, tm=True):
    """The three op outputs under the rule; returns the worst ratio."""
    rmse_map, crop_sums, target_mean = got
    assert rmse_map.dtype == torch.float32 and crop_sums.dtype == torch.float64 and rmse_map.shape == o64[0].shape
    assert crop_sums.shape == o64[1].shape
    worst = vo.value_rule(f"{label}/map", rmse_map.flatten(), o64[0].flatten(), c32[0].flatten())
    worst = max(worst, vo.value_rule(f"{label}/crop", crop_sums, o64[1], c32[1]))
    if tm:
        assert target_mean.dtype == torch.float32 and target_mean.shape == o64[2].shape
        worst = max(worst, vo.value_rule(f"{label}/mean", target_mean.flatten(), o64[2].flatten(), c32[2].flatten()))
    else:
        assert target_mean.numel() == 0
    return worst


def _ids(s):
    return "x".join(map(str, s))


def test_tile_is_what_the_shapes_assume():
    from torchmetrics_forked_amd.ops.image import box_tile

    assert box_tile() == (R, CW)


# ------------------------------------------------------------------------------------------------------ smallest planes
@pytest.mark.parametrize("scale", [1.0, 255.0])
@pytest.mark.parametrize("ws", [2, 3, 5, 7, 8, 15, 16])
def test_smallest_plane(ws, scale):
    """``H = 2 crop + 1``, ``W = 2 crop + 2``: one cropped row, and every window reflects on both sides."""
    c = bo.crop_of(ws)
    shape = (1, CH, 2 * c + 1, 2 * c + 2)
    p, t, o64, c32 = _case(shape, ws, scale)
    _check(f"ws{ws}/{_ids(shape)}@{scale}", _op(p.cuda(), t.cuda(), ws, True), o64, c32)


# ----------------------------------------------------------------------------------------------------------- tile edges
def _edge_shapes(ws):
    c = bo.crop_of(ws)
    rows = [(2, CH, h, 2 * c + 3) for h in (R - 1, R, R + 1, R + 1 + ws)]
    cols = [(2, CH, 2 * c + 1, w) for w in (CW - 1, CW, CW + 1, CW + 1 + ws)]
    return [(ws, s) for s in rows + cols]


@pytest.mark.parametrize("ws,shape", _edge_shapes(8) + _edge_shapes(7), ids=lambda v: _ids(v) if isinstance(v, tuple) else f"ws{v}")
def test_tile_edges(ws, shape):
    p, t, o64, c32 = _case(shape, ws)
    _check(f"ws{ws}/{_ids(shape)}", _op(p.cuda(), t.cuda(), ws, True), o64, c32)


@pytest.mark.parametrize("ws,shape", [(8, (2, CH, R + 1, CW + 1)), (15, (3, CH, 40, 37)), (3, (5, CH, 75, 70))],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else f"ws{v}")
def test_scale_255(ws, shape):
    p, t, o64, c32 = _case(shape, ws, 255.0)
    _check(f"ws{ws}/{_ids(shape)}@255", _op(p.cuda(), t.cuda(), ws, True), o64, c32)


# ---------------------------------------------------------------------------------------------------------- batch sizes
def _sum_in_op_order(p, t, ws, tm):
    """The fp32 sum of the one-image maps in the order the op documents: chunk by chunk, images in order inside a chunk."""
    from torchmetrics_forked_amd.ops.image import box_batch_chunks

    b = p.shape[0]
    chunks = box_batch_chunks(*p.shape)
    per = -(-b // chunks)
    ones = [_op(p[i:i + 1], t[i:i + 1], ws, tm) for i in range(b)]
    out = []
    for k in (0, 2) if tm else (0,):
        total = None
        for c in range(chunks):
            part = None
            for i in range(c * per, min(b, (c + 1) * per)):
                part = ones[i][k] if part is None else part + ones[i][k]
            total = part if total is None else total + part
        out.append(total)
    return out, chunks, per


@pytest.mark.parametrize("b", [1, 2, 5])
def test_batch_sizes(b):
    shape = (b, CH, 40, 37)
    p, t, o64, c32 = _case(shape, 8)
    pd, td = p.cuda(), t.cuda()
    got = _op(pd, td, 8, True)
    _check(f"b{b}", got, o64, c32)
    again = _op(pd, td, 8, True)
    assert all(torch.equal(a, g) for a, g in zip(again, got))
    (want_map, want_mean), _, _ = _sum_in_op_order(pd, td, 8, True)
    assert torch.equal(got[0], want_map) and torch.equal(got[2], want_mean)


def test_batch_chunks_on_the_grid():
    """599 images of a 9 x 10 plane: 7 workgroups per image set, so the batch is split on the grid; the last chunk is short."""
    from torchmetrics_forked_amd.ops.image import box_batch_chunks

    shape = (599, CH, 9, 10)
    p, t, o64, c32 = _case(shape, 8)
    pd, td = p.cuda(), t.cuda()
    got = _op(pd, td, 8, True)
    _check("b599-chunks", got, o64, c32)
    (want_map, want_mean), chunks, per = _sum_in_op_order(pd, td, 8, True)
    assert chunks > 1 and per > 1 and 599 % per != 0, (chunks, per)  # several images per chunk and a remainder
    assert torch.equal(got[0], want_map) and torch.equal(got[2], want_mean)
    again = _op(pd, td, 8, True)
    assert all(torch.equal(a, g) for a, g in zip(again, got))
    # the chunk count is a function of the shape alone, and large planes are not split
    assert box_batch_chunks(*shape) == chunks and box_batch_chunks(4, 3, 4096, 4096) == 1 and box_batch_chunks(1, 1, 9, 10) == 1


def test_target_mean_on_and_off():
    for shape, ws in (((3, CH, 40, 37), 8), ((599, CH, 9, 10), 8), ((2, CH, R + 1, CW + 1), 7)):
        p, t, o64, c32 = _case(shape, ws)
        pd, td = p.cuda(), t.cuda()
        on, off = _op(pd, td, ws, True), _op(pd, td, ws, False)
        assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
        _check(f"tm-off/{_ids(shape)}", off, o64, c32, tm=False)


# --------------------------------------------------------------------------------------------------- dtypes and layouts
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_inputs_convert_on_load(dtype):
    p, t = vo.noisy_pair((3, CH, 40, 37), 16)
    p16, t16 = p.to(dtype), t.to(dtype)
    got = _op(p16.cuda(), t16.cuda(), 8, True)
    up = _op(p16.float().cuda(), t16.float().cuda(), 8, True)
    assert all(torch.equal(a, b) for a, b in zip(got, up))
    _check(f"{dtype}", got, bo.box_outputs(p16.float(), t16.float(), 8), bo.box_outputs(p16.float(), t16.float(), 8, torch.float32))


def test_non_contiguous_inputs():
    p, t = vo.noisy_pair((6, CH + 2, 40, 37), 21)
    pd, td = p.cuda(), t.cuda()
    for label, sl in (("channel-slice", (slice(None), slice(1, CH + 1))), ("batch-stride", (slice(None, None, 2), slice(0, CH)))):
        pv, tv = pd[sl], td[sl]
        assert not pv.is_contiguous()
        _check(label, _op(pv, tv, 8, True), bo.box_outputs(p[sl], t[sl], 8), bo.box_outputs(p[sl], t[sl], 8, torch.float32))


def test_identical_images_give_exact_zeros():
    _, t, _, _ = _case((3, CH, 40, 37), 8)
    td = t.cuda()
    rmse_map, crop_sums, _ = _op(td, td.clone(), 7, True)
    assert not rmse_map.any() and not crop_sums.any()


def test_nan_stays_in_its_channel_and_its_windows_reach():
    """Window 8 covers rows ``y − 4 .. y + 3``: a NaN at row 20, column 15 reaches outputs 17 .. 24 x 12 .. 19 and no others."""
    p, t, _, _ = _case((3, CH, 40, 37), 8)
    pd, td = p.cuda(), t.cuda().clone()
    clean = _op(pd, td, 8, True)
    td[1, 3, 20, 15] = float("nan")
    got = _op(pd, td, 8, True)
    reach = torch.zeros(CH, 40, 37, dtype=torch.bool, device="cuda")
    reach[3, 17:25, 12:20] = True
    for k in (0, 2):
        assert bool(torch.isnan(got[k][reach]).all()) and torch.equal(got[k][~reach], clean[k][~reach])
    keep = [0, 1, 2, 4, 5, 6]
    assert bool(torch.isnan(got[1][3])) and torch.equal(got[1][keep], clean[1][keep])


# ------------------------------------------------------------------------------------------------------------ rase_fold
@pytest.mark.parametrize("ws,shape", [(8, (3, CH, 40, 37)), (7, (2, CH, 9, 10)), (15, (5, 3, 70, 300))],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else f"ws{v}")
def test_rase_fold(ws, shape):
    from torchmetrics_forked_amd.ops.image import rase_fold

    p, t = vo.noisy_pair(shape, 90 + ws, 255.0)
    rmse_map, _, target_mean = _op(p.cuda(), t.cuda(), ws, True)
    for n in (torch.tensor(float(shape[0])), torch.tensor(shape[0])):  # the functional's float and the update's int64 count
        got = rase_fold(rmse_map, target_mean, n.cuda(), bo.crop_of(ws))
        assert got.dtype == torch.float64 and got.is_cuda and got.dim() == 0
        want = bo.rase_from_maps(rmse_map.double().cpu().numpy(), target_mean.double().cpu().numpy(), shape[0], ws)
        assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want)), (float(got), float(want))
    assert float(want) > 0


# ------------------------------------------------------------------------------------------- functionals and modules
def _seven(ws, shape, scale=1.0):
    return [_case(shape, ws, scale, seed=500 + s) for s in range(7)]


@pytest.mark.parametrize("ws,scale", [(8, 1.0), (7, 255.0)])
def test_functionals_and_modules_end_to_end(ws, scale):
    from torchmetrics_forked_amd.functional.image.rase import relative_average_spectral_error
    from torchmetrics_forked_amd.functional.image.rmse_sw import root_mean_squared_error_using_sliding_window as rmse_sw
    from torchmetrics_forked_amd.image import RelativeAverageSpectralError, RootMeanSquaredErrorUsingSlidingWindow

    shape = (5, CH, 40, 37)
    b, c, h, w = shape
    crop = bo.crop_of(ws)
    count = c * (h - 2 * crop) * (w - 2 * crop)
    got = {k: [] for k in ("rmse", "rmse_module", "rase", "rase_module")}
    want64 = {k: [] for k in ("rmse", "rase")}
    want32 = {k: [] for k in ("rmse", "rase")}
    for i, (p, t, o64, c32) in enumerate(_seven(ws, shape, scale)):
        pd, td = p.cuda(), t.cuda()
        val, rmse_map = rmse_sw(pd, td, ws, return_rmse_map=True)
        assert val.dtype == torch.float32 and val.is_cuda and val.dim() == 0 and rmse_map.shape == (c, h, w)
        assert torch.equal(val, rmse_sw(pd, td, ws))
        m1, m2 = RootMeanSquaredErrorUsingSlidingWindow(ws).cuda(), RelativeAverageSpectralError(ws).cuda()
        for m in (m1, m2):  # two unequal batches
            m.update(pd[:2], td[:2])
            m.update(pd[2:], td[2:])
        got["rmse"].append(val)
        got["rmse_module"].append(m1.compute())
        got["rase"].append(relative_average_spectral_error(pd, td, ws))
        got["rase_module"].append(m2.compute())
        want64["rmse"].append(o64[1].sum() / count / b)
        want32["rmse"].append((c32[1].sum() / count).float() / b)
        want64["rase"].append(o64[3])
        want32["rase"].append(c32[3])
        if i == 0:
            vo.value_rule(f"ws{ws}/returned-map", rmse_map.flatten(), o64[0].flatten() / b, c32[0].flatten() / b)
            assert m1.rmse_map.shape == (c, h, w) and m1.rmse_map.dtype == torch.float32
            vo.value_rule(f"ws{ws}/module-map", m1.rmse_map.flatten(), o64[0].flatten(), c32[0].flatten())
    for k, v in got.items():
        o = k.split("_")[0]
        vo.value_rule(f"ws{ws}@{scale}/{k}", torch.stack([x.double().cpu() for x in v]), torch.stack(want64[o]).double(),
                      torch.stack(want32[o]).double())


def test_16_bit_functionals_return_the_input_dtype():
    from torchmetrics_forked_amd.functional.image.rase import relative_average_spectral_error
    from torchmetrics_forked_amd.functional.image.rmse_sw import root_mean_squared_error_using_sliding_window as rmse_sw

    p, t = vo.noisy_pair((3, CH, 40, 37), 77)
    for dtype, rel in ((torch.bfloat16, 2.0**-8), (torch.float16, 2.0**-11)):
        p16, t16 = p.to(dtype), t.to(dtype)
        o64 = bo.box_outputs(p16.float(), t16.float(), 8)
        val, rmse_map = rmse_sw(p16.cuda(), t16.cuda(), return_rmse_map=True)
        rase = relative_average_spectral_error(p16.cuda(), t16.cuda())
        assert val.dtype == dtype and rmse_map.dtype == dtype and rase.dtype == dtype
        want = float(o64[1].sum() / (CH * 32 * 29) / 3)
        # the value and the map are rounded to the input dtype once (half an ulp), then divided by the count (another half)
        assert abs(float(val) - want) <= 2 * rel * want
        assert float((rmse_map.double().cpu() - o64[0] / 3).abs().max()) <= 2 * rel * float(o64[0].max() / 3)
        assert abs(float(rase) - float(o64[3])) <= 4 * rel * float(o64[3])  # two rounded maps and the result's own rounding


# --------------------------------------------------------------------------------------------------------------- routes
_CONV_MARKS = ("conv", "Conv", "Cijk", "Im2", "im2col", "igemm", "miopen", "MIOpen")


def test_kernels_run():
    from torchmetrics_forked_amd.functional.image.rase import relative_average_spectral_error as rase
    from torchmetrics_forked_amd.functional.image.rmse_sw import root_mean_squared_error_using_sliding_window as rmse_sw

    p, t = vo.noisy_pair((2, 3, 40, 37), 66)
    pd, td = p.cuda(), t.cuda()
    names = kernels_run(lambda: rmse_sw(pd, td))
    print("rmse_sw_kernels " + repr(sorted(set(names))))
    assert_route(names, present=("box_rmse_kernel",), absent=_CONV_MARKS)
    assert sum("box_rmse_kernel" in n for n in names) == 1
    names = kernels_run(lambda: rase(pd, td))
    print("rase_kernels " + repr(sorted(set(names))))
    assert_route(names, present=("box_rmse_kernel", "rase_fold_kernel"), absent=_CONV_MARKS)
    assert sum("box_rmse_kernel" in n for n in names) == 1  # one read of the inputs for both maps

    def kept(fn, *args):
        comp = kernels_run(lambda: fn(*args))
        assert any(m in n for n in comp for m in _CONV_MARKS), sorted(set(comp))
        assert not any("box_rmse_kernel" in n or "rase_fold_kernel" in n for n in comp), sorted(set(comp))

    for fn in (rmse_sw, rase):
        kept(fn, pd, td, 1)
        kept(fn, pd, td, 17)
        kept(fn, pd.double(), td.double(), 8)
        kept(fn, pd.clone().requires_grad_(), td, 8)
        kept(fn, pd[:, :, :8], td[:, :, :8], 8)  # H = 2 crop: the crop is empty
        assert bool(torch.isnan(fn(pd[:, :, :8], td[:, :, :8], 8)))  # NaN as before
        assert bool(torch.isfinite(fn(pd[:, :, :9], td[:, :, :9], 8)))


def test_kept_routes_never_reach_the_ops(monkeypatch):
    import torchmetrics_forked_amd.functional.image.rase as rase_mod
    import torchmetrics_forked_amd.functional.image.rmse_sw as rmse_mod

    calls = count_calls(monkeypatch, rmse_mod, "_box_rmse_maps")
    folds = count_calls(monkeypatch, rase_mod, "_rase_fold")
    p, t, o64, _ = _case((3, CH, 40, 37), 8)
    pd, td = p.cuda(), t.cuda()
    want = float(o64[1].sum() / (CH * 32 * 29) / 3)
    pg = pd.clone().requires_grad_()
    out = rmse_mod.root_mean_squared_error_using_sliding_window(pg, td)
    out.backward()
    assert pg.grad is not None and bool(torch.isfinite(pg.grad).all()) and abs(float(out.detach()) - want) <= 1e-5 * want
    out64 = rmse_mod.root_mean_squared_error_using_sliding_window(pd.double(), td.double())
    assert out64.dtype == torch.float64 and abs(float(out64) - want) <= 1e-10 * want
    assert abs(float(rase_mod.relative_average_spectral_error(pd.double(), td.double())) - float(o64[3])) <= 1e-10 * float(o64[3])
    assert abs(float(rmse_mod.root_mean_squared_error_using_sliding_window(p, t)) - want) <= 1e-5 * want  # CPU
    assert not calls and not folds
    rmse_mod.root_mean_squared_error_using_sliding_window(pd, td)
    rase_mod.relative_average_spectral_error(pd, td)
    assert len(calls) == 2 and len(folds) == 1  # the observers themselves are live
    assert calls[0][0][4] is False and calls[1][0][4] is True


def test_no_host_read():
    from torchmetrics_forked_amd.functional.image.rase import relative_average_spectral_error as rase
    from torchmetrics_forked_amd.functional.image.rmse_sw import root_mean_squared_error_using_sliding_window as rmse_sw

    p, t = vo.noisy_pair((2, 3, 40, 37), 67)
    pd, td = p.cuda(), t.cuda()
    want, want_rase = rmse_sw(pd, td, return_rmse_map=True), rase(pd, td)  # (first calls outside the guarded region)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got, got_rase = rmse_sw(pd, td, return_rmse_map=True), rase(pd, td)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got_rase, want_rase)
