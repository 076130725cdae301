"""Native UQI (``tmx::uqi_sums`` / ``tmx::uqi_band_pair_sums``, ``csrc/uqi.hip``) against the dense-window fp64 oracle of
``tests/helpers/uqi_oracle.py``, and the routes of ``universal_image_quality_index`` and ``spectral_distortion_index``.

Value rule (``vif_oracle.value_rule``), as a maximum over the plane pairs of a case:
``|native − oracle64| <= 4 |comp32 − oracle64| + 1e-6 max|oracle64|`` with ``comp32`` the same oracle in fp32 on the CPU (per-window
values added in fp64).  Inputs are ``vif_oracle.noisy_pair``: every window's variance is far above ``eps``.  Every comparison
prints one ``vif_err`` line (``-s`` shows them).

Planes per case.  The rule compares two rounding errors of the same class, so with one plane a single draw of the composition's
error is below a quarter of an equally distributed native one about one time in six, for any correct fp32 kernel
(``tests/test_vif_gpu.py`` has the argument).  Every tolerance case therefore has seven planes (six at the largest shape), and a
one-plane call is held to more than the rule: bit equality with its plane of the batch.

Scalars (the functionals' and modules' results) are held to the rule propagated through the mean: a mean of per-plane sums
divided by the window count errs by at most the largest per-plane error divided by the windows per plane, so the bound is
the rule's bound over the planes divided by that count; the result's own fp32 rounding (2^-24 relative) is inside the 1e-6
term.  D-lambda is ``(mean |t_ij − p_ij|^p)^(1/p)``, a norm of the matrix difference that the maximum norm bounds, so its error is
at most the largest entry error of the target matrix plus that of the preds matrix: the sum of the two matrices' bounds.

A constant non-zero plane is left out on purpose: its variance is rounding noise against ``eps`` in any arithmetic, and no rule
can hold it.

Measured on MI355X, error / bound: per-pair sums 0.013 to 0.29 (median 0.13, 35 comparisons), the functionals' and modules'
scalars at most 0.17, D-lambda at most 0.007.

Mutants of the op, built one at a time outside the tree, and the tests that catch each (the unchanged source built the same
way passes in full; the mutants are of ``uqi_pair_kernel`` and the host code, ``uqi_pair_v2_kernel`` is held to bit equality with
that kernel below):
* first output row one early (the row guard's ``<=`` for ``<``): 33 tests, ``test_value_rule_default_window[7x11x11]`` first;
* column guard ``<=`` for ``<``: 32 tests, the same first;
* strip count floored: ``test_value_rule_default_window[7x75x14]``, ``[6x150x131]`` and ``test_value_rule_scale_255[6x150x131]``;
* column-block count floored: ``test_value_rule_default_window[7x13x267]`` and 10 more (every shape wider than one block);
* band row of the pair decode one less, and image / pair order of the result swapped: ``test_band_pairs``,
  ``test_more_band_pairs_than_a_grid_axis_of_65535``, ``test_channel_sliced_batch``, the three D-lambda value tests and
  ``test_bad_plane_stays_in_its_plane``;
* ``wy`` and ``wx`` swapped: both cases of ``test_unequal_sigmas_on_a_non_square_plane``, and nothing else;
* ``eps`` dropped: 18 tests, ``test_fp16_inputs_with_the_fp16_eps`` among them (the fp32 ``eps`` is 1e-5 of these windows' variance
  and shows under the rule too; a hard-coded fp32 ``eps`` shows only in the fp16 test).
Swapping ``a`` and ``b`` is no mutant: UQI is symmetric in its two planes.
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import uqi_oracle as uo
from tests.helpers import vif_oracle as vo
from tests.helpers.routes import assert_route, count_calls, kernels_run
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu

KS, SIGMA = (11, 11), (1.5, 1.5)
EPS32 = torch.finfo(torch.float32).eps
R, C = 64, 256  # asserted against uqi_tile() below: parametrisation happens before the library is loaded


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _windows(kernel_size, sigma):
    from torchmetrics_forked_amd.functional.image.uqi import _uqi_windows

    return _uqi_windows(kernel_size, sigma, torch.device("cuda"))


def _sums(p, t, kernel_size=KS, sigma=SIGMA, eps=EPS32):
    from torchmetrics_forked_amd.ops.image import uqi_sums

    wy, wx = _windows(kernel_size, sigma)
    return uqi_sums(p, t, wy, wx, eps)


def _band_sums(x, kernel_size=KS, sigma=SIGMA, eps=EPS32):
    from torchmetrics_forked_amd.ops.image import uqi_band_pair_sums

    wy, wx = _windows(kernel_size, sigma)
    return uqi_band_pair_sums(x, wy, wx, eps)


@functools.lru_cache(maxsize=None)
def _case(shape, scale=1.0, kernel_size=KS, sigma=SIGMA, eps=EPS32):
    """(preds, target, oracle64, comp32) of one noisy ``[P, H, W]`` case, computed once."""
    p, t = vo.noisy_pair(shape, 1000 * shape[0] + 7 * shape[1] + shape[2], scale)
    return p, t, uo.uqi_sums(p, t, kernel_size, sigma, eps), uo.uqi_sums(p, t, kernel_size, sigma, eps, torch.float32)


def _check(label, sums, o64, c32):
    assert sums.shape == o64.shape and sums.dtype == torch.float64
    return vo.value_rule(label, sums, o64, c32)


def _mean_rule(label, got, o64, c32, windows_per_plane):
    """The value rule propagated through the mean over planes and windows (module docstring)."""
    want = o64.sum() / (o64.numel() * windows_per_plane)
    bound = (4 * (c32 - o64).abs().max() + 1e-6 * o64.abs().max()) / windows_per_plane
    err = abs(float(got.detach().double().cpu() - want))
    print(f'vif_err {{"case": "{label}", "ratio": {err / float(bound)}, "err": {err}, "bound": {float(bound)}}}')
    assert err <= float(bound), (label, err, float(bound))


def _check_bands(label, got, o64, c32):
    """Band results ``[npairs, B]``: the rule as a maximum over all entries (``B`` alone may be two or three draws)."""
    assert got.shape == o64.shape and got.dtype == torch.float64
    return vo.value_rule(label, got.flatten(), o64.flatten(), c32.flatten())


def _ids(s):
    return "x".join(map(str, s))


def test_tile_is_what_the_shapes_assume():
    from torchmetrics_forked_amd.ops.image import uqi_tile

    assert uqi_tile() == (R, C)


# ---------------------------------------------------------------------------------------------------- cases 1 and 2
_SHAPES = [(7, 11, 11), (7, 12, 13), (7, 13, 12), (6, 150, 131)]
_EDGES = [(7, 13, C - 1 + 10), (7, 13, C + 10), (7, 13, C + 1 + 10), (7, R - 1 + 10, 14), (7, R + 10, 14), (7, R + 1 + 10, 14)]


@pytest.mark.parametrize("shape", _SHAPES + _EDGES, ids=_ids)
def test_value_rule_default_window(shape):
    p, t, o64, c32 = _case(shape)
    _check(f"{shape}", _sums(p.cuda(), t.cuda()), o64, c32)


@pytest.mark.parametrize("shape", [(7, 12, 13), (6, 150, 131), (7, 13, C + 1 + 10)], ids=_ids)
def test_value_rule_scale_255(shape):
    p, t, o64, c32 = _case(shape, 255.0)
    _check(f"{shape}@255", _sums(p.cuda(), t.cuda()), o64, c32)


# ----------------------------------------------------------------------------------------------------------- case 3
@pytest.mark.parametrize("scale", [1.0, 255.0])
@pytest.mark.parametrize("ks", [3, 7, 15])
def test_value_rule_other_windows(ks, scale):
    for shape in [(7, ks, ks), (7, ks + 3, C + ks)]:
        p, t, o64, c32 = _case(shape, scale, (ks, ks))
        _check(f"ks{ks}/{shape}@{scale}", _sums(p.cuda(), t.cuda(), (ks, ks)), o64, c32)


@pytest.mark.parametrize("sigma", [(0.8, 1.5), (1.5, 0.8)])
def test_unequal_sigmas_on_a_non_square_plane(sigma):
    """``wy`` weighs H and ``wx`` weighs W: swapped, the sums move by far more than the bound (asserted on the oracle)."""
    shape = (7, 10, C + 7)
    p, t, o64, c32 = _case(shape, 1.0, (7, 7), sigma)
    swapped = uo.uqi_sums(p, t, (7, 7), sigma[::-1], EPS32)
    bound = 4 * (c32 - o64).abs().max() + 1e-6 * o64.abs().max()
    assert float((swapped - o64).abs().min()) > 100 * float(bound)
    _check(f"sigma{sigma}", _sums(p.cuda(), t.cuda(), (7, 7), sigma), o64, c32)


# ----------------------------------------------------------------------------------------------------------- case 4
@pytest.mark.parametrize("shape", [(7, 11, 11), (7, 13, C + 1 + 10), (7, R + 1 + 10, 14), (6, 150, 131)], ids=_ids)
def test_one_plane_is_bit_equal_to_its_plane_of_the_batch(shape):
    p, t, _, _ = _case(shape)
    pd, td = p.cuda(), t.cuda()
    whole = _sums(pd, td)
    for i in (0, shape[0] - 1):
        one = _sums(pd[i:i + 1], td[i:i + 1])
        assert one.shape == (1,) and torch.equal(one, whole[i:i + 1])


def test_deterministic():
    p, t, _, _ = _case((6, 150, 131))
    pd, td = p.cuda(), t.cuda()
    assert torch.equal(_sums(pd, td), _sums(pd, td))
    x = _bands((3, 5, 40, 45), 31).cuda()
    assert torch.equal(_band_sums(x), _band_sums(x))


def _offset_1(x):
    """The same values at storage offset 1: not 16-byte aligned."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.storage_offset() == 1 and view.data_ptr() % 16 != 0
    return view


@pytest.mark.parametrize("ks", [3, 7, 11, 15])
def test_fast_kernel_is_bit_equal_to_the_generic_kernel(ks):
    """fp32 planes with ``W % 4 == 0`` at a 16-byte aligned address take ``uqi_pair_v2_kernel``; the same values one element off
    take ``uqi_pair_kernel``, which the value-rule cases hold to the oracle.  Same windows, same arithmetic, same order: the
    two must agree to the bit.  Two column blocks, two strips, a last group of fewer than KS rows."""
    p, t = vo.noisy_pair((3, R + ks + 2, C + ks + 1 + (-(C + ks + 1)) % 4), 70 + ks, 1.0)
    assert p.shape[-1] % 4 == 0 and p.shape[-1] - ks + 1 > C and p.shape[-2] - ks + 1 > R
    pd, td = p.cuda(), t.cuda()
    assert pd.data_ptr() % 16 == 0 and td.data_ptr() % 16 == 0
    fast, generic = _sums(pd, td, (ks, ks)), _sums(_offset_1(pd), _offset_1(td), (ks, ks))
    assert torch.equal(fast, generic)
    names = kernels_run(lambda: _sums(pd, td, (ks, ks)))
    assert_route(names, present=("uqi_pair_v2_kernel",), absent=("uqi_pair_kernel",))
    po, to = _offset_1(pd), _offset_1(td)
    names = kernels_run(lambda: _sums(po, to, (ks, ks)))
    assert_route(names, present=("uqi_pair_kernel",), absent=("uqi_pair_v2_kernel",))
    x = _bands((2, 4, 30, 44), 80 + ks).cuda()
    assert torch.equal(_band_sums(x, (ks, ks)), _band_sums(_offset_1(x), (ks, ks)))
    names = kernels_run(lambda: _band_sums(x, (ks, ks)))
    assert_route(names, present=("uqi_pair_v2_kernel",), absent=("uqi_pair_kernel",))


# ----------------------------------------------------------------------------------------------------------- case 5
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_inputs_convert_on_load(dtype):
    p, t = vo.noisy_pair((3, 70, 45), 16, 1.0)
    p16, t16 = p.to(dtype).cuda(), t.to(dtype).cuda()
    eps = torch.finfo(dtype).eps
    assert torch.equal(_sums(p16, t16, eps=eps), _sums(p16.float(), t16.float(), eps=eps))
    x16 = _bands((2, 3, 30, 41), 17).to(dtype).cuda()
    assert torch.equal(_band_sums(x16, eps=eps), _band_sums(x16.float(), eps=eps))


def test_fp16_inputs_with_the_fp16_eps():
    """``eps`` = ``finfo(fp16).eps`` = 2^-10 is a tenth of these windows' variance: dropped or replaced by the fp32 constant, the
    sums move by percents (asserted on the oracle), far more than the fp32 ``eps`` does."""
    eps = torch.finfo(torch.float16).eps
    p, t = vo.noisy_pair((7, 40, 45), 18, 1.0)
    p16, t16 = p.half(), t.half()
    o64, c32 = uo.uqi_sums(p16.float(), t16.float(), KS, SIGMA, eps), uo.uqi_sums(p16.float(), t16.float(), KS, SIGMA, eps, torch.float32)
    other = uo.uqi_sums(p16.float(), t16.float(), KS, SIGMA, EPS32)
    assert float(((other - o64).abs() / o64.abs()).min()) > 0.01
    _check("fp16-eps", _sums(p16.cuda(), t16.cuda(), eps=eps), o64, c32)
    # the functional passes that eps for fp16 inputs; its result is rounded to fp16 (half an ulp: 2^-11 relative)
    from torchmetrics_forked_amd.functional.image.uqi import universal_image_quality_index

    b = 7 * 30 * 35
    got = universal_image_quality_index(p16.cuda()[:, None], t16.cuda()[:, None])
    assert got.dtype == torch.float16
    want = float(o64.sum() / b)
    bound = float(4 * (c32 - o64).abs().max() + 1e-6 * o64.abs().max()) / (30 * 35)
    assert abs(float(got) - want) <= 2.0**-11 * abs(want) + bound
    assert abs(float(other.sum() / b) - want) > 10 * (2.0**-11 * abs(want) + bound)  # the fp32 eps would not pass


# ----------------------------------------------------------------------------------------------------------- case 6
def test_unaligned_storage_offset():
    p, t, o64, c32 = _case((7, 13, C + 1 + 10))

    _check("offset-1", _sums(_offset_1(p.cuda()), _offset_1(t.cuda())), o64, c32)


def _batch(shape, seed, scale=1.0):
    """[B, C, H, W] noisy batch whose planes differ in their noise level, so that every plane has its own sum."""
    p, t = vo.noisy_pair(shape, seed, scale)
    b, c = shape[:2]
    k = torch.linspace(0.4, 2.0, b * c).reshape(b, c, 1, 1)
    return (t + k * (p - t)).contiguous(), t


def _bands(shape, seed, scale=1.0):
    """[B, L, H, W] whose bands share a scene and differ in how much independent noise they carry: every band pair of every
    image has its own UQI."""
    p, t = vo.noisy_pair(shape, seed, scale)
    b, length = shape[:2]
    k = torch.linspace(0.3, 2.5, b * length).reshape(b, length, 1, 1)
    return (t[:, :1] + k * (p - t)).contiguous()


def _plane_oracles(p, t, kernel_size=KS, sigma=SIGMA, eps=EPS32):
    b, c, h, w = p.shape
    pp, tt = p.reshape(b * c, h, w), t.reshape(b * c, h, w)
    return uo.uqi_sums(pp, tt, kernel_size, sigma, eps), uo.uqi_sums(pp, tt, kernel_size, sigma, eps, torch.float32)


def test_planes_in_batch_channel_order():
    p, t = _batch((2, 3, 24, 29), 22)
    o64, c32 = _plane_oracles(p, t)
    srt = o64.sort().values
    assert float((srt[1:] - srt[:-1]).min()) > 1e3 * float(4 * (c32 - o64).abs().max())  # distinct planes: a wrong order shows
    _check("b-c-order", _sums(p.cuda().view(6, 24, 29), t.cuda().view(6, 24, 29)), o64, c32)


def test_channel_sliced_batch():
    from torchmetrics_forked_amd.functional.image.uqi import universal_image_quality_index

    p, t = _batch((2, 4, 24, 29), 21)
    pv, tv = p.cuda()[:, 1:3], t.cuda()[:, 1:3]
    assert not pv.is_contiguous()
    o64, c32 = _plane_oracles(p[:, 1:3], t[:, 1:3])
    _check("channel-slice/op", _sums(pv.reshape(4, 24, 29), tv.reshape(4, 24, 29)), o64, c32)
    _mean_rule("channel-slice/functional", universal_image_quality_index(pv, tv), o64, c32, 14 * 19)
    # the band op on a non-contiguous view against its gathered oracle
    x = _bands((2, 5, 24, 29), 23)
    xo64, xc32 = uo.band_pair_sums(x[:, 1:4], KS, SIGMA, EPS32), uo.band_pair_sums(x[:, 1:4], KS, SIGMA, EPS32, torch.float32)
    _check_bands("channel-slice/bands", _band_sums(x.cuda()[:, 1:4]), xo64, xc32)


# ---------------------------------------------------------------------------------------------------- cases 7 and 8
def test_band_pairs():
    x = _bands((3, 5, 40, 45), 31)
    o64, c32 = uo.band_pair_sums(x, KS, SIGMA, EPS32), uo.band_pair_sums(x, KS, SIGMA, EPS32, torch.float32)
    assert o64.shape == (10, 3)
    srt = o64.flatten().sort().values
    bound = float(4 * (c32 - o64).abs().max() + 1e-6 * o64.abs().max())
    assert float((srt[1:] - srt[:-1]).min()) > 10 * bound  # distinct entries: a wrong (i, j) decode or b / pair order shows
    _check_bands("bands-3x5", _band_sums(x.cuda()), o64, c32)


def test_band_pairs_two_bands_and_one_band():
    x = _bands((7, 2, 20, 23), 32)
    o64, c32 = uo.band_pair_sums(x, KS, SIGMA, EPS32), uo.band_pair_sums(x, KS, SIGMA, EPS32, torch.float32)
    _check_bands("bands-L2", _band_sums(x.cuda()), o64, c32)
    # L = 2 is the identity pairing of band 0 with band 1
    assert torch.equal(_band_sums(x.cuda())[0], _sums(x.cuda()[:, 0].contiguous(), x.cuda()[:, 1].contiguous()))
    names = kernels_run(lambda: _band_sums(x.cuda()[:, :1]))  # (the upload and the windows do launch: the profile is not empty)
    one = _band_sums(x.cuda()[:, :1])
    assert one.shape == (0, 7) and one.dtype == torch.float64
    assert not any("uqi_pair_" in n for n in names), names


def test_more_band_pairs_than_a_grid_axis_of_65535():
    x = _bands((70, 44, 11, 11), 33)
    assert 70 * 44 * 43 // 2 == 66220
    o64, c32 = uo.band_pair_sums(x, KS, SIGMA, EPS32), uo.band_pair_sums(x, KS, SIGMA, EPS32, torch.float32)
    got = _band_sums(x.cuda())
    assert got.shape == (946, 70)
    _check("bands-66220", got, o64, c32)


# ----------------------------------------------------------------------------------------------------------- case 9
def _d_lambda_oracle(preds, target, p, dtype):
    b, length, h, w = preds.shape
    count = b * (h - 10) * (w - 10)
    mp = uo.band_matrix(uo.band_pair_sums(preds, KS, SIGMA, EPS32, dtype), length, count)
    mt = uo.band_matrix(uo.band_pair_sums(target, KS, SIGMA, EPS32, dtype), length, count)
    return mp, mt


def _d_lambda_check(label, got, preds, target, p):
    (mp, mt), (mp32, mt32) = _d_lambda_oracle(preds, target, p, torch.float64), _d_lambda_oracle(preds, target, p, torch.float32)
    want = uo.d_lambda(mp, mt, p)
    # the sum of the two matrices' value-rule bounds (module docstring)
    bound = sum(float(4 * (c - o).abs().max() + 1e-6 * o.abs().max()) for o, c in ((mp, mp32), (mt, mt32)))
    err = abs(float(got.detach().double().cpu() - want))
    print(f'vif_err {{"case": "{label}", "ratio": {err / bound}, "err": {err}, "bound": {bound}}}')
    assert float(want) > 1e3 * bound  # the index itself is far above the bound: the check is not vacuous
    assert err <= bound, (label, err, bound)


@pytest.mark.parametrize("p", [1, 2])
def test_spectral_distortion_index(p):
    from torchmetrics_forked_amd.functional.image.d_lambda import spectral_distortion_index

    preds, target = _bands((3, 4, 30, 33), 41), _bands((3, 4, 30, 33), 42).flip(1)
    got = spectral_distortion_index(preds.cuda(), target.cuda(), p=p)
    assert got.dtype == torch.float32 and got.is_cuda and got.dim() == 0
    _d_lambda_check(f"d_lambda-p{p}", got, preds, target, p)


def test_spectral_distortion_module_two_updates_of_different_batch_sizes():
    from torchmetrics_forked_amd.image import SpectralDistortionIndex

    preds, target = _bands((5, 4, 30, 33), 43), _bands((5, 4, 30, 33), 44).flip(1)
    metric = SpectralDistortionIndex().cuda()
    metric.update(preds[:2].cuda(), target[:2].cuda())
    metric.update(preds[2:].cuda(), target[2:].cuda())
    _d_lambda_check("d_lambda-module", metric.compute(), preds, target, 1)


# ---------------------------------------------------------------------------------------------------------- case 10
@pytest.mark.parametrize("bad", ["zero", float("nan"), float("inf")])
def test_bad_plane_stays_in_its_plane(bad):
    p, t, _, _ = _case((7, 30, 35))
    pd, td = p.cuda().clone(), t.cuda().clone()
    clean = _sums(pd, td)
    if bad == "zero":  # 0 / 0, as the reference gives
        pd[3] = 0.0
        td[3] = 0.0
    else:
        pd[3, 20, 30] = bad
    got = _sums(pd, td)
    keep = [0, 1, 2, 4, 5, 6]
    assert torch.isnan(got[3]) and torch.equal(got[keep], clean[keep])
    # band pairing: a bad band spoils exactly the pairs that hold it
    x = _bands((2, 4, 30, 35), 51).cuda()
    clean = _band_sums(x)
    if bad == "zero":
        x[1, 2] = 0.0
        x[1, 0] = 0.0
        spoiled = [(1, 1)]  # pair index 1 = bands (0, 2): both planes zero
    else:
        x[1, 2, 5, 6] = bad
        spoiled = [(1, 1), (3, 1), (5, 1)]  # pairs (0, 2), (1, 2), (2, 3) of image 1
    got = _band_sums(x)
    mask = torch.zeros(6, 2, dtype=torch.bool)
    for k, n in spoiled:
        mask[k, n] = True
    assert bool(torch.isnan(got.cpu()[mask]).all())
    if bad == "zero":  # the pairs with one zero band are finite but changed: only image 0 is untouched
        assert torch.equal(got[:, 0], clean[:, 0])
    else:
        assert torch.equal(got.cpu()[~mask], clean.cpu()[~mask])


# ---------------------------------------------------------------------------------------------------------- case 11
def _raise_conv(*a, **k):
    raise AssertionError("the composition ran: conv2d called on the native route")


def _raise_native(*a, **k):
    raise AssertionError("the native UQI op was entered on a kept route")


def _no_conv(monkeypatch, uqi_mod):
    monkeypatch.setattr(uqi_mod, "F", types.SimpleNamespace(conv2d=_raise_conv, pad=F.pad))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_functional_and_module_take_the_native_route(dtype, monkeypatch):
    import torchmetrics_forked_amd.functional.image.uqi as uqi_mod
    from torchmetrics_forked_amd.image import UniversalImageQualityIndex

    p, t = _batch((2, 3, 24, 29), 61)
    p, t = p.to(dtype), t.to(dtype)
    o64, c32 = _plane_oracles(p.float(), t.float(), eps=torch.finfo(dtype).eps)  # oracle of the rounded inputs
    _no_conv(monkeypatch, uqi_mod)
    calls = count_calls(monkeypatch, uqi_mod, "_uqi_sums")
    got = uqi_mod.universal_image_quality_index(p.cuda(), t.cuda())
    total = uqi_mod.universal_image_quality_index(p.cuda(), t.cuda(), reduction="sum")
    metric = UniversalImageQualityIndex().cuda()
    metric.update(p[:1].cuda(), t[:1].cuda())
    metric.update(p[1:].cuda(), t[1:].cuda())
    assert len(calls) == 4 and got.dtype == dtype and got.is_cuda and got.dim() == 0
    if dtype == torch.float32:
        _mean_rule("functional", got, o64, c32, 14 * 19)
        _mean_rule("functional-sum", total / (6 * 14 * 19), o64, c32, 14 * 19)
        _mean_rule("module", metric.compute(), o64, c32, 14 * 19)
    else:
        # results (below 1 in magnitude as means) are rounded to bf16 on return: half an ulp, 2^-9 relative; the module adds two
        # such rounded sums in fp32
        want = float(o64.sum() / (6 * 14 * 19))
        assert abs(float(got) - want) <= 2.0**-8 * abs(want)
        assert abs(float(metric.compute()) - want) <= 2.0**-8 * abs(want)


def test_d_lambda_takes_the_native_route(monkeypatch):
    import torchmetrics_forked_amd.functional.image.d_lambda as dl_mod
    import torchmetrics_forked_amd.functional.image.uqi as uqi_mod

    preds, target = _bands((2, 3, 24, 29), 62), _bands((2, 3, 24, 29), 63)
    _no_conv(monkeypatch, uqi_mod)
    calls = count_calls(monkeypatch, dl_mod, "_uqi_band_pair_sums")
    out = dl_mod.spectral_distortion_index(preds.cuda(), target.cuda())
    assert len(calls) == 2 and bool(torch.isfinite(out))


def test_kept_routes_never_reach_the_op(monkeypatch):
    import torchmetrics_forked_amd.functional.image.d_lambda as dl_mod
    import torchmetrics_forked_amd.functional.image.uqi as uqi_mod

    monkeypatch.setattr(uqi_mod, "_uqi_sums", _raise_native)
    monkeypatch.setattr(dl_mod, "_uqi_band_pair_sums", _raise_native)
    uqi = uqi_mod.universal_image_quality_index
    p, t = _batch((1, 2, 40, 45), 64)
    o64, _ = _plane_oracles(p, t)
    want = float(o64.sum() / (2 * 30 * 35))
    pg = p.cuda().requires_grad_()
    out = uqi(pg, t.cuda())
    out.backward()
    assert pg.grad is not None and bool(torch.isfinite(pg.grad).all())
    assert abs(float(out.detach()) - want) <= 1e-4  # the fp32 composition on the GPU
    out64 = uqi(p.double().cuda(), t.double().cuda())
    want64 = float(_plane_oracles(p, t, eps=torch.finfo(torch.float64).eps)[0].sum() / (2 * 30 * 35))  # fp64 inputs: fp64's eps
    assert out64.dtype == torch.float64 and abs(float(out64) - want64) <= 1e-9
    assert abs(float(uqi(p, t)) - want) <= 1e-4  # CPU
    full = uqi(p.cuda(), t.cuda(), reduction="none")
    assert full.shape == (1, 2, 30, 35) and abs(float(full.mean()) - want) <= 1e-4
    assert bool(torch.isfinite(uqi(p.cuda(), t.cuda(), kernel_size=(11, 7))))
    o17, _ = _plane_oracles(p, t, (17, 17))
    assert abs(float(uqi(p.cuda(), t.cuda(), kernel_size=(17, 17))) - float(o17.sum() / (2 * 24 * 29))) <= 1e-4
    x = _bands((2, 3, 24, 29), 65)
    assert bool(torch.isfinite(dl_mod.spectral_distortion_index(x.double().cuda(), x.flip(1).double().cuda())))
    with pytest.raises(AssertionError, match="kept route"):  # the guards themselves are live
        uqi(p.cuda(), t.cuda())
    with pytest.raises(AssertionError, match="kept route"):
        dl_mod.spectral_distortion_index(x.cuda(), x.flip(1).cuda())


_CONV_MARKS = ("conv", "Conv", "Cijk", "Im2", "im2col", "igemm", "miopen", "MIOpen")


def test_kernels_run():
    import torchmetrics_forked_amd.functional.image.d_lambda as dl_mod
    import torchmetrics_forked_amd.functional.image.uqi as uqi_mod

    p, t = _batch((2, 3, 24, 29), 66)
    pd, td = p.cuda(), t.cuda()
    names = kernels_run(lambda: uqi_mod.universal_image_quality_index(pd, td))
    print("uqi_kernels " + repr(sorted(set(names))))
    assert_route(names, present=("uqi_pair_",), absent=_CONV_MARKS)
    assert sum("uqi_pair_" in n for n in names) == 1
    names = kernels_run(lambda: dl_mod.spectral_distortion_index(pd, td))
    print("d_lambda_kernels " + repr(sorted(set(names))))
    assert_route(names, present=("uqi_pair_",), absent=_CONV_MARKS)
    assert sum("uqi_pair_" in n for n in names) == 2
    # the composition does show a convolution kernel under one of these marks: the absence above is not vacuous
    comp = kernels_run(lambda: uqi_mod.universal_image_quality_index(pd, td, reduction="none"))
    print("uqi_composition_kernels " + repr(sorted(set(comp))))
    assert any(m in n for n in comp for m in _CONV_MARKS), sorted(set(comp))
    assert not any("uqi_pair_" in n for n in comp)


# ---------------------------------------------------------------------------------------------------------- case 12
def test_no_host_read(monkeypatch):
    import torchmetrics_forked_amd.functional.image.d_lambda as dl_mod
    import torchmetrics_forked_amd.functional.image.uqi as uqi_mod

    p, t = _batch((2, 3, 24, 29), 67)
    pd, td = p.cuda(), t.cuda()
    want = uqi_mod.universal_image_quality_index(pd, td)  # (first calls outside the guarded region)
    want_dl = dl_mod.spectral_distortion_index(pd, td)
    _no_conv(monkeypatch, uqi_mod)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = uqi_mod.universal_image_quality_index(pd, td)
        got_dl = dl_mod.spectral_distortion_index(pd, td)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(got, want) and torch.equal(got_dl, want_dl)
