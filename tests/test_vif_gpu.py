"""Native VIF-p (``tmx::vif_sums``, ``csrc/vif.hip``) against the dense-window fp64 oracle of ``tests/helpers/vif_oracle.py``.

Value rule (``vif_oracle.value_rule``), per scale, for ``num`` and ``den`` separately and for the final score, as a maximum over
planes: ``|native − oracle64| <= 4 |comp32 − oracle64| + 1e-6 max|oracle64|`` with ``comp32`` the same oracle in fp32 on the CPU.
Tolerance inputs are "noisy" (``vif_oracle.noisy_pair``): every window's variance is far from the 1e-10 mask threshold.  The
branch cases use regions that are exactly zero, where the mask decision is exact in any arithmetic.  Every comparison
prints one ``vif_err`` line (``-s`` shows them).

Planes per case.  The rule compares two rounding errors of the same class (a separable fp32 filter on the GPU, a dense fp32
filter on the CPU), and the deep scales of the small shapes have few windows (one at 41 x 41, scale 3).  With one plane
the maximum over planes is a single draw on either side, and a single draw of the composition's error is below a
quarter of an equally distributed native one about one time in six (``2/pi atan(1/4)``) — for any correct fp32 kernel.
With seven planes both sides are maxima of seven draws and that chance is below 1e-3.  So every tolerance case has
P = 7 (6 at the largest shape), and P = 1 is held to more than the rule: a one-plane call must be bit-equal to that
plane of the seven-plane call (planes are independent and the fold order is fixed).

Measured on MI355X, error / bound: per-scale sums 0.18 to 0.55 (median 0.30), scores at most 0.20, branch and layout
cases at most 0.29.
"""
import functools

import pytest
import torch

from tests.helpers import vif_oracle as vo
from tests.helpers.routes import assert_route, count_calls, kernels_run
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu

SN = 2.0


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _tile():
    from torchmetrics_forked_amd.ops.image import vif_tile

    return vif_tile()


def _sums(p, t, sn=SN):
    from torchmetrics_forked_amd.ops.image import vif_sums

    return vif_sums(p, t, sn)


@functools.lru_cache(maxsize=None)
def _case(shape, scale, sn=SN):
    """(preds, target, oracle64, comp32) of one noisy ``[P, H, W]`` case, computed once."""
    p, t = vo.noisy_pair(shape, 1000 * shape[0] + 7 * shape[1] + shape[2], scale)
    return p, t, vo.vif_scale_sums(p, t, sn), vo.vif_scale_sums(p, t, sn, torch.float32)


def _check(label, sums, o64, c32):
    assert sums.shape == o64.shape and sums.dtype == torch.float64
    vo.value_rule(label, sums, o64, c32)
    vo.value_rule(label + "/score", vo.scores(sums), vo.scores(o64), vo.scores(c32.double()))


def _level1_dim(valid):
    """An input size whose level 1 has ``valid`` windows of 9: level size ``valid + 8`` = ``ceil((dim − 8) / 2)``."""
    return 2 * (valid + 8) + 8


def _shapes():
    th, tw = 32, 32  # asserted against vif_tile() below: parametrisation happens before the library is loaded
    shapes = [(41, 41), (42, 41), (43, 44), (44, 43), (41, 131), (131, 41)]
    # one short of and one past the scale kernel's footprint on each axis, at scale 0 (window 17) and at scale 1
    shapes += [(th - 1 + 16, tw + 1 + 16), (th + 1 + 16, tw - 1 + 16), (th + 16, tw + 16)]
    shapes += [(_level1_dim(th - 1), _level1_dim(tw + 1)), (_level1_dim(th + 1) - 1, _level1_dim(tw - 1) - 1)]
    # level sizes 31 / 33 and 32: the 16 x 16 footprint of the decimating kernel, two tiles per axis, both sides of its edge
    shapes += [(2 * 31 + 8, 2 * 33 + 8), (2 * 32 + 8, 2 * 32 + 7)]
    return [(7, h, w) for h, w in shapes] + [(6, 150, 131)]


def test_tile_is_what_the_shapes_assume():
    assert _tile() == (32, 32)


@pytest.mark.parametrize("scale", [1.0, 255.0])
@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: "x".join(map(str, s)))
def test_value_rule(shape, scale):
    p, t, o64, c32 = _case(shape, scale)
    _check(f"{shape}@{scale}", _sums(p.cuda(), t.cuda()), o64, c32)


@pytest.mark.parametrize("shape", [(7, 41, 41), (7, 44, 43), (7, 47, 49), (6, 150, 131)], ids=lambda s: "x".join(map(str, s)))
def test_one_plane_is_bit_equal_to_its_plane_of_the_batch(shape):
    p, t, _, _ = _case(shape, 255.0)
    pd, td = p.cuda(), t.cuda()
    whole = _sums(pd, td)
    for i in (0, shape[0] - 1):
        one = _sums(pd[i:i + 1], td[i:i + 1])
        assert one.shape == (4, 2, 1) and torch.equal(one, whole[:, :, i:i + 1])


def test_other_sigma_n_sq():
    p, t, o64, c32 = _case((7, 50, 47), 255.0, 0.1)
    _check("sn=0.1", _sums(p.cuda(), t.cuda(), 0.1), o64, c32)


# ------------------------------------------------------------------------------------------------------ branch cases
def _branch(name):
    p, t = vo.noisy_pair((7, 64, 64), 64, 255.0)
    if name == "target_zero_left":  # mask 1: windows without target signal
        t[..., :40] = 0.0
    elif name == "preds_zero_top":  # mask 2: windows without preds signal
        p[:, :40] = 0.0
    elif name == "negated":  # mask 3: g < 0 everywhere
        p = 255.0 - t
    elif name == "preds_zero":
        p = torch.zeros_like(t)
    return p, t


@pytest.mark.parametrize("name", ["target_zero_left", "preds_zero_top", "negated", "preds_zero"])
def test_branch_cases(name):
    p, t = _branch(name)
    o64, c32 = vo.vif_scale_sums(p, t, SN), vo.vif_scale_sums(p, t, SN, torch.float32)
    sums = _sums(p.cuda(), t.cuda())
    if name in ("negated", "preds_zero"):
        assert torch.equal(o64[:, 0], torch.zeros(4, 7, dtype=torch.float64))
        assert torch.equal(sums[:, 0].cpu(), torch.zeros(4, 7, dtype=torch.float64)), sums[:, 0]
    _check(name, sums, o64, c32)


# ------------------------------------------------------------------------------------------------------ 16-bit inputs
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_inputs_convert_on_load(dtype):
    p, t = vo.noisy_pair((3, 70, 45), 16, 1.0)
    p16, t16 = p.to(dtype).cuda(), t.to(dtype).cuda()
    assert torch.equal(_sums(p16, t16), _sums(p16.float(), t16.float()))


# ------------------------------------------------------------------------------------------------------------- layout
def _plane_scores(p, t, sn=SN):
    from torchmetrics_forked_amd.functional.image.vif import _vif_plane_scores

    return _vif_plane_scores(p, t, sn)


def _batch(shape, seed, scale=1.0):
    """[B, C, H, W] noisy batch whose planes differ in their noise level, so that every plane has its own score."""
    p, t = vo.noisy_pair(shape, seed, scale)
    b, c = shape[:2]
    k = torch.linspace(0.4, 2.0, b * c).reshape(b, c, 1, 1)
    return (t + k * (p - t)).contiguous(), t


def _oracle_planes(p, t, dtype=torch.float64):
    """Per-plane scores in the reference's (channel-major) plane order."""
    b, c, h, w = p.shape
    pp, tt = p.transpose(0, 1).reshape(c * b, h, w), t.transpose(0, 1).reshape(c * b, h, w)
    return vo.scores(vo.vif_scale_sums(pp, tt, SN, dtype).double())


def test_unaligned_storage_offset():
    p, t, o64, c32 = _case((7, 45, 43), 1.0)

    def dev(x):
        buf = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
        view = buf[1:].view(x.shape)
        view.copy_(x)
        assert view.is_contiguous() and view.storage_offset() == 1 and view.data_ptr() % 16 != 0
        return view

    _check("offset-1", _sums(dev(p), dev(t)), o64, c32)


def test_channel_sliced_batch():
    p, t = _batch((2, 4, 47, 41), 21)
    pv, tv = p.cuda()[:, 1:3], t.cuda()[:, 1:3]
    assert not pv.is_contiguous()
    vo.value_rule("channel-slice", _plane_scores(pv, tv), _oracle_planes(p[:, 1:3], t[:, 1:3]),
                  _oracle_planes(p[:, 1:3], t[:, 1:3], torch.float32))


def test_three_channels_in_the_reference_plane_order():
    p, t = _batch((2, 3, 44, 49), 22)
    want = _oracle_planes(p, t)
    assert float((want[1:] - want[:-1]).abs().min()) > 1e-3  # distinct planes: a wrong b / c reorder shows
    got = _plane_scores(p.cuda(), t.cuda())
    assert got.shape == (6,) and got.dtype == torch.float32
    vo.value_rule("b-c-order", got, want, _oracle_planes(p, t, torch.float32))


# -------------------------------------------------------------------------------------------------------------- route
def _raise_conv(*a, **k):
    raise AssertionError("the composition ran: conv2d called on the native route")


def _raise_native(*a, **k):
    raise AssertionError("the native VIF op was entered on a kept route")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_functional_and_module_take_the_native_route(dtype, monkeypatch):
    import torchmetrics_forked_amd.functional.image.vif as vif_mod
    from torchmetrics_forked_amd.image import VisualInformationFidelity

    p, t = _batch((2, 3, 44, 49), 23)
    p, t = p.to(dtype), t.to(dtype)
    want = _oracle_planes(p.float(), t.float()).mean()  # oracle of the rounded inputs
    c32 = _oracle_planes(p.float(), t.float(), torch.float32).mean()
    monkeypatch.setattr(vif_mod, "conv2d", _raise_conv)
    calls = count_calls(monkeypatch, vif_mod, "_vif_sums")
    got = vif_mod.visual_information_fidelity(p.cuda(), t.cuda())
    metric = VisualInformationFidelity().cuda()
    metric.update(p.cuda(), t.cuda())
    assert len(calls) == 2 and got.dtype == dtype and got.is_cuda
    if dtype == torch.float32:
        vo.value_rule("functional", got, want, c32)
        vo.value_rule("module", metric.compute(), want, c32)
    else:
        # the plane scores (below 1) are rounded to bf16 on return, half an ulp = 2^-9 each, and their mean is rounded once
        # more: 2^-8.  The module also rounds the channel mean and a batch sum below 2 (half an ulp 2^-8): 2^-7.
        assert abs(float(got.double().cpu() - want)) <= 2.0**-8
        assert abs(float(metric.compute().double().cpu() - want)) <= 2.0**-7


def test_kept_routes_never_reach_the_op(monkeypatch):
    import torchmetrics_forked_amd.functional.image.vif as vif_mod

    monkeypatch.setattr(vif_mod, "_vif_sums", _raise_native)
    p, t = _batch((1, 2, 44, 49), 24)
    want = _oracle_planes(p, t).mean()
    pg = p.cuda().requires_grad_()
    out = vif_mod.visual_information_fidelity(pg, t.cuda())
    out.backward()
    assert pg.grad is not None and bool(torch.isfinite(pg.grad).all())
    assert abs(float(out.detach().double().cpu() - want)) <= 1e-4  # the fp32 composition on the GPU
    out64 = vif_mod.visual_information_fidelity(p.double().cuda(), t.double().cuda())
    assert out64.dtype == torch.float64 and abs(float(out64.cpu() - want)) <= 1e-9
    assert abs(float(vif_mod.visual_information_fidelity(p, t).double() - want)) <= 1e-4
    with pytest.raises(AssertionError, match="kept route"):  # the guard itself is live
        vif_mod.visual_information_fidelity(p.cuda(), t.cuda())


_CONV_MARKS = ("conv", "Conv", "Cijk", "Im2", "im2col", "igemm", "miopen", "MIOpen")


def test_kernels_run():
    import torchmetrics_forked_amd.functional.image.vif as vif_mod

    p, t = _batch((2, 3, 44, 49), 25)
    pd, td = p.cuda(), t.cuda()
    names = kernels_run(lambda: vif_mod.visual_information_fidelity(pd, td))
    print("vif_kernels " + repr(sorted(set(names))))
    assert_route(names, present=("vif_scale_kernel", "vif_decim_kernel", "vif_fold_kernel"), absent=_CONV_MARKS)
    assert sum("vif_scale_kernel" in n for n in names) == 4 and sum("vif_decim_kernel" in n for n in names) == 3
    # the composition does show a convolution kernel under one of these marks: the absence above is not vacuous
    b, c, h, w = pd.shape
    comp = kernels_run(lambda: vif_mod._vif_planes(pd.reshape(b * c, 1, h, w), td.reshape(b * c, 1, h, w), SN))
    print("vif_composition_kernels " + repr(sorted(set(comp))))
    assert any(m in n for n in comp for m in _CONV_MARKS), sorted(set(comp))
    assert not any("vif_" in n for n in comp)


# ------------------------------------------------------------------------- determinism, no host read, module, NaN / inf
def test_deterministic():
    p, t, _, _ = _case((6, 150, 131), 255.0)
    pd, td = p.cuda(), t.cuda()
    assert torch.equal(_sums(pd, td), _sums(pd, td))


def test_no_host_read(monkeypatch):
    import torchmetrics_forked_amd.functional.image.vif as vif_mod

    p, t = _batch((2, 3, 44, 49), 26)
    pd, td = p.cuda(), t.cuda()
    want = vif_mod.visual_information_fidelity(pd, td)  # (first call outside the guarded region)
    monkeypatch.setattr(vif_mod, "conv2d", _raise_conv)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = vif_mod.visual_information_fidelity(pd, td)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(got, want)


def test_module_two_updates_of_different_batch_sizes():
    from torchmetrics_forked_amd.image import VisualInformationFidelity

    p, t = _batch((5, 2, 47, 44), 27)
    metric = VisualInformationFidelity().cuda()
    metric.update(p[:2].cuda(), t[:2].cuda())
    metric.update(p[2:].cuda(), t[2:].cuda())
    want, c32 = _oracle_planes(p, t).mean(), _oracle_planes(p, t, torch.float32).mean()
    vo.value_rule("module-two-updates", metric.compute(), want, c32)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_pixel_stays_in_its_plane(bad):
    p, t = _batch((3, 1, 50, 45), 28)
    pd, td = p.cuda(), t.cuda()
    clean = _plane_scores(pd, td)
    pd[1, 0, 20, 30] = bad
    got = _plane_scores(pd, td)
    assert torch.isnan(got[1]) and torch.equal(got[[0, 2]], clean[[0, 2]])
