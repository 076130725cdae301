"""The three 2-D SSIM forward kernels behind ``tmx::ssim_sums`` (``ssim_valid_kernel`` in ``csrc/image.hip``, ``ssim_v2_kernel`` and
``ssim_mfma_kernel`` in ``csrc/ssim_kernels.h``) against the dense-window fp64 oracle of ``tests/helpers/ssim_oracle.py``, at every
block, strip and tile edge, and the functional / module routes that reach them.

Value rule (``vif_oracle.value_rule``), as a maximum over the seven planes (or images) of a case:
``|native − oracle64| <= 4 |comp32 − oracle64| + 1e-6 max|oracle64|``, with ``comp32`` the same oracle in fp32 on the CPU (per-window values
added in fp64) at op level and the package's own CPU composition in fp32 for the functionals (their oracle is that composition in
fp64, pinned to the reference by ``tests/unittests/image/test_image.py``).  The matrix-core kernel is granted ``1e-6 · Hv · Wv`` more on a
plane's sums, the allowance ``test_ssim_mfma_vs_fp32_kernel`` gives it over the fp32 kernel (1e-6 on the per-plane mean); on a
per-image mean that is 1e-6.  A one-plane call is held to bit equality with its plane of the seven-plane batch
(``tests/test_vif_gpu.py`` has the argument why one plane cannot be held to the rule).  Every comparison prints one ``ssim2d_err`` line
(``-s`` shows them).

Routes.  Every case asserts the kernel names of its call (``tests.helpers.routes``).  The matrix-core route always launches
``ssim_v2_kernel`` too (its device-side fallback, which exits at once on clean data), so those cases also assert that the result
differs in bits from the two-constant call: the fallback's sums would be equal to it.

Geometry (``ops.image.ssim_tile``, asserted below): ``ssim_valid_kernel`` 256 output columns x 64 output rows per block; ``ssim_v2_kernel``
256 x 128; ``ssim_mfma_kernel`` 16 x 16 output tiles, four column tiles per workgroup, 1024 output rows per strip, bands of 16 input
rows with a fast load path when all 32 input columns of a tile lie inside the plane.  With windows up to 15 the last column tile
never has them all inside (it would need ``Wv − c0 + KS − 1 >= 32``); the tile before it has at KS 15 and has not at KS 3 when the last
tile holds two columns, which is what the ``Wv`` 18, 66 and 130 cases vary.

Squared error (``with_sse=True``): relative ``4 · 2^-24`` against the fp64 sum of ``(p − t)²`` (the fp32 rounding of the difference enters the
square twice, the square rounds once, one unit of margin; the fp32 partial sums of 8 to 16 terms round in both directions and
vanish in a plane's total).

Scalars.  PSNR of the fused collection: the state is fp32, so the per-update totals round on their way into it and their sum rounds
once more (at most ``2 · 2^-24`` relative on top of the kernel's ``4 · 2^-24``), and ``10 / ln 10`` times that relative error is the error in dB; the fp32 evaluation of
``compute`` (a division, a logarithm near −6 whose ulp is ``2^-21`` and is multiplied by 4.34, a subtraction, a product) is granted six
ulps of the fp32 result.  MS-SSIM is a product of powers ``cs_i^β_i`` of per-image means, each below 1, with ``β x^(β−1) <= 1`` for the
values here (``cs >= 0.25`` at ``β = 0.5``), so the matrix-core allowance of its first level stays 1e-6 on the result.

Measured on MI355X, error / bound (minimum, median, maximum): generic kernel fp32 0.017 / 0.085 / 0.30 (32 comparisons), 16-bit inputs
0.057 / 0.16 / 0.21 (12); packed-fp32 kernel 0.027 / 0.048 / 0.16 (14); matrix-core kernel 0.012 / 0.19 / 0.995 (43: the three largest are
3-tap windows, 0.995 at 1 x 2 outputs and 0.73 / 0.69 at the two-strip shapes; below 0.42 for the other windows); functionals in fp32
0.028 / 0.14 / 0.26 (26), with 16-bit results 0.86 to 0.97 (half an ulp of the result is the bound's largest term); 70 000 planes
0.14 to 0.24; the fused squared error at most 0.023 of ``4 · 2^-24``; the collection's SSIM 0.18, squared-error state 0.061, PSNR 0.097.

Mutants, each built on its own as a library outside the tree and run once under this file (the unchanged source built the same way
passes in full); the first test that fails is named:
* ``ssim_mfma_kernel``: ``nb`` one less, ``orows`` taken as ``strip`` in the last strip, ``c1`` and ``c2`` swapped:
  ``test_matrix_core_kernel_value_rule[1x2-k3g-unit]``; ``oy0`` of strip 1 off by 16: ``test_matrix_core_kernel_value_rule[1025x2-k3g-unit]``;
  ``own_row_end`` always ``H`` (the halo rows' squared error counted twice): ``test_fused_squared_error[mfma-two-strips]`` (106 tests pass
  before it: only the squared-error cases see it); ``own_lo`` without ``last_tile``:
  ``test_fused_squared_error[mfma-last-tile-of-24-columns]`` (the two-strips case before it passes: its last tile owns 12 columns);
* ``ssim_v2_kernel``: ``col_ok`` with ``<=``, ``c1`` and ``c2`` swapped: ``test_packed_fp32_kernel_value_rule[1x254-k3g-unit]``;
* ``ssim_valid_kernel``: ``col_ok`` with ``<=``, ``c1`` and ``c2`` swapped: ``test_generic_kernel_value_rule[1x1-k3g-unit]``;
* host code of both fp32 kernels: strip count floored (at least 1): ``test_generic_kernel_value_rule[65x31-k3g-unit]``; column-block
  count floored (at least 1): ``test_generic_kernel_value_rule[1x257-k3u-255]``;
* functional: ``n_valid`` with ``H · W``: ``test_functional_data_range[float-44]``; the kernel fed the inputs from before the clamp:
  ``test_functional_data_range[tuple-44]``.
``wx`` and ``wy`` swapped is equivalent here: the op is called with the same window on both axes by every caller.

Left out because they index out of bounds (a mutant may not fault): ``out_rows`` without the ``min`` (the staging loads of the last
strip run past the plane, past the allocation for the last plane), ``cols_in`` as ``c0 + 16 <= W`` (unmasked 16-byte loads past the row's
end, past the allocation in the last row), the partial index with ``gridDim.x · 4`` for ``ntx`` (a store past the partial tensor whenever
``ntx % 4 != 0``).
"""
import functools
import math

import pytest
import torch

from tests.helpers import ssim_oracle as so
from tests.helpers import vif_oracle as vo
from tests.helpers.routes import assert_route, kernels_run
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu

# asserted against ssim_tile() below: parametrisation happens before the library is loaded
ROWS, ROWS_V2, COLS, TILE, GROUP_COLS, STRIP = 64, 128, 256, 16, 64, 1024
SIGMA = {3: 0.6, 7: 1.0, 11: 1.5, 15: 2.0}
GENERIC, V2, MFMA = "ssim_valid_kernel", "ssim_v2_kernel", "ssim_mfma_kernel"
U32 = 2.0**-24


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def test_tile_is_what_the_shapes_assume():
    from torchmetrics_forked_amd.ops.image import ssim_tile

    assert ssim_tile() == (ROWS, ROWS_V2, COLS, TILE, GROUP_COLS, STRIP)


# ------------------------------------------------------------------------------------------------------------ helpers
def _rule(label, got, o64, c32, extra=0.0):
    """``vif_oracle.value_rule`` with ``extra`` added to the bound (0 calls the rule itself as well); prints one ``ssim2d_err`` line."""
    got, o64, c32 = (x.detach().double().cpu() for x in (got, o64, c32))
    assert got.shape == o64.shape == c32.shape, (label, got.shape, o64.shape, c32.shape)
    if got.dim() == 0:
        got, o64, c32 = got[None], o64[None], c32[None]
    err = (got - o64).abs().amax(-1)
    bound = 4 * (c32 - o64).abs().amax(-1) + 1e-6 * o64.abs().amax(-1) + extra
    ratio = float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max())
    so.print_err(label, ratio, float(err.max()), float(bound.max()))
    assert torch.isfinite(got).all(), label
    assert bool((err <= bound).all()), (label, err.tolist(), bound.tolist())
    if extra == 0.0:
        vo.value_rule(label, got, o64, c32)
    return ratio


def _routed(fn, present, absent=()):
    """The result of ``fn()`` from a profiled call whose kernel names are asserted."""
    box = []
    names = kernels_run(lambda: box.append(fn()))
    assert_route(names, present=present, absent=absent)
    return box[-1]


def _spec_id(spec):
    hv, wv, ks, win, kind = spec[:5]
    return f"{hv}x{wv}-k{ks}{win[0]}-{kind}" + "".join(f"-{str(x).split('.')[-1]}" for x in spec[5:])


@functools.lru_cache(maxsize=None)
def _case(hv, wv, ks, win, kind, dtype=None):
    """One seven-plane case of output size ``hv x wv``, computed once: inputs (rounded to ``dtype`` if given), window, constants and the two
    oracles ``[3, 7]``."""
    shape = (7, hv + ks - 1, wv + ks - 1)
    p, t, data_range = so.planes(shape, 1000 * hv + 7 * wv + ks, kind)
    if dtype is not None:
        p, t = p.to(dtype), t.to(dtype)
    w = so.gaussian(ks, SIGMA[ks]) if win == "gaussian" else so.uniform(ks)
    c1, c2 = so.consts(data_range)
    o64 = so.valid_window_sums(p.float(), t.float(), w, w, c1, c2)
    c32 = so.valid_window_sums(p.float(), t.float(), w, w, c1, c2, torch.float32)
    return {"p": p, "t": t, "w": w, "consts": torch.tensor([c1, c2, data_range], dtype=torch.float32), "o64": o64, "c32": c32,
            "n": hv * wv}


def _op(p, t, w, consts, sse=False):
    return torch.ops.tmx.ssim_sums(p, t, w, w, consts, sse)


def _dev(c, nconst):
    return c["p"].cuda(), c["t"].cuda(), c["w"].cuda(), c["consts"][:nconst].cuda()


def _mix(shapes, windows=(3, 7, 11, 15), every=True):
    """Shapes x windows with the window kind and the data scale alternating, so that every window meets both kinds and both
    scales without the full cross product; ``every=False`` gives each shape one window, in turn."""
    out = []
    for i, (hv, wv) in enumerate(shapes):
        for j, ks in enumerate(windows):
            if every or j == i % len(windows):
                out.append((hv, wv, ks, ("gaussian", "uniform")[(i + j) % 2], ("unit", "255")[(i + j // 2) % 2]))
    return out


def _fit(wv, ks, aligned):
    """The nearest output width at or above ``wv`` whose plane width ``wv + ks − 1`` is (``aligned``) or is not a multiple of four."""
    while ((wv + ks - 1) % 4 == 0) != aligned:
        wv += 1
    return wv


# ------------------------------------------------------------------------------------------- generic kernel, op level
_GENERIC_SHAPES = [(1, 1), (1, COLS + 1), (ROWS - 1, 30), (ROWS, 30), (ROWS + 1, 30), (2 * ROWS + 1, COLS - 1), (2 * ROWS + 1, COLS),
                   (2 * ROWS + 1, COLS + 1)]
_GENERIC_CASES = [(hv, _fit(wv, ks, False) if wv == 30 else wv, ks, win, kind) for hv, wv, ks, win, kind in _mix(_GENERIC_SHAPES)]


@pytest.mark.parametrize("spec", _GENERIC_CASES, ids=_spec_id)
def test_generic_kernel_value_rule(spec):
    c = _case(*spec)
    assert c["p"].shape[-1] % 4 != 0
    p, t, w, k = _dev(c, 3)
    got = _routed(lambda: _op(p, t, w, k), present=(GENERIC,), absent=(V2, MFMA))
    assert got.shape == (2, 7) and got.dtype == torch.float64
    _rule("generic/" + _spec_id(spec), got, c["o64"][:2], c["c32"][:2])


_HALF_CASES = [(hv, wv, ks, win, "unit", dtype)
               for dtype in (torch.bfloat16, torch.float16)
               for hv, wv, ks, win in [(ROWS, 30, 11, "gaussian"), (ROWS + 1, 30, 11, "gaussian"), (ROWS + 1, 29, 7, "uniform"),
                                       (2 * ROWS + 1, COLS, 11, "gaussian"), (2 * ROWS + 1, COLS + 1, 11, "gaussian"),
                                       (2 * ROWS + 1, COLS + 1, 7, "uniform")]]


@pytest.mark.parametrize("spec", _HALF_CASES, ids=_spec_id)
def test_generic_kernel_16_bit_inputs(spec):
    """The sums are fp64 for every input dtype: the same rule, on the rounded inputs."""
    c = _case(*spec)
    assert c["p"].dtype == spec[5]
    p, t, w, k = _dev(c, 3)
    got = _routed(lambda: _op(p, t, w, k), present=(GENERIC,), absent=(V2, MFMA))
    _rule("generic16/" + _spec_id(spec), got, c["o64"][:2], c["c32"][:2])


# ------------------------------------------------------------------------------------------ packed-fp32 kernel, op level
_V2_SHAPES = [(1, COLS - 2), (1, 2 * COLS + 2), (ROWS_V2 - 1, COLS + 2), (ROWS_V2, COLS - 2), (ROWS_V2, COLS + 2), (ROWS_V2 + 1, COLS - 2),
              (ROWS_V2 + 1, 2 * COLS - 2), (ROWS_V2 + 1, 2 * COLS + 2), (2 * ROWS_V2 + 1, COLS - 2), (2 * ROWS_V2 + 1, COLS + 2)]
_V2_CASES = _mix(_V2_SHAPES, every=False) + [(ROWS_V2 + 1, COLS + 2, ks, win, kind) for ks, win, kind in
                                             [(3, "uniform", "255"), (7, "gaussian", "255"), (11, "uniform", "unit"), (15, "gaussian", "unit")]]


@pytest.mark.parametrize("spec", _V2_CASES, ids=_spec_id)
def test_packed_fp32_kernel_value_rule(spec):
    c = _case(*spec)
    assert c["p"].shape[-1] % 4 == 0
    p, t, w, k = _dev(c, 2)
    assert p.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0
    got = _routed(lambda: _op(p, t, w, k), present=(V2,), absent=(GENERIC, MFMA))
    assert got.shape == (2, 7) and got.dtype == torch.float64
    _rule("v2/" + _spec_id(spec), got, c["o64"][:2], c["c32"][:2])


# ------------------------------------------------------------------------------------------ matrix-core kernel, op level
_MFMA_WV = (2, TILE - 2, TILE + 2, GROUP_COLS - 2, GROUP_COLS + 2, 2 * GROUP_COLS + 2)
_MFMA_SHORT = _mix([(hv, wv) for hv in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1) for wv in _MFMA_WV], every=False)
_MFMA_LONG = [(STRIP - 1, TILE + 2, 11, "gaussian", "unit"), (STRIP, TILE - 2, 7, "uniform", "255"), (STRIP, TILE + 2, 11, "gaussian", "unit"),
              (STRIP + 1, 2, 3, "gaussian", "unit"), (STRIP + 1, 2, 15, "uniform", "255"),
              (STRIP + 1, TILE + 2, 3, "uniform", "255"), (STRIP + 1, TILE + 2, 11, "gaussian", "unit"), (STRIP + 1, TILE + 2, 15, "gaussian", "unit"),
              (STRIP + 1, GROUP_COLS + 2, 11, "uniform", "unit"),
              (STRIP + TILE + 1, TILE - 2, 3, "gaussian", "unit"), (STRIP + TILE + 1, TILE - 2, 15, "gaussian", "255"),
              (STRIP + TILE + 1, TILE + 2, 3, "uniform", "unit"), (STRIP + TILE + 1, TILE + 2, 15, "uniform", "unit")]


def _mfma_sums(c, sse=False):
    """The three-constant call (route asserted, and not the fallback: its bits differ from the two-constant call's)."""
    p, t, w, k = _dev(c, 3)
    assert c["p"].shape[-1] % 4 == 0 and p.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0
    got = _routed(lambda: _op(p, t, w, k, sse), present=(MFMA,), absent=(GENERIC,))
    assert not torch.equal(got[:2], _op(p, t, w, k[:2], sse)[:2])
    return got


@pytest.mark.parametrize("spec", _MFMA_SHORT + _MFMA_LONG, ids=_spec_id)
def test_matrix_core_kernel_value_rule(spec):
    c = _case(*spec)
    got = _mfma_sums(c)
    assert got.shape == (2, 7) and got.dtype == torch.float64
    _rule("mfma/" + _spec_id(spec), got, c["o64"][:2], c["c32"][:2], extra=1e-6 * c["n"])


# -------------------------------------------------------------------------------------- one plane: bit equality
_TWO_STRIPS = (STRIP + 1, TILE + 2, 11, "gaussian", "unit")
_WIDE_V2 = (ROWS_V2 + 1, COLS + 2, 11, "uniform", "unit")
_ONE_PLANE = [(3, _TWO_STRIPS), (3, (2 * TILE + 1, GROUP_COLS + 2, 7, "uniform", "unit")), (2, _WIDE_V2),
              (3, (2 * ROWS + 1, COLS + 1, 11, "gaussian", "255"))]


@pytest.mark.parametrize(("nconst", "spec"), _ONE_PLANE, ids=lambda x: x if isinstance(x, int) else _spec_id(x))
def test_one_plane_is_bit_equal_to_its_plane_of_the_batch(nconst, spec):
    """The two window sums on every route, and the squared error where a kernel adds it (on the generic route it is a separate
    fp64 torch reduction over the plane, whose order may depend on the batch: held to 1e-12 relative there)."""
    c = _case(*spec)
    p, t, w, k = _dev(c, nconst)
    whole = _op(p, t, w, k, True)
    fused_sse = c["p"].shape[-1] % 4 == 0
    for i in (0, 6):
        one = _op(p[i:i + 1], t[i:i + 1], w, k, True)
        assert one.shape == (3, 1) and torch.equal(one[:2], whole[:2, i:i + 1])
        if fused_sse:
            assert torch.equal(one[2], whole[2, i:i + 1])
        else:
            assert abs(float(one[2] - whole[2, i])) <= 1e-12 * float(whole[2, i])


# ------------------------------------------------------------------------------------------------- squared error
_SSE = {
    "mfma-two-strips": (3, _TWO_STRIPS, (MFMA,), (GENERIC,)),
    "mfma-last-tile-of-24-columns": (3, (2 * TILE + 1, TILE - 2, 11, "gaussian", "unit"), (MFMA,), (GENERIC,)),
    "mfma-two-strips-255": (3, (STRIP + TILE + 1, TILE - 2, 15, "gaussian", "255"), (MFMA,), (GENERIC,)),
    "v2": (2, _WIDE_V2, (V2,), (GENERIC, MFMA)),
    "generic": (3, (ROWS + 1, 31, 11, "gaussian", "unit"), (GENERIC,), (V2, MFMA)),
}


@pytest.mark.parametrize("name", list(_SSE))
def test_fused_squared_error(name):
    nconst, spec, present, absent = _SSE[name]
    c = _case(*spec)
    p, t, w, k = _dev(c, nconst)
    got = _routed(lambda: _op(p, t, w, k, True), present=present, absent=absent)
    assert got.shape == (3, 7) and got.dtype == torch.float64
    want = c["o64"][2]
    rel = float(((got[2].cpu() - want).abs() / want).max())
    so.print_err("sse/" + name, rel / (4 * U32), rel, 4 * U32)
    assert rel <= 4 * U32, (name, rel)
    _rule("sse-sums/" + name, got[:2], c["o64"][:2], c["c32"][:2], extra=1e-6 * c["n"] if MFMA in present else 0.0)


# ------------------------------------------------------------------------------------------ the device-side fallback
@pytest.mark.parametrize("spec", [_TWO_STRIPS, _WIDE_V2], ids=_spec_id)
@pytest.mark.parametrize("bad", ["range", "nan", "inf"])
def test_fallback_at_edges(bad, spec):
    """Plane 3 holds data the matrix-core kernel cannot take (ten times the data range, or one NaN / inf pixel in the last strip and
    the last column tile): the three-constant call returns the fallback kernel's sums bit for bit, those pass the rule on the finite
    planes, and the other planes are bit-equal to a clean run of the fallback kernel."""
    c = _case(*spec)
    p, t = c["p"].clone(), c["t"]
    if bad == "range":
        p[3] *= 10
    else:
        p[3, -2, -2] = float(bad)
    w = c["w"]
    c1, c2 = float(c["consts"][0]), float(c["consts"][1])
    pd, td, wd, k = p.cuda(), t.cuda(), w.cuda(), c["consts"].cuda()
    three = _routed(lambda: _op(pd, td, wd, k, True), present=(MFMA, V2), absent=(GENERIC,))
    two = _routed(lambda: _op(pd, td, wd, k[:2], True), present=(V2,), absent=(GENERIC, MFMA))
    assert torch.equal(three.isnan(), two.isnan()) and torch.equal(three.nan_to_num(0.0), two.nan_to_num(0.0))
    clean = _op(c["p"].cuda(), td, wd, k[:2], True)
    keep = [0, 1, 2, 4, 5, 6]
    assert torch.equal(two[:, keep], clean[:, keep])
    if bad == "range":
        o64, c32 = so.valid_window_sums(p, t, w, w, c1, c2), so.valid_window_sums(p, t, w, w, c1, c2, torch.float32)
        assert not torch.equal(two[:, 3], clean[:, 3])
        _rule(f"fallback/{bad}/" + _spec_id(spec), two[:2], o64[:2], c32[:2])
    else:
        assert bool(two[:2, 3].isnan().all())
        _rule(f"fallback/{bad}/" + _spec_id(spec), two[:2, keep], c["o64"][:2, keep], c["c32"][:2, keep])


# ---------------------------------------------------------------------------------------------------- misaligned base
def _offset_1(x):
    """The same values at storage offset 1: not 16-byte aligned."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.storage_offset() == 1 and view.data_ptr() % 16 != 0
    return view


@pytest.mark.parametrize("which", ["both", "preds", "target"])
def test_misaligned_base_takes_the_generic_kernel(which):
    """fp32 planes with ``W % 4 == 0`` whose base is not 16-byte aligned.  Agreement with the aligned copy: both results are within the
    rule's bound of the oracle, so they are within twice the bound of each other."""
    c = _case(*_WIDE_V2)
    p, t, w, k = _dev(c, 3)
    po = _offset_1(p) if which in ("both", "preds") else p
    to = _offset_1(t) if which in ("both", "target") else t
    got = _routed(lambda: _op(po, to, w, k), present=(GENERIC,), absent=(V2, MFMA))
    _rule("misaligned/" + which, got, c["o64"][:2], c["c32"][:2])
    aligned = _routed(lambda: _op(p, t, w, k[:2]), present=(V2,), absent=(GENERIC, MFMA))
    bound = 4 * (c["c32"][:2] - c["o64"][:2]).abs().amax(-1) + 1e-6 * c["o64"][:2].abs().amax(-1)
    assert bool(((got - aligned).abs().amax(-1).cpu() <= 2 * bound).all())


# ------------------------------------------------------------------------------------------- functional and module cases
def _ssim(*a, **k):
    from torchmetrics_forked_amd.functional.image import structural_similarity_index_measure

    return structural_similarity_index_measure(*a, **k)


def _msssim(*a, **k):
    from torchmetrics_forked_amd.functional.image import multiscale_structural_similarity_index_measure

    return multiscale_structural_similarity_index_measure(*a, **k)


_ON_MFMA = ((MFMA,), (GENERIC,), 1e-6)
_ON_GENERIC = ((GENERIC,), (V2, MFMA), 0.0)


def _functional(label, p, t, route, fn=_ssim, view=None, half_ulp=0.0, **kw):
    """``fn`` on the GPU (``view`` makes the device inputs from the uploaded ones) against the CPU composition in fp64 and in fp32."""
    present, absent, extra = route
    want = fn(p.double(), t.double(), **kw)
    comp = fn(p.float(), t.float(), **kw)
    pd, td = (p.cuda(), t.cuda()) if view is None else view(p.cuda(), t.cuda())
    got = _routed(lambda: fn(pd, td, **kw), present=present, absent=absent)
    if not isinstance(got, tuple):
        got, want, comp = (got,), (want,), (comp,)
    for i, (g, o, c) in enumerate(zip(got, want, comp)):
        assert g.dtype == p.dtype and g.is_cuda and g.shape == o.shape
        _rule(f"{label}/{i}", g, o, c, extra=extra + half_ulp)
    return got


def _batch(shape, seed, kind="unit"):
    return so.planes(shape, seed, kind)[:2]


@pytest.mark.parametrize("width", [44, 45])
@pytest.mark.parametrize("data_range", [1.0, (0.1, 0.9), None], ids=["float", "tuple", "none"])
def test_functional_data_range(data_range, width):
    """``(0.1, 0.9)`` on data in [0, 1]: the clamp happens before the kernel (the oracle composition clamps too; without the clamp the
    result moves by far more than the bound, asserted on the oracle)."""
    p, t = _batch((7, 2, 40, width), 4000 + width)
    route = _ON_MFMA if width % 4 == 0 else _ON_GENERIC
    _functional(f"range-{data_range}/w{width}", p, t, route, reduction="none", data_range=data_range)
    if isinstance(data_range, tuple):
        assert float(p.min()) < 0.1 and float(p.max()) > 0.9
        clamped = _ssim(p.double(), t.double(), reduction="none", data_range=data_range)
        unclamped = _ssim(p.double(), t.double(), reduction="none", data_range=data_range[1] - data_range[0])
        comp = _ssim(p, t, reduction="none", data_range=data_range)
        bound = 4 * float((comp - clamped).abs().max()) + 1e-6 * float(clamped.abs().max()) + route[2]
        assert float((clamped - unclamped).abs().min()) > 10 * bound


@pytest.mark.parametrize("width", [44, 45])
@pytest.mark.parametrize("kind", ["negative", "shifted", "shifted_low"])
def test_functional_negative_and_shifted_data(kind, width):
    """The matrix-core kernel takes pixel pairs with ``p² + t² <= 2 data_range²`` at a power-of-two range: data in [−0.5, 0.5] and in
    [0.2, 0.95] stay on it, data in [0.2, 1.2] holds pairs beyond that (both values near the top) and takes the device-side
    fallback, whose sums are those of the two-constant call."""
    p, t = _batch((7, 2, 40, width), 4100 + width, kind)
    lo, hi = {"negative": (-0.5, 0.5), "shifted": (0.2, 1.2), "shifted_low": (0.2, 0.95)}[kind]
    assert lo <= float(p.min()) < lo + 0.05 and hi - 0.05 < float(p.max()) <= hi + 1e-6
    falls_back = kind == "shifted"
    assert (float((p.double() ** 2 + t.double() ** 2).max()) > 2.0) == falls_back
    route = _ON_GENERIC if width % 4 else ((MFMA, V2), (GENERIC,), 0.0) if falls_back else _ON_MFMA
    _functional(f"{kind}/w{width}", p, t, route, reduction="none", data_range=1.0)
    if width % 4 == 0:  # which of the two launches the result came from: the two-constant call gives the fallback's bits
        w = so.gaussian(11, 1.5).cuda()
        k = torch.tensor([*so.consts(1.0), 1.0]).cuda()
        pd, td = p.cuda().reshape(14, 40, width), t.cuda().reshape(14, 40, width)
        assert torch.equal(_op(pd, td, w, k), _op(pd, td, w, k[:2])) == falls_back


@pytest.mark.parametrize("width", [44, 45])
def test_functional_contrast_sensitivity(width):
    p, t = _batch((7, 2, 40, width), 4200 + width)
    route = _ON_MFMA if width % 4 == 0 else _ON_GENERIC
    got = _functional(f"cs/w{width}", p, t, route, reduction="none", data_range=1.0, return_contrast_sensitivity=True)
    assert len(got) == 2 and not torch.equal(got[0], got[1])


def _channels_last(p, t):
    p, t = p.contiguous(memory_format=torch.channels_last), t.contiguous(memory_format=torch.channels_last)
    assert not p.is_contiguous()
    return p, t


def _column_slice(p, t):
    assert not p[..., 1:].is_contiguous()
    return p[..., 1:], t[..., 1:]


def _expanded_target(p, t):
    t = t[:, :1].expand(-1, p.shape[1], -1, -1)
    assert not t.is_contiguous()
    return p, t


@pytest.mark.parametrize("width", [44, 45])
@pytest.mark.parametrize("view", [_channels_last, _column_slice, _expanded_target])
def test_functional_non_contiguous_inputs(view, width):
    extra_col = 1 if view is _column_slice else 0
    p, t = _batch((7, 3, 40, width + extra_col), 4300 + width)
    route = _ON_MFMA if width % 4 == 0 else _ON_GENERIC
    pc, tc = view(p, t)  # the oracle sees the same values
    _functional(f"{view.__name__}/w{width}", pc.contiguous(), tc.contiguous(), route,
                view=lambda a, b: view(p.cuda(), t.cuda()), reduction="none", data_range=1.0)


@pytest.mark.parametrize("shape", [(7, 2, 40, 44), (7, 1, ROWS + 11, COLS + 12)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_functional_16_bit_results(dtype, shape):
    """Against the fp64 composition of the rounded inputs: the rule plus half an ulp of the output dtype at values up to 1."""
    p, t = _batch(shape, 4400 + shape[-1])
    half_ulp = 2.0**-9 if dtype == torch.bfloat16 else 2.0**-12
    _functional(f"{dtype}/{shape}", p.to(dtype), t.to(dtype), _ON_GENERIC, half_ulp=half_ulp, reduction="none", data_range=1.0)


@pytest.mark.parametrize("normalize", [None, "relu", "simple"])
def test_ms_ssim_default_betas(normalize):
    """Levels 177 x 180 (matrix-core), 88 x 90, 44 x 45, 22 x 22 (generic) and 11 x 11 (generic, one window)."""
    p, t = _batch((7, 1, 177, 180), 4500)
    _functional(f"ms-ssim/{normalize}", p, t, ((MFMA, GENERIC), (), 1e-6), fn=_msssim, reduction="none", data_range=1.0, normalize=normalize)


def test_ms_ssim_two_betas():
    p, t = _batch((7, 1, 48, 52), 4600)
    _functional("ms-ssim/betas2", p, t, ((MFMA, GENERIC), (), 1e-6), fn=_msssim, reduction="none", data_range=1.0, betas=(0.5, 0.5))


def test_collection_of_ssim_and_psnr_over_two_strips():
    """``MetricCollection{SSIM, PSNR}`` over two updates of ``[1, 7, 1055, 40]`` (two strips of the matrix-core kernel): SSIM under the rule
    (with the matrix-core allowance on a mean: 1e-6), the PSNR state and result against fp64 (module docstring)."""
    from torchmetrics_forked_amd import MetricCollection
    from torchmetrics_forked_amd.image import PeakSignalNoiseRatio, StructuralSimilarityIndexMeasure

    coll = MetricCollection({"ssim": StructuralSimilarityIndexMeasure(data_range=1.0), "psnr": PeakSignalNoiseRatio(data_range=1.0)}).cuda()
    batches = [_batch((1, 7, STRIP + 31, 40), seed) for seed in (4700, 4701)]

    def updates():
        coll.reset()
        for p, t in batches:
            coll.update(p.cuda(), t.cuda())

    names = kernels_run(updates)
    assert_route(names, present=(MFMA,), absent=(GENERIC,))
    assert coll._fused_plans and type(coll._fused_plans[0]).__name__ == "_ImagePairPlan"
    out = coll.compute()
    want = torch.stack([_ssim(p.double(), t.double(), data_range=1.0) for p, t in batches]).mean()
    comp = torch.stack([_ssim(p, t, data_range=1.0) for p, t in batches]).mean()
    _rule("collection/ssim", out["ssim"], want, comp, extra=1e-6)
    sse = sum(float(((p.double() - t.double()) ** 2).sum()) for p, t in batches)
    n = sum(p.numel() for p, _ in batches)
    state = float(coll["psnr"].sum_squared_error)
    assert int(coll["psnr"].total) == n
    rel = abs(state - sse) / sse
    so.print_err("collection/sse-state", rel / (6 * U32), rel, 6 * U32)
    assert rel <= 6 * U32
    psnr = 10 * math.log10(1.0 / (sse / n))
    bound = 10 / math.log(10) * 6 * U32 + 6 * 2.0 ** (math.floor(math.log2(psnr)) - 23)
    err = abs(float(out["psnr"]) - psnr)
    so.print_err("collection/psnr", err / bound, err, bound)
    assert err <= bound


# -------------------------------------------------------------------------------------------------------- plane count
_MANY = 70000


@functools.lru_cache(maxsize=None)
def _patches(size):
    """70 000 patches of ``1 x size x size`` (more than a grid axis of 65 535 holds) and their oracles ``[2, 70000]``."""
    g = torch.Generator().manual_seed(size)
    t = torch.rand(_MANY, 1, size, size, generator=g)
    p = (t + 0.1 * torch.randn(_MANY, 1, size, size, generator=g)).clamp(0, 1)
    w = so.gaussian(11, 1.5)
    c1, c2 = so.consts(1.0)
    o64 = so.valid_window_sums(p[:, 0], t[:, 0], w, w, c1, c2)
    c32 = so.valid_window_sums(p[:, 0], t[:, 0], w, w, c1, c2, torch.float32)
    return p, t, o64, c32


@pytest.mark.parametrize("size", [12, 11])
def test_more_planes_than_a_grid_axis_of_65535(size):
    """12 x 12: the matrix-core route (four windows per plane); 11 x 11: the generic route (one window)."""
    p, t, o64, c32 = _patches(size)
    n = (size - 10) ** 2
    pd, td = p.cuda(), t.cuda()
    present, absent, extra = _ON_MFMA if size % 4 == 0 else _ON_GENERIC
    got = _routed(lambda: _ssim(pd, td, data_range=1.0, reduction="none", return_contrast_sensitivity=True), present=present, absent=absent)
    assert got[0].shape == (_MANY,) and got[1].shape == (_MANY,)
    _rule(f"70000x{size}/sim", got[0], o64[0] / n, c32[0] / n, extra=extra)
    _rule(f"70000x{size}/cs", got[1], o64[1] / n, c32[1] / n, extra=extra)
    # the op itself, fused squared error included, and the packed-fp32 kernel at that plane count
    w, k = so.gaussian(11, 1.5).cuda(), torch.tensor([*so.consts(1.0), 1.0]).cuda()
    sums = _op(pd[:, 0], td[:, 0], w, k, True)
    assert sums.shape == (3, _MANY)
    _rule(f"70000x{size}/op", sums[:2], o64[:2], c32[:2], extra=extra * n)
    want_sse = ((p.double() - t.double()) ** 2).sum((1, 2, 3))
    assert float(((sums[2].cpu() - want_sse).abs() / want_sse).max()) <= 4 * U32
    if size % 4 == 0:
        two = _routed(lambda: _op(pd[:, 0], td[:, 0], w, k[:2], True), present=(V2,), absent=(GENERIC, MFMA))
        assert not torch.equal(two[:2], sums[:2])
        _rule(f"70000x{size}/v2", two[:2], o64[:2], c32[:2])
        # a bad pixel in the second launch's planes sends the whole call to the fallback kernel
        pd[_MANY - 1, 0, 3, 3] = float("nan")
        bad = _op(pd[:, 0], td[:, 0], w, k, True)
        assert bool(bad[:2, -1].isnan().all()) and torch.equal(bad[:, :-1], two[:, :-1])


def test_backward_with_more_planes_than_a_grid_axis_of_65535():
    """The gradient of the mean over 70 000 patches, on a random subset of 64 images, against the composition's gradient with the
    bound of ``tests/test_ssim_grad_gpu.py``: ``err_native <= 4 err_comp32 + 1e-7 max|g64|``."""
    p, t, _, _ = _patches(12)
    pd = p.cuda().requires_grad_()
    out = _routed(lambda: _ssim(pd, t.cuda(), data_range=1.0), present=(MFMA,), absent=(GENERIC,))
    pd.grad = None
    out.backward()
    assert pd.grad is not None and pd.grad.shape == p.shape
    idx = torch.randperm(_MANY, generator=torch.Generator().manual_seed(64))[:64]
    idx[0], idx[1] = _MANY - 1, 65535  # the last plane, and the first plane of the second launch

    def comp_grad(dtype):
        q = p[idx].to(dtype).requires_grad_()
        (_ssim(q, t[idx].to(dtype), data_range=1.0, reduction="sum") / _MANY).backward()
        return q.grad.double()

    g64, g32 = comp_grad(torch.float64), comp_grad(torch.float32)
    got = pd.grad[idx.cuda()].double().cpu()
    err, err_comp, gmax = float((got - g64).abs().max()), float((g32 - g64).abs().max()), float(g64.abs().max())
    bound = 4 * err_comp + 1e-7 * gmax
    so.print_err("70000x12/grad", err / bound, err, bound)
    assert gmax > 0 and err <= bound, (err, err_comp, gmax)
