"""Native spectral angle mapper and ERGAS (``tmx::sam_map`` / ``tmx::sam_sums`` / ``tmx::ergas_scores``, ``csrc/spectral.hip``) against the
dense fp64 oracles of ``tests/helpers/spectral_oracle.py``, and the routes of ``spectral_angle_mapper`` and
``error_relative_global_dimensionless_synthesis``.

Value rule (``vif_oracle.value_rule``): ``|native − oracle64| <= 4 |comp32 − oracle64| + 1e-6 max|oracle64|`` with ``comp32`` the same oracle
in fp32 on the CPU.  Inputs are ``vif_oracle.noisy_pair``.  Every comparison takes its maximum over at least 64 entries for maps
and at least 7 for per-image vectors (a 1 x 1 plane is run with 64 images, scalars as vectors over seven seeds): with one
scalar a single draw of the composition's error is below a quarter of an equally distributed native one about one time in six
for any correct fp32 kernel (``tests/test_vif_gpu.py`` has the argument).  Every comparison prints one ``vif_err`` line (``-s``).

What is held to more than the rule: two runs are bit-equal; the 16-byte-load kernels are bit-equal to the generic ones (every
value case runs the same data a second time at a one-element storage offset, which only the generic kernels accept); 16-bit
inputs give the bits of their up-cast; identical inputs give exact zeros; a zero vector gives NaN in its pixel and its image's
sum and changes no other bit; anti-parallel vectors give pi within one fp32 ulp.

``sam_sums`` against ``sam_map``: within 1e-12 relative of ``sam_map(...).double().sum((1, 2))``, not bit-equal.  The op adds the same fp32
angles in fp64, but in its own order (a thread's pixels, the lanes of a wave by an xor tree, the waves, then the workgroups of
an image); fp64 sums of at most a few million fp32 values in two orders differ by a few 2^-53 of the sum.  Where an image is
one pixel the two are bit-equal, and ``test_large_batch`` asserts that.

Measured on MI355X, error / bound: SAM maps 0.013 to 0.18 (median 0.049, 43 comparisons), per-image sums at most 0.18 (median 0.048,
42), 16-bit inputs at most 0.25, ERGAS scores at most 0.003 (69), the functionals' and modules' results at most 0.096 (18).  With
the three band sums of a pixel kept in fp32 (sequential fused multiply-adds) ``test_sam_many_bands`` stood at 1.34 (scale 1) and
0.99 (scale 255) of the bound at 200 bands: the op sums in fp64.

Mutants of ``csrc/spectral.hip``, the op built alone as a library outside the tree and run under this file one at a time (the
unchanged source built the same way passes in full), and the tests that catch each:
* clamp through ``fmin`` / ``fmax``: the two ``test_zero_vectors_give_nan_in_their_pixel_only`` cases, nothing else;
* last vector of the plane dropped in the vector kernel (with ``H·W`` a multiple of the vector width there is no partial vector):
  27 tests, ``test_sam_planes`` at ``P`` and ``2P + 4`` and every ``test_sam_bands`` case among them;
* band loop remainder dropped: 31, ``test_sam_bands`` at 2, 3, 5, 7 and 9 bands (4 and 8 pass, as they must);
* workgroup count floored: 10, ``test_sam_planes`` at ``P + 1``, ``2P + 3`` and ``2P + 4`` first;
* image index masked to 16 bits: ``test_large_batch`` alone;
* ``Σt`` divided by ``HW`` twice: 38, every ``test_ergas_planes`` case; ``ratio`` inside the root: the same 38;
* chunk remainder dropped: the 12 ``test_ergas_planes`` cases with two chunks (``2E + 3`` and ``2E + 8``).
(Counted with ``test_ergas_planes`` at the scale and ratio pairs (1, 4) and (255, 0.5); it now runs all four combinations.)
Not run: pixel guard ``<=`` for ``<``.  At the thread's guard ``pix0 < H·W`` the change is equivalent (a thread at ``pix0 == H·W`` gets
``valid == 0``).  At the generic kernels' per-pixel guard ``j < valid`` it reads one element past a thread's pixels and, for the last
image, stores past the end of the map, and a kernel that writes out of bounds is not run on a shared device.  By construction
it adds one more angle to an image's sum wherever ``H·W`` is no multiple of the vector width, about 1e-3 of the sum against the
1e-12 that ``_sam_check`` allows between ``sam_sums`` and the fp64 sum of ``sam_map`` (``test_sam_planes`` at ``P − 1``, ``P + 1`` and ``2P + 3``).
"""
import functools
import math

import pytest
import torch

from tests.helpers import spectral_oracle as so
from tests.helpers import vif_oracle as vo
from tests.helpers.routes import assert_route, count_calls, kernels_run
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu

P, E = 1024, 4096  # asserted against spectral_tile() below: parametrisation happens before the library is loaded


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _ops():
    from torchmetrics_forked_amd.ops import image

    return image


def _offset(x):
    """The same values at a one-element storage offset: contiguous, never 16-byte aligned."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    buf[1:].copy_(x.flatten())
    out = buf[1:].view(x.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


def _ids(s):
    return "x".join(map(str, s))


def _same_bits(a, b):
    """Bit equality, NaN included (``torch.equal`` takes NaN for unequal to itself)."""
    view = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


@functools.lru_cache(maxsize=None)
def _sam_case(shape, scale=1.0, seed=None):
    """(preds, target, angles64, angles32) of one noisy ``[B, C, H, W]`` case, computed once."""
    seed = 1000 * shape[0] + 7 * shape[1] + shape[2] * shape[3] if seed is None else seed
    p, t = vo.noisy_pair(shape, seed, scale)
    return p, t, so.sam_angles(p, t), so.sam_angles(p, t, torch.float32)


def _sam_run(pd, td):
    """``(map, sums)`` of the ops; asserts on the way that a second run and the run at a storage offset give the same bits."""
    img = _ops()
    got_map, got_sums = img.sam_map(pd, td), img.sam_sums(pd, td)
    assert got_map.dtype == torch.float32 and got_map.shape == (pd.shape[0], pd.shape[2], pd.shape[3])
    assert got_sums.dtype == torch.float64 and got_sums.shape == (pd.shape[0],)
    assert _same_bits(img.sam_map(pd, td), got_map) and _same_bits(img.sam_sums(pd, td), got_sums)
    po, to = _offset(pd), _offset(td)
    assert _same_bits(img.sam_map(po, to), got_map) and _same_bits(img.sam_sums(po, to), got_sums)
    return got_map, got_sums


def _sam_check(label, shape, scale=1.0):
    p, t, a64, a32 = _sam_case(shape, scale)
    got_map, got_sums = _sam_run(p.cuda(), t.cuda())
    worst = vo.value_rule(f"sam/{label}/map", got_map.flatten(), a64.flatten(), a32.flatten())
    if shape[0] >= 7:
        worst = max(worst, vo.value_rule(f"sam/{label}/sums", got_sums, a64.sum((1, 2)), a32.sum((1, 2))))
    want = got_map.double().sum((1, 2))
    assert bool(((got_sums - want).abs() <= 1e-12 * want.abs()).all()), (label, got_sums.tolist(), want.tolist())
    return worst


def test_tile_is_what_the_shapes_assume():
    assert _ops().spectral_tile() == (P, E)


# ------------------------------------------------------------------------------------------------------------------ SAM
@pytest.mark.parametrize("scale", [1.0, 255.0])
@pytest.mark.parametrize("shape", [(64, 7, 1, 1), (7, 7, 1, P - 1), (7, 7, 2, P // 2), (7, 7, 1, P + 1), (7, 7, 1, 2 * P + 3),
                                   (7, 7, 2, P + 2)], ids=_ids)
def test_sam_planes(shape, scale):
    """Planes of 1, ``P − 1``, ``P``, ``P + 1``, ``2P + 3`` and ``2P + 4`` pixels (the last: the vector kernel with a part-filled third workgroup)."""
    _sam_check(f"{_ids(shape)}@{scale}", shape, scale)


@pytest.mark.parametrize("scale", [1.0, 255.0])
@pytest.mark.parametrize("c", [2, 3, 4, 5, 7, 8, 9])
def test_sam_bands(c, scale):
    """Band counts on both sides of the band loop's unroll of four, on a vector-kernel plane (12 x 28) and a generic one (9 x 37)."""
    _sam_check(f"c{c}-vec@{scale}", (7, c, 12, 28), scale)
    _sam_check(f"c{c}-generic@{scale}", (7, c, 9, 37), scale)


@pytest.mark.parametrize("scale", [1.0, 255.0])
def test_sam_many_bands(scale):
    _sam_check(f"c200@{scale}", (7, 200, 3, 5), scale)


def test_large_batch():
    """70 000 images of one pixel: the image index does not fit a 16-bit grid axis."""
    shape = (70000, 2, 1, 1)
    p, t, a64, a32 = _sam_case(shape)
    got_map, got_sums = _sam_run(p.cuda(), t.cuda())
    vo.value_rule("sam/b70000/map", got_map.flatten(), a64.flatten(), a32.flatten())
    assert torch.equal(got_sums, got_map.double().flatten())  # one pixel per image: nothing to reorder


def test_kernel_choice_by_alignment():
    img = _ops()
    p, t = vo.noisy_pair((2, 3, 12, 28), 3)
    pd, td = p.cuda(), t.cuda()
    odd_p, odd_t = pd[..., :27].contiguous(), td[..., :27].contiguous()  # 324 pixels: a multiple of 4, not of 8
    for fn, vec, generic in ((img.sam_map, "sam_vec_kernel", "sam_generic_kernel"), (img.sam_sums, "sam_vec_kernel", "sam_generic_kernel"),
                             (lambda a, b: img.ergas_scores(a, b, 4.0), "ergas_plane_vec_kernel", "ergas_plane_generic_kernel")):
        assert_route(kernels_run(lambda: fn(pd, td)), present=(vec,), absent=(generic,))
        assert_route(kernels_run(lambda: fn(_offset(pd), _offset(td))), present=(generic,), absent=(vec,))
        assert_route(kernels_run(lambda: fn(pd[..., :27], td[..., :27])), present=(vec,), absent=(generic,))  # made contiguous: 324 = 4 · 81
        assert_route(kernels_run(lambda: fn(pd[..., :11, :27], td[..., :11, :27])), present=(generic,), absent=(vec,))  # 297 pixels
        assert_route(kernels_run(lambda: fn(odd_p.half(), odd_t.half())), present=(generic,), absent=(vec,))  # 324 is no multiple of 8
        assert_route(kernels_run(lambda: fn(pd.half(), td.half())), present=(vec,), absent=(generic,))  # 336 = 8 · 42


def test_identical_inputs_give_exact_zeros():
    for shape in ((3, 7, 12, 28), (3, 7, 9, 37), (2, 3, 1, 2 * P + 4)):
        _, t, _, _ = _sam_case(shape, 255.0)
        td = t.cuda()
        got_map, got_sums = _sam_run(td, td.clone())
        assert not got_map.any() and not got_sums.any()
        assert not torch.isnan(got_map).any()


@pytest.mark.parametrize("which", ["preds", "target"])
def test_zero_vectors_give_nan_in_their_pixel_only(which):
    for shape in ((3, 7, 12, 28), (3, 7, 9, 37)):
        p, t, _, _ = _sam_case(shape)
        pd, td = p.cuda().clone(), t.cuda().clone()
        clean_map, clean_sums = _sam_run(pd, td)
        (pd if which == "preds" else td)[1, :, 5, 11] = 0.0
        got_map, got_sums = _sam_run(pd, td)
        hit = torch.zeros_like(got_map, dtype=torch.bool)
        hit[1, 5, 11] = True
        assert bool(torch.isnan(got_map[hit]).all()) and torch.equal(got_map[~hit], clean_map[~hit])
        assert bool(torch.isnan(got_sums[1])) and torch.equal(got_sums[[0, 2]], clean_sums[[0, 2]])


def test_clamp_keeps_antiparallel_vectors_at_pi():
    p, _, _, _ = _sam_case((3, 7, 12, 28), 255.0)
    pd = p.cuda() + 1.0  # no zero vector
    got_map, got_sums = _sam_run(pd, -pd)
    pi32 = torch.tensor(math.pi, dtype=torch.float32)
    ulp = float(torch.nextafter(pi32, torch.tensor(4.0)) - pi32)
    assert not torch.isnan(got_map).any()
    assert float((got_map.cpu() - pi32).abs().max()) <= ulp
    assert float((got_sums.cpu() / (12 * 28) - math.pi).abs().max()) <= ulp


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16_bit_inputs_convert_on_load(dtype):
    img = _ops()
    for shape in ((7, 5, 16, 24), (7, 5, 9, 37), (7, 3, 1, 4 * P + 8)):  # vector, generic, vector with a part-filled third workgroup
        p, t = vo.noisy_pair(shape, 16)
        p16, t16 = p.to(dtype), t.to(dtype)
        got_map, got_sums = _sam_run(p16.cuda(), t16.cuda())
        assert torch.equal(got_map, img.sam_map(p16.float().cuda(), t16.float().cuda()))
        assert torch.equal(got_sums, img.sam_sums(p16.float().cuda(), t16.float().cuda()))
        a64, a32 = so.sam_angles(p16.float(), t16.float()), so.sam_angles(p16.float(), t16.float(), torch.float32)
        vo.value_rule(f"sam/{dtype}/{_ids(shape)}", got_map.flatten(), a64.flatten(), a32.flatten())
        scores = img.ergas_scores(p16.cuda(), t16.cuda(), 4.0)
        assert torch.equal(scores, img.ergas_scores(_offset(p16.cuda()), _offset(t16.cuda()), 4.0))
        # ERGAS adds fp32 sums of one 16-byte vector (8 elements here, 4 of the up-cast) in fp64: each vector sum of positive terms
        # is within 7 · 2^-24 of exact, so SSE and Σt are, and the score sqrt(SSE) / Σt within 1.5 times that on either side
        up = img.ergas_scores(p16.float().cuda(), t16.float().cuda(), 4.0)
        assert bool(((scores - up).abs() <= 2 * 1.5 * 7 * 2.0**-24 * up).all())
        vo.value_rule(f"ergas/{dtype}/{_ids(shape)}", scores, so.ergas_scores(p16.float(), t16.float(), 4.0),
                      so.ergas_scores(p16.float(), t16.float(), 4.0, torch.float32))


def test_non_contiguous_inputs():
    img = _ops()
    p, t = vo.noisy_pair((14, 9, 12, 28), 21)
    pd, td = p.cuda(), t.cuda()
    for label, sl in (("channel-slice", (slice(0, 7), slice(1, 8))), ("batch-stride", (slice(None, None, 2), slice(0, 7)))):
        pv, tv = pd[sl], td[sl]
        assert not pv.is_contiguous()
        a64, a32 = so.sam_angles(p[sl], t[sl]), so.sam_angles(p[sl], t[sl], torch.float32)
        vo.value_rule(f"sam/{label}", img.sam_map(pv, tv).flatten(), a64.flatten(), a32.flatten())
        vo.value_rule(f"ergas/{label}", img.ergas_scores(pv, tv, 4.0), so.ergas_scores(p[sl], t[sl], 4.0),
                      so.ergas_scores(p[sl], t[sl], 4.0, torch.float32))


# ---------------------------------------------------------------------------------------------------------------- ERGAS
@functools.lru_cache(maxsize=None)
def _ergas_case(shape, scale, ratio):
    p, t = vo.noisy_pair(shape, 900 + 7 * shape[1] + shape[2] * shape[3], scale)
    return p, t, so.ergas_scores(p, t, ratio), so.ergas_scores(p, t, ratio, torch.float32)


def _ergas_check(label, shape, scale, ratio):
    img = _ops()
    p, t, e64, e32 = _ergas_case(shape, scale, ratio)
    pd, td = p.cuda(), t.cuda()
    got = img.ergas_scores(pd, td, ratio)
    assert got.dtype == torch.float64 and got.shape == (shape[0],)
    assert torch.equal(img.ergas_scores(pd, td, ratio), got)
    assert torch.equal(img.ergas_scores(_offset(pd), _offset(td), ratio), got)  # the generic kernel
    return vo.value_rule(f"ergas/{label}", got, e64, e32)


@pytest.mark.parametrize("ratio", [4.0, 0.5])
@pytest.mark.parametrize("scale", [1.0, 255.0])
@pytest.mark.parametrize("c", [1, 3, 8])
@pytest.mark.parametrize("hw", [(1, E - 1), (2, E // 2), (1, E + 1), (1, 2 * E + 3), (4, E // 2 + 2)], ids=_ids)
def test_ergas_planes(hw, c, scale, ratio):
    """Planes of ``E − 1``, ``E``, ``E + 1``, ``2E + 3`` and ``2E + 8`` elements; the last two are split into two chunks, the second one short."""
    shape = (7, c, *hw)
    n = hw[0] * hw[1]
    assert _ops().ergas_chunks(*shape) == (2 if n > 2 * E else 1)
    _ergas_check(f"{_ids(shape)}@{scale}x{ratio}", shape, scale, ratio)


def test_ergas_chunks_is_a_function_of_the_shape():
    chunks = _ops().ergas_chunks
    assert chunks(7, 3, 1, 2 * E + 3) == 2 and chunks(7, 3, 1, 2 * E - 1) == 1 and chunks(7, 3, 1, 1) == 1
    assert chunks(1, 7, 512, 2048) == 256 and chunks(7, 1, 512, 2048) == 256  # min(ceil(2048 / 7), 2^20 / E) chunks of E elements
    assert chunks(64, 32, 100, 100) == 1 and chunks(4096, 1, 1000, 1000) == 1  # enough planes: no split
    assert chunks(16, 3, 256, 256) == 16 and chunks(4, 8, 1024, 1024) == 64


def test_ergas_long_sums():
    """Seven one-band images of 512 x 2048: a million-term sum per plane, which a long fp32 running sum does not hold to the rule."""
    _ergas_check("7x1x512x2048", (7, 1, 512, 2048), 255.0, 4.0)


def test_ergas_zero_mean_band():
    import torchmetrics_forked_amd.functional.image.ergas as ergas_mod

    p, t = vo.noisy_pair((4, 3, 12, 28), 41)
    sign = torch.ones(12, 28)
    sign[:, 1::2] = -1.0
    t[0, 1] = sign  # mean exactly 0 in any order, SSE > 0: x / 0 = inf
    p[1, 0] = 0.0
    t[1, 0] = 0.0  # 0 / 0 = NaN
    t[2, 2] = -t[2, 2]  # a negative mean is squared away: finite
    got = _ops().ergas_scores(p.cuda(), t.cuda(), 4.0).cpu()
    with torch.no_grad():
        comp = ergas_mod._ergas_compute(p, t, 4.0, "none")  # the composition, on the CPU
    assert torch.equal(torch.isinf(got), torch.isinf(comp)) and torch.equal(torch.isnan(got), torch.isnan(comp))
    assert torch.isinf(got).tolist() == [True, False, False, False] and torch.isnan(got).tolist() == [False, True, False, False]
    fin = [2, 3]
    want = so.ergas_scores(p, t, 4.0)
    assert float((got[fin] - want[fin]).abs().max()) <= 1e-5 * float(want[fin].max())


# --------------------------------------------------------------------------------------------------------------- routes
_COMPOSITION_MARKS = ("acos", "norm", "Norm")
_ERGAS_COMPOSITION_MARKS = ("sqrt", "pow")  # the native route takes its root inside ergas_fold_kernel
_NATIVE_MARKS = ("sam_vec_kernel", "sam_generic_kernel", "ergas_plane", "ergas_fold_kernel")


def test_routes(monkeypatch):
    from torchmetrics_forked_amd.functional.image.ergas import error_relative_global_dimensionless_synthesis as ergas
    from torchmetrics_forked_amd.functional.image.sam import spectral_angle_mapper as sam
    from torchmetrics_forked_amd.image import ErrorRelativeGlobalDimensionlessSynthesis, SpectralAngleMapper

    tmx = torch.ops.tmx
    maps, sums, scores = (count_calls(monkeypatch, tmx, n) for n in ("sam_map", "sam_sums", "ergas_scores"))
    p, t = vo.noisy_pair((5, 3, 12, 28), 66)
    pd, td = p.cuda(), t.cuda()

    def seen():
        return len(maps), len(sums), len(scores)

    for i, reduction in enumerate(("elementwise_mean", "sum")):
        names = kernels_run(lambda: sam(pd, td, reduction=reduction))  # (two calls: a warm-up and the profiled one)
        assert_route(names, present=("sam_vec_kernel",), absent=_COMPOSITION_MARKS)
        assert seen() == (0, 2 * (i + 1), 0)
    for i, reduction in enumerate(("none", None)):
        names = kernels_run(lambda: sam(pd, td, reduction=reduction))
        assert_route(names, present=("sam_vec_kernel",), absent=_COMPOSITION_MARKS)
        assert seen() == (2 * (i + 1), 4, 0)
    for i, reduction in enumerate(("elementwise_mean", "sum", "none", None)):
        names = kernels_run(lambda: ergas(pd, td, 4, reduction))
        assert_route(names, present=("ergas_plane_vec_kernel", "ergas_fold_kernel"), absent=_ERGAS_COMPOSITION_MARKS)
        assert seen() == (4, 4, 2 * (i + 1))

    def module_run(m):
        m.reset()
        m.update(pd[:2], td[:2])
        m.update(pd[2:], td[2:])
        return m.compute()

    before = seen()
    m = SpectralAngleMapper("sum").cuda()
    assert_route(kernels_run(lambda: module_run(m)), present=("sam_vec_kernel",), absent=_COMPOSITION_MARKS)
    assert seen() == (before[0], before[1] + 4, before[2])
    m = SpectralAngleMapper("none").cuda()
    assert_route(kernels_run(lambda: module_run(m)), present=("sam_vec_kernel",), absent=_COMPOSITION_MARKS)
    assert seen() == (before[0] + 2, before[1] + 4, before[2])
    m = ErrorRelativeGlobalDimensionlessSynthesis().cuda()
    assert_route(kernels_run(lambda: module_run(m)), present=("ergas_plane_vec_kernel", "ergas_fold_kernel"), absent=_ERGAS_COMPOSITION_MARKS)
    assert seen() == (before[0] + 2, before[1] + 4, before[2] + 2)

    # kept on the composition: fp64, gradients; 3-D inputs raise before the gate
    before = seen()
    names = kernels_run(lambda: sam(pd.double(), td.double()))
    assert any("acos" in n for n in names), sorted(set(names))  # the mark is a real kernel name
    assert_route(names, absent=_NATIVE_MARKS)
    names = kernels_run(lambda: ergas(pd.double(), td.double()))
    assert any("sqrt" in n for n in names), sorted(set(names))
    assert_route(names, absent=_NATIVE_MARKS)
    pg = pd.clone().requires_grad_()
    assert_route(kernels_run(lambda: sam(pg, td)), absent=_NATIVE_MARKS)
    assert_route(kernels_run(lambda: ergas(pg, td)), absent=_NATIVE_MARKS)
    out = sam(pg, td) + ergas(pg, td)
    out.backward()
    assert pg.grad is not None and bool(torch.isfinite(pg.grad).all())
    for fn in (sam, ergas):
        with pytest.raises(ValueError, match="BxCxHxW"):
            fn(pd[0], td[0])
    assert seen() == before


def _seven(shape, scale):
    return [vo.noisy_pair(shape, 500 + s, scale) for s in range(7)]


@pytest.mark.parametrize("scale,ratio", [(1.0, 4.0), (255.0, 0.5)])
def test_functionals_and_modules_end_to_end(scale, ratio):
    from torchmetrics_forked_amd.functional.image.ergas import error_relative_global_dimensionless_synthesis as ergas
    from torchmetrics_forked_amd.functional.image.sam import spectral_angle_mapper as sam
    from torchmetrics_forked_amd.image import ErrorRelativeGlobalDimensionlessSynthesis, SpectralAngleMapper

    shape = (5, 7, 9, 37)
    keys = ("sam_mean", "sam_sum", "sam_mean_module", "sam_sum_module", "ergas_mean", "ergas_sum", "ergas_mean_module")
    got = {k: [] for k in keys}
    want64 = {k: [] for k in ("sam_mean", "sam_sum", "ergas_mean", "ergas_sum")}
    want32 = {k: [] for k in want64}
    for i, (p, t) in enumerate(_seven(shape, scale)):
        pd, td = p.cuda(), t.cuda()
        a64, a32 = so.sam_angles(p, t), so.sam_angles(p, t, torch.float32)
        e64, e32 = so.ergas_scores(p, t, ratio), so.ergas_scores(p, t, ratio, torch.float32)
        got["sam_mean"].append(sam(pd, td))
        got["sam_sum"].append(sam(pd, td, reduction="sum"))
        got["ergas_mean"].append(ergas(pd, td, ratio))
        got["ergas_sum"].append(ergas(pd, td, ratio, "sum"))
        assert all(got[k][-1].dtype == torch.float32 and got[k][-1].dim() == 0 for k in want64)
        for k, m in (("sam_mean_module", SpectralAngleMapper()), ("sam_sum_module", SpectralAngleMapper("sum")),
                     ("ergas_mean_module", ErrorRelativeGlobalDimensionlessSynthesis(ratio))):
            m = m.cuda()
            m.update(pd[:2], td[:2])  # two unequal batches
            m.update(pd[2:], td[2:])
            got[k].append(m.compute())
        for k, (o, c) in (("sam_mean", (a64.mean(), a32.mean())), ("sam_sum", (a64.sum(), a32.sum())), ("ergas_mean", (e64.mean(), e32.mean())),
                          ("ergas_sum", (e64.sum(), e32.sum()))):
            want64[k].append(o.double())
            want32[k].append(c.double())
        if i == 0:
            out = sam(pd, td, reduction="none")
            assert out.dtype == torch.float32 and out.shape == a64.shape
            vo.value_rule(f"functional@{scale}/sam_none", out.flatten(), a64.flatten(), a32.flatten())
            m = SpectralAngleMapper("none").cuda()
            m.update(pd[:2], td[:2])
            m.update(pd[2:], td[2:])
            assert torch.equal(m.compute(), out)
            vo.value_rule(f"functional@{scale}/ergas_none", torch.cat([ergas(pd, td, ratio, "none"), ergas(pd[:2], td[:2], ratio, None)]),
                          torch.cat([e64, e64[:2]]), torch.cat([e32, e32[:2]]))
    for k, v in got.items():
        o = "_".join(k.split("_")[:2])
        vo.value_rule(f"functional@{scale}/{k}", torch.stack([x.double().cpu() for x in v]), torch.stack(want64[o]), torch.stack(want32[o]))


def test_16_bit_functionals_return_the_input_dtype():
    from torchmetrics_forked_amd.functional.image.ergas import error_relative_global_dimensionless_synthesis as ergas
    from torchmetrics_forked_amd.functional.image.sam import spectral_angle_mapper as sam

    p, t = vo.noisy_pair((3, 7, 12, 28), 77)
    for dtype, rel in ((torch.bfloat16, 2.0**-8), (torch.float16, 2.0**-11)):
        p16, t16 = p.to(dtype), t.to(dtype)
        a64, e64 = so.sam_angles(p16.float(), t16.float()), so.ergas_scores(p16.float(), t16.float(), 4.0)
        for reduction, want in (("none", a64), ("sum", a64.sum()), ("elementwise_mean", a64.mean())):
            out = sam(p16.cuda(), t16.cuda(), reduction=reduction)
            assert out.dtype == dtype and out.shape == want.shape
            # fp32-class values (1e-5 relative at the most) rounded once to the input dtype (half an ulp)
            assert float((out.double().cpu() - want).abs().max()) <= (rel + 1e-5) * float(want.abs().max())
        out = ergas(p16.cuda(), t16.cuda(), 4.0, "none")
        assert out.dtype == dtype and float((out.double().cpu() - e64).abs().max()) <= (rel + 1e-5) * float(e64.max())


def test_no_host_read():
    from torchmetrics_forked_amd.functional.image.ergas import error_relative_global_dimensionless_synthesis as ergas
    from torchmetrics_forked_amd.functional.image.sam import spectral_angle_mapper as sam

    p, t = vo.noisy_pair((3, 3, 1, 2 * P + 4), 67)  # three workgroups per image: the fold kernel runs too
    pd, td = p.cuda(), t.cuda()

    def run():
        return [sam(pd, td), sam(pd, td, reduction="sum"), sam(pd, td, reduction="none"), ergas(pd, td), ergas(pd, td, 0.5, "none")]

    want = run()  # (first calls outside the guarded region)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = run()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
