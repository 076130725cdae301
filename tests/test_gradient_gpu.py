"""Native PSNR with blocked effect, total variation and image gradients (``tmx::psnrb_sums`` / ``tmx::tv_sums`` / ``tmx::image_gradients``,
``csrc/neighbour_diff.hip``) against the dense fp64 oracles of ``tests/helpers/gradient_oracle.py``, and the routes of
``peak_signal_noise_ratio_with_blocked_effect``, ``total_variation``, ``image_gradients`` and the two modules.

Value rule (``vif_oracle.value_rule``): ``|native − oracle64| <= 4 |comp32 − oracle64| + 1e-6 max|oracle64|`` with ``comp32`` the same oracle in fp32 on
the CPU.  Inputs are ``vif_oracle.noisy_pair``.  Every comparison takes its maximum over at least 7 entries: ``tv_sums`` runs on seven
images, the scalars of ``psnrb_sums`` and of the functionals as vectors over seven seeds (``tests/test_vif_gpu.py`` has the argument).
Every comparison prints one ``vif_err`` line (``-s``).

What is held to more than the rule: two runs are bit-equal; the 16-byte-load kernels are bit-equal to the generic ones (every
value case runs the same data a second time at a one-element storage offset, which only the generic kernels accept); the minimum
and maximum of ``target`` are exact; a single planted integer pixel gives exact integer sums, each pair in exactly the right one
of ``D_B`` and ``D_BC``; ``image_gradients`` gives the bits of the CPU composition for fp32, bf16 and fp16, zeros included.

16-bit ``tv_sums`` and ``psnrb_sums`` against the same call on the up-cast input: bit-equal.  A thread owns eight 16-bit columns and four fp32
ones, so the two calls add in different orders; but bf16 / fp16 values at or above 2^-10 (the test asserts that of its inputs) are
multiples of 2^-20, their differences too and the squares of those of 2^-40, and a sum below 2^13 of such terms is exact in fp64 in
any order.

Measured on MI355X, error / bound: ``tv_sums`` at most 0.021 (median 0.0003, 97 comparisons), ``psnrb_sums`` at the tile edges at most 0.041
(median 0.0012, 70), over the block sizes at most 0.050 (54), 16-bit inputs 0 (their sums are exact), the functional's and the
module's ``sse``, ``bef``, data range and score (vectors over seven seeds) at most 0.14.

Mutants of ``csrc/neighbour_diff.hip``, the op built alone as a library outside the tree and run under this file one at a time (the
unchanged source built the same way passes in full), the first failing test of each and how many fail:
* last row owning a vertical pair dropped (``i < H − 1`` as ``i < H − 2``): ``test_tv_tile_edges[2-1-1.0]``, 196 of 220;
* strip count floored: ``test_tv_tile_edges[33-2-1.0]``, 77 (every ``H`` of ``RS + 1`` and ``2 RS + 1``);
* column-block count floored: ``test_tv_tile_edges[1-515-1.0]``, 76 (every ``W`` of ``CW + 1`` and ``2 CW + 3``);
* halo row not read (each wave's last pair dropped): ``test_tv_tile_edges[31-1-1.0]``, 150;
* cross-vector pair dropped: ``test_tv_tile_edges[1-5-1.0]``, 155;
* boundary test ``(j + 1) % bs`` written as ``j % bs``: ``test_psnrb_tile_edges[2-2-1.0]``, 88, no ``tv`` or ``image_gradients`` test among them;
* row and column boundary flags swapped: ``test_psnrb_tile_edges[2-255-1.0]``, 78 (the square ``2 x 2`` plane passes, as it must);
* ``D_B`` and ``D_BC`` swapped: ``test_psnrb_tile_edges[2-2-1.0]``, 89;
* plane index masked to 16 bits: ``test_many_planes`` alone;
* ``dx`` zero column not written: ``test_image_gradients_tile_edges[torch.float32-1]``, 32, with ``test_many_planes`` and ``test_no_host_read``.
Not built: any guard ``<=`` for ``<`` on a load or a store (``r < nrows``, ``k < valid``, ``row0 + r < H``): each reads or writes one row or one
element past a plane, for the last plane past the end of the allocation, and a kernel that reads or writes out of bounds is not
run on a shared device.  By construction each adds a pair or a pixel that ``test_pair_ownership`` counts exactly.
"""
import functools

import pytest
import torch

from tests.helpers import gradient_oracle as go
from tests.helpers import vif_oracle as vo
from tests.helpers.routes import assert_route, count_calls, kernels_run
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu

CW, RS, V = 256, 32, 4  # asserted against gradient_tile() below: parametrisation happens before the library is loaded
WR = 8  # rows a wave walks down inside a strip
_HS = [2, RS - 1, RS, RS + 1, 2 * RS + 1]
_WS = [2, V - 1, V + 1, CW - 1, CW, CW + 1, 2 * CW + 3]


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


def _same_bits(a, b):
    """Bit equality, NaN included (``torch.equal`` takes NaN for unequal to itself)."""
    view = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16, torch.float16: torch.int16}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def test_tile_is_what_the_shapes_assume():
    assert _ops().gradient_tile() == (CW, RS)


# ------------------------------------------------------------------------------------------------------- total variation
def _tv_run(d):
    """``tv_sums``; asserts on the way that a second run and the run at a storage offset give the same bits."""
    img = _ops()
    got = img.tv_sums(d)
    assert got.dtype == torch.float64 and got.shape == (d.shape[0],)
    assert _same_bits(img.tv_sums(d), got) and _same_bits(img.tv_sums(_offset(d)), got)
    return got


@functools.lru_cache(maxsize=None)
def _tv_case(shape, scale):
    x, _ = vo.noisy_pair(shape, 7 * shape[2] + shape[3], scale)
    return x, go.tv(x), go.tv(x, torch.float32)


@pytest.mark.parametrize("scale", [1.0, 255.0])
@pytest.mark.parametrize("w", [1, *_WS])
@pytest.mark.parametrize("h", [1, *_HS])
def test_tv_tile_edges(h, w, scale):
    x, t64, t32 = _tv_case((7, 2, h, w), scale)
    got = _tv_run(x.cuda())
    if h == 1 and w == 1:
        assert not got.any()
    vo.value_rule(f"tv/{h}x{w}@{scale}", got, t64, t32)


# ---------------------------------------------------------------------------------------------------------------- PSNR-B
def _psnrb_run(pd, td, bs):
    img = _ops()
    got = img.psnrb_sums(pd, td, bs)
    assert got.dtype == torch.float64 and got.shape == (5,)
    assert _same_bits(img.psnrb_sums(pd, td, bs), got) and _same_bits(img.psnrb_sums(_offset(pd), _offset(td), bs), got)
    return got


def _psnrb_check(label, shape, bs, scale=1.0, seeds=7):
    """Seven seeds of one shape: the three sums by the value rule as vectors over the seeds, minimum and maximum exactly."""
    got, s64, s32 = [], [], []
    for seed in range(seeds):
        p, t = vo.noisy_pair(shape, 100 * seed + shape[2] + 3 * shape[3], scale)
        got.append(_psnrb_run(p.cuda(), t.cuda(), bs).cpu())
        s64.append(go.psnrb_sums(p, t, bs))
        s32.append(go.psnrb_sums(p, t, bs, torch.float32))
    got, s64, s32 = (torch.stack(v).T for v in (got, s64, s32))  # [5, seeds]: the rule's maximum runs over the seeds
    assert torch.equal(got[3:], s64[3:])
    return vo.value_rule(f"psnrb/{label}", got[:3], s64[:3], s32[:3].double())


@pytest.mark.parametrize("scale", [1.0, 255.0])
@pytest.mark.parametrize("w", _WS)
@pytest.mark.parametrize("h", _HS)
def test_psnrb_tile_edges(h, w, scale):
    _psnrb_check(f"{h}x{w}@{scale}", (2, 1, h, w), 8, scale)


@pytest.mark.parametrize("bs", [1, 2, 3, 5, 8, 16])
def test_psnrb_block_sizes(bs):
    """``W − 1`` and ``H − 1`` of ``bs − 1``, ``bs`` and ``bs + 1``: no boundary pair on the axis, the first one, and one pair past it."""
    sizes = [n for n in (bs, bs + 1, bs + 2) if n >= 2]
    for h in sizes:
        for w in sizes:
            _psnrb_check(f"bs{bs}/{h}x{w}", (2, 1, h, w), bs)


@pytest.mark.parametrize("shape,bs", [((2, 1, 33, 20), 50), ((2, 1, 20, 33), 34), ((2, 1, 65, 20), 8), ((2, 1, 20, 65), 8), ((2, 1, 41, 300), 7)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_psnrb_block_sizes_on_unequal_axes(shape, bs):
    """``bs > max(H, W)`` (no boundary pair at all: ``D_B`` is exactly 0) and planes whose two axes hold different numbers of boundaries."""
    _psnrb_check(f"bs{bs}/{shape[2]}x{shape[3]}", shape, bs)
    if bs > max(shape[2:]):
        p, t = vo.noisy_pair(shape, 5)
        assert float(_ops().psnrb_sums(p.cuda(), t.cuda(), bs)[1]) == 0.0


# -------------------------------------------------------------------------------------------------------- pair ownership
_PH, _PW, _PBS = 2 * RS + 1, 2 * CW + 4, 8  # a multiple of the vector width: the planted planes run the vector kernels too
_POSITIONS = sorted({(i, j) for i in (0, 1, WR - 1, WR, RS - 1, RS, 2 * RS - 1, 2 * RS) for j in (0, 1, V - 1, V, CW - 1, CW, 2 * CW - 1, 2 * CW, _PW - 2, _PW - 1)}
                    | {(i, j) for i in (_PH - 2, _PH - 1) for j in (0, 5, CW - 1, CW, _PW - 1)})


def _pairs_of(i, j):
    """``(neighbours, boundary pairs)`` of the pixel ``(i, j)`` of a ``_PH`` x ``_PW`` plane with ``_PBS`` blocks."""
    pairs = [(a + 1) % _PBS == 0 for a, n in ((j - 1, _PW), (j, _PW), (i - 1, _PH), (i, _PH)) if 0 <= a < n - 1]
    return len(pairs), sum(pairs)


def test_pair_ownership():
    """One pixel of value 3 in a zero plane, moved over the corners, the last row and column, and the rows and columns on both sides
    of a wave, strip, vector and workgroup edge: integers, so every sum is exact."""
    assert {n for n, _ in map(_pairs_of, *zip(*_POSITIONS))} == {2, 3, 4}
    x = torch.zeros(len(_POSITIONS), 1, _PH, _PW)
    for n, (i, j) in enumerate(_POSITIONS):
        x[n, 0, i, j] = 3.0
    d = x.cuda()
    want = torch.tensor([3.0 * _pairs_of(i, j)[0] for i, j in _POSITIONS], dtype=torch.float64)
    assert torch.equal(_tv_run(d).cpu(), want), [(p, float(g), float(w)) for p, g, w in zip(_POSITIONS, _tv_run(d).cpu(), want) if g != w]
    zeros = torch.zeros(1, 1, _PH, _PW, device="cuda")
    for n, (i, j) in enumerate(_POSITIONS):
        pairs, boundary = _pairs_of(i, j)
        got = _psnrb_run(d[n:n + 1], zeros, _PBS).tolist()
        assert got == [9.0, 9.0 * boundary, 9.0 * (pairs - boundary), 0.0, 0.0], ((i, j), got)
    # every pair of the plane at once: a plane of alternating rows and columns differs by 1 across every pair
    yy, xx = torch.meshgrid(torch.arange(_PH), torch.arange(_PW), indexing="ij")
    board = ((yy + xx) % 2).float()[None, None].cuda()
    nb = _PH * len(go.pair_lists(_PW, _PBS)[0]) + _PW * len(go.pair_lists(_PH, _PBS)[0])
    every = _PH * (_PW - 1) + _PW * (_PH - 1)
    assert float(_tv_run(board)) == every
    assert _psnrb_run(board, board, _PBS).tolist() == [0.0, float(nb), float(every - nb), 0.0, 1.0]


# ------------------------------------------------------------------------------------------------------ PSNR-B end to end
def _module_oracle(parts, bs, dtype):
    """What the module holds after one update per part: ``sse`` and ``bef`` added per update, the widest data range, then the score."""
    sums = [go.psnrb_sums(p, t, bs, dtype) for p, t in parts]
    h, w = parts[0][0].shape[2:]
    sse = sum(s[0] for s in sums)
    bef = sum(go.bef(s, h, w, bs) for s in sums)
    data_range = max(s[4] - s[3] for s in sums)
    mse = sse / sum(p.numel() for p, _ in parts) + bef
    score = 10 * torch.log10(data_range**2 / mse) if bool(data_range > 2) else 10 * torch.log10(1.0 / mse)
    return torch.stack([sse, bef, data_range, score]).double()


@pytest.mark.parametrize("scale", [1.0, 255.0])
@pytest.mark.parametrize("kind", ["blocky", "unblocky"])
def test_psnrb_end_to_end(kind, scale):
    from torchmetrics_forked_amd.functional.image.psnrb import _psnrb_update_with_range
    from torchmetrics_forked_amd.functional.image.psnrb import peak_signal_noise_ratio_with_blocked_effect as psnrb
    from torchmetrics_forked_amd.image import PeakSignalNoiseRatioWithBlockedEffect

    shape, bs = (5, 1, 37, 43), 8
    got_f, got_m, f64, f32, m64, m32 = [], [], [], [], [], []
    for seed in range(7):
        p, t = go.planted_pair(shape, 300 + seed, scale, kind, bs)
        parts = [(p[:2], t[:2]), (p[2:], t[2:])]  # two updates of different batch sizes
        for a, b in [(p, t), *parts]:
            # the comparison never rests on a coin-flip branch: both oracles take the planted branch, by a wide margin
            for dtype in (torch.float64, torch.float32):
                is_blocky, margin = go.blocky(go.psnrb_sums(a, b, bs, dtype), shape[2], shape[3], bs)
                assert is_blocky == (kind == "blocky") and margin > 1e-3
        pd, td = p.cuda(), t.cuda()
        sse, bef, n, data_range = _psnrb_update_with_range(pd, td, bs)
        assert n == p.numel() and all(v.dtype == torch.float32 and v.dim() == 0 for v in (sse, bef, data_range))
        score = psnrb(pd, td, block_size=bs)
        assert score.dtype == torch.float32 and score.dim() == 0
        got_f.append(torch.stack([sse, bef, data_range, score]).double().cpu())
        f64.append(_module_oracle([(p, t)], bs, torch.float64))
        f32.append(_module_oracle([(p, t)], bs, torch.float32))
        m = PeakSignalNoiseRatioWithBlockedEffect(block_size=bs).cuda()
        for a, b in parts:
            m.update(a.cuda(), b.cuda())
        assert int(m.total) == p.numel()
        got_m.append(torch.stack([m.sum_squared_error, m.bef, m.data_range, m.compute()]).double().cpu())
        m64.append(_module_oracle(parts, bs, torch.float64))
        m32.append(_module_oracle(parts, bs, torch.float32))
    for label, got, o64, o32 in (("functional", got_f, f64, f32), ("module", got_m, m64, m32)):
        got, o64, o32 = (torch.stack(v).T for v in (got, o64, o32))  # [sse, bef, data range, score] x seeds
        assert bool((got[1] > 0).all()) if kind == "blocky" else not got[1].any()
        vo.value_rule(f"psnrb_{label}/{kind}@{scale}", got, o64, o32)


# ------------------------------------------------------------------------------------------------------- image gradients
def _gradients_check(x):
    """``image_gradients`` of the CPU tensor ``x`` on the GPU, aligned and at a storage offset, into buffers the caching allocator hands
    back full of NaN: the bits of the CPU composition, and exact zeros in the last row of ``dy`` and the last column of ``dx``."""
    import torchmetrics_forked_amd.functional.image.gradients as grad_mod

    want_dy, want_dx = grad_mod._compute_image_gradients(x)
    o_dy, o_dx = go.gradients(x)
    assert _same_bits(want_dy, o_dy) and _same_bits(want_dx, o_dx)
    for d in (x.cuda(), _offset(x.cuda())):
        poison = [torch.full(x.shape, float("nan"), dtype=x.dtype, device="cuda") for _ in range(2)]
        del poison
        dy, dx = _ops().image_gradients(d)
        assert dy.shape == x.shape and dx.shape == x.shape and dy.is_contiguous() and dx.is_contiguous()
        assert _same_bits(dy.cpu(), want_dy) and _same_bits(dx.cpu(), want_dx), tuple(x.shape)
        assert not dy[:, :, -1, :].any() and not dx[:, :, :, -1].any()
        assert not torch.isnan(dy).any() and not torch.isnan(dx).any()


@pytest.mark.parametrize("h", [1, 2, WR - 1, WR, WR + 1, RS - 1, RS, RS + 1, 2 * RS + 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
def test_image_gradients_tile_edges(dtype, h):
    v = 16 // torch.empty(0, dtype=dtype).element_size()
    cw = 64 * v
    for w in (1, 2, v - 1, v, v + 1, cw - 1, cw, cw + 1, 2 * cw + 3, 2 * cw + v):
        x, _ = vo.noisy_pair((2, 2, h, w), h + w, 255.0)
        _gradients_check(x.to(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
def test_image_gradients_non_contiguous(dtype):
    import torchmetrics_forked_amd.functional.image.gradients as grad_mod

    x, _ = vo.noisy_pair((3, 5, RS + 1, 2 * CW), 12, 255.0)
    x = x.to(dtype)
    d = x.cuda()
    for label, sl in (("channel-slice", (slice(None), slice(1, 4))), ("batch-stride", (slice(None, None, 2),)),
                      ("column-slice", (slice(None), slice(None), slice(None), slice(3, 2 * CW - 2)))):
        view = d[sl]
        assert not view.is_contiguous(), label
        want_dy, want_dx = grad_mod._compute_image_gradients(x[sl])
        dy, dx = grad_mod.image_gradients(view)
        assert _same_bits(dy.cpu(), want_dy) and _same_bits(dx.cpu(), want_dx), label


# ---------------------------------------------------------------------------------------------------------- 16-bit sums
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_16_bit_sums_convert_on_load(dtype):
    from torchmetrics_forked_amd.functional.image.psnrb import peak_signal_noise_ratio_with_blocked_effect as psnrb
    from torchmetrics_forked_amd.functional.image.tv import total_variation

    img = _ops()
    # vector kernel, generic kernel, and three 16-bit workgroups across (five fp32 ones) with a part-filled last one
    for shape in ((7, 1, RS + 1, 24), (7, 1, 2 * RS + 1, 37), (7, 1, 9, 4 * CW + 8)):
        p, t = vo.noisy_pair(shape, 16)
        p16, t16 = p.to(dtype), t.to(dtype)
        for v in (p16, t16):  # (the docstring's exactness argument)
            assert float(v[v != 0].float().abs().min()) >= 2.0**-10
        got = _tv_run(p16.cuda())
        assert _same_bits(got, img.tv_sums(p16.float().cuda()))
        vo.value_rule(f"tv/{dtype}/{shape[2]}x{shape[3]}", got, go.tv(p16.float()), go.tv(p16.float(), torch.float32))
        sums = torch.stack([_psnrb_run(p16[n:n + 1].cuda(), t16[n:n + 1].cuda(), 8) for n in range(7)])
        up = torch.stack([img.psnrb_sums(p16[n:n + 1].float().cuda(), t16[n:n + 1].float().cuda(), 8) for n in range(7)])
        assert _same_bits(sums, up)
        s64 = torch.stack([go.psnrb_sums(p16[n:n + 1].float(), t16[n:n + 1].float(), 8) for n in range(7)])
        s32 = torch.stack([go.psnrb_sums(p16[n:n + 1].float(), t16[n:n + 1].float(), 8, torch.float32) for n in range(7)])
        vo.value_rule(f"psnrb/{dtype}/{shape[2]}x{shape[3]}", sums.T.cpu(), s64.T, s32.T.double())
        out = total_variation(p16.cuda(), reduction="none")
        assert out.dtype == dtype and out.shape == (7,)
        rel = 2.0**-8 if dtype == torch.bfloat16 else 2.0**-11
        # fp64 sums rounded once to the input dtype (half an ulp)
        assert float((out.double().cpu() - go.tv(p16.float())).abs().max()) <= (rel + 1e-6) * float(go.tv(p16.float()).max())
        score = psnrb(p16.cuda(), t16.cuda())
        assert score.dtype == dtype and score.dim() == 0 and bool(torch.isfinite(score))


# -------------------------------------------------------------------------------------------------------------- specials
def test_nan_and_inf_pixels():
    from torchmetrics_forked_amd.functional.image.psnrb import peak_signal_noise_ratio_with_blocked_effect as psnrb
    from torchmetrics_forked_amd.functional.image.tv import total_variation

    p, t = vo.noisy_pair((2, 1, RS + 3, CW + 5), 31)
    pd, td = p.cuda(), t.cuda()
    clean = _psnrb_run(pd, td, 8)
    nan = float("nan")
    # target: NaN minimum, maximum and sse; no bit of D_B or D_BC changes
    tn = td.clone()
    tn[1, 0, 17, 100] = nan
    got = _psnrb_run(pd, tn, 8)
    assert torch.isnan(got).tolist() == [True, False, False, True, True] and _same_bits(got[1:3], clean[1:3])
    # preds: exactly the sums the pixel's pairs belong to.  (3, 3): four inner pairs; (3, 7): the pair (7, 8) crosses a boundary
    for (i, j), d_b_nan in (((3, 3), False), ((3, 7), True), ((RS - 1, CW), True), ((RS + 1, CW + 2), False)):
        pn = pd.clone()
        pn[0, 0, i, j] = nan
        got = _psnrb_run(pn, td, 8)
        assert torch.isnan(got).tolist() == [True, d_b_nan, True, False, False], ((i, j), got.tolist())
        assert _same_bits(got[3:], clean[3:]) and (d_b_nan or _same_bits(got[1], clean[1]))
        tv = _tv_run(pn)
        assert torch.isnan(tv).tolist() == [True, False] and _same_bits(tv[1], _tv_run(pd)[1])
    pn = pd.clone()
    pn[0, 0, 3, 3] = nan
    got = _psnrb_run(pn, td, 1)  # block size 1: every pair is a boundary pair
    assert torch.isnan(got).tolist() == [True, True, False, False, False] and float(got[2]) == 0.0
    # infinities do not raise
    for value in (float("inf"), -float("inf")):
        pi, ti = pd.clone(), td.clone()
        pi[0, 0, 3, 7] = value
        ti[1, 0, 5, 5] = value
        got = _psnrb_run(pi, ti, 8)
        assert float(got[0]) == float("inf") and float(got[1]) == float("inf") and float(got[2]) == float("inf")
        assert float(got[3 if value < 0 else 4]) == value
        psnrb(pi, ti)
        assert float(total_variation(pi)) == float("inf")
        dy, dx = _ops().image_gradients(pi)
        assert int(torch.isinf(dy).sum()) == 2 and int(torch.isinf(dx).sum()) == 2


# ----------------------------------------------------------------------------------------------------------- many planes
def test_many_planes():
    """70 000 planes of 2 x 3: the plane index does not fit a 16-bit grid axis."""
    import torchmetrics_forked_amd.functional.image.gradients as grad_mod

    shape = (70000, 1, 2, 3)
    x, _ = vo.noisy_pair(shape, 70)
    got = _tv_run(x.cuda())
    vo.value_rule("tv/b70000", got, go.tv(x), go.tv(x, torch.float32))
    dy, dx = _ops().image_gradients(x.cuda())
    want_dy, want_dx = grad_mod._compute_image_gradients(x)
    assert _same_bits(dy.cpu(), want_dy) and _same_bits(dx.cpu(), want_dx)


# ---------------------------------------------------------------------------------------------------------------- routes
_NATIVE_MARKS = ("tv_vec_kernel", "tv_generic_kernel", "tv_fold_kernel", "psnrb_vec_kernel", "psnrb_generic_kernel", "psnrb_fold_kernel",
                 "gradients_vec_kernel", "gradients_generic_kernel")
_TV_MARKS = ("abs", "Abs")
_PSNRB_MARKS = ("pow", "Pow")
_GRADIENTS_MARKS = ("elementwise_kernel",)  # the composition's subtractions and pad copies; the native route launches one kernel


def _composition(names, marks):
    assert any(m in n for n in names for m in marks), sorted(set(names))  # the mark is a real kernel name
    assert_route(names, absent=_NATIVE_MARKS)


def test_kernel_choice_by_alignment():
    img = _ops()
    x, t = vo.noisy_pair((2, 1, 12, 28), 3)
    d, td = x.cuda(), t.cuda()
    for fn, name in ((img.tv_sums, "tv"), (img.image_gradients, "gradients"), (lambda a: img.psnrb_sums(a, td[..., :a.shape[-1]], 8), "psnrb")):
        vec, generic = f"{name}_vec_kernel", f"{name}_generic_kernel"
        assert_route(kernels_run(lambda: fn(d)), present=(vec,), absent=(generic,))
        assert_route(kernels_run(lambda: fn(d[..., :27])), present=(generic,), absent=(vec,))  # made contiguous: 27 columns
        assert_route(kernels_run(lambda: fn(d[..., :24])), present=(vec,), absent=(generic,))
    assert_route(kernels_run(lambda: img.tv_sums(_offset(d))), present=("tv_generic_kernel",), absent=("tv_vec_kernel",))
    assert_route(kernels_run(lambda: img.psnrb_sums(d, _offset(td), 8)), present=("psnrb_generic_kernel",), absent=("psnrb_vec_kernel",))
    assert_route(kernels_run(lambda: img.tv_sums(d[..., :28].half())), present=("tv_generic_kernel",), absent=("tv_vec_kernel",))  # 28 is no multiple of 8
    assert_route(kernels_run(lambda: img.tv_sums(d[..., :24].half())), present=("tv_vec_kernel",), absent=("tv_generic_kernel",))


def test_routes(monkeypatch):
    import torchmetrics_forked_amd.functional.image.gradients as grad_mod
    import torchmetrics_forked_amd.functional.image.psnrb as psnrb_mod
    import torchmetrics_forked_amd.functional.image.tv as tv_mod
    from torchmetrics_forked_amd.image import PeakSignalNoiseRatioWithBlockedEffect, TotalVariation

    psnrb, tv, gradients = psnrb_mod.peak_signal_noise_ratio_with_blocked_effect, tv_mod.total_variation, grad_mod.image_gradients
    tmx = torch.ops.tmx
    calls = [count_calls(monkeypatch, tmx, n) for n in ("psnrb_sums", "tv_sums", "image_gradients")]

    def seen():
        return tuple(len(c) for c in calls)

    p, t = vo.noisy_pair((5, 1, 2 * RS + 1, 28), 66)
    pd, td = p.cuda(), t.cuda()
    x = vo.noisy_pair((5, 3, 2 * RS + 1, 28), 67)[0].cuda()  # three strips and three planes per image: the fold kernel runs

    # routed calls (kernels_run makes two calls: a warm-up and the profiled one)
    assert_route(kernels_run(lambda: psnrb(pd, td)), present=("psnrb_vec_kernel", "psnrb_fold_kernel"), absent=_PSNRB_MARKS)
    assert seen() == (2, 0, 0)
    assert_route(kernels_run(lambda: tv(x)), present=("tv_vec_kernel", "tv_fold_kernel"), absent=_TV_MARKS)
    assert_route(kernels_run(lambda: tv(x.bfloat16(), "none")), present=("tv_generic_kernel",), absent=_TV_MARKS)  # 28 is no multiple of 8
    assert seen() == (2, 4, 0)
    names = kernels_run(lambda: gradients(x))
    assert_route(names, present=("gradients_vec_kernel",), absent=_GRADIENTS_MARKS)
    assert seen() == (2, 4, 2)

    def module_run(m, *batches):
        m.reset()
        for b in batches:
            m.update(*b)
        return m.compute()

    m = PeakSignalNoiseRatioWithBlockedEffect().cuda()
    assert_route(kernels_run(lambda: module_run(m, (pd[:2], td[:2]), (pd[2:], td[2:]))), present=("psnrb_vec_kernel",), absent=_PSNRB_MARKS)
    assert seen() == (6, 4, 2)
    m = TotalVariation().cuda()
    assert_route(kernels_run(lambda: module_run(m, (x[:2],), (x[2:],))), present=("tv_vec_kernel",), absent=_TV_MARKS)
    assert seen() == (6, 8, 2)

    # kept on the composition: fp64, integer images, gradients, PSNR-B on a single row, and the knob
    before = seen()
    _composition(kernels_run(lambda: psnrb(pd.double(), td.double())), _PSNRB_MARKS)
    _composition(kernels_run(lambda: tv(x.double())), _TV_MARKS)
    _composition(kernels_run(lambda: gradients(x.double())), _GRADIENTS_MARKS)
    ints = (x * 255).long()
    _composition(kernels_run(lambda: tv(ints)), _TV_MARKS)
    _composition(kernels_run(lambda: gradients(ints)), _GRADIENTS_MARKS)
    _composition(kernels_run(lambda: psnrb(ints[:, :1], ints[:, :1] + 1)), _PSNRB_MARKS)
    row_p, row_t = (v.cuda() for v in go.planted_pair((5, 1, 1, 28), 9, 1.0, "unblocky"))  # H == 1 (d_b = 0: the composition's log2(1) stays unused)
    _composition(kernels_run(lambda: psnrb(row_p, row_t)), _PSNRB_MARKS)
    xg, pg = x.clone().requires_grad_(), pd.clone().requires_grad_()
    _composition(kernels_run(lambda: tv(xg)), _TV_MARKS)
    _composition(kernels_run(lambda: gradients(xg)), _GRADIENTS_MARKS)
    _composition(kernels_run(lambda: psnrb(pg, td)), _PSNRB_MARKS)
    (tv(xg) + sum(g.sum() for g in gradients(xg))).backward()
    psnrb(pg, td).backward()
    assert bool(torch.isfinite(xg.grad).all()) and bool(torch.isfinite(pg.grad).all())
    for mod in (psnrb_mod, tv_mod, grad_mod):
        monkeypatch.setattr(mod, "_GRADIENT_NATIVE", False)
    _composition(kernels_run(lambda: psnrb(pd, td)), _PSNRB_MARKS)
    _composition(kernels_run(lambda: tv(x)), _TV_MARKS)
    _composition(kernels_run(lambda: gradients(x)), _GRADIENTS_MARKS)
    with pytest.raises(ValueError, match="grayscale"):
        psnrb(x, x)
    assert seen() == before


def test_no_host_read():
    from torchmetrics_forked_amd.functional.image.gradients import image_gradients
    from torchmetrics_forked_amd.image import PeakSignalNoiseRatioWithBlockedEffect, TotalVariation

    p, t = vo.noisy_pair((3, 1, 2 * RS + 1, CW + 4), 67)  # several workgroups per image: the fold kernels run too
    pd, td = p.cuda(), t.cuda()
    x = vo.noisy_pair((3, 3, 2 * RS + 1, CW + 4), 68)[0].cuda()
    def fresh():
        return PeakSignalNoiseRatioWithBlockedEffect().cuda(), TotalVariation().cuda(), TotalVariation("none").cuda()

    def run(modules):
        modules[0].update(pd, td)
        modules[0].update(pd[:2], td[:2])
        for m in modules[1:]:
            m.update(x)
            m.update(x[:2])
        return [modules[0].sum_squared_error, modules[0].bef, modules[0].data_range, modules[0].total, modules[1].score,
                torch.cat(modules[2].score_list), *image_gradients(x)]

    want = run(fresh())  # (first calls outside the guarded region)
    guarded = fresh()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = run(guarded)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
