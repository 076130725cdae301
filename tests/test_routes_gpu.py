"""Which native route ran.  Ops that dispatch between several kernels inside one call are profiled
(``tests/helpers/routes.py`` ``kernels_run``) at the smallest shapes on each side of every gate: the kernel names that
must appear and those that must not, and the result against the oracle the op's own tests use (``torch.sort(stable=True)``,
the fp64 composition).  Python-level routes are observed by call counts (``count_calls``).

The native gates read their A/B environment knobs once per process, so the other arm of a gate is reached here by shape,
dtype or alignment only.  Run with one of those knobs set, exactly the cases of that route fail on their kernel names
while their result checks still pass."""
import pytest
import torch

from tests.helpers.routes import assert_route, count_calls, kernels_run
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _profiled(fn):
    """(kernel names, result) of the profiled call of ``fn``."""
    box = []
    names = kernels_run(lambda: box.append(fn()))
    return names, box[-1]


# ---------------------------------------------------------------------------------------------------- radix_sort
# radix_sort_impl (csrc/radix.hip): n <= 4096 per row -> one 256-thread workgroup per row; up to 8192 keys per row (any
# key width) -> one 1024-thread workgroup per row; one row up to 2^22 keys -> one-sweep passes; everything
# else -> prep / per-digit histogram + scatter launches / final, with a device-side digit plan for integer keys.
_SORT_KERNELS = ("sort_tile_kernel", "sort_block_kernel", "os_pass_kernel", "sort_prep_kernel", "rs_scatter_kernel",
                 "sort_plan_kernel", "sort_final_kernel", "sort_coop_kernel")
_SORT_ARMS = {
    "tile": ("sort_tile_kernel",),
    "block": ("sort_block_kernel",),
    "onesweep": ("os_pass_kernel",),
    "multi": ("sort_prep_kernel", "rs_scatter_kernel", "sort_final_kernel"),
    "multi-planned": ("sort_prep_kernel", "rs_scatter_kernel", "sort_plan_kernel", "sort_final_kernel"),
}
SORT_CASES = [
    (torch.float32, (4096,), "tile"),
    (torch.float32, (4097,), "block"),
    (torch.float32, (8192,), "block"),
    (torch.float32, (8193,), "onesweep"),
    (torch.float32, (16384,), "onesweep"),  # (no 16384-key workgroup kernel for 32-bit keys: 8 keys per lane, all widths)
    (torch.float32, (16385,), "onesweep"),
    (torch.int64, (8192,), "block"),
    (torch.int64, (8193,), "onesweep"),
    (torch.float32, (5, 8000), "block"),
    (torch.int64, (4, 70001), "multi-planned"),
    (torch.float32, (1 << 22,), "onesweep"),
    (torch.int32, (1 << 22,), "onesweep"),
    (torch.float32, ((1 << 22) + 1,), "multi"),
    (torch.int32, ((1 << 22) + 1,), "multi-planned"),
]


def _sort_data(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        x = ((torch.randn(shape, generator=g) * 100).round() / 4).to(dtype)  # many ties
        flat = x.view(-1)
        flat[3::97] = float("nan")
        flat[5::89] = float("inf")
        flat[7::83] = float("-inf")
        flat[11::79] = -0.0
        return x
    x = torch.randint(-(1 << 20), 1 << 20, shape, generator=g, dtype=dtype)
    flat = x.view(-1)
    flat[::5] = 7  # long tie run
    flat[1::101] = torch.iinfo(dtype).min
    flat[2::103] = torch.iinfo(dtype).max
    return x


@pytest.fixture(scope="module")
def sort_inputs():
    """Every case's input and its host ``torch.sort(stable=True)`` in both directions, computed once."""
    cache = {}

    def get(dtype, shape):
        key = (dtype, shape)
        if key not in cache:
            x = _sort_data(shape, dtype, seed=sum(shape))
            cache[key] = (x, {d: torch.sort(x, dim=-1, descending=d, stable=True) for d in (False, True)})
        return cache[key]

    return get


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype,shape,arm", SORT_CASES, ids=[f"{str(d)[6:]}-{'x'.join(map(str, s))}-{a}" for d, s, a in SORT_CASES])
def test_radix_sort_route(sort_inputs, dtype, shape, arm, descending):
    x, refs = sort_inputs(dtype, shape)
    xd = x.cuda()
    names, (v, i) = _profiled(lambda: torch.ops.tmx.radix_sort(xd, descending))
    ref = refs[descending]
    assert torch.equal(i.cpu(), ref.indices)
    bits = torch.int64 if x.element_size() == 8 else torch.int32
    assert torch.equal(v.cpu().view(bits), ref.values.view(bits))  # bit-identical (NaN payloads, signed zeros)
    want = _SORT_ARMS[arm]
    assert_route(names, present=want, absent=[k for k in _SORT_KERNELS if k not in want])


def test_sort_wrapper_calls_the_native_op_exactly_where_it_is_faster(monkeypatch):
    """``ops.sort.sort`` over the cases of ``test_sort_routing_picks_the_faster_engine``: ``tmx::radix_sort`` is called
    exactly where ``_faster_than_aten`` says so (not merely predicted), with the stable order either way."""
    from torchmetrics_forked_amd.ops import sort as S

    calls = count_calls(monkeypatch, torch.ops.tmx, "radix_sort")
    cases = [(torch.randn(3, 9000), True), (torch.randn(4000), True), (torch.randn(8000), True), (torch.randn(8000, dtype=torch.float64), False),
             (torch.randn(70_000), False), (torch.randn(300_000), True),
             (torch.randn(70_000, dtype=torch.float64), False), (torch.randint(0, 9, (1 << 20,)), True)]
    for x, native in cases:
        before = len(calls)
        v, i = S.sort(x.cuda())
        assert len(calls) - before == int(native) == int(S._faster_than_aten(x.cuda())), (x.shape, x.dtype)
        ref = torch.sort(x, stable=True)
        assert torch.equal(i.cpu(), ref.indices) and torch.equal(v.cpu(), ref.values)


# ----------------------------------------------------------------------------------------------------- ssim_sums
# ssim_sums (csrc/image.hip): fp32, W % 4 == 0, 16-B aligned planes, odd window <= 15 -> the packed fp32 kernel
# (ssim_v2_kernel); with the data range among the constants the matrix-core kernel runs first and ssim_v2_kernel is its
# device-side fallback launch; everything else -> ssim_valid_kernel.
_KS = 11


def _window(ks=_KS, sigma=1.5):
    w = torch.exp(-((torch.arange(ks, dtype=torch.float64) - (ks - 1) / 2) ** 2) / (2 * sigma**2))
    return w / w.sum()


def _ssim_sums_fp64(p, t, c1, c2):
    """Per-plane sums of SSIM and contrast sensitivity over the valid windows, composed in fp64 on the host."""
    w = _window()
    k = (w[:, None] * w[None, :])[None, None]
    conv = lambda x: torch.nn.functional.conv2d(x[:, None], k)[:, 0]  # noqa: E731
    p, t = p.double().cpu(), t.double().cpu()
    mp, mt = conv(p), conv(t)
    spp, stt, spt = conv(p * p) - mp * mp, conv(t * t) - mt * mt, conv(p * t) - mp * mt
    cs = (2 * spt + c2) / (spp + stt + c2)
    sim = (2 * mp * mt + c1) / (mp * mp + mt * mt + c1) * cs
    return torch.stack([sim.sum((1, 2)), cs.sum((1, 2))])


def _planes(shape, dtype, offset):
    g = torch.Generator().manual_seed(sum(shape))
    t = torch.rand(*shape, generator=g)
    p = (t + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
    out = []
    for x in (p, t):
        x = x.to(dtype)
        if offset:  # contiguous planes whose storage starts one element past a 16-B boundary
            buf = torch.empty(x.numel() + 1, dtype=dtype, device="cuda")
            view = buf[1:].view(shape)
            view.copy_(x)
            assert view.is_contiguous() and view.data_ptr() % 16 == x.element_size()
            out.append(view)
        else:
            out.append(x.cuda())
    return out


SSIM_CASES = [
    # (id, planes, dtype, storage offset, constants, present, absent)
    ("mfma", (6, 64, 64), torch.float32, False, 3, ["ssim_mfma_kernel"], ["ssim_valid_kernel"]),
    ("v2", (6, 64, 64), torch.float32, False, 2, ["ssim_v2_kernel"], ["ssim_mfma_kernel", "ssim_valid_kernel"]),
    ("W66", (6, 64, 66), torch.float32, False, 3, ["ssim_valid_kernel"], ["ssim_mfma_kernel", "ssim_v2_kernel"]),
    ("bf16", (6, 64, 64), torch.bfloat16, False, 3, ["ssim_valid_kernel"], ["ssim_mfma_kernel", "ssim_v2_kernel"]),
    ("offset", (6, 64, 64), torch.float32, True, 3, ["ssim_valid_kernel"], ["ssim_mfma_kernel", "ssim_v2_kernel"]),
]


@pytest.mark.parametrize("shape,dtype,offset,nconst,present,absent", [c[1:] for c in SSIM_CASES], ids=[c[0] for c in SSIM_CASES])
def test_ssim_sums_route(shape, dtype, offset, nconst, present, absent):
    p, t = _planes(shape, dtype, offset)
    c1, c2 = 0.01**2, 0.03**2
    consts = torch.tensor([c1, c2, 1.0][:nconst]).cuda()
    w = _window().float().cuda()
    names, sums = _profiled(lambda: torch.ops.tmx.ssim_sums(p, t, w, w, consts, False))
    nv = (shape[1] - _KS + 1) * (shape[2] - _KS + 1)
    ref = _ssim_sums_fp64(p, t, c1, c2)  # (on the quantised planes)
    # per-plane means: the 2e-5 of the fp32 SSIM tests, the 1e-2 of the 16-bit one (tests/test_ops_image_gpu.py)
    torch.testing.assert_close(sums[:2].cpu() / nv, ref / nv, rtol=0, atol=2e-5 if dtype == torch.float32 else 1e-2)
    assert_route(names, present, absent)


@pytest.mark.parametrize("data_range", [1.0, None])
def test_ssim_functional_takes_the_matrix_core_kernel(data_range):
    from torchmetrics_forked_amd.functional.image import structural_similarity_index_measure as ssim

    g = torch.Generator().manual_seed(7)
    t = torch.rand(2, 3, 64, 64, generator=g)
    p = (t + 0.1 * torch.randn(2, 3, 64, 64, generator=g)).clamp(0, 1)
    pd, td = p.cuda(), t.cuda()
    names, got = _profiled(lambda: ssim(pd, td, data_range=data_range, reduction="none"))
    assert torch.allclose(got.cpu(), ssim(p, t, data_range=data_range, reduction="none"), atol=2e-5)
    assert_route(names, present=["ssim_mfma_kernel"], absent=["ssim_valid_kernel"])


# ------------------------------------------------------------------ pairwise_gemm / pairwise_abs_cos_rowmax / kid
# csrc/pairwise.hip: >= 256 output tiles of 128 x 128 -> fp32 linear / cosine on the f16-split matrix-core route
# (x3_split_kernel + pairwise_gemm_x3_kernel; linear also launches the exact kernel as its device-side fallback for
# non-finite operands), 16-bit linear / cosine on pairwise_gemm_h16_kernel; fewer tiles, euclidean (fp64 accumulation)
# and fp64 -> pairwise_gemm_kernel.  (1921, D) x (2048, D) is 16 x 16 = 256 tiles, (1920, D) x (2048, D) 15 x 16 = 240.
_D, _M, _N_X3, _N_EXACT = 64, 2048, 1921, 1920
_PG_KERNELS = ("x3_split_kernel", "pairwise_gemm_x3_kernel", "pairwise_gemm_h16_kernel", "pairwise_gemm_kernel")


def _pg_ref(mode, x, y):
    xd, yd = x.double(), y.double()
    if mode == 0:
        return xd @ yd.T
    if mode == 1:
        return (xd / xd.norm(dim=1, keepdim=True)) @ (yd / yd.norm(dim=1, keepdim=True)).T
    return ((xd * xd).sum(1, keepdim=True) + (yd * yd).sum(1) - 2 * xd @ yd.T).to(x.dtype).double().sqrt()


def _pg_tol(mode, dtype):
    """rtol, atol of tests/test_pairwise_gemm_gpu.py for this op."""
    if dtype == torch.float32:
        return (2e-5, 2e-5 * _D**0.5) if mode == 0 else (1e-5, 1e-5)
    return 1e-2, (1e-2 * _D**0.5 if mode == 0 else 1e-2)


PG_CASES = [
    # (dtype, mode, rows of x, kernels that run)
    (torch.float32, 0, _N_X3, ("x3_split_kernel", "pairwise_gemm_x3_kernel", "pairwise_gemm_kernel")),
    (torch.float32, 1, _N_X3, ("x3_split_kernel", "pairwise_gemm_x3_kernel")),
    (torch.float32, 0, _N_EXACT, ("pairwise_gemm_kernel",)),
    (torch.float32, 1, _N_EXACT, ("pairwise_gemm_kernel",)),
    (torch.float32, 2, _N_X3, ("pairwise_gemm_kernel",)),  # euclidean: always the exact kernel
    (torch.bfloat16, 0, _N_X3, ("pairwise_gemm_h16_kernel",)),
    (torch.float16, 1, _N_X3, ("pairwise_gemm_h16_kernel",)),
    (torch.bfloat16, 1, _N_EXACT, ("pairwise_gemm_kernel",)),
    (torch.float16, 0, _N_EXACT, ("pairwise_gemm_kernel",)),
    (torch.bfloat16, 2, _N_X3, ("pairwise_gemm_kernel",)),
]


@pytest.mark.parametrize("dtype,mode,n,want", PG_CASES,
                         ids=[f"{str(d)[6:]}-{('linear', 'cosine', 'euclidean')[m]}-{n}" for d, m, n, _ in PG_CASES])
def test_pairwise_gemm_route(dtype, mode, n, want):
    g = torch.Generator().manual_seed(n + mode)
    x = torch.randn(n, _D, generator=g).to(dtype).cuda()
    y = torch.randn(_M, _D, generator=g).to(dtype).cuda()
    names, out = _profiled(lambda: torch.ops.tmx.pairwise_gemm(x, y, mode, False))
    rtol, atol = _pg_tol(mode, dtype)
    torch.testing.assert_close(out.double(), _pg_ref(mode, x, y), rtol=rtol, atol=atol)
    assert_route(names, present=want, absent=[k for k in _PG_KERNELS if k not in want])


def test_pairwise_gemm_inf_operand_runs_both_kernels():
    """An inf in a linear operand on the x3 route: the split kernel flags it and the exact kernel redoes the product."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(_N_X3, _D, generator=g).cuda()
    y = torch.randn(_M, _D, generator=g).cuda()
    x[5, 3] = float("inf")
    names, out = _profiled(lambda: torch.ops.tmx.pairwise_gemm(x, y, 0, False))
    torch.testing.assert_close(out.double(), _pg_ref(0, x, y), rtol=2e-5, atol=2e-4, equal_nan=True)
    assert torch.isinf(out[5]).any()
    assert_route(names, present=["x3_split_kernel", "pairwise_gemm_x3_kernel", "pairwise_gemm_kernel"], absent=["pairwise_gemm_h16_kernel"])


@pytest.mark.parametrize("n,want", [(_N_X3, ("x3_split_kernel", "pairwise_gemm_x3_kernel")), (_N_EXACT, ("pairwise_gemm_kernel",))])
def test_abs_cos_rowmax_route(n, want):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, _D, generator=g).cuda()
    y = torch.randn(_M, _D, generator=g).cuda()
    names, got = _profiled(lambda: torch.ops.tmx.pairwise_abs_cos_rowmax(x, y))
    ref = _pg_ref(1, x, y).abs().max(dim=1).values
    torch.testing.assert_close(got.double(), ref, rtol=2e-6, atol=2e-6)  # (test_pairwise_abs_cos_rowmax_vs_torch's)
    assert_route(names, present=want, absent=[k for k in _PG_KERNELS if k not in want])


@pytest.mark.parametrize("d,want,unwanted", [(256, "kid_poly_x3_kernel", "kid_poly_kernel"), (255, "kid_poly_kernel", "kid_poly_x3_kernel")])
def test_kid_poly_sums_route(d, want, unwanted):
    m, degree = 300, 3
    g = torch.Generator().manual_seed(d)
    real = torch.rand(m + 50, d, generator=g).cuda()
    fake = (torch.rand(m + 20, d, generator=g) * 1.1).cuda()
    ir, jf = torch.randperm(m + 50, generator=g)[:m], torch.randperm(m + 20, generator=g)[:m]
    gamma, coef = 1.0 / d, 1.0
    names, sums = _profiled(lambda: torch.ops.tmx.kid_poly_sums(real, fake, ir, jf, degree, gamma, coef))
    a, b = real.double()[ir.cuda()], fake.double()[jf.cuda()]
    k = lambda u, v: (u @ v.T * gamma + coef) ** degree  # noqa: E731
    kxx, kyy, kxy = k(a, a), k(b, b), k(a, b)
    ref = torch.stack([kxx.sum() - kxx.diag().sum(), kyy.sum() - kyy.diag().sum(), kxy.sum()])
    torch.testing.assert_close(sums, ref, rtol=2e-5, atol=2e-5 * m * m)  # (test_kid_poly_sums_vs_torch's fp32 bound)
    assert_route(names, present=[want], absent=[unwanted])
