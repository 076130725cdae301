"""The regression moment kernels of csrc/regression.hip (``regression_sums``, ``pearson_update``,
``regression_accumulate``) against the independent fp64 oracles of tests/helpers/oracles.py, at every lane mapping of
the kernel, on every op branch, and on data that sits far from zero, where raw moments cancel.  Every comparison is
``error <= budget`` with the budget derived in the oracle's docstring; each test prints its largest error / budget."""
import functools

import pytest
import torch

from tests.helpers import oracles as O
from torchmetrics_forked_amd import ops
from torchmetrics_forked_amd.ops import regression as K

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
STATE_NAMES = ("mean_x", "mean_y", "var_x", "var_y", "corr_xy", "n_total")


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _report(name: str, ratio: float) -> None:
    print(f"[moments] {name}: max error/budget {ratio:.3g}")


def _ratio(err: torch.Tensor, budget: torch.Tensor) -> float:
    """Largest err / budget; an entry with zero budget must have zero error."""
    assert (err[budget == 0] == 0).all()
    return float((err / budget.clamp(min=torch.finfo(torch.float64).tiny)).max()) if err.numel() else 0.0


# --------------------------------------------------------------------------------- a. table channels 0-6

# every mapping of the kernel: W = tile width, R = 64 / W rows packed per wave, 16 or 4·R rows per block
SHAPES = [(1, 1), (2, 1), (63, 1), (257, 3), (130, 63), (9, 64), (9, 65), (5000, 65), (300, 67), (70, 96), (40, 129),
          (20011, 64), (525065, 1)]


@functools.lru_cache(maxsize=None)
def _column_data(shape, dtype, seed=0):
    """Column c has offset 3c − D and scale 1 + c/8 (sign-mixed): a column or lane mix-up moves every channel."""
    n, d = shape
    g = torch.Generator().manual_seed(1000 * seed + n + d)
    c = torch.arange(d, dtype=torch.float64)
    p = ((3 * c - d) + (1 + c / 8) * torch.randn(n, d, generator=g, dtype=torch.float64)).to(dtype)
    t = ((3 * c - d) + (1 + c / 8) * torch.randn(n, d, generator=g, dtype=torch.float64)).to(dtype)
    table, budget = O.regression_table_exact(p, t)
    return p, t, table, budget


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_table_channels_vs_oracle(shape, dtype):
    p, t, table, budget = _column_data(shape, dtype)
    pg, tg = p.cuda(), t.cuda()
    out = torch.ops.tmx.regression_sums(pg, tg, O.REG_NONE, 0.0)
    again = torch.ops.tmx.regression_sums(pg, tg, O.REG_NONE, 0.0)
    assert out.shape == (8, shape[1]) and out.dtype == torch.float64
    assert torch.equal(out, again)
    err = (out.cpu() - table).abs()
    ratios = [_ratio(err[ch], budget[ch]) for ch in range(7)]
    _report(f"table {shape} {dtype} per channel " + " ".join(f"{r:.2g}" for r in ratios), max(ratios))
    for ch in range(7):
        assert ratios[ch] <= 1.0, (ch, ratios[ch], out[ch].cpu(), table[ch])
    assert torch.equal(out[7].cpu(), torch.zeros(shape[1], dtype=torch.float64))


def test_table_strided_views_and_mixed_dtypes():
    """A transposed view, a ``[:, ::2]`` slice and fp32 preds with an fp64 target through the Python entry point."""
    p, t, _, _ = _column_data((300, 67), torch.float32)
    pg, tg = p.cuda(), t.cuda()
    ratios = []
    for name, view in (("transposed", lambda a: a.t()), ("sliced", lambda a: a[:, ::2])):
        table, budget = O.regression_table_exact(view(p).contiguous(), view(t).contiguous())
        assert not view(pg).is_contiguous()
        out = K.regression_sums(view(pg), view(tg))
        assert out.shape == table.shape
        ratios.append(_ratio((out.cpu() - table).abs()[:7], budget[:7]))
    t64 = t.double() + 1e-9  # not representable in fp32: a demotion of the target would show
    table, budget = O.regression_table_exact(p, t64)
    out = K.regression_sums(pg, t64.cuda())
    ratios.append(_ratio((out.cpu() - table).abs()[:7], budget[:7]))
    _report("table views / mixed dtypes", max(ratios))
    assert max(ratios) <= 1.0, ratios


# ------------------------------------------------------------------------------------------- b. channel 7

def _signed(g, shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * 2


def _op_data(kind: str, shape, g):
    if kind == "zeros":  # sign-mixed, exact zeros in t (rows 0, 7, ...) and in both p and t (rows 0, 14, ...)
        p, t = _signed(g, shape), _signed(g, shape)
        t[::7] = 0.0
        p[::14] = 0.0
        return p, t
    if kind == "signed":
        return _signed(g, shape), _signed(g, shape)
    if kind == "sle":  # values in (−0.9, 3.1)
        return (torch.rand(*shape, generator=g, dtype=torch.float64) * 4 - 0.9 for _ in range(2))
    if kind == "logcosh":  # d within ±6
        p = torch.randn(*shape, generator=g, dtype=torch.float64)
        return p, p + torch.rand(*shape, generator=g, dtype=torch.float64) * 11.8 - 5.9
    if kind == "count":  # p > 0, t ≥ 0 with exact zeros
        p = torch.rand(*shape, generator=g, dtype=torch.float64) * 3 + 0.05
        t = torch.rand(*shape, generator=g, dtype=torch.float64) * 3
        t[::5] = 0.0
        return p, t
    assert kind == "positive"
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 3 + 0.05 for _ in range(2))


OP_CASES = [("ape", O.REG_APE, 0.0, "zeros"), ("sape", O.REG_SAPE, 0.0, "zeros"), ("sle", O.REG_SLE, 0.0, "sle"),
            ("logcosh", O.REG_LOGCOSH, 0.0, "logcosh"), ("minkowski1", O.REG_MINKOWSKI, 1.0, "signed"),
            ("minkowski2", O.REG_MINKOWSKI, 2.0, "signed"), ("minkowski3", O.REG_MINKOWSKI, 3.0, "signed"),
            ("minkowski2.5", O.REG_MINKOWSKI, 2.5, "signed"), ("abs_t", O.REG_ABS_T, 0.0, "signed"),
            ("tweedie0", O.REG_TWEEDIE, 0.0, "signed"), ("tweedie1", O.REG_TWEEDIE, 1.0, "count"),
            ("tweedie1.5", O.REG_TWEEDIE, 1.5, "count"), ("tweedie-1", O.REG_TWEEDIE, -1.0, "count"),
            ("tweedie2", O.REG_TWEEDIE, 2.0, "positive"), ("tweedie3", O.REG_TWEEDIE, 3.0, "positive")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", [(4099, 3), (513, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name,op,param,kind", OP_CASES, ids=[c[0] for c in OP_CASES])
def test_op_channel_vs_oracle(name, op, param, kind, shape, dtype):
    g = torch.Generator().manual_seed(op * 100 + int(abs(param) * 10) + shape[1])
    p, t = (v.to(dtype) for v in _op_data(kind, shape, g))
    if kind == "zeros":
        assert int((t == 0).sum()) > 0 and int(((t == 0) & (p == 0)).sum()) > 0
    table, budget = O.regression_table_exact(p, t, op, param)
    out = torch.ops.tmx.regression_sums(p.cuda(), t.cuda(), op, param).cpu()
    assert torch.isfinite(out).all()
    err = (out - table).abs()
    r7, r06 = _ratio(err[7], budget[7]), _ratio(err[:7], budget[:7])
    _report(f"op {name} {shape} {dtype} (budget/|sum| {float((budget[7] / table[7].abs()).max()):.2g})", r7)
    assert (budget[7] <= 1e-5 * table[7].abs()).all(), budget[7] / table[7].abs()
    assert r7 <= 1.0, (r7, out[7], table[7])
    assert r06 <= 1.0, r06


# ------------------------------------------------------------- c. pearson_update on data far from zero

def _run_pearson_update(batches, state_dtype, d_cols):
    states = [torch.zeros(d_cols, dtype=state_dtype, device="cuda") for _ in range(6)]
    for p, t in batches:
        torch.ops.tmx.pearson_update(p.cuda(), t.cuda(), *states)
    return {k: s.cpu().double() for k, s in zip(STATE_NAMES, states)}


def _check_states(name, got, want, bud):
    ratios = {}
    for k in ("var_x", "var_y", "corr_xy"):
        assert (bud[k] <= 1e-3 * want[k].abs()).all(), (k, bud[k] / want[k].abs())
        ratios[k] = _ratio((got[k] - want[k]).abs(), bud[k])
    _report(f"pearson_update {name} (budget/|state| {O.relative_state_budget(want, bud):.2g})", max(ratios.values()))
    assert max(ratios.values()) <= 1.0, ratios
    assert torch.equal(got["n_total"], want["n_total"])


# (name, batch sizes, mean, std)
F64_STATE_CASES = [("300x1", [1] * 300, 1e4, 1.0), ("100x17", [17] * 100, 273.15, 0.5), ("mixed", [1, 2, 4096, 17], 1e5, 10.0)]


@pytest.mark.parametrize("d_cols", [1, 3, 65])
@pytest.mark.parametrize("name,sizes,mean,std", F64_STATE_CASES, ids=[c[0] for c in F64_STATE_CASES])
def test_pearson_update_offset_fp64_states(name, sizes, mean, std, d_cols):
    batches = O.offset_batches(sizes, d_cols, mean, std, seed=d_cols)
    want, bud = O.pearson_states_exact(batches, torch.float64)
    got = _run_pearson_update(batches, torch.float64, d_cols)
    _check_states(f"{name} D={d_cols} fp64 states", got, want, bud)
    for k in ("mean_x", "mean_y"):  # every batch mean carries (N_b+2)·2⁻⁵³ of its sum, every stored update one rounding
        assert ((got[k] - want[k]).abs() <= (sum(sizes) + 4 * len(sizes)) * 2.0 ** -53 * want[k].abs()).all(), k


@pytest.mark.parametrize("d_cols", [1, 3, 65])
def test_pearson_update_empty_batch_and_single_first_sample(d_cols):
    batches = O.offset_batches([1, 40, 0, 9], d_cols, 1e4, 1.0, seed=20 + d_cols)
    states = [torch.zeros(d_cols, dtype=torch.float64, device="cuda") for _ in range(6)]
    torch.ops.tmx.pearson_update(batches[0][0].cuda(), batches[0][1].cuda(), *states)
    for s in states[2:5]:  # one sample: x·x − x·(x/1) with exact products is exactly 0
        assert torch.equal(s.cpu(), torch.zeros(d_cols, dtype=torch.float64))
    assert torch.equal(states[0].cpu(), batches[0][0][0].double()) and torch.equal(states[5].cpu(), torch.ones(d_cols, dtype=torch.float64))
    torch.ops.tmx.pearson_update(batches[1][0].cuda(), batches[1][1].cuda(), *states)
    before = [s.clone() for s in states]
    assert batches[2][0].shape == (0, d_cols)
    torch.ops.tmx.pearson_update(batches[2][0].cuda(), batches[2][1].cuda(), *states)
    assert all(torch.equal(a, b) for a, b in zip(before, states))
    torch.ops.tmx.pearson_update(batches[3][0].cuda(), batches[3][1].cuda(), *states)
    want, bud = O.pearson_states_exact(batches, torch.float64)
    _check_states(f"empty batch D={d_cols}", {k: s.cpu() for k, s in zip(STATE_NAMES, states)}, want, bud)


# (name, batch sizes, D, rho).  3 x 20000 has rho = 0.95: its raw-moment budget 4(N+2)·2⁻⁵³·Σ|xy| is 9e-4 of N·std², and
# it has to stay below 1e-3 of corr_xy = rho·N·std² as well
F32_STATE_CASES = [("4x4096", [4096] * 4, 1, 0.5), ("4x4096", [4096] * 4, 65, 0.5), ("3x20000", [20000] * 3, 3, 0.95)]


@pytest.mark.parametrize("name,sizes,d_cols,rho", F32_STATE_CASES, ids=[f"{c[0]}xD{c[2]}" for c in F32_STATE_CASES])
def test_pearson_update_offset_fp32_states(name, sizes, d_cols, rho):
    batches = O.offset_batches(sizes, d_cols, 1e4, 1.0, seed=30 + d_cols, rho=rho)
    want, bud = O.pearson_states_exact(batches, torch.float32)
    got = _run_pearson_update(batches, torch.float32, d_cols)
    _check_states(f"{name} D={d_cols} fp32 states", got, want, bud)


def test_pearson_update_fp64_inputs_at_the_raw_moment_limit():
    """fp64 inputs at |mean| / std = 1e4: the products are rounded in fp64, so the raw moments lose up to
    (mean/std)²·N·2⁻⁵³ of the variance (1.8e-4 at N = 4096 with the budget's factor 4).  This pins that limit."""
    batches = O.offset_batches([4096, 4096], 3, 1e4, 1.0, dtype=torch.float64, seed=40)
    want, bud = O.pearson_states_exact(batches, torch.float64)
    got = _run_pearson_update(batches, torch.float64, 3)
    _check_states("fp64 inputs mean/std=1e4", got, want, bud)


def test_pearson_update_bf16_inputs_fp32_states():
    batches = O.offset_batches([4096, 100, 4096], 3, 273.0, 0.5, dtype=torch.bfloat16, seed=41)
    want, bud = O.pearson_states_exact(batches, torch.float32)
    assert (want["var_x"] > 0).all() and (want["corr_xy"].abs() > 0).all()
    got = _run_pearson_update(batches, torch.float32, 3)
    _check_states("bf16 inputs 273 +- 0.5", got, want, bud)


# ------------------------------------------------------------------- d. modules and functionals

MODULE_CASES = [("4x4096", [4096] * 4, 1e4, 1.0), ("100x17", [17] * 100, 273.15, 0.5), ("1x4096", [4096], 273.15, 0.5)]


@pytest.mark.parametrize("use_forward", [False, True], ids=["update", "forward"])
@pytest.mark.parametrize("d_cols", [1, 3])
@pytest.mark.parametrize("name,sizes,mean,std", MODULE_CASES, ids=[c[0] for c in MODULE_CASES])
def test_modules_on_offset_data(name, sizes, mean, std, d_cols, use_forward):
    import torchmetrics_forked_amd.regression as RG

    batches = O.offset_batches(sizes, d_cols, mean, std, seed=50 + d_cols)
    want, bud = O.pearson_states_exact(batches, torch.float32)
    tol = 3 * O.relative_state_budget(want, bud)
    assert tol <= 3e-3
    worst = 0.0
    for cls, coef in ((RG.PearsonCorrCoef, O.pearson_from_states), (RG.ConcordanceCorrCoef, O.concordance_from_states)):
        m = cls(num_outputs=d_cols).cuda()
        for i, (p, t) in enumerate(batches):
            args = (p[:, 0].cuda(), t[:, 0].cuda()) if d_cols == 1 else (p.cuda(), t.cuda())
            if not use_forward:
                m.update(*args)
                continue
            batch_val = m(*args)
            if i in (0, len(batches) - 1):  # forward returns the value of this batch alone
                w1, b1 = O.pearson_states_exact([(p, t)], torch.float32)
                e1 = ((batch_val.cpu().double().reshape(-1) - coef(w1)) / coef(w1)).abs()
                # a small batch: the moment budget is a few 2⁻²⁴, and concordance also reads the fp32 means
                tol1 = 3 * O.relative_state_budget(w1, b1) + (O.concordance_mean_slack(w1, b1) if cls is RG.ConcordanceCorrCoef else 0.0)
                assert (e1 <= tol1).all(), (cls.__name__, "batch value", e1, tol1)
        ref = coef(want)
        err = float(((m.compute().cpu().double().reshape(-1) - ref) / ref).abs().max())
        worst = max(worst, err / tol)
        assert err <= tol, (cls.__name__, err, tol)
    _report(f"modules {name} D={d_cols} {'forward' if use_forward else 'update'} (tol {tol:.2g})", worst)


@pytest.mark.parametrize("d_cols", [1, 3])
@pytest.mark.parametrize("mean,std,n", [(273.15, 0.5, 4096), (1e4, 1.0, 4096), (1e4, 1.0, 20000)])
def test_functionals_on_offset_data(mean, std, n, d_cols):
    import torchmetrics_forked_amd.functional.regression as FR

    (p, t), = O.offset_batches([n], d_cols, mean, std, seed=60 + d_cols, rho=0.95 if n == 20000 else 0.5)
    want, bud = O.pearson_states_exact([(p, t)], torch.float32)
    tol = 3 * O.relative_state_budget(want, bud)
    assert tol <= 3e-3
    args = (p[:, 0].cuda(), t[:, 0].cuda()) if d_cols == 1 else (p.cuda(), t.cuda())
    worst = 0.0
    for fn, coef in ((FR.pearson_corrcoef, O.pearson_from_states), (FR.concordance_corrcoef, O.concordance_from_states)):
        ref = coef(want)
        err = float(((fn(*args).cpu().double().reshape(-1) - ref) / ref).abs().max())
        worst = max(worst, err / tol)
        assert err <= tol, (fn.__name__, err, tol)
    _report(f"functionals mean={mean} n={n} D={d_cols} (tol {tol:.2g})", worst)


@pytest.mark.parametrize("ndim", [1, 2])
def test_explained_variance_sum_error_on_offset_data(ndim):
    """Σ(t−p) within (u + N·2⁻⁵³)·Σ|t−p| of the exact value: Σt − Σp in fp64, rounded once to the output dtype."""
    from torchmetrics_forked_amd.functional.regression.explained_variance import _explained_variance_update

    g = torch.Generator().manual_seed(5)
    n = 20000
    p = (1e4 + 1.0 + torch.randn(n, 2, generator=g, dtype=torch.float64)).float()
    t = (1e4 + torch.randn(n, 2, generator=g, dtype=torch.float64)).float()
    if ndim == 1:
        p, t = p[:, 0], t[:, 0]
    num, sum_error, _, sum_target, _ = _explained_variance_update(p.cuda(), t.cuda())
    d = (t.double() - p.double()).reshape(n, -1)
    exact, bound = d.sum(0), (2.0 ** -24 + n * 2.0 ** -53) * d.abs().sum(0)
    assert num == n and sum_error.dtype == torch.float32 and sum_error.shape == p.shape[1:]
    err = (sum_error.cpu().double().reshape(-1) - exact).abs()
    _report(f"explained variance sum_error ndim={ndim}", _ratio(err, bound))
    assert (err <= bound).all(), (sum_error, exact)
    assert torch.equal(sum_target.cpu().reshape(-1), t.double().reshape(n, -1).sum(0).float())


# ------------------------------------------------------------------------- e. regression_accumulate

def _spacing(v: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Distance from |v| to the next larger value of ``dtype`` (one ulp of v in that type), as fp64."""
    a = v.abs().to(dtype)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


ACC_CASES = [(torch.float32, torch.float32), (torch.float32, torch.float64), (torch.float64, torch.float32)]


@pytest.mark.parametrize("in_dtype,state_dtype", ACC_CASES, ids=["f32->f32", "f32->f64", "f64->f32"])
@pytest.mark.parametrize("chans", [[5], [6, 0], [4, 7, 2], [3, 6, 1, 5]], ids=lambda c: "ch" + "".join(map(str, c)))
def test_regression_accumulate_vs_oracle(chans, in_dtype, state_dtype):
    """``state += table[chan]`` by the kernel's rounding rule: the fp64 column sum is cast to the inputs' dtype O, added
    in promote(S, O) and stored in the state dtype S.  The rule is applied to the oracle table.  The kernel's own sum
    may differ from the oracle's within the table budget, so the rule is also applied to table − budget and
    table + budget: where both give the same state (the rule is monotone), the kernel's state must equal it bit for
    bit; elsewhere a cast may fall on the other side of a rounding boundary, and agreement is asked to one ulp in the
    coarser of O and S, the precision the rule leaves in the state."""
    n, d_cols = 777, 65
    p, t, _, _ = _column_data((n, d_cols), in_dtype, seed=3)
    table, budget = O.regression_table_exact(p, t, O.REG_SAPE, 0.0)
    g = torch.Generator().manual_seed(sum(chans))
    start = [(torch.randn(d_cols, generator=g, dtype=torch.float64) * 100).to(state_dtype) for _ in chans]
    states = [s.cuda() for s in start]
    total = torch.tensor(5, dtype=torch.long, device="cuda")
    pg, tg = p.cuda(), t.cuda()
    torch.ops.tmx.regression_accumulate(pg[:0], tg[:0], O.REG_SAPE, 0.0, chans, states, total, 0)  # N = 0: a no-op
    assert all(torch.equal(a.cpu(), b) for a, b in zip(states, start)) and int(total) == 5
    torch.ops.tmx.regression_accumulate(pg, tg, O.REG_SAPE, 0.0, chans, states, total, n)
    assert int(total) == 5 + n
    coarse = torch.float32  # one of O and S in every case here
    acc = torch.promote_types(in_dtype, state_dtype)
    worst, pinned = 0.0, 0
    for ch, s0, s1 in zip(chans, start, states):
        rule = lambda v: (s0.to(acc) + v.to(in_dtype).to(acc)).to(state_dtype).double()  # noqa: E731
        want, lo, hi = rule(table[ch]), rule(table[ch] - budget[ch]), rule(table[ch] + budget[ch])
        exact = lo == hi
        pinned += int(exact.sum())
        ulp = torch.maximum(_spacing(want, coarse), _spacing(table[ch], coarse))
        err = (s1.cpu().double() - want).abs()
        worst = max(worst, float((err / ulp).max()))
        assert (err[exact] == 0).all(), (ch, "not bit-equal where the budget leaves one value", float(err[exact].max()))
        assert (err <= ulp).all(), (ch, float((err / ulp).max()))
    _report(f"accumulate {chans} {in_dtype}->{state_dtype} ({pinned} of {len(chans) * d_cols} bit-exact; rest in ulp)", worst)
    # without the counter: only the states move
    torch.ops.tmx.regression_accumulate(pg, tg, O.REG_SAPE, 0.0, chans, states, None, n)
    assert int(total) == 5 + n
