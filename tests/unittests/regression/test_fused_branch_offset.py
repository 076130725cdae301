"""The Python algebra of the fused branches (Pearson, Concordance, explained variance) on the CPU: ``fused_ok`` is
patched to True, so the branches run on the eager moment table, whose rounding is the kernel's.  Data sits far from
zero, where raw moments cancel; the reference is the centred fp64 oracle with its error budget."""
import pytest
import torch

from tests.helpers import oracles as O
from torchmetrics_forked_amd.ops import regression as reg_ops


@pytest.fixture()
def fused_on_cpu(monkeypatch):
    monkeypatch.setattr(reg_ops, "fused_ok", lambda *tensors: True)


def test_eager_table_matches_oracle_on_offset_data():
    p, t = O.offset_batches([4099], 3, 1e4, 1.0, seed=1)[0]
    table, budget = O.regression_table_exact(p, t)
    err = (reg_ops.regression_sums(p, t) - table).abs()
    assert (err[:7] <= budget[:7]).all(), err[:7] / budget[:7]
    assert (budget[:7] <= 1e-6 * table[:7].abs()).all()


# (batch sizes, mean, std, state dtype, correlation).  The last case has rho = 0.95: its raw-moment budget,
# 4(N+2)·2⁻⁵³·Σ|xy| = 9e-4 of N·std², has to stay below 1e-3 of corr_xy = rho·N·std² as well
CASES = [([4096], 273.15, 0.5, torch.float32, 0.5), ([4096] * 4, 1e4, 1.0, torch.float32, 0.5), ([1] * 300, 1e4, 1.0, torch.float64, 0.5),
         ([17] * 100, 273.15, 0.5, torch.float64, 0.5), ([1, 2, 4096, 17], 1e5, 10.0, torch.float64, 0.5),
         ([20000] * 3, 1e4, 1.0, torch.float32, 0.95)]


@pytest.mark.parametrize("sizes,mean,std,state_dtype,rho", CASES)
@pytest.mark.parametrize("d_cols", [1, 3])
def test_fused_pearson_states_on_offset_data(fused_on_cpu, sizes, mean, std, state_dtype, rho, d_cols):
    from torchmetrics_forked_amd.functional.regression.concordance import _concordance_corrcoef_compute
    from torchmetrics_forked_amd.functional.regression.pearson import _pearson_corrcoef_compute, _pearson_corrcoef_update

    batches = O.offset_batches(sizes, d_cols, mean, std, seed=7 + d_cols, rho=rho)
    want, bud = O.pearson_states_exact(batches, state_dtype)
    states = tuple(torch.zeros(d_cols, dtype=state_dtype) for _ in range(6))
    for p, t in batches:
        states = _pearson_corrcoef_update(p, t, *states, num_outputs=d_cols)
    got = dict(zip(("mean_x", "mean_y", "var_x", "var_y", "corr_xy", "n_total"), states))
    for k in ("var_x", "var_y", "corr_xy"):
        err = (got[k].double() - want[k]).abs()
        assert (bud[k] <= 1e-3 * want[k].abs()).all(), (k, bud[k] / want[k].abs())
        assert (err <= bud[k]).all(), (k, err / bud[k])
    assert torch.equal(got["n_total"].double(), want["n_total"])
    tol = 3 * O.relative_state_budget(want, bud)
    vx, vy, cxy, n = got["var_x"], got["var_y"], got["corr_xy"], got["n_total"]
    ref = O.pearson_from_states(want)
    assert ((_pearson_corrcoef_compute(vx, vy, cxy, n).double().reshape(-1) - ref) / ref).abs().max() <= tol
    ccc = _concordance_corrcoef_compute(got["mean_x"], got["mean_y"], vx, vy, cxy, n)
    ref = O.concordance_from_states(want)
    assert ((ccc.double().reshape(-1) - ref) / ref).abs().max() <= tol


def test_fused_pearson_first_single_sample_has_zero_variance(fused_on_cpu):
    from torchmetrics_forked_amd.functional.regression.pearson import _pearson_corrcoef_update

    p, t = O.offset_batches([1], 3, 1e4, 1.0, seed=2)[0]
    states = _pearson_corrcoef_update(p, t, *(torch.zeros(3, dtype=torch.float64) for _ in range(6)), num_outputs=3)
    assert all(torch.equal(s, torch.zeros(3, dtype=torch.float64)) for s in states[2:5])
    assert torch.equal(states[0], p[0].double()) and torch.equal(states[1], t[0].double())


@pytest.mark.parametrize("ndim", [1, 2])
def test_fused_explained_variance_sum_error(fused_on_cpu, ndim):
    """Σ(t−p) from the fused table: Σt and Σp are subtracted in fp64 and rounded once to the output dtype (the u term),
    so the result is within (u + N·2⁻⁵³)·Σ|t−p| of the exact value.  Casting both sums to fp32 first was off by about
    15 at N = 20000, mean 1e4."""
    from torchmetrics_forked_amd.functional.regression.explained_variance import _explained_variance_update

    g = torch.Generator().manual_seed(5)
    p = (1e4 + 1.0 + torch.randn(20000, 2, generator=g, dtype=torch.float64)).float()
    t = (1e4 + torch.randn(20000, 2, generator=g, dtype=torch.float64)).float()
    if ndim == 1:
        p, t = p[:, 0], t[:, 0]
    n, sum_error, sse, st, sst = _explained_variance_update(p, t)
    d = (t.double() - p.double()).reshape(20000, -1)
    exact, mag = d.sum(0), d.abs().sum(0)
    bound = (2.0 ** -24 + 20000 * 2.0 ** -53) * mag
    assert n == 20000 and sum_error.dtype == torch.float32 and sum_error.shape == p.shape[1:]
    assert ((sum_error.double().reshape(-1) - exact).abs() <= bound).all(), (sum_error, exact)
    assert torch.equal(st.reshape(-1), t.double().reshape(20000, -1).sum(0).float())
