"""Native ``signal_distortion_ratio`` (``tmx::sdr_scores`` / ``tmx::sdr_correlations``, ``csrc/sdr.hip``) against the longdouble oracle of
``tests/helpers/sdr_oracle.py``, and the routes of ``signal_distortion_ratio``, ``SignalDistortionRatio`` and ``permutation_invariant_training``.

Lag sums: on integer-valued signals in ``[-8, 8]`` every product and partial sum is an integer far below 2^53, so ``sdr_correlations`` must
equal the ``int64`` oracle exactly, whatever the order of the sums.

dB values: vectors of seven signals (or the entries of a pair matrix), each held to ``sdr_oracle.bound``:
``|got_i − oracle_i| <= 4 max_i |ref64_i − oracle_i| + L 2^-53 (10 / ln 10) / (coh_i (1 − coh_i))``, plus half an fp32 ulp of the result for the
functionals' fp32 values.  Every comparison prints one ``sdr_err`` line (``-s``) with error / bound.

Not pinned: ``preds == target``.  ``coh`` rounds to either side of 1 there (in the reference too), so the result is +inf, NaN or a very
large value depending on the last bit.

``test_exact_lag_sums*``, ``test_routes*`` and ``test_no_expansion`` need the ops, the gate and the route and fail without them.

Measured on MI355X, error / bound (minimum, median, maximum): ``test_values`` 0.016, 0.078, 0.28 over 20 cases; ``L = 513`` 0.013; ``test_pair_matrix`` 0.017,
0.033, 0.066 over six cases and 0.0055 for the row at ``L = 600``; one chunk and 13 forced chunks 0.082 and 0.11; 70 000 rows 0.044; the functionals' fp32 results 0.84 and 0.90 (the bound
there is little more than half an fp32 ulp); PIT's best metric 0.23 and 0.34; the matrix-core form (``TMX_SDR_CORR_FORM=mfma``, and as the default at ``T = 16 500``) 0.031, 0.11, 0.20 over four cases.  ``test_no_expansion`` measured a peak growth of 1.29 MiB
on the native route and 1.19 GiB through the composition, against the limit of 16 MiB.  The README names the mutants of ``csrc/sdr.hip``
this file was run against and the first test each fails.
"""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import sdr_oracle as so
from tests.helpers.routes import assert_route, count_calls, kernels_run
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu

LAG_TILE, LANE_LAGS, STAGE, MAX_L, WAVE_L, MAX_RHS, MFMA_LAGS, MFMA_MIN_T = 64, 16, 2048, 2048, 512, 8, 256, 16384  # asserted against sdr_tile() below
DIAG, ALL = 0, 1


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()
    so.require_longdouble()


def _op():
    from torchmetrics_forked_amd.ops import audio

    return audio


def _sdr_mod():
    from torchmetrics_forked_amd.functional.audio import sdr

    return sdr


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float64 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _offset(x):
    """The same values at a one-element storage offset: contiguous, 4-byte aligned only (2-byte for 16-bit types)."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    buf[1:].copy_(x.flatten())
    out = buf[1:].view(x.shape)
    assert out.is_contiguous() and out.data_ptr() % 8 != 0
    return out


def _report(label, ratio):
    print(f"sdr_err {label}: error/bound {ratio:.3g}")
    assert ratio <= 1.0, f"{label}: error is {ratio:.3g} of the bound"


def test_tile_is_what_the_shapes_assume():
    assert _op().sdr_tile() == (LAG_TILE, LANE_LAGS, STAGE, MAX_L, WAVE_L, MAX_RHS, MFMA_LAGS, MFMA_MIN_T)
    assert _sdr_mod()._SDR_MAX_FILTER == MAX_L


# -------------------------------------------------------------------------------------------------------- exact lag sums
def _check_exact(p, t, L, zero_mean=False, pairing=DIAG, means=None, pd=None, td=None):
    """``sdr_correlations`` of ``[G, S, T]`` integer-valued inputs against the int64 oracle, entry by entry."""
    pd = p.cuda() if pd is None else pd
    td = t.cuda() if td is None else td
    r, c, pp = _op().sdr_correlations(pd, td, L, zero_mean, pairing)
    G, S, _ = p.shape
    assert r.dtype == c.dtype == pp.dtype == torch.float64
    assert r.shape == (G, S, L) and pp.shape == (G, S) and c.shape == ((G, S, S, L) if pairing == ALL else (G, S, L))
    r, c, pp = r.cpu().numpy(), c.cpu().numpy(), pp.cpu().numpy()
    pf, tf = p.float(), t.float()
    for g in range(G):
        for j in range(S):
            for i in range(S) if pairing == ALL else [j]:
                mp, mt = (0, 0) if means is None else (int(means[0][g, i]), int(means[1][g, j]))
                wr, wc, wpp = so.lag_sums_int(pf[g, i], tf[g, j], L, mp, mt)
                where = f"g={g} target={j} pred={i} T={p.shape[-1]} L={L}"
                assert np.array_equal(r[g, j], wr.astype(np.float64)), f"autocorrelation, {where}"
                assert np.array_equal(c[g, j, i] if pairing == ALL else c[g, j], wc.astype(np.float64)), f"cross-correlation, {where}"
                assert pp[g, i] == float(wpp), f"pred energy, {where}"


def _ints(shape, seed):
    return so.small_ints(shape, seed), so.small_ints(shape, seed + 1000)


@pytest.mark.parametrize("T,L", [(1, 65), (2, 65), (64, 65), (65, 65), (66, 65), (5, 8), (1, 1), (130, 1), (130, 2), (130, 3),
                                 (130, LAG_TILE - 1), (130, LAG_TILE), (130, LAG_TILE + 1), (530, 512), (511, 512), (513, 512)])
def test_exact_lag_sums(monkeypatch, T, L):
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    p, t = _ints((3, 2, T), 10 * T + L)
    _check_exact(p, t, L)
    _check_exact(p, t, L, pairing=ALL)


@pytest.mark.parametrize("chunk", [100, 512, STAGE])
def test_exact_lag_sums_at_chunk_edges(monkeypatch, chunk):
    monkeypatch.setenv("TMX_SDR_CHUNK", str(chunk))
    for T in (chunk - 1, chunk, chunk + 1, 2 * chunk + 3):
        assert _op().sdr_chunks(2, 3, T, 70, ALL) == -(-T // chunk)
        p, t = _ints((2, 3, T), T)
        _check_exact(p, t, 70, pairing=ALL)
        _check_exact(p, t, 70)


@pytest.mark.parametrize("T,L,chunk", [(1, 1, None), (5, 8, None), (66, 65, None), (530, 255, None), (530, 256, None), (530, 257, None), (600, 512, None),
                                       (2500, 300, None), (4200, 65, 2048), (2063, 270, 2048), (350, 70, 100), (2049, 16, 2049)])
def test_exact_lag_sums_matrix_core_form(monkeypatch, T, L, chunk):
    """``TMX_SDR_CORR_FORM=mfma``: the 256-lag ``v_mfma_f64_16x16x4_f64`` form of the correlation pass, at its tile, stage, halo and chunk edges,
    with ``zero_mean`` off and (integer means) on, and for 16-bit inputs at a storage offset."""
    monkeypatch.setenv("TMX_SDR_CORR_FORM", "mfma")
    if chunk is None:
        monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    else:
        monkeypatch.setenv("TMX_SDR_CHUNK", str(chunk))
    p, t = _ints((2, 2, T), 7 * T + L)
    _check_exact(p, t, L, pairing=ALL)
    _check_exact(p, t, L)
    _check_exact(p, t, L, pairing=ALL, pd=_offset(p.cuda().bfloat16()), td=_offset(t.cuda().bfloat16()))
    if T % 2 == 0:  # every signal's sum made a multiple of T through two samples: integer means, exact centred sums
        means = []
        for k, x in enumerate((p, t)):
            want = torch.tensor([[1, -2], [2, -1]]) * (1 if k == 0 else -1)
            x[..., 0] += want * T - x.sum(-1)
            means.append(want)
        _check_exact(p, t, L, zero_mean=True, pairing=ALL, means=means)


@pytest.mark.parametrize("T,L,form", [(MFMA_MIN_T, 192, "mfma"), (MFMA_MIN_T - 1, 192, "valu"), (MFMA_MIN_T, 191, "valu"), (MFMA_MIN_T + 5, 256, "mfma"),
                                      (MFMA_MIN_T, 257, "valu"), (MFMA_MIN_T + 5, 384, "mfma"), (MFMA_MIN_T, 64, "valu")])
def test_form_of_the_correlation_pass(monkeypatch, T, L, form):
    """Without the knob the form follows the filter and the signal length alone: the matrix-core kernel from ``T = 16 384`` on when the
    filter fills three quarters of its 256-lag tiles.  (These signals are longer than the other cases': the rule's edge is there.)  Exact
    on either side, and the diagonal and the pair-matrix call take the same form."""
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    monkeypatch.delenv("TMX_SDR_CORR_FORM", raising=False)
    p, t = _ints((1, 2, T), T + L)
    pd, td = p.cuda(), t.cuda()
    want, other = ("sdr_corr_mfma_kernel", "sdr_corr_kernel") if form == "mfma" else ("sdr_corr_kernel", "sdr_corr_mfma_kernel")
    for pairing in (DIAG, ALL):
        assert_route(kernels_run(lambda: _op().sdr_correlations(pd, td, L, False, pairing)), present=(want,), absent=(other,))
    _check_exact(p, t, L, pairing=ALL)


def test_values_with_the_default_matrix_core_form(monkeypatch):
    """``T = 16 500``, ``L = 200``: the scores through the form the library picks there, under the rule; every entry of the pair matrix has the
    bits of the diagonal call on its pair."""
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    monkeypatch.delenv("TMX_SDR_CORR_FORM", raising=False)
    T, L = 16500, 200
    p, t = _seven("white", T, 300)
    p, t = p[:4].reshape(2, 2, T), t[:4].reshape(2, 2, T)
    pd, td = p.cuda(), t.cuda()
    assert_route(kernels_run(lambda: _op().sdr_scores(pd, td, L, True, None, ALL)), present=("sdr_corr_mfma_kernel", "sdr_solve_kernel"), absent=("sdr_corr_kernel",))
    got = _op().sdr_scores(pd, td, L, True, None, ALL)
    diag = _op().sdr_scores(pd, td, L, True, None, DIAG)
    assert _op().sdr_chunks(2, 2, T, L, ALL) == _op().sdr_chunks(2, 2, T, L, DIAG)
    assert _same_bits(torch.diagonal(got, dim1=1, dim2=2).contiguous(), diag)
    coh, want = so.sdr(p.reshape(4, T), t.reshape(4, T), L, True)
    _report("default mfma form", so.error_over_bound(diag.flatten(), so.ref64(p.reshape(4, T), t.reshape(4, T), L, True), want, coh, L))


def test_values_matrix_core_form(monkeypatch):
    """The scores through the matrix-core form under the rule, and bit-equal from run to run."""
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    monkeypatch.setenv("TMX_SDR_CORR_FORM", "mfma")
    for name, T, L, zero_mean, load_diag in (("white", 700, 512, True, 1e-3), ("ar1", 4099, 8, True, None), ("60dB", 2000, 64, False, None)):
        p, t, coh, want, ref = _case(name, T, L, zero_mean, load_diag)
        pd, td = p.cuda()[:, None], t.cuda()[:, None]
        got = _op().sdr_scores(pd, td, L, zero_mean, load_diag, DIAG)
        assert _same_bits(_op().sdr_scores(pd, td, L, zero_mean, load_diag, DIAG), got)
        _report(f"mfma {name} T={T} L={L}", so.error_over_bound(got[:, 0], ref, want, coh, L))


def test_exact_lag_sums_zero_mean(monkeypatch):
    """``T = 64`` and every signal's sum a non-zero multiple of 64: the mean is an exact integer, so the centred sums stay exact."""
    monkeypatch.setenv("TMX_SDR_CHUNK", "24")
    means = []
    both = []
    for k, x in enumerate(_ints((2, 3, 64), 5)):
        want = torch.tensor([[1, -2, 3], [2, 1, -1]]) * (1 if k == 0 else -1)  # the integer mean of every signal
        x[..., 0] += want * 64 - x.sum(-1)
        assert bool((x.sum(-1) == want * 64).all()) and float(x.abs().max()) < 2**20
        means.append(want)
        both.append(x)
    _check_exact(both[0], both[1], 20, zero_mean=True, pairing=ALL, means=means)
    _check_exact(both[0], both[1], 20, zero_mean=True, means=means)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_exact_lag_sums_16_bit(monkeypatch, dtype):
    monkeypatch.setenv("TMX_SDR_CHUNK", "300")
    p, t = _ints((2, 2, 700), 3)  # integers up to 8 are exact in both types
    _check_exact(p, t, 65, pairing=ALL, pd=p.cuda().to(dtype), td=t.cuda().to(dtype))


def test_exact_lag_sums_at_a_storage_offset(monkeypatch):
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    p, t = _ints((2, 2, 2500), 8)
    _check_exact(p, t, 65, pd=_offset(p.cuda()), td=_offset(t.cuda()))
    _check_exact(p, t, 65, pairing=ALL, pd=_offset(p.cuda().half()), td=_offset(t.cuda().half()))


# ---------------------------------------------------------------------------------------------------------------- values
def _seven(name, T, seed):
    """Seven signals of one generator, each drawn with its own seed."""
    pairs = [so.GENERATORS[name](1, T, seed + k) for k in range(7)]
    return torch.cat([p for p, _ in pairs]), torch.cat([t for _, t in pairs])


@functools.lru_cache(maxsize=None)
def _case(name, T, L, zero_mean, load_diag, seed=100):
    """``(preds, target, coh, oracle dB, ref64 dB)`` of one case, computed once."""
    p, t = _seven(name, T, seed)
    coh, want = so.sdr(p, t, L, zero_mean, load_diag)
    return p, t, coh, want, so.ref64(p, t, L, zero_mean, load_diag)


CONFIGS = [(2000, 64, False, None), (700, 512, True, 1e-3), (4099, 8, True, None), (2000, 1, False, 1e-3)]


@pytest.mark.parametrize("T,L,zero_mean,load_diag", CONFIGS)
@pytest.mark.parametrize("name", sorted(so.GENERATORS))
def test_values(monkeypatch, name, T, L, zero_mean, load_diag):
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    p, t, coh, want, ref = _case(name, T, L, zero_mean, load_diag)
    pd, td = p.cuda()[:, None], t.cuda()[:, None]
    got = _op().sdr_scores(pd, td, L, zero_mean, load_diag, DIAG)
    assert got.dtype == torch.float64 and got.shape == (7, 1)
    assert _same_bits(_op().sdr_scores(pd, td, L, zero_mean, load_diag, DIAG), got)
    assert _same_bits(_op().sdr_scores(_offset(pd), _offset(td), L, zero_mean, load_diag, DIAG), got)
    _report(f"{name} T={T} L={L} zero_mean={zero_mean} load_diag={load_diag}", so.error_over_bound(got[:, 0], ref, want, coh, L))
    if load_diag is not None:  # the loading moves the value by far more than the rule allows
        bare = _op().sdr_scores(pd, td, L, zero_mean, None, DIAG)[:, 0].cpu()
        assert float(((bare - want).abs() / so.bound(ref, want, coh, L)).min()) > 10.0


def test_values_with_the_block_wide_solve_against_the_oracle(monkeypatch):
    """``L = 513``, the first filter past the single-wave solve, under the rule."""
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    L = 513
    p, t = _seven("white", 3 * L, 7)
    p, t = p[:3], t[:3]
    coh, want = so.sdr(p, t, L)
    got = _op().sdr_scores(p.cuda()[:, None], t.cuda()[:, None], L, False, None, DIAG)[:, 0]
    _report("L=513", so.error_over_bound(got, so.ref64(p, t, L), want, coh, L))


@pytest.mark.parametrize("L", [1100, MAX_L])
def test_values_with_the_block_wide_solve(monkeypatch, L):
    """Longer filters, and at ``MAX_L`` the full LDS budget."""
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    p, t = so.white(2, 3 * L, L)
    pd, td = p.cuda()[:, None], t.cuda()[:, None]
    got = _op().sdr_scores(pd, td, L, False, None, DIAG)[:, 0].cpu()
    # the longdouble elimination is O(L^3); at these sizes the fp64 reference arithmetic is the yardstick, to 1e-6 dB (it is
    # 1e-13 to 1e-11 dB from the oracle on 14 dB white noise in the cases above, a dropped lag shows at 1e-3 dB)
    assert float((got - so.ref64(p, t, L)).abs().max()) <= 1e-6


# ----------------------------------------------------------------------------------------------------------- pair matrix
@functools.lru_cache(maxsize=None)
def _speaker_case(B, S, T, L, zero_mean, seed):
    p, t = so.speakers((B, S, T), seed)
    coh, want, ref = (torch.empty(B, S, S, dtype=torch.float64) for _ in range(3))
    for j in range(S):
        for i in range(S):
            coh[:, j, i], want[:, j, i] = so.sdr(p[:, i], t[:, j], L, zero_mean)
            ref[:, j, i] = so.ref64(p[:, i], t[:, j], L, zero_mean)
    return p, t, coh, want, ref


@pytest.mark.parametrize("S,L", [(2, 40), (3, 40), (5, 40), (9, 40), (3, 200), (5, 200)])
def test_pair_matrix(monkeypatch, S, L):
    """``L = 40``: the solve with 2 elements per lane; ``L = 200``: 8 per lane, with 4 and 8 right-hand sides per recursion."""
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    zero_mean = S == 3
    p, t, coh, want, ref = _speaker_case(2, S, 1500, L, zero_mean, 30 + S)
    pd, td = p.cuda(), t.cuda()
    got = _op().sdr_scores(pd, td, L, zero_mean, None, ALL)
    assert got.shape == (2, S, S) and _same_bits(_op().sdr_scores(pd, td, L, zero_mean, None, ALL), got)
    _report(f"pair matrix S={S}", so.error_over_bound(got.flatten(), ref.flatten(), want.flatten(), coh.flatten(), L))
    # the speakers' noise levels differ: the transposed matrix is tenths of a dB away, far outside the rule
    assert so.error_over_bound(got.transpose(1, 2).flatten(), ref.flatten(), want.flatten(), coh.flatten(), L) > 1e6
    assert _op().sdr_chunks(2, S, 1500, L, ALL) == _op().sdr_chunks(2, 1, 1500, L, DIAG) == 1
    for j in range(S):
        for i in range(S):
            one = _op().sdr_scores(pd[:, i : i + 1], td[:, j : j + 1], L, zero_mean, None, DIAG)
            assert _same_bits(one[:, 0].contiguous(), got[:, j, i].contiguous()), f"target {j}, pred {i}"


def test_pair_matrix_with_the_block_wide_solve(monkeypatch):
    """``L = 600``, ``S = 3``: 256 threads and four right-hand sides per recursion.  Every entry has the bits of the diagonal call on its pair
    (one right-hand side); the longdouble elimination is O(L^3), so the rule is applied to one target's row."""
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    L, S = 600, 3
    p, t = so.speakers((2, S, 1800), 61)
    pd, td = p.cuda(), t.cuda()
    got = _op().sdr_scores(pd, td, L, False, None, ALL)
    assert _same_bits(_op().sdr_scores(pd, td, L, False, None, ALL), got)
    for j in range(S):
        for i in range(S):
            one = _op().sdr_scores(pd[:, i : i + 1], td[:, j : j + 1], L, False, None, DIAG)
            assert _same_bits(one[:, 0].contiguous(), got[:, j, i].contiguous()), f"target {j}, pred {i}"
    j = 1
    pj, tj = p[0], t[0, j].expand(S, -1)
    coh, want = so.sdr(pj, tj, L)
    ref = so.ref64(pj, tj, L)
    _report("pair matrix L=600, target 1", so.error_over_bound(got[0, j], ref, want, coh, L))
    assert so.error_over_bound(got[0, :, j], ref, want, coh, L) > 1e6  # the column is not the row


# -------------------------------------------------------------------------------------------------------------- chunking
def test_sdr_chunks_is_a_function_of_the_shape(monkeypatch):
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    chunks = _op().sdr_chunks
    assert chunks(1, 1, 1, 1, DIAG) == 1 and chunks(7, 1, 2 * STAGE - 1, 64, DIAG) == 1 and chunks(7, 1, 2 * STAGE, 64, DIAG) == 2
    assert chunks(4096, 1, 400, 64, DIAG) == 1 and chunks(4096, 1, 160000, 64, DIAG) == 1  # enough rows: no split
    assert chunks(16, 2, 64000, 512, DIAG) == 4  # 512 rows of (signal, series, lag tile): 4 chunks of 8 stages
    assert chunks(16, 2, 64000, 64, DIAG) == 16 and chunks(16, 4, 64000, 512, ALL) == 1
    monkeypatch.setenv("TMX_SDR_CHUNK", "1")
    assert chunks(7, 1, 5, 3, DIAG) == 5
    monkeypatch.setenv("TMX_SDR_CHUNK", "1000")
    assert chunks(7, 1, 2003, 3, DIAG) == 3 and chunks(7, 3, 2003, 3, ALL) == 3


def test_forced_chunks_agree_with_one(monkeypatch):
    p, t, coh, want, ref = _case("ar1", 4099, 8, True, None)
    pd, td = p.cuda()[:, None], t.cuda()[:, None]
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    assert _op().sdr_chunks(7, 1, 4099, 8, DIAG) == 2
    monkeypatch.setenv("TMX_SDR_CHUNK", "100000")
    assert _op().sdr_chunks(7, 1, 4099, 8, DIAG) == 1
    one = _op().sdr_scores(pd, td, 8, True, None, DIAG)
    monkeypatch.setenv("TMX_SDR_CHUNK", "333")
    assert _op().sdr_chunks(7, 1, 4099, 8, DIAG) == 13
    many = _op().sdr_scores(pd, td, 8, True, None, DIAG)
    assert _same_bits(_op().sdr_scores(pd, td, 8, True, None, DIAG), many)
    _report("one chunk", so.error_over_bound(one[:, 0], ref, want, coh, 8))
    _report("13 chunks", so.error_over_bound(many[:, 0], ref, want, coh, 8))


# ----------------------------------------------------------------------------------------------------------- containment
def test_nan_reaches_its_own_outputs_only(monkeypatch):
    monkeypatch.setenv("TMX_SDR_CHUNK", "700")
    p, t = so.speakers((3, 4, 1500), 9)
    pd, td = p.cuda(), t.cuda()
    clean, clean_diag = _op().sdr_scores(pd, td, 30, True, None, ALL), _op().sdr_scores(pd, td, 30, True, None, DIAG)
    assert bool(torch.isfinite(clean).all())
    bad = pd.clone()
    bad[1, 2, 800] = float("nan")
    got, got_diag = _op().sdr_scores(bad, td, 30, True, None, ALL), _op().sdr_scores(bad, td, 30, True, None, DIAG)
    hit = torch.zeros(3, 4, 4, dtype=torch.bool, device="cuda")
    hit[1, :, 2] = True  # pred 2 of group 1 under every target
    assert torch.equal(torch.isnan(got), hit) and _same_bits(got[~hit], clean[~hit])
    assert torch.equal(torch.isnan(got_diag), hit.diagonal(dim1=1, dim2=2)) and _same_bits(got_diag[~torch.isnan(got_diag)], clean_diag[~torch.isnan(got_diag)])
    bad = td.clone()
    bad[1, 2, 800] = float("nan")
    got = _op().sdr_scores(pd, bad, 30, True, None, ALL)
    hit = torch.zeros(3, 4, 4, dtype=torch.bool, device="cuda")
    hit[1, 2, :] = True  # that target's row of the matrix
    assert torch.equal(torch.isnan(got), hit) and _same_bits(got[~hit], clean[~hit])


# ------------------------------------------------------------------------------------------ more rows than a grid axis
def test_more_rows_than_a_grid_axis(monkeypatch):
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    rows = 70000
    g = torch.Generator().manual_seed(12)
    t = torch.randn(rows, 1, 8, generator=g)
    p = t + 0.3 * torch.randn(rows, 1, 8, generator=g)
    got = _op().sdr_scores(p.cuda(), t.cuda(), 2, False, None, DIAG)
    assert got.shape == (rows, 1)
    pick = [0, 1, 65534, 65535, 65536, 69998, 69999]
    coh, want = so.sdr(p[pick, 0], t[pick, 0], 2)
    _report("70000 rows", so.error_over_bound(got[pick, 0], so.ref64(p[pick, 0], t[pick, 0], 2), want, coh, 2))
    r, c, pp = _op().sdr_correlations(p.cuda(), t.cuda(), 2, False, DIAG)
    assert torch.allclose(r[:, 0, 0].cpu(), (t.double() ** 2).sum(-1)[:, 0], rtol=1e-14, atol=0)
    assert torch.allclose(pp[:, 0].cpu(), (p.double() ** 2).sum(-1)[:, 0], rtol=1e-14, atol=0)


# ---------------------------------------------------------------------------------------------------- degenerate systems
def test_degenerate_systems(monkeypatch):
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    sdr = _sdr_mod()
    g = torch.Generator().manual_seed(2)
    p = torch.randn(7, 900, generator=g).cuda()
    t = torch.randn(7, 900, generator=g).cuda()
    t[2] = 0.0
    t[5] = 0.0
    for L in (1, 16, 600):
        got = _op().sdr_scores(p[:, None], t[:, None], L, False, None, DIAG)[:, 0]
        silent = torch.zeros(7, dtype=torch.bool, device="cuda")
        silent[[2, 5]] = True
        assert torch.equal(torch.isnan(got), silent)
        # with diagonal loading the system is regular and b is zero: what the composition gives on the same tensors
        got = sdr.signal_distortion_ratio(p, t, filter_length=L, load_diag=1e-3)
        comp = sdr._sdr_composition(p, t, None, L, False, 1e-3)
        assert got.dtype == comp.dtype == torch.float32
        assert torch.equal(torch.isnan(got), torch.isnan(comp))
        assert torch.equal(got[silent].nan_to_num(nan=1.0), comp[silent].nan_to_num(nan=1.0))
        assert torch.allclose(got[~silent], comp[~silent], rtol=0, atol=1e-4)
    # preds == target is not pinned (see the module docstring); it must not raise
    sdr.signal_distortion_ratio(t, t, filter_length=16)
    sdr.signal_distortion_ratio(torch.zeros(3, 50, device="cuda"), torch.zeros(3, 50, device="cuda"), filter_length=16)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- routes
NATIVE = ("sdr_corr_kernel", "sdr_solve_kernel")
PARENT = ("fft", "levinson_kernel")


def test_routes_of_the_functional_and_the_module(monkeypatch):
    from torchmetrics_forked_amd.audio import SignalDistortionRatio

    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    sdr = _sdr_mod()
    calls = count_calls(monkeypatch, torch.ops.tmx, "sdr_scores")
    p, t = so.white(6, 1000, 1)
    pd, td = p.cuda().reshape(2, 3, 1000), t.cuda().reshape(2, 3, 1000)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        n = len(calls)
        names = kernels_run(lambda: sdr.signal_distortion_ratio(pd.to(dtype), td.to(dtype), filter_length=32))
        assert_route(names, present=NATIVE, absent=PARENT)
        assert len(calls) == n + 2 and calls[-1][0][0].shape == (6, 1, 1000)  # kernels_run calls twice
    assert_route(kernels_run(lambda: sdr.signal_distortion_ratio(pd, td, filter_length=32, zero_mean=True)), present=NATIVE + ("sdr_mean_kernel",), absent=PARENT)
    metric = SignalDistortionRatio(filter_length=32).cuda()
    n = len(calls)
    assert_route(kernels_run(lambda: metric.update(pd, td)), present=NATIVE, absent=PARENT)
    assert len(calls) == n + 2
    # kept on the composition
    n = len(calls)
    long_p, long_t = so.white(1, 3 * MAX_L, 2)
    long_p, long_t = long_p.cuda(), long_t.cuda()
    for keep in (lambda: sdr.signal_distortion_ratio(pd.double(), td.double(), filter_length=32),
                 lambda: sdr.signal_distortion_ratio(pd.clone().requires_grad_(), td, filter_length=32),
                 lambda: sdr.signal_distortion_ratio(long_p, long_t, filter_length=MAX_L + 1)):
        assert_route(kernels_run(keep), absent=("sdr_",))
    assert len(calls) == n
    with torch.no_grad():
        sdr.signal_distortion_ratio(pd.clone().requires_grad_(), td, filter_length=32)
    assert len(calls) == n + 1
    # a backward through the composition still gives a finite gradient
    pg = pd.clone().requires_grad_()
    sdr.signal_distortion_ratio(pg, td, filter_length=32).sum().backward()
    assert pg.grad is not None and bool(torch.isfinite(pg.grad).all()) and float(pg.grad.abs().max()) > 0
    assert len(calls) == n + 1


@pytest.mark.parametrize("S,search", [(2, "exhaustive"), (5, "hungarian_kernel")])
def test_routes_of_pit(monkeypatch, S, search):
    from torchmetrics_forked_amd.audio import PermutationInvariantTraining
    from torchmetrics_forked_amd.functional.audio.pit import permutation_invariant_training as pit

    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    sdr = _sdr_mod()
    fn = sdr.signal_distortion_ratio
    calls = count_calls(monkeypatch, torch.ops.tmx, "sdr_scores")
    inner = count_calls(monkeypatch, sdr, "_sdr_composition")
    p, t = so.speakers((3, S, 800), 6)
    pd, td = p.cuda(), t.cuda()
    names = kernels_run(lambda: pit(pd, td, fn, filter_length=24, zero_mean=True, load_diag=1e-4, use_cg_iter=5))
    assert_route(names, present=NATIVE + (() if search == "exhaustive" else (search,)), absent=PARENT)
    assert len(calls) == 2 and calls[-1][0][0].shape == (3, S, 800) and calls[-1][0][2:] == (24, True, 1e-4, ALL) and not inner
    metric = PermutationInvariantTraining(fn, filter_length=24).cuda()
    assert_route(kernels_run(lambda: metric.update(pd, td)), present=NATIVE, absent=PARENT)
    assert len(calls) == 4 and not inner
    # kept on the code below the branch: a user function, an unknown keyword, fp64
    assert_route(kernels_run(lambda: pit(pd.double(), td.double(), fn, filter_length=24)), absent=("sdr_",))
    with pytest.raises(TypeError):
        pit(pd, td, fn, filter_length=24, other=1)
    assert len(calls) == 4
    assert_route(kernels_run(lambda: pit(pd, td, lambda a, b: sdr._sdr_composition(a, b, None, 24))), absent=("sdr_",))
    assert len(calls) == 4 and len(inner) == 2 + 2 * S * S  # (the fp64 call above went through the composition twice)
    n = len(inner)
    pit(pd, td, lambda a, b: fn(a, b, filter_length=24))  # the S² loop calls the functional, which takes its own route on 2-D rows
    assert len(calls) == 4 + S * S and len(inner) == n and all(c[0][0].shape == (3, 1, 800) for c in calls[4:])


# ------------------------------------------------------------------------------------------------------------ end to end
def test_functional_end_to_end(monkeypatch):
    from torchmetrics_forked_amd.audio import SignalDistortionRatio

    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    sdr = _sdr_mod()
    p, t, coh, want, ref = _case("white", 2000, 64, False, None)
    p8, t8 = torch.cat([p, p[:1]]).reshape(2, 2, 2, 2000), torch.cat([t, t[:1]]).reshape(2, 2, 2, 2000)
    got = sdr.signal_distortion_ratio(p8.cuda(), t8.cuda(), filter_length=64)
    assert got.dtype == torch.float32 and got.shape == (2, 2, 2)
    _report("functional fp32", so.error_over_bound(got.flatten()[:7], ref, want, coh, 64, fp32_result=True))
    one = sdr.signal_distortion_ratio(p[3].cuda(), t[3].cuda(), filter_length=64)
    assert one.shape == () and float(one) == float(got.flatten()[3])
    metric = SignalDistortionRatio(filter_length=64).cuda()
    metric.update(p[:3].cuda(), t[:3].cuda())
    metric.update(p[3:].cuda(), t[3:].cuda())
    assert abs(float(metric.compute()) - float(want.mean())) <= 1e-5  # the mean of seven fp32 values near 14 dB


def test_docstring_example_shapes(monkeypatch):
    """The shapes of the reference's docstring examples, default ``filter_length``: 8000 samples, and 4 x 2 x 8000."""
    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    sdr = _sdr_mod()
    g = torch.Generator().manual_seed(1)
    p, t = torch.randn(9, 8000, generator=g), torch.randn(9, 8000, generator=g)
    coh, want = so.sdr(p, t)
    ref = so.ref64(p, t)
    got = torch.cat([sdr.signal_distortion_ratio(p[0].cuda(), t[0].cuda()).reshape(1),
                     sdr.signal_distortion_ratio(p[1:].cuda().reshape(4, 2, 8000), t[1:].cuda().reshape(4, 2, 8000)).flatten()])
    assert got.dtype == torch.float32 and float(want.max()) < -8.0  # independent noise: about -12 dB
    _report("docstring shapes", so.error_over_bound(got, ref, want, coh, 512, fp32_result=True))


@pytest.mark.parametrize("S", [2, 5])
def test_pit_end_to_end(monkeypatch, S):
    from torchmetrics_forked_amd.functional.audio.pit import permutation_invariant_training as pit
    from torchmetrics_forked_amd.functional.audio.pit import pit_permutate

    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    fn = _sdr_mod().signal_distortion_ratio
    L = 40
    p, t, coh, want, ref = _speaker_case(7, S, 1200, L, False, 50 + S)
    g = torch.Generator().manual_seed(S)
    perm = torch.stack([torch.randperm(S, generator=g) for _ in range(7)])
    pp = pit_permutate(p, perm)
    best, got = pit(pp.cuda(), t.cuda(), fn, filter_length=L)
    best_c, got_c = pit(pp, t, fn, filter_length=L)
    assert torch.equal(got.cpu(), got_c) and torch.equal(pit_permutate(pp, got.cpu()), p)
    # the best metric is the fp32 mean of the S diagonal entries of the unpermuted matrix, each an fp32 value within the rule
    tol = torch.diagonal(so.bound(ref.flatten(), want.flatten(), coh.flatten(), L, fp32_result=True).reshape(7, S, S), dim1=1, dim2=2).max(-1).values
    diag = torch.diagonal(want, dim1=1, dim2=2)
    top = diag.abs().max(-1).values.float()
    tol = tol + 0.5 * torch.tensor(np.spacing((S * top).numpy()) + np.spacing(top.numpy()), dtype=torch.float64)  # S − 1 additions and a division
    ratio = float(((best.cpu().double() - diag.mean(-1)).abs() / tol).max())
    _report(f"pit best metric S={S}", ratio)
    assert float((best.cpu() - best_c).abs().max()) <= 1e-4


# ---------------------------------------------------------------------------------------------------------- no expansion
def test_no_expansion(monkeypatch):
    """``B = 4, S = 8, T = 32 768``, ``L = 64``, fp32.  The first thing the composition allocates is an fp64 copy of the two (expanded) inputs;
    the native call allocates lag sums only."""
    from torchmetrics_forked_amd.functional.audio.pit import permutation_invariant_training as pit

    monkeypatch.delenv("TMX_SDR_CHUNK", raising=False)
    sdr = _sdr_mod()
    B, S, T = 4, 8, 32768
    g = torch.Generator().manual_seed(4)
    t = torch.randn(B, S, T, generator=g)
    p = t + 0.2 * torch.randn(B, S, T, generator=g)
    pd, td = p.cuda(), t.cuda()
    limit = 2 * B * S * T * 8

    def growth():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        best, perm = pit(pd, td, sdr.signal_distortion_ratio, filter_length=64)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, perm

    grew, perm = growth()
    print(f"pit peak growth {grew} bytes native, limit {limit}")
    assert grew < limit and torch.equal(perm.cpu(), torch.arange(S).expand(B, S))
    monkeypatch.setattr(sdr, "_SDR_NATIVE", False)
    grew_comp, perm = growth()
    print(f"pit peak growth {grew_comp} bytes through the composition")
    assert grew_comp > limit and torch.equal(perm.cpu(), torch.arange(S).expand(B, S))


# ----------------------------------------------------------------------------------------------------------- host checks
def test_host_checks_raise():
    x = torch.randn(2, 2, 100, device="cuda")
    scores, corr = torch.ops.tmx.sdr_scores, torch.ops.tmx.sdr_correlations
    with pytest.raises(RuntimeError, match="matching"):
        scores(x, x[..., :99], 8, False, None, DIAG)
    with pytest.raises(RuntimeError, match="matching"):
        corr(x, x[:, :1], 8, False, DIAG)
    with pytest.raises(RuntimeError, match="dtype"):
        scores(x, x.half(), 8, False, None, DIAG)
    with pytest.raises(RuntimeError, match="dtype"):
        scores(x.double(), x.double(), 8, False, None, DIAG)
    for L in (0, -1, MAX_L + 1):
        with pytest.raises(RuntimeError, match="filter_length"):
            scores(x, x, L, False, None, DIAG)
        with pytest.raises(RuntimeError, match="filter_length"):
            corr(x, x, L, False, ALL)
    with pytest.raises(RuntimeError, match="pairing"):
        scores(x, x, 8, False, None, 2)
    with pytest.raises(RuntimeError, match="empty"):
        scores(x[:0], x[:0], 8, False, None, DIAG)
    with pytest.raises(RuntimeError):  # no CPU implementation is registered
        scores(x.cpu(), x.cpu(), 8, False, None, DIAG)
    torch.cuda.synchronize()
