"""``signal_distortion_ratio`` on the CPU: the longdouble oracle of ``tests/helpers/sdr_oracle.py`` against this package's CPU functional under
the oracle's own rule (which validates the oracle too), the int64 lag sums against the longdouble ones, and the native gate and PIT's
second helper arm by arm with the op faked."""
import numpy as np
import pytest
import torch

import torchmetrics_forked_amd.functional.audio.pit as pit_mod
import torchmetrics_forked_amd.functional.audio.sdr as sdr_mod
import torchmetrics_forked_amd.ops.audio as ops_audio
from tests.helpers import sdr_oracle as so
from tests.helpers.routes import count_calls


@pytest.fixture(autouse=True)
def _longdouble():
    so.require_longdouble()


@pytest.mark.parametrize("name", sorted(so.GENERATORS))
def test_oracle_agrees_with_the_cpu_functional(name):
    for T, L, zero_mean, load_diag in ((1000, 48, False, None), (600, 130, True, 1e-3), (1000, 1, True, None)):
        p, t = so.GENERATORS[name](7, T, 17)
        coh, want = so.sdr(p, t, L, zero_mean, load_diag)
        ref = so.ref64(p, t, L, zero_mean, load_diag)
        got = sdr_mod.signal_distortion_ratio(p.double(), t.double(), filter_length=L, zero_mean=zero_mean, load_diag=load_diag)
        assert got.dtype == torch.float64
        ratio = so.error_over_bound(got, ref, want, coh, L)
        print(f"sdr_err cpu {name} T={T} L={L}: error/bound {ratio:.3g}")
        assert ratio <= 1.0
        got32 = sdr_mod.signal_distortion_ratio(p, t, filter_length=L, zero_mean=zero_mean, load_diag=load_diag)
        assert got32.dtype == torch.float32 and so.error_over_bound(got32, ref, want, coh, L, fp32_result=True) <= 1.0
        # the rule is not loose: one dropped sample of the target is far outside it
        cut = t.clone()
        cut[:, T // 2] = 0
        moved = sdr_mod.signal_distortion_ratio(p.double(), cut.double(), filter_length=L, zero_mean=zero_mean, load_diag=load_diag)
        assert so.error_over_bound(moved, ref, want, coh, L) > 100.0


def test_oracle_levels():
    for name, level in (("white", 14.0), ("60dB", 60.0)):
        p, t = so.GENERATORS[name](7, 2000, 3)
        _, db = so.sdr(p, t, 1)
        assert float((db - level).abs().max()) < 0.5
    p, t = so.dc_offset(7, 2000, 3)
    assert abs(float(t.mean()) - 5.0) < 0.1 and abs(float(so.sdr(p, t, 8, True)[1].mean()) - 14.0) < 0.5
    p, t = so.ar1(3, 4000, 3)
    r, _, _ = so.lag_sums(p[0], t[0], 2)
    assert abs(float(r[1] / r[0]) - 0.95) < 0.02
    p, t = so.int16_scale(3, 500, 3)
    assert bool((p == p.round()).all()) and bool((t == t.round()).all()) and float(t.abs().max()) > 3000


@pytest.mark.parametrize("T,L", [(1, 1), (5, 8), (64, 3), (300, 65)])
def test_int64_lag_sums_agree_with_longdouble(T, L):
    p, t = so.small_ints((T,), T), so.small_ints((T,), T + 1)
    r, c, pp = so.lag_sums(p, t, L)
    ri, ci, ppi = so.lag_sums_int(p, t, L)
    assert np.array_equal(r, ri.astype(np.longdouble)) and np.array_equal(c, ci.astype(np.longdouble)) and pp == ppi
    if T > 1:
        assert int(ci[1]) == int((t[:-1] * p[1:]).sum())  # the target is the unshifted factor
    # centred: the signals' integer means subtracted first
    p2, t2 = p + 3, t - 2
    r2, c2, pp2 = so.lag_sums_int(p2, t2, L, 3, -2)
    assert np.array_equal(r2, ri) and np.array_equal(c2, ci) and pp2 == ppi
    with pytest.raises(AssertionError):
        so.lag_sums_int(p + 0.5, t, L)


class _OnGpu(torch.Tensor):
    """A plain CPU tensor that answers ``is_cuda`` with True: reaches the gate's later arms without a GPU."""

    is_cuda = property(lambda self: True)


def _gpu_like(*shape, dtype=torch.float32):
    return torch.rand(*shape).to(dtype).as_subclass(_OnGpu)


def test_gate_arm_by_arm(monkeypatch):
    ok = sdr_mod._native_sdr_ok
    seen = []

    def use_native(*tensors):
        seen.append(tensors)
        return True

    monkeypatch.setattr(sdr_mod.ops, "use_native", use_native)
    monkeypatch.setattr(sdr_mod, "_SDR_NATIVE", True)
    monkeypatch.setattr(sdr_mod, "_native_signal_ok", lambda p, t: False)  # not this gate's business
    p, t = _gpu_like(2, 3, 50), _gpu_like(2, 3, 50)
    assert ok(p, t, 512) and len(seen) == 1 and seen[0][0] is p and seen[0][1] is t
    for dtype in (torch.bfloat16, torch.float16):
        assert ok(_gpu_like(2, 50, dtype=dtype), _gpu_like(2, 50, dtype=dtype), 512)
    assert ok(_gpu_like(50), _gpu_like(50), 1) and ok(p, t, sdr_mod._SDR_MAX_FILTER)
    # filter length
    assert not ok(p, t, sdr_mod._SDR_MAX_FILTER + 1) and not ok(p, t, 0) and not ok(p, t, -3) and not ok(p, t, 8.0) and not ok(p, t, None)
    assert ok(p, t, np.int64(8)) and ok(p, t, np.int32(512)) and not ok(p, t, np.float64(8))
    # device
    assert not ok(torch.rand(2, 50), torch.rand(2, 50), 8) and not ok(p, torch.rand(2, 3, 50), 8) and not ok(torch.rand(2, 3, 50), t, 8)
    # dtype
    assert not ok(_gpu_like(2, 50, dtype=torch.float64), _gpu_like(2, 50, dtype=torch.float64), 8)
    assert not ok(p, _gpu_like(2, 3, 50, dtype=torch.bfloat16), 8)
    assert not ok(torch.randint(0, 9, (2, 50)).as_subclass(_OnGpu), torch.randint(0, 9, (2, 50)).as_subclass(_OnGpu), 8)
    # shape, empty
    assert not ok(p, _gpu_like(2, 3, 51), 8) and not ok(_gpu_like(0, 50), _gpu_like(0, 50), 8) and not ok(_gpu_like(2, 0), _gpu_like(2, 0), 8)
    assert not ok(torch.tensor(1.0).as_subclass(_OnGpu), torch.tensor(1.0).as_subclass(_OnGpu), 8)
    # autograd
    pg = _gpu_like(2, 3, 50).requires_grad_()
    assert not ok(pg, t, 8) and not ok(t, pg, 8)
    with torch.no_grad():
        assert ok(pg, t, 8)
    # the library's own answer and the knob
    n = len(seen)
    monkeypatch.setattr(sdr_mod.ops, "use_native", lambda *a: False)
    assert not ok(p, t, 8)
    monkeypatch.setattr(sdr_mod.ops, "use_native", use_native)
    monkeypatch.setattr(sdr_mod, "_SDR_NATIVE", False)
    assert not ok(p, t, 8) and len(seen) == n


def test_the_gates_cap_is_the_librarys():
    from torchmetrics_forked_amd import ops

    if not ops.available():
        pytest.skip("native library not built")
    assert ops_audio.sdr_tile()[3] == sdr_mod._SDR_MAX_FILTER


def test_functional_behind_the_gate(monkeypatch):
    calls = []

    def fake(preds, target, filter_length, zero_mean, load_diag, pairing):
        calls.append((tuple(preds.shape), tuple(target.shape), filter_length, zero_mean, load_diag, pairing))
        return torch.arange(preds.shape[0], dtype=torch.float64).reshape(-1, 1) + 0.1

    monkeypatch.setattr(sdr_mod, "_native_sdr_ok", lambda p, t, length: True)
    monkeypatch.setattr(sdr_mod, "_sdr_scores", fake)
    p, t = torch.rand(2, 3, 50), torch.rand(2, 3, 50)
    out = sdr_mod.signal_distortion_ratio(p, t)
    assert out.dtype == torch.float32 and torch.equal(out, (torch.arange(6, dtype=torch.float64) + 0.1).float().reshape(2, 3))
    assert calls[-1] == ((6, 1, 50), (6, 1, 50), 512, False, None, 0)
    out = sdr_mod.signal_distortion_ratio(p[0, 0].bfloat16(), t[0, 0].bfloat16(), use_cg_iter=10, filter_length=16, zero_mean=True, load_diag=1e-3)
    assert out.shape == () and out.dtype == torch.float32 and calls[-1] == ((1, 1, 50), (1, 1, 50), 16, True, 1e-3, 0)
    n = len(calls)
    with pytest.raises(RuntimeError, match="same shape"):
        sdr_mod.signal_distortion_ratio(p, t[..., :49])
    assert len(calls) == n


def test_pit_helper_arm_by_arm(monkeypatch):
    calls = []

    def fake(preds, target, filter_length, zero_mean, load_diag, pairing):
        calls.append((filter_length, zero_mean, load_diag, pairing))
        b, s = preds.shape[:2]
        out = torch.empty(b, s, s, dtype=torch.float64)
        for j in range(s):  # out[b, t, p]
            for i in range(s):
                out[:, j, i] = sdr_mod._sdr_composition(preds[:, i].double(), target[:, j].double(), None, filter_length, zero_mean, load_diag)
        return out

    gate = []
    monkeypatch.setattr(sdr_mod, "_native_sdr_ok", lambda p, t, length: gate.append(length) or True)
    monkeypatch.setattr(ops_audio, "sdr_scores", fake)
    p, t = so.speakers((3, 3, 400), 8)
    mtx, fn = pit_mod._native_sdr_pair_matrix, sdr_mod.signal_distortion_ratio
    for kwargs, want in (({}, (512, False, None, 1)), ({"filter_length": 16}, (16, False, None, 1)), ({"zero_mean": True, "filter_length": 8}, (8, True, None, 1)),
                         ({"load_diag": 1e-3, "use_cg_iter": 7, "filter_length": 8}, (8, False, 1e-3, 1))):
        out = mtx(p, t, fn, kwargs)
        assert out is not None and out.dtype == torch.float32 and out.shape == (3, 3, 3) and calls[-1] == want and gate[-1] == want[0]
    # the layout [b, t, p]: entry (1, 0) is target 1 against pred 0
    out = mtx(p, t, fn, {"filter_length": 8})
    want = sdr_mod._sdr_composition(p[:, 0].double(), t[:, 1].double(), None, 8).float()
    assert torch.equal(out[:, 1, 0], want) and not torch.allclose(out[:, 0, 1], want, atol=0.5)
    n, g = len(calls), len(gate)
    assert pit_mod._native_pair_matrix(p, t, fn, {}) is None  # the first helper keeps refusing SDR
    assert mtx(p, t, lambda a, b: fn(a, b), {}) is None and mtx(p, t, sdr_mod.scale_invariant_signal_distortion_ratio, {}) is None
    assert mtx(p, t, fn, {"filter_length": 8, "other": 1}) is None
    assert mtx(p[..., None], t[..., None], fn, {}) is None and mtx(p[:, 0], t[:, 0], fn, {}) is None  # 4-D, 2-D
    assert len(calls) == n and len(gate) == g  # none of them asked the gate
    monkeypatch.setattr(sdr_mod, "_native_sdr_ok", lambda p, t, length: False)
    assert mtx(p, t, fn, {}) is None and len(calls) == n
    # the whole call through the helper equals the call through the composition
    monkeypatch.setattr(sdr_mod, "_native_sdr_ok", lambda p, t, length: p.ndim == 3)
    perm = torch.tensor([[2, 0, 1], [0, 1, 2], [1, 0, 2]])
    pp = pit_mod.pit_permutate(p, perm)
    best, got = pit_mod.permutation_invariant_training(pp, t, fn, filter_length=8)
    assert len(calls) == n + 1
    monkeypatch.setattr(sdr_mod, "_native_sdr_ok", lambda p, t, length: False)
    best_c, got_c = pit_mod.permutation_invariant_training(pp, t, fn, filter_length=8)
    assert len(calls) == n + 1 and torch.equal(got, got_c) and float((best - best_c).abs().max()) <= 1e-5
    assert torch.equal(pit_mod.pit_permutate(pp, got), p)


def _no_native(*a, **k):
    raise AssertionError("the native SDR op was entered for CPU tensors")


def test_cpu_calls_never_reach_the_op(monkeypatch):
    calls = [count_calls(monkeypatch, sdr_mod, "_sdr_scores", guard=_no_native), count_calls(monkeypatch, ops_audio, "sdr_scores", guard=_no_native)]
    p, t = so.speakers((2, 3, 500), 5)
    out = sdr_mod.signal_distortion_ratio(p, t, filter_length=16)
    assert out.dtype == torch.float32 and out.shape == (2, 3)
    best, perm = pit_mod.permutation_invariant_training(p, t, sdr_mod.signal_distortion_ratio, filter_length=16)
    assert torch.equal(perm, torch.arange(3).expand(2, 3))
    assert not any(calls)
