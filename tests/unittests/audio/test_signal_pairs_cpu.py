"""SNR, SI-SDR, SA-SDR and the PIT pair matrix on the CPU: the test oracle against the reference and this package's composition, the
native gate and PIT's branch arm by arm, and no native call for CPU tensors."""
import pytest
import torch

import torchmetrics_forked_amd.functional.audio.pit as pit_mod
import torchmetrics_forked_amd.functional.audio.sdr as sdr_mod
import torchmetrics_forked_amd.functional.audio.snr as snr_mod
import torchmetrics_forked_amd.ops.audio as ops_audio
from tests.helpers import audio_oracle as ao
from tests.helpers.routes import count_calls
from torchmetrics_forked_amd import ops

_CASES = [((3, 2, 1000), 1.0, 0.0), ((2, 3, 777), 3000.0, 0.0), ((2, 2, 501), 1.0, 100.0)]
_FLAGS = [False, True]


def _rel(got, want):
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("shape,scale,offset", _CASES)
def test_oracle_matches_the_reference_in_fp64(reference, shape, scale, offset):
    p, t = ao.speakers(shape, 11 + shape[-1], scale, offset)
    p, t = p.double(), t.double()
    ref = reference.functional.audio
    # two fp64 evaluations of one formula: 1e-15-class differences; 1e-10 relative is far below what a wrong mean, scale or eps gives
    for zm in _FLAGS:
        assert _rel(ao.snr(p, t, zm), ref.signal_noise_ratio(p, t, zero_mean=zm)) <= 1e-10
        assert _rel(ao.si_sdr(p, t, zm), ref.scale_invariant_signal_distortion_ratio(p, t, zero_mean=zm)) <= 1e-10
        assert _rel(ao.snr(p, t, zm), snr_mod.signal_noise_ratio(p, t, zero_mean=zm)) <= 1e-10
        assert _rel(ao.si_sdr(p, t, zm), sdr_mod.scale_invariant_signal_distortion_ratio(p, t, zero_mean=zm)) <= 1e-10
        for si in _FLAGS:
            want = ao.sa_sdr(p, t, si, zm)
            assert _rel(want, ref.source_aggregated_signal_distortion_ratio(p, t, scale_invariant=si, zero_mean=zm)) <= 1e-10
            assert _rel(want, sdr_mod.source_aggregated_signal_distortion_ratio(p, t, scale_invariant=si, zero_mean=zm)) <= 1e-10
    assert _rel(ao.si_sdr(p, t, True), ref.scale_invariant_signal_noise_ratio(p, t)) <= 1e-10
    assert _rel(ao.si_sdr(p, t, True), snr_mod.scale_invariant_signal_noise_ratio(p, t)) <= 1e-10


@pytest.mark.parametrize("shape,scale,offset", _CASES)
def test_oracle_fp32_variant(shape, scale, offset):
    p, t = ao.speakers(shape, 5, scale, offset)
    for zm in _FLAGS:
        for a64, a32 in ((ao.snr(p, t, zm), ao.snr(p, t, zm, torch.float32)), (ao.si_sdr(p, t, zm), ao.si_sdr(p, t, zm, torch.float32)),
                         (ao.sa_sdr(p, t, True, zm), ao.sa_sdr(p, t, True, zm, torch.float32)),
                         (ao.sa_sdr(p, t, False, zm), ao.sa_sdr(p, t, False, zm, torch.float32))):
            assert a64.dtype == torch.float64 and a32.dtype == torch.float32 and a32.shape == a64.shape
            assert bool(torch.isfinite(a32).all()) and bool(torch.isfinite(a64).all())
            assert bool((a32.double() != a64).any())
            # a dB value from two fp32 sums of up to 3000 terms: 1e-4 relative is generous, a wrong formula is off by dBs; data at
            # +100 without zero_mean measures a -40 dB residual, where fp32 holds less
            assert _rel(a32, a64) <= (1e-4 if offset == 0 or zm else 1e-2)


def test_oracle_eps_is_the_input_dtype_constant():
    z = torch.zeros(3, 16)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        p = torch.ones(3, 16, dtype=dtype)
        eps = torch.finfo(dtype).eps
        want = 10 * torch.log10(torch.tensor(eps / (16 + eps), dtype=torch.float64))
        assert _rel(ao.snr(p, z.to(dtype)), want.expand(3)) <= 1e-12  # silent target: eps / (Σp² + eps)
        assert _rel(ao.si_sdr(p, z.to(dtype)), want.expand(3)) <= 1e-12  # α = eps / eps = 1
        assert torch.equal(ao.snr(z.to(dtype), z.to(dtype)), torch.zeros(3, dtype=torch.float64))  # both silent: exactly 0 dB
    assert _rel(ao.snr(torch.ones(3, 16), z, eps=0.5), 10 * torch.log10(torch.tensor(0.5 / 16.5, dtype=torch.float64)).expand(3)) <= 1e-12


def test_speakers_make_an_asymmetric_pair_matrix():
    p, t = ao.speakers((2, 4, 4000), 3)
    m = ao.pair_matrix(p, t, ao.si_sdr)
    assert float((m - m.transpose(1, 2)).abs().max()) > 1.0  # dB
    diag = torch.diagonal(m, dim1=1, dim2=2)
    assert bool((diag[:, :-1] > diag[:, 1:]).all())  # the noise level rises with the speaker index
    assert abs(float(diag[:, 0].mean()) - 14.0) < 0.5


class _OnGpu(torch.Tensor):
    """A plain CPU tensor that answers ``is_cuda`` with True: reaches the gate's later arms without a GPU."""

    is_cuda = property(lambda self: True)


def _gpu_like(*shape, dtype=torch.float32):
    return torch.rand(*shape).to(dtype).as_subclass(_OnGpu)


def test_gate_arm_by_arm(monkeypatch):
    ok = sdr_mod._native_signal_ok
    seen = []

    def use_native(*tensors):
        seen.append(tensors)
        return True

    monkeypatch.setattr(sdr_mod.ops, "use_native", use_native)
    monkeypatch.setattr(sdr_mod, "_AUDIO_NATIVE", True)
    p, t = _gpu_like(2, 3, 50), _gpu_like(2, 3, 50)
    assert ok(p, t) and len(seen) == 1 and seen[0][0] is p and seen[0][1] is t
    for dtype in (torch.bfloat16, torch.float16):
        assert ok(_gpu_like(2, 50, dtype=dtype), _gpu_like(2, 50, dtype=dtype))
    assert ok(_gpu_like(50), _gpu_like(50)) and ok(_gpu_like(2, 3, 4, 1), _gpu_like(2, 3, 4, 1))
    # device
    assert not ok(torch.rand(2, 50), torch.rand(2, 50))
    assert not ok(p, torch.rand(2, 3, 50)) and not ok(torch.rand(2, 3, 50), t)
    # dtype
    assert not ok(_gpu_like(2, 50, dtype=torch.float64), _gpu_like(2, 50, dtype=torch.float64))
    assert not ok(p, _gpu_like(2, 3, 50, dtype=torch.bfloat16))
    assert not ok(_gpu_like(2, 50, dtype=torch.complex64), _gpu_like(2, 50, dtype=torch.complex64))
    assert not ok(torch.randint(0, 9, (2, 50)).as_subclass(_OnGpu), torch.randint(0, 9, (2, 50)).as_subclass(_OnGpu))
    # shape, empty
    assert not ok(p, _gpu_like(2, 3, 51))
    assert not ok(_gpu_like(0, 50), _gpu_like(0, 50)) and not ok(_gpu_like(2, 0), _gpu_like(2, 0))
    assert not ok(torch.tensor(1.0).as_subclass(_OnGpu), torch.tensor(1.0).as_subclass(_OnGpu))
    # autograd: a requires_grad input under grad mode keeps the composition; under no_grad it does not
    pg = _gpu_like(2, 3, 50).requires_grad_()
    assert not ok(pg, t) and not ok(t, pg)
    with torch.no_grad():
        assert ok(pg, t)
    # the library's own answer and the knob
    n = len(seen)
    monkeypatch.setattr(sdr_mod.ops, "use_native", lambda *a: False)
    assert not ok(p, t)
    monkeypatch.setattr(sdr_mod.ops, "use_native", use_native)
    monkeypatch.setattr(sdr_mod, "_AUDIO_NATIVE", False)
    assert not ok(p, t) and len(seen) == n


def test_functionals_behind_the_gate(monkeypatch):
    """With the gate open the functionals hand the op ``[rows, 1, T]`` (SA-SDR ``[groups, S, T]``), the right flags and the dtype's eps, and
    give its result the input dtype and the leading shape."""
    calls = []

    def fake(preds, target, scale_invariant, zero_mean, pairing, eps):
        calls.append((tuple(preds.shape), tuple(target.shape), scale_invariant, zero_mean, pairing, eps))
        g, s = preds.shape[:2]
        return torch.arange(g if pairing == 2 else g * s, dtype=torch.float64).reshape((g,) if pairing == 2 else (g, s))

    monkeypatch.setattr(sdr_mod, "_native_signal_ok", lambda p, t: True)
    monkeypatch.setattr(snr_mod, "_native_signal_ok", lambda p, t: True)
    monkeypatch.setattr(sdr_mod, "_signal_pair_ratios", fake)
    p, t = torch.rand(2, 3, 50), torch.rand(2, 3, 50)
    eps = torch.finfo(torch.float32).eps
    rows = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    assert torch.equal(snr_mod.signal_noise_ratio(p, t), rows) and calls[-1] == ((6, 1, 50), (6, 1, 50), False, False, 0, eps)
    assert torch.equal(snr_mod.signal_noise_ratio(p, t, zero_mean=True), rows) and calls[-1][2:] == (False, True, 0, eps)
    assert torch.equal(sdr_mod.scale_invariant_signal_distortion_ratio(p, t), rows) and calls[-1][2:] == (True, False, 0, eps)
    assert torch.equal(snr_mod.scale_invariant_signal_noise_ratio(p, t), rows) and calls[-1][2:] == (True, True, 0, eps)
    out = sdr_mod.source_aggregated_signal_distortion_ratio(p, t, scale_invariant=False, zero_mean=True)
    assert torch.equal(out, torch.arange(2, dtype=torch.float32)) and calls[-1] == ((2, 3, 50), (2, 3, 50), False, True, 2, eps)
    out = sdr_mod.source_aggregated_signal_distortion_ratio(p[0], t[0])
    assert out.shape == () and calls[-1] == ((1, 3, 50), (1, 3, 50), True, False, 2, eps)
    out = snr_mod.signal_noise_ratio(p[0, 0].bfloat16(), t[0, 0].bfloat16())
    assert out.shape == () and out.dtype == torch.bfloat16 and calls[-1] == ((1, 1, 50), (1, 1, 50), False, False, 0, 2.0**-7)
    c = torch.view_as_complex(torch.rand(2, 5, 10, 2))
    out = snr_mod.complex_scale_invariant_signal_noise_ratio(c, c)
    assert out.shape == (2,) and calls[-1] == ((2, 1, 100), (2, 1, 100), True, False, 0, eps)
    # validation stays ahead of the gate
    n = len(calls)
    for fn in (snr_mod.signal_noise_ratio, sdr_mod.scale_invariant_signal_distortion_ratio, sdr_mod.source_aggregated_signal_distortion_ratio):
        with pytest.raises(RuntimeError, match="same shape"):
            fn(p, t[..., :49])
    with pytest.raises(RuntimeError, match="spk, time"):
        sdr_mod.source_aggregated_signal_distortion_ratio(p[0, 0], t[0, 0])
    assert len(calls) == n


def test_pit_branch_arm_by_arm(monkeypatch):
    calls = []

    def fake(preds, target, scale_invariant, zero_mean, pairing, eps):
        calls.append((scale_invariant, zero_mean, pairing, eps))
        return ao.pair_matrix(preds, target, ao.si_sdr if scale_invariant else ao.snr, zero_mean=zero_mean)

    gate = []
    monkeypatch.setattr(sdr_mod, "_native_signal_ok", lambda p, t: gate.append(1) or True)
    monkeypatch.setattr(ops_audio, "signal_pair_ratios", fake)
    p, t = ao.speakers((3, 3, 400), 8)
    eps = torch.finfo(torch.float32).eps
    mtx = pit_mod._native_pair_matrix
    si_sdr, si_snr, snr = sdr_mod.scale_invariant_signal_distortion_ratio, snr_mod.scale_invariant_signal_noise_ratio, snr_mod.signal_noise_ratio
    for fn, kwargs, flags in ((snr, {}, (False, False)), (snr, {"zero_mean": True}, (False, True)), (si_sdr, {}, (True, False)),
                              (si_sdr, {"zero_mean": True}, (True, True)), (si_sdr, {"zero_mean": False}, (True, False)), (si_snr, {}, (True, True))):
        out = mtx(p, t, fn, kwargs)
        assert out is not None and out.dtype == torch.float32 and out.shape == (3, 3, 3) and calls[-1] == (*flags, 1, eps)
    n, g = len(calls), len(gate)
    assert mtx(p, t, lambda a, b: si_sdr(a, b), {}) is None  # a user function
    assert mtx(p, t, sdr_mod.signal_distortion_ratio, {}) is None
    assert mtx(p, t, si_sdr, {"zero_mean": True, "other": 1}) is None and mtx(p, t, snr, {"other": 1}) is None
    assert mtx(p, t, si_snr, {"zero_mean": True}) is None  # SI-SNR takes no keyword: the composition raises as before
    assert mtx(p[..., None], t[..., None], si_sdr, {}) is None and mtx(p[:, 0], t[:, 0], si_sdr, {}) is None  # 4-D, 2-D
    assert len(calls) == n and len(gate) == g  # none of them asked the gate
    monkeypatch.setattr(sdr_mod, "_native_signal_ok", lambda p, t: False)
    assert mtx(p, t, si_sdr, {}) is None and len(calls) == n
    # the whole call through the branch equals the call through the composition
    monkeypatch.setattr(sdr_mod, "_native_signal_ok", lambda p, t: p.ndim == 3)  # (the row functionals inside the composition: 2-D)
    perm = torch.tensor([[2, 0, 1], [0, 1, 2], [1, 0, 2]])
    pp = pit_mod.pit_permutate(p, perm)
    best, got = pit_mod.permutation_invariant_training(pp, t, si_sdr)
    assert len(calls) == n + 1
    monkeypatch.setattr(sdr_mod, "_native_signal_ok", lambda p, t: False)
    best_c, got_c = pit_mod.permutation_invariant_training(pp, t, si_sdr)
    assert len(calls) == n + 1 and torch.equal(got, got_c) and _rel(best, best_c) <= 1e-5
    assert torch.equal(pit_mod.pit_permutate(pp, got), p)


def _no_native(*a, **k):
    raise AssertionError("the native signal-pair op was entered for CPU tensors")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_calls_never_reach_the_op(monkeypatch, dtype):
    from torchmetrics_forked_amd.audio import PermutationInvariantTraining, ScaleInvariantSignalDistortionRatio, SignalNoiseRatio

    calls = [count_calls(monkeypatch, sdr_mod, "_signal_pair_ratios", guard=_no_native),
             count_calls(monkeypatch, ops_audio, "signal_pair_ratios", guard=_no_native)]
    if ops.available():
        calls.append(count_calls(monkeypatch, torch.ops.tmx, "signal_pair_ratios", guard=_no_native))
    p, t = ao.speakers((3, 3, 800), 5)
    p, t = p.to(dtype), t.to(dtype)
    tol = 1e-10 if dtype == torch.float64 else 1e-4  # fp32: the composition's own error (test_oracle_fp32_variant)
    for zm in _FLAGS:
        out = snr_mod.signal_noise_ratio(p, t, zero_mean=zm)
        assert out.dtype == dtype and _rel(out, ao.snr(p, t, zm)) <= tol
        out = sdr_mod.scale_invariant_signal_distortion_ratio(p, t, zero_mean=zm)
        assert out.dtype == dtype and _rel(out, ao.si_sdr(p, t, zm)) <= tol
        for si in _FLAGS:
            out = sdr_mod.source_aggregated_signal_distortion_ratio(p, t, scale_invariant=si, zero_mean=zm)
            assert out.dtype == dtype and _rel(out, ao.sa_sdr(p, t, si, zm)) <= tol
    assert _rel(snr_mod.scale_invariant_signal_noise_ratio(p, t), ao.si_sdr(p, t, True)) <= tol
    for cls, want in ((SignalNoiseRatio, ao.snr(p, t)), (ScaleInvariantSignalDistortionRatio, ao.si_sdr(p, t))):
        m = cls()
        m.update(p[:1], t[:1])
        m.update(p[1:], t[1:])
        assert _rel(m.compute(), want.mean()) <= max(tol, 1e-6)
    want = ao.pair_matrix(p, t, ao.si_sdr)
    best, perm = pit_mod.permutation_invariant_training(p, t, sdr_mod.scale_invariant_signal_distortion_ratio)
    assert torch.equal(perm, torch.arange(3).expand(3, 3))
    assert _rel(best, torch.diagonal(want, dim1=1, dim2=2).mean(-1)) <= tol
    m = PermutationInvariantTraining(snr_mod.signal_noise_ratio, zero_mean=True)
    m.update(p, t)
    assert _rel(m.compute(), ao.snr(p, t, True).mean()) <= max(tol, 1e-6)
    assert not any(calls)
