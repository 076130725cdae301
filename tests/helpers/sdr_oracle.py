"""CPU oracle of ``signal_distortion_ratio``, written from the formula in ``numpy.longdouble`` (nothing imported from the package).

For one pair ``(preds, target)`` of length ``T`` and a filter of ``L`` taps:

* ``t~ = t − mean(t)``, ``p~ = p − mean(p)`` when ``zero_mean``;
* direct lag sums ``r[k] = Σ_n t~[n] t~[n + k]``, ``c[k] = Σ_n t~[n] p~[n + k]`` (``k < L``; the target is the unshifted factor) and ``pp = Σ p~²``;
* the normalisation of the signals applied to the sums: ``s_t = 1 / max(sqrt(r[0]), 1e-6)``, ``s_p = 1 / max(sqrt(pp), 1e-6)``, ``r <- r s_t²``,
  ``b = c s_t s_p``; then ``r[0] += load_diag``;
* the dense symmetric Toeplitz matrix of ``r`` solved by Gaussian elimination with partial pivoting (deliberately not Levinson);
* ``coh = Σ b x`` and ``10 log10(coh / (1 − coh))``.

``longdouble`` has a 64-bit mantissa on x86; ``require_longdouble()`` skips where it has not.  ``lag_sums_int`` is the same lag sums in
``int64`` for integer-valued signals (exact).  ``ref64`` is the reference arithmetic in fp64 (FFT correlations, dense
``torch.linalg.solve``): its distance from the oracle is the yardstick of ``bound``.

``bound`` is the tolerance rule for dB values of a vector of signals: ``|got_i − oracle_i| <= 4 max_i |ref64_i − oracle_i| + L 2⁻⁵³ (10 / ln 10)
/ (coh_i (1 − coh_i))``: one rounding error per recursion step in ``coh``, pushed through the derivative of the dB map.

Generators return fp32 ``(preds, target)`` of ``[n, T]``.
"""
import math
from typing import Optional, Tuple

import numpy as np
import pytest
import torch
from torch import Tensor

from tests.helpers.audio_oracle import speakers  # noqa: F401  (asymmetric pair matrices)

LD = np.longdouble


def require_longdouble() -> None:
    if np.finfo(LD).nmant < 63:
        pytest.skip("numpy.longdouble has no 64-bit mantissa on this host")


def _np(x: Tensor) -> np.ndarray:
    return x.detach().cpu().to(torch.float64).numpy()


def lag_sums(preds: Tensor, target: Tensor, filter_length: int, zero_mean: bool = False) -> Tuple[np.ndarray, np.ndarray, np.longdouble]:
    """``(r[L], c[L], pp)`` of one 1-D pair in longdouble; lags from ``T`` on are zero."""
    assert np.finfo(LD).nmant >= 63
    p, t = _np(preds).astype(LD), _np(target).astype(LD)
    n = t.shape[0]
    if zero_mean:
        p, t = p - p.sum() / LD(n), t - t.sum() / LD(n)
    r, c = np.zeros(filter_length, dtype=LD), np.zeros(filter_length, dtype=LD)
    for k in range(min(filter_length, n)):
        r[k] = (t[: n - k] * t[k:]).sum()
        c[k] = (t[: n - k] * p[k:]).sum()
    return r, c, (p * p).sum()


def lag_sums_int(preds: Tensor, target: Tensor, filter_length: int, mean_p: int = 0, mean_t: int = 0) -> Tuple[np.ndarray, np.ndarray, int]:
    """The lag sums of one integer-valued 1-D pair in ``int64`` (the integer means subtracted first)."""
    p = _np(preds).astype(np.int64) - int(mean_p)
    t = _np(target).astype(np.int64) - int(mean_t)
    assert np.array_equal(p + int(mean_p), _np(preds)) and np.array_equal(t + int(mean_t), _np(target)), "signals are not integer-valued"
    n = t.shape[0]
    r, c = np.zeros(filter_length, dtype=np.int64), np.zeros(filter_length, dtype=np.int64)
    for k in range(min(filter_length, n)):
        r[k] = int((t[: n - k] * t[k:]).sum())
        c[k] = int((t[: n - k] * p[k:]).sum())
    return r, c, int((p * p).sum())


def _solve(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Gaussian elimination with partial pivoting and back substitution, longdouble."""
    a, b = a.copy(), b.copy()
    n = b.shape[0]
    for k in range(n - 1):
        piv = k + int(np.argmax(np.abs(a[k:, k])))
        if piv != k:
            a[[k, piv]] = a[[piv, k]]
            b[[k, piv]] = b[[piv, k]]
        f = a[k + 1 :, k] / a[k, k]
        a[k + 1 :, k:] -= f[:, None] * a[k, k:][None, :]
        b[k + 1 :] -= f * b[k]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - (a[i, i + 1 :] * x[i + 1 :]).sum()) / a[i, i]
    return x


def sdr_pair(preds: Tensor, target: Tensor, filter_length: int = 512, zero_mean: bool = False, load_diag: Optional[float] = None) -> Tuple[float, float]:
    """``(coh, dB)`` of one 1-D pair, evaluated in longdouble and rounded once to fp64."""
    r, c, pp = lag_sums(preds, target, filter_length, zero_mean)
    s_t = LD(1) / max(np.sqrt(r[0]), LD(1e-6))
    s_p = LD(1) / max(np.sqrt(pp), LD(1e-6))
    r, b = r * s_t * s_t, c * s_t * s_p
    if load_diag is not None:
        r[0] = r[0] + LD(load_diag)
    idx = np.abs(np.arange(filter_length)[:, None] - np.arange(filter_length)[None, :])
    x = _solve(r[idx], b)
    coh = (b * x).sum()
    return float(coh), float(LD(10) * np.log10(coh / (LD(1) - coh)))


def sdr(preds: Tensor, target: Tensor, filter_length: int = 512, zero_mean: bool = False, load_diag: Optional[float] = None) -> Tuple[Tensor, Tensor]:
    """``(coh, dB)`` fp64 tensors over the leading dims of ``(..., T)`` inputs, one pair at a time."""
    lead = preds.shape[:-1]
    p, t = preds.reshape(-1, preds.shape[-1]), target.reshape(-1, target.shape[-1])
    both = [sdr_pair(p[i], t[i], filter_length, zero_mean, load_diag) for i in range(p.shape[0])]
    coh = torch.tensor([v[0] for v in both], dtype=torch.float64).reshape(lead)
    return coh, torch.tensor([v[1] for v in both], dtype=torch.float64).reshape(lead)


def ref64(preds: Tensor, target: Tensor, filter_length: int = 512, zero_mean: bool = False, load_diag: Optional[float] = None) -> Tensor:
    """The reference arithmetic in fp64 on the CPU: normalised signals, FFT correlations, dense ``torch.linalg.solve``."""
    p, t = preds.detach().cpu().double(), target.detach().cpu().double()
    if zero_mean:
        p, t = p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True)
    t = t / torch.clamp(torch.linalg.norm(t, dim=-1, keepdim=True), min=1e-6)
    p = p / torch.clamp(torch.linalg.norm(p, dim=-1, keepdim=True), min=1e-6)
    n_fft = 2 ** math.ceil(math.log2(p.shape[-1] + t.shape[-1] - 1))
    t_fft = torch.fft.rfft(t, n=n_fft, dim=-1)
    r = torch.fft.irfft(t_fft.real**2 + t_fft.imag**2, n=n_fft)[..., :filter_length]
    b = torch.fft.irfft(t_fft.conj() * torch.fft.rfft(p, n=n_fft, dim=-1), n=n_fft, dim=-1)[..., :filter_length]
    if load_diag is not None:
        r[..., 0] += load_diag
    idx = (torch.arange(filter_length)[:, None] - torch.arange(filter_length)[None, :]).abs()
    sol = torch.linalg.solve(r[..., idx], b)
    coh = torch.einsum("...l,...l->...", b, sol)
    return 10.0 * torch.log10(coh / (1 - coh))


def bound(ref_db: Tensor, oracle_db: Tensor, coh: Tensor, filter_length: int, fp32_result: bool = False) -> Tensor:
    """The tolerance of every signal of a vector (see the module docstring); ``fp32_result`` adds half an fp32 ulp of the result."""
    ref_err = float((ref_db.double() - oracle_db).abs().max())
    tol = 4.0 * ref_err + filter_length * 2.0**-53 * (10.0 / math.log(10.0)) / (coh * (1.0 - coh))
    if fp32_result:
        ulp = torch.tensor(np.spacing(oracle_db.abs().float().numpy()), dtype=torch.float64).reshape(oracle_db.shape)
        tol = tol + 0.5 * ulp
    return tol


def error_over_bound(got: Tensor, ref_db: Tensor, oracle_db: Tensor, coh: Tensor, filter_length: int, fp32_result: bool = False) -> float:
    """``max_i |got_i − oracle_i| / bound_i``: at most 1 for a result within the rule."""
    err = (got.detach().cpu().double() - oracle_db).abs()
    return float((err / bound(ref_db, oracle_db, coh, filter_length, fp32_result)).max())


# ------------------------------------------------------------------------------------------------------------------ generators
def _randn(rng: np.random.RandomState, *shape: int) -> np.ndarray:
    return rng.standard_normal(shape)


def _pair(p: np.ndarray, t: np.ndarray) -> Tuple[Tensor, Tensor]:
    return torch.from_numpy(p).float(), torch.from_numpy(t).float()


def white(n: int, time: int, seed: int, snr_db: float = 14.0) -> Tuple[Tensor, Tensor]:
    """A white target plus white noise ``snr_db`` below it."""
    rng = np.random.RandomState(seed)
    t = _randn(rng, n, time)
    return _pair(t + 10.0 ** (-snr_db / 20.0) * _randn(rng, n, time), t)


def ar1(n: int, time: int, seed: int, pole: float = 0.95) -> Tuple[Tensor, Tensor]:
    """An AR(1) target (an ill-conditioned Toeplitz matrix) plus white noise at 0.2 of its innovation's level."""
    rng = np.random.RandomState(seed)
    e = _randn(rng, n, time)
    t = np.zeros_like(e)
    t[:, 0] = e[:, 0]
    for i in range(1, time):
        t[:, i] = pole * t[:, i - 1] + e[:, i]
    return _pair(t + 0.2 * _randn(rng, n, time), t)


def int16_scale(n: int, time: int, seed: int) -> Tuple[Tensor, Tensor]:
    """Integer-valued signals at the scale of 16-bit audio."""
    rng = np.random.RandomState(seed)
    t = np.clip(np.round(3000.0 * _randn(rng, n, time)), -32768, 32767)
    p = np.clip(t + np.round(600.0 * _randn(rng, n, time)), -32768, 32767)
    return _pair(p, t)


def high_snr(n: int, time: int, seed: int) -> Tuple[Tensor, Tensor]:
    """60 dB: ``1 − coh`` cancels."""
    return white(n, time, seed, 60.0)


def dc_offset(n: int, time: int, seed: int, offset: float = 5.0) -> Tuple[Tensor, Tensor]:
    """The white pair with ``offset`` added to both signals."""
    rng = np.random.RandomState(seed)
    t = _randn(rng, n, time)
    return _pair(t + 10.0 ** (-14.0 / 20.0) * _randn(rng, n, time) + offset, t + offset)


def small_ints(shape: Tuple[int, ...], seed: int, low: int = -8, high: int = 8) -> Tensor:
    """Integer-valued fp32 values in ``[low, high]``."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(low, high + 1, shape, generator=g).float()


GENERATORS = {"white": white, "ar1": ar1, "int16": int16_scale, "60dB": high_snr, "dc": dc_offset}
