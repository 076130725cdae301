"""An independent NumPy statement of the SRMR chain of ``functional/audio/srmr.py``, vectorised over signals and channels with one
Python step per sample.  Nothing is imported from the library: the filter design is restated here.

Stages: the four direct-form-I gammatone biquads with a clamp to ``[-1, 1]`` after each and the division by the gain; the Hilbert
transform at ``nfft = ceil(T / 16) * 16``; the eight modulation biquads on the envelope; the energies of the periodic-Hamming frames;
the score with its ``k90`` and ``k*``.  Every stage takes a ``dtype``: ``np.longdouble`` is the reference, ``np.float64`` the statement
whose distance from it (``err_comp64``) sizes the bounds of ``tests/test_srmr_gpu.py``.  On a host whose long double is no wider than
a double that distance is zero and the value tests fail; ``test_srmr_native_cpu.py`` asserts the extended type is there.
"""
import math
from functools import lru_cache
from typing import NamedTuple, Optional

import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
EAR_Q, MIN_BW = 9.26449, 24.7


class Design(NamedTuple):
    coefs: np.ndarray  # [N, 10] fp64: A0, A11, A12, A13, A14, A2, B0, B1, B2, gain; channel 0 is the highest in frequency
    mod: np.ndarray  # [8, 2 (b, a), 3] fp64
    cutoffs: np.ndarray  # [8] lower cutoffs of the modulation filters
    erbs: np.ndarray  # [N] bandwidths from the lowest channel upwards (the order k90 counts in)
    window: np.ndarray  # [w_length] fp64
    w_length: int
    w_inc: int


def centre_freqs(fs, n, low):
    k = EAR_Q * MIN_BW
    frac = np.arange(1, n + 1, dtype=np.float64) / n
    return -k + np.exp(frac * (-np.log(fs / 2 + k) + np.log(low + k))) * (fs / 2 + k)


@lru_cache(maxsize=None)
def design(fs, n=23, low=125.0, min_cf=4.0, max_cf=128.0):
    cf = centre_freqs(fs, n, low)
    t = 1.0 / fs
    erb = cf / EAR_Q + MIN_BW
    b = 1.019 * 2 * math.pi * erb
    arg = 2 * cf * math.pi * t
    vec = np.exp(2j * arg)
    rp, rn = math.sqrt(3 + 2**1.5), math.sqrt(3 - 2**1.5)
    common = -t * np.exp(-(b * t))
    k1 = [np.cos(arg) + rp * np.sin(arg), np.cos(arg) - rp * np.sin(arg), np.cos(arg) + rn * np.sin(arg), np.cos(arg) - rn * np.sin(arg)]
    ga = np.exp(1j * arg - b * t)
    gain = np.abs((vec - ga * k1[0]) * (vec - ga * k1[1]) * (vec - ga * k1[2]) * (vec - ga * k1[3])
                  * (t * np.exp(b * t) / (-1 / np.exp(b * t) + 1 + vec * (1 - np.exp(b * t)))) ** 4)
    coefs = np.stack([np.full_like(cf, t), common * k1[0], common * k1[1], common * k1[2], common * k1[3], np.zeros_like(cf), np.ones_like(cf),
                      -2 * np.cos(arg) / np.exp(b * t), np.exp(-2 * b * t), gain], axis=1)
    spacing = (max_cf / min_cf) ** (1.0 / 7)
    cfs = np.array([min_cf * spacing**k for k in range(8)], dtype=np.float64)
    w0 = np.tan(2 * math.pi * cfs / fs / 2)
    b0 = w0 / 2
    mod = np.stack([np.stack([b0, np.zeros_like(b0), -b0], axis=1), np.stack([1 + b0 + w0**2, 2 * w0**2 - 2, 1 - b0 + w0**2], axis=1)], axis=1)
    bw = np.tan(2 * math.pi * cfs / fs / 2) / 2 * fs / (2 * math.pi)
    w_length, w_inc = math.ceil(0.256 * fs), math.ceil(0.064 * fs)
    window = 0.54 - 0.46 * np.cos(2 * math.pi * np.arange(w_length, dtype=np.float64) / (w_length + 1))  # periodic Hamming of w_length + 1, last tap dropped
    return Design(coefs, mod, cfs - bw, erb[::-1].copy(), window, w_length, w_inc)


def _biquad(x, b, a, dtype, clamp):
    """Direct-form-I along the last axis of ``x [..., T]`` with ``b / a [..., 3]`` broadcast against ``x[..., 0]``: the b terms in tap
    order, then the a terms subtracted in tap order, on coefficients divided by ``a[0]`` once.  Returns the (clamped) output and
    whether the clamp changed a value."""
    b, a = np.asarray(b, dtype=dtype), np.asarray(a, dtype=dtype)
    b0, b1, b2 = (b[..., i] / a[..., 0] for i in range(3))
    a1, a2 = a[..., 1] / a[..., 0], a[..., 2] / a[..., 0]
    x = np.asarray(x, dtype=dtype)
    y = np.zeros(x.shape, dtype=dtype)
    zero = np.zeros(x.shape[:-1], dtype=dtype)
    x1, x2, y1, y2 = zero, zero, zero, zero
    for n in range(x.shape[-1]):
        xn = x[..., n]
        acc = b0 * xn
        acc = acc + b1 * x1
        acc = acc + b2 * x2
        acc = acc - a1 * y1
        acc = acc - a2 * y2
        x2, x1, y2, y1 = x1, xn, y1, acc
        y[..., n] = acc
    if not clamp:
        return y, False
    out = np.minimum(np.maximum(y, dtype(-1)), dtype(1))
    return out, bool((out != y).any())


def gammatone(x, coefs, dtype=LD):
    """``x [B, T]`` -> ``([B, N, T]`` in ``dtype``, the four stages' clipped flags)``."""
    x = np.asarray(x, dtype=dtype)
    y = np.broadcast_to(x[:, None, :], (x.shape[0], coefs.shape[0], x.shape[1]))
    clipped = []
    for col in (1, 2, 3, 4):
        y, c = _biquad(y, coefs[None, :, (0, col, 5)], coefs[None, :, 6:9], dtype, clamp=True)
        clipped.append(c)
    return y / np.asarray(coefs[:, 9], dtype=dtype)[None, :, None], tuple(clipped)


def hilbert(g):
    """Analytic signal of ``g [..., T]`` in its own precision (pocketfft runs in long double for long double input)."""
    t = g.shape[-1]
    nfft = math.ceil(t / 16) * 16
    h = np.zeros(nfft, dtype=g.dtype)
    h[0] = h[nfft // 2] = 1  # nfft is even
    h[1 : nfft // 2] = 2
    return np.fft.ifft(np.fft.fft(g, nfft, axis=-1) * h, axis=-1)[..., :t]


def energies(analytic, mod, window, w_inc, dtype=LD):
    """``analytic [B, N, T]`` complex -> ``[B, N, 8, F]`` in ``dtype``."""
    cdtype = np.clongdouble if dtype is LD else np.complex128
    env = np.abs(np.asarray(analytic, dtype=cdtype)).astype(dtype)
    t, wl = env.shape[-1], window.shape[0]
    y, _ = _biquad(np.broadcast_to(env[:, :, None, :], (*env.shape[:2], mod.shape[0], t)), mod[None, None, :, 0, :], mod[None, None, :, 1, :], dtype, clamp=False)
    frames = 1 + (t - wl) // w_inc
    w = np.asarray(window, dtype=dtype)
    return np.stack([((y[..., f * w_inc : f * w_inc + wl] * w) ** 2).sum(axis=-1) for f in range(frames)], axis=-1)


class Score(NamedTuple):
    value: float  # NaN where there is no k90
    k90: Optional[int]
    kstar: Optional[int]
    cum_before: float  # cumulative percentage one channel before k90 (0 when k90 is the first)
    cum_at: float


def kstar_of(bw, cutoffs):
    if cutoffs[4] <= bw < cutoffs[5]:
        return 5
    if cutoffs[5] <= bw < cutoffs[6]:
        return 6
    if cutoffs[6] <= bw < cutoffs[7]:
        return 7
    return 8 if cutoffs[7] <= bw else None


def score(energy, erbs, cutoffs, norm=False, kstar=None):
    """One signal: ``energy [N, 8, F]``.  ``kstar`` (``[N]``, indexed by k90) replaces the table derived from ``erbs`` / ``cutoffs``."""
    e = np.asarray(energy, dtype=LD)
    if norm:
        peak = e.mean(axis=0).max()
        floor = peak * LD(10.0 ** (-30.0 / 10.0))
        e = np.where(e < floor, floor, e)
        e = np.where(e > peak, peak, e)
    avg = e.mean(axis=-1)
    ac = avg.sum(axis=1) * 100 / avg.sum()
    cum = np.cumsum(ac[::-1])
    above = np.nonzero(cum > 90)[0]
    if above.size == 0:
        return Score(float("nan"), None, None, float("nan"), float("nan"))
    k90 = int(above[0])
    ks = int(kstar[k90]) if kstar is not None else kstar_of(erbs[k90], cutoffs)
    assert ks is not None, "bandwidth below every cutoff"
    return Score(float(avg[:, :4].sum() / avg[:, 4:ks].sum()), k90, ks, float(cum[k90 - 1]) if k90 else 0.0, float(cum[k90]))


def assert_margin(s, d):
    """The hard decisions of a value case are safe: the cumulative percentages around k90 keep 1e-6 from 90, no bandwidth is a cutoff."""
    assert s.k90 is not None and s.cum_at - 90 >= 1e-6 and 90 - s.cum_before >= 1e-6, s
    assert not np.isin(d.erbs, d.cutoffs).any()


def normalise(x):
    x = np.asarray(x, dtype=np.float64)
    peak = np.abs(x).max(axis=-1, keepdims=True)
    return x / np.where(peak > 1, peak, 1.0)


class Chain(NamedTuple):
    gam: np.ndarray  # [B, N, T] long double
    gam64: np.ndarray
    clipped: tuple
    analytic64: np.ndarray  # [B, N, T] complex128: the Hilbert transform of gam64, the input of both energy statements
    energy: np.ndarray  # [B, N, 8, F] long double, from analytic64
    energy64: np.ndarray
    scores: list  # Score per signal of the whole chain in long double (its own Hilbert transform)
    scores64: list  # ... of the whole chain in fp64


def chain(x, d, norm=False):
    """Every stage of ``x [B, T]`` (already normalised) in both precisions."""
    gam, clipped = gammatone(x, d.coefs, LD)
    gam64, _ = gammatone(x, d.coefs, np.float64)
    analytic64 = hilbert(gam64)
    energy = energies(analytic64, d.mod, d.window, d.w_inc, LD)
    energy64 = energies(analytic64, d.mod, d.window, d.w_inc, np.float64)
    whole = energies(hilbert(gam), d.mod, d.window, d.w_inc, LD)
    return Chain(gam, gam64, clipped, analytic64, energy, energy64, [score(e, d.erbs, d.cutoffs, norm) for e in whole],
                 [score(e, d.erbs, d.cutoffs, norm) for e in energy64])


def signals(fs, t, seed, b=3):
    """Amplitude-modulated tones plus noise (the shape of ``test_srmr.py``'s signal), one tone and one modulation rate per signal."""
    rng = np.random.default_rng(seed)
    n = np.arange(t) / fs
    rows = []
    for i in range(b):
        tone, rate = 300 - 70 * (i % 3), 4 + 3 * (i % 3)  # below the Nyquist frequency of every rate the tests use (>= 1 kHz)
        rows.append(0.3 * np.sin(2 * math.pi * tone * n) * (1 + np.sin(2 * math.pi * rate * n)) + 0.05 * rng.standard_normal(t))
    return np.stack(rows)
