"""Thin wrappers of the signal-pair ops of ``csrc/signal_pairs.hip`` (SNR, SI-SDR, SA-SDR and the PIT pair matrix), of the
STOI / ESTOI ops of ``csrc/stoi.hip``, of the SRMR ops of ``csrc/srmr.hip`` and of the SDR ops of ``csrc/sdr.hip``."""
import math
from typing import Dict, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

PAIR_DIAGONAL, PAIR_ALL, PAIR_AGGREGATED = 0, 1, 2

_STOI_FS = 10000
_stoi_table_cache: Dict[torch.device, Tensor] = {}
_stoi_filter_cache: Dict[Tuple[int, torch.device], Tuple[Tensor, int, int, int]] = {}


def _stoi_tables(device: torch.device) -> Tensor:
    """Hann window ``np.hanning(258)[1:-1]``, then ``cos`` and ``sin`` of ``2 pi i / 512``: 1280 fp64 values, uploaded once per device."""
    tab = _stoi_table_cache.get(device)
    if tab is None:
        k = torch.arange(1, 257, dtype=torch.float64)
        a = 2 * math.pi * torch.arange(512, dtype=torch.float64) / 512
        tab = torch.cat([0.5 - 0.5 * torch.cos(2 * math.pi * k / 257), torch.cos(a), torch.sin(a)]).to(device)
        _stoi_table_cache[device] = tab
    return tab


def _stoi_filter(fs: int, device: torch.device) -> Tuple[Tensor, int, int, int]:
    """``(h', up, down, n_pre_remove)`` of ``_resample_poly`` for ``fs -> 10 kHz``: the Octave filter scaled by ``up`` and padded in
    front, uploaded once per ``(fs, device)``.  The trailing padding of ``_resample_poly`` is zeros only: the kernel reads a tap past
    the end as 0, so the filter does not depend on the signal length."""
    key = (int(fs), device)
    hit = _stoi_filter_cache.get(key)
    if hit is None:
        g = math.gcd(_STOI_FS, int(fs))
        up, down = _STOI_FS // g, int(fs) // g
        if up == down:
            hit = (torch.empty(0, dtype=torch.float64, device=device), 1, 1, 0)
        else:
            from torchmetrics_forked_amd.functional.audio.stoi import _octave_filter

            h = torch.tensor(_octave_filter(_STOI_FS, int(fs)), dtype=torch.float64) * up
            half_len = (h.numel() - 1) // 2
            n_pre_pad = down - half_len % down
            hit = (torch.nn.functional.pad(h, (n_pre_pad, 0)).to(device), up, down, (half_len + n_pre_pad) // down)
        _stoi_filter_cache[key] = hit
    return hit


def stoi_scores(preds: Tensor, target: Tensor, fs: int, extended: bool) -> Tuple[Tensor, Tensor]:
    """``tmx::stoi_scores``: STOI (or ESTOI) of every signal of ``preds`` / ``target`` ``[B, T]`` (fp32 / fp64 / bf16 / fp16, read in
    place; ``target`` is the clean signal) sampled at ``fs``: ``(scores fp64 [B], frames int32 [B])``, ``frames`` the number of STFT frames
    left after the silent frames are removed; a signal with fewer than 30 scores exactly ``1e-5``.  fp64 on the up-cast samples, the
    stages of ``functional/audio/stoi.py``; no host read, no atomics (two runs are bit-equal).  No autograd."""
    filt, up, down, pre = _stoi_filter(fs, preds.device)
    return torch.ops.tmx.stoi_scores(preds, target, _stoi_tables(preds.device), filt, up, down, pre, bool(extended))


def stoi_bands(preds: Tensor, target: Tensor, fs: int) -> Tuple[Tensor, Tensor, Tensor]:
    """``tmx::stoi_bands``: the third-octave envelopes ``stoi_scores`` correlates, ``(x_tob, y_tob, frames)``: fp64 ``[B, 15, Jmax]`` of the
    clean and the processed signal (zero past ``frames[b]``) and int32 ``[B]``.  For tests: a window or band gain cancels out of the score."""
    filt, up, down, pre = _stoi_filter(fs, preds.device)
    return torch.ops.tmx.stoi_bands(preds, target, _stoi_tables(preds.device), filt, up, down, pre)


def stoi_tile() -> Tuple[int, int, int, int, int]:
    """``(STFT frames per workgroup of the band kernel, segments per workgroup of the segment kernel, outputs per workgroup of the
    resampler, frames per strip of the kept-frame scan, frames per workgroup of the energy kernel)``."""
    return tuple(int(v) for v in torch.ops.tmx.stoi_tile())  # type: ignore[return-value]


class SrmrTables(NamedTuple):
    """What the SRMR ops read besides the signal, on one device: ``coefs [N, 10]`` (``_make_erb_filters``), ``mod [8, 2, 3]``
    (``_compute_modulation_filterbank_and_cutoffs``), the periodic Hamming ``window [w_length]``, ``kstar [N]`` int32 (``None`` when some
    bandwidth falls below every cutoff ``_cal_srmr_score`` accepts), ``w_length`` and ``w_inc``."""

    coefs: Tensor
    mod: Tensor
    window: Tensor
    kstar: Optional[Tensor]
    w_length: int
    w_inc: int


_srmr_table_cache: Dict[Tuple[int, int, float, float, float, torch.device], SrmrTables] = {}
_srmr_hilbert_cache: Dict[Tuple[int, torch.device], Tensor] = {}


def srmr_kstar(erbs: Tensor, cutoffs: Tensor) -> Optional[Tuple[int, ...]]:
    """``k*`` of ``_cal_srmr_score`` for every bandwidth of ``erbs`` (fp64, host), with its comparisons on the same fp64 values;
    ``None`` where it would raise.  The bandwidth of a signal can only be one of these, so the choice is made ahead of the kernel."""
    out = []
    for bw in erbs:
        if (cutoffs[4] <= bw) and (cutoffs[5] > bw):
            out.append(5)
        elif (cutoffs[5] <= bw) and (cutoffs[6] > bw):
            out.append(6)
        elif (cutoffs[6] <= bw) and (cutoffs[7] > bw):
            out.append(7)
        elif cutoffs[7] <= bw:
            out.append(8)
        else:
            return None
    return tuple(out)


def srmr_tables(fs: int, n_cochlear_filters: int, low_freq: float, min_cf: float, max_cf: float, device: torch.device) -> SrmrTables:
    """The tables of one argument set, designed on the host in fp64 and uploaded once per
    ``(fs, n_cochlear_filters, low_freq, min_cf, max_cf, device)``: a second call with the same arguments uploads nothing."""
    key = (int(fs), int(n_cochlear_filters), float(low_freq), float(min_cf), float(max_cf), device)
    hit = _srmr_table_cache.get(key)
    if hit is None:
        from torchmetrics_forked_amd.functional.audio import srmr

        cpu = torch.device("cpu")
        w_length, w_inc = math.ceil(0.256 * fs), math.ceil(0.064 * fs)
        coefs = srmr._make_erb_filters(fs, n_cochlear_filters, low_freq, device=cpu)
        _, mod, cutoffs, _ = srmr._compute_modulation_filterbank_and_cutoffs(min_cf, max_cf, n=8, fs=fs, q=2, device=cpu)
        erbs = torch.flipud(srmr._calc_erbs(low_freq, fs, n_cochlear_filters, device=cpu))
        ks = srmr_kstar(erbs, cutoffs)
        window = torch.hamming_window(w_length + 1, dtype=torch.float64)[:-1]
        hit = SrmrTables(coefs.contiguous().to(device), mod.contiguous().to(device), window.contiguous().to(device),
                         None if ks is None else torch.tensor(ks, dtype=torch.int32).to(device), w_length, w_inc)
        if len(_srmr_table_cache) >= 64:
            _srmr_table_cache.clear()
        _srmr_table_cache[key] = hit
    return hit


def srmr_hilbert_weights(nfft: int, device: torch.device) -> Tensor:
    """The one-sided weights of ``_hilbert`` (1 at DC and Nyquist, 2 between, 0 above), fp64 ``[nfft]``, uploaded once per length and device."""
    key = (int(nfft), device)
    h = _srmr_hilbert_cache.get(key)
    if h is None:
        h = torch.zeros(nfft, dtype=torch.float64)
        if nfft % 2 == 0:
            h[0] = h[nfft // 2] = 1
            h[1 : nfft // 2] = 2
        else:
            h[0] = 1
            h[1 : (nfft + 1) // 2] = 2
        h = h.to(device)
        if len(_srmr_hilbert_cache) >= 16:
            _srmr_hilbert_cache.clear()
        _srmr_hilbert_cache[key] = h
    return h


def srmr_gammatone(preds: Tensor, coefs: Tensor, nfft: int) -> Tensor:
    """``tmx::srmr_gammatone``: the 4-stage gammatone cascade of ``_erb_filterbank`` on ``preds`` ``[B, T]`` (fp32 / fp64 / bf16 / fp16, read in
    place with its row stride, up-cast per sample) with the ``[N, 10]`` fp64 table ``coefs``: fp64 ``[B, N, nfft]``, ``nfft >= T``, zeros from
    ``T`` on.  Per channel four direct-form-I biquads in ``tmx::iir_filter``'s operation order, each stage clamped to ``[-1, 1]`` before it
    feeds the next (the recursion itself runs on the unclamped values, as ``lfilter``), then the division by the gain.  One thread per
    (signal, channel); no host read, no atomics (two runs are bit-equal, a signal alone has its bits in a batch).  No autograd."""
    return torch.ops.tmx.srmr_gammatone(preds, coefs, int(nfft))


def srmr_energies(analytic: Tensor, time: int, mod: Tensor, window: Tensor, w_inc: int) -> Tensor:
    """``tmx::srmr_energies``: modulation-band frame energies of the analytic signal ``[B, N, nfft]`` complex128 (read in place with its row
    stride; only the first ``time`` samples are used): ``|z|`` through the ``M`` biquads of ``mod`` ``[M, 2, 3]`` (no clamp), then
    ``Σ_n (y[n] window[n − f w_inc])²`` over the ``F = 1 + (time − w_length) // w_inc`` frames, samples in order: fp64 ``[B, N, M, F]``.
    Needs ``w_length <= 4 w_inc`` (true of SRMR's 256 ms / 64 ms at every rate).  Neither the ``[B, N, M, time]`` filter output nor a frame
    tensor is allocated.  No host read, no atomics.  No autograd."""
    return torch.ops.tmx.srmr_energies(analytic, int(time), mod, window, int(w_inc))


def srmr_scores(energy: Tensor, kstar: Tensor, norm: bool) -> Tensor:
    """``tmx::srmr_scores``: SRMR of every signal from its energies ``[B, N, M, F]`` fp64: the optional 30 dB normalisation (``norm``), the
    frame means, the cumulative energy percentage from the lowest channel (index ``N − 1``) upwards, ``k90`` = the first count above 90,
    ``k* = kstar[k90]`` (int32 ``[N]``, see ``srmr_kstar``) and ``Σ avg[:, :4] / Σ avg[:, 4:k*]``: fp64 ``[B]``.  A signal without a ``k90``
    (silent, NaN) scores NaN and leaves the others as they are.  No host read, no atomics.  No autograd."""
    return torch.ops.tmx.srmr_scores(energy, kstar, bool(norm))


def srmr_tile() -> Tuple[int, int, int]:
    """``(time steps per staged block and threads per workgroup of the two filter kernels, frames that can hold one sample, bytes up to
    which the zero-filled window is kept in LDS)``."""
    return tuple(int(v) for v in torch.ops.tmx.srmr_tile())  # type: ignore[return-value]


def sdr_scores(preds: Tensor, target: Tensor, filter_length: int, zero_mean: bool, load_diag: Optional[float], pairing: int) -> Tensor:
    """``tmx::sdr_scores``: fp64 ``signal_distortion_ratio`` in dB of ``preds`` / ``target`` ``[G, S, T]`` (fp32 / bf16 / fp16 of one dtype, made
    contiguous and read in place).  In fp64 on the up-cast samples: the means are subtracted on load when ``zero_mean``; the first
    ``filter_length`` lags of the target's autocorrelation and of the cross-correlation are summed directly (no FFT; on
    ``v_mfma_f64_16x16x4_f64`` for signals of 16 384 samples or more whose filter fills its 256-lag tiles, else on the vector ALU); the composition's
    normalisation ``1 / max(‖·‖, 1e-6)`` is applied to the sums; ``load_diag`` is added to lag 0; the symmetric Toeplitz system is solved
    by the Levinson recursion in LDS; ``10 log10(coh / (1 − coh))`` with ``coh = Σ b x``.  ``pairing`` ``PAIR_DIAGONAL``: ``[G, S]``, the pairs
    ``(p_s, t_s)``; ``PAIR_ALL``: ``[G, S, S]`` with ``out[g, j, i] = SDR(preds[g, i], target[g, j])``, every target's autocorrelation and Durbin
    vector computed once.  ``1 <= filter_length <= sdr_tile()[3]``.  A silent or NaN target scores NaN.  No full-size temporary, no
    host read, no atomics (two runs are bit-equal).  No autograd."""
    return torch.ops.tmx.sdr_scores(preds, target, int(filter_length), bool(zero_mean), None if load_diag is None else float(load_diag), int(pairing))


def sdr_correlations(preds: Tensor, target: Tensor, filter_length: int, zero_mean: bool, pairing: int) -> Tuple[Tensor, Tensor, Tensor]:
    """``tmx::sdr_correlations``: the raw fp64 lag sums ``sdr_scores`` starts from, before any scaling: ``r[g, j, k] = Σ_n t~_j[n] t~_j[n + k]``
    ``[G, S, L]``; ``c = Σ_n t~_j[n] p~_i[n + k]`` as ``[G, S, L]`` (``PAIR_DIAGONAL``, ``i = j``) or ``[G, S(target), S(preds), L]`` (``PAIR_ALL``);
    ``pp[g, i] = Σ p~_i²`` ``[G, S]``.  For tests: on integer-valued signals every one of them is exact."""
    r, c, pp = torch.ops.tmx.sdr_correlations(preds, target, int(filter_length), bool(zero_mean), int(pairing))
    return r, c, pp


def sdr_chunks(g: int, s: int, t: int, filter_length: int, pairing: int) -> int:
    """How many chunks the correlation pass of ``sdr_scores`` splits every signal of a ``[g, s, t]`` call into: a function of the shape,
    the filter length and the pairing alone, unless ``TMX_SDR_CHUNK`` (samples per chunk, read per call) overrides it.  Only the last
    chunk may be short."""
    return int(torch.ops.tmx.sdr_chunks(int(g), int(s), int(t), int(filter_length), int(pairing)))


def sdr_tile() -> Tuple[int, int, int, int, int, int, int, int]:
    """``(lags per workgroup of the VALU form of the correlation pass, adjacent lags per lane, samples staged in LDS at a time, the largest
    filter_length (3 L fp64 values in LDS), the longest filter the solve runs in a single wave, right-hand sides one recursion serves
    at most, lags per workgroup of the matrix-core form, the signal length from which that form is used)``."""
    return tuple(int(v) for v in torch.ops.tmx.sdr_tile())  # type: ignore[return-value]


def signal_pair_ratios(preds: Tensor, target: Tensor, scale_invariant: bool, zero_mean: bool, pairing: int, eps: float) -> Tensor:
    """``tmx::signal_pair_ratios``: fp64 ratios in dB of ``preds`` / ``target`` ``[G, S, T]`` (fp32 / bf16 / fp16, made contiguous and read
    in place; no expanded copy).  Per pair, in fp64 on the up-cast samples: ``p~ = p − mean(p)``, ``t~ = t − mean(t)`` when ``zero_mean``;
    ``α = (Σ p~ t~ + eps) / (Σ t~² + eps)`` when ``scale_invariant``, else 1; ``10 log10((α² Σ t~² + eps) / (Σ (α t~ − p~)² + eps))``.
    ``pairing`` 0: ``[G, S]``, the pairs ``(p_s, t_s)``; 1: ``[G, S, S]`` with ``out[g, j, i]`` the ratio of ``(preds[g, i], target[g, j])``; 2: ``[G]``, one
    ``α`` and one ratio over the ``S`` pairs ``(p_s, t_s)`` of a group.  ``eps`` is the caller's ``torch.finfo(dtype).eps``: silent targets,
    ``p == t`` and ``T == 1`` give the composition's finite values.  One fp64 partial per workgroup added in a fixed order (no atomics:
    two runs are bit-equal).  No host read.  No autograd."""
    return torch.ops.tmx.signal_pair_ratios(preds, target, bool(scale_invariant), bool(zero_mean), int(pairing), float(eps))


def signal_chunks(g: int, s: int, t: int, pairing: int) -> int:
    """How many chunks the pair passes of ``signal_pair_ratios`` split every signal of a ``[g, s, t]`` call into: a function of the
    shape and the pairing alone, unless ``TMX_SIGNAL_CHUNK`` (samples per chunk, read per call, rounded up to the alignment of
    ``signal_tile``) overrides it.  Only the last chunk may be short."""
    return int(torch.ops.tmx.signal_chunks(int(g), int(s), int(t), int(pairing)))


def signal_tile() -> Tuple[int, int, int, int]:
    """``(threads per workgroup, fp32 samples per 16-byte load, largest pair-tile extent, chunk alignment in samples)``; 16-bit inputs
    take twice the samples per load."""
    threads, width, tile, align = torch.ops.tmx.signal_tile()
    return int(threads), int(width), int(tile), int(align)
