"""Native STOI / ESTOI (``tmx::stoi_scores``, ``tmx::stoi_bands``, ``csrc/stoi.hip``) against the NumPy + SciPy fp64 oracle of
``tests/helpers/stoi_oracle.py``, and the route of ``short_time_objective_intelligibility`` and its module.

Value rule: scores within 1e-9 absolute of the oracle (what ``test_stoi_vs_numpy`` holds the fp64 composition to), the band envelopes within
``1e-9 max|oracle|`` per signal, frame counts equal.  The kept mask is a hard decision, so every value case first asserts on the oracle that
no frame energy is within 0.01 dB of the silence threshold.  Every case is a batch of 7 signals unless it says otherwise; all inputs are
fp32-representable, so fp32 and fp64 inputs share one oracle.  Each comparison prints a ``stoi_err`` line (``-s``).

``test_routes``, ``test_one_op_call_per_functional_call_and_per_update``, ``test_peak_memory``, ``test_knob_keeps_the_composition`` and every test
that calls the ops fail on the composition alone (there is no ``tmx::stoi_scores`` there, its launches grow with the batch, and its
resampling gather allocates tens of MiB).

Measured on MI355X over the 80 comparisons: scores at most 1.2e-15 from the oracle, envelopes at most 1.0e-15 of the largest envelope
value, smallest mask margin 4.5 dB, peak allocated growth of 7 x 16 000 at 16 kHz 1.2 MiB.

Mutants of ``csrc/stoi.hip``, the op built alone as a library outside the tree and run under this file one at a time (the unchanged source
built the same way passes in full), none of which reads or writes past a buffer, and the first test that fails:
* a band edge off by one: 70 tests, ``test_values[10000-False-dtype0]`` first;
* ``J = K`` for the strict STFT frame count (one more envelope column allocated): 73, the same first;
* threshold comparison with ``<=``: none; equivalent unless a frame energy is exactly 40 dB below the maximum, which the margin condition excludes;
* kept-slot index off by one in the overlap-add: 70, ``test_values[10000-False-dtype0]`` first;
* second Hann window dropped: 70, the same first; the score-only cases fail too (the window changes the leakage, not only a gain);
* clip taken against ``y``: 21, the same first;  the clip constant with 14 dB: 24, the same first;
* EPS dropped from the norms: ``test_silent_signals_and_identity`` alone (0 / 0 for a silent target);
* ESTOI columns normalised before rows: 23, ``test_values[10000-True-dtype0]`` first;
* resampler phase off by one: 24, ``test_values[16000-False-dtype0]`` first;
* the segment-count divisor taken as ``J``: 61, ``test_values[10000-False-dtype0]`` first.
"""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from tests.helpers import stoi_oracle as so
from tests.helpers.routes import assert_route, count_calls, kernels_run
from torchmetrics_forked_amd import ops

pytestmark = pytest.mark.gpu

TILE_FRAMES, SEG_BLOCK, RESAMPLE_STRIP, KEEP_STRIP, ENERGY_FRAMES = 16, 32, 256, 256, 4  # asserted against stoi_tile() below
WARNING = "Not enough STFT frames"
_NATIVE_MARKS = ("stoi_energy_kernel", "stoi_keep_kernel", "stoi_bands_kernel", "stoi_segments_kernel", "stoi_final_kernel")
_FORBIDDEN = ("index", "fft", "gather")  # lower-cased substrings of the composition's index_add_, rfft and resampling-gather kernels
_ORACLES = {}


@pytest.fixture(scope="module", autouse=True)
def _need_native(device):
    ops.require()


def _op():
    from torchmetrics_forked_amd.ops import audio

    return audio


def _functional():
    from torchmetrics_forked_amd.functional.audio.stoi import short_time_objective_intelligibility

    return short_time_objective_intelligibility


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _speech_batch(fs, n, seed0, b=7):
    pairs = [so.speechlike(seed0 + i, n, fs) for i in range(b)]
    return _f32(np.stack([c for c, _ in pairs])), _f32(np.stack([y for _, y in pairs]))


def _noise_batch(n, seed, b=7):
    rng = np.random.default_rng(seed)
    clean = rng.standard_normal((b, n))
    return _f32(clean), _f32(clean + 0.5 * rng.standard_normal((b, n)))


def _planted_batch(mask, seed0, b=7, tail=0):
    hops = so.hops_for_frames(mask)
    pairs = [so.planted(seed0 + i, hops, tail) for i in range(b)]
    return _f32(np.stack([c for c, _ in pairs])), _f32(np.stack([y for _, y in pairs]))


def _oracle(key, clean, noisy, fs, extended):
    """One oracle run per signal, computed once per ``key`` and shared."""
    full = (key, fs, extended)
    if full not in _ORACLES:
        _ORACLES[full] = [so.stoi(c.astype(np.float64), y.astype(np.float64), fs, extended) for c, y in zip(clean, noisy)]
    return _ORACLES[full]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _check(key, clean, noisy, fs, extended=False, dtype=torch.float32, bands=True):
    """Scores, frame counts and (optionally) band envelopes of one batch against the oracle; returns ``(scores, frames, oracle results)``."""
    res = _oracle(key, clean, noisy, fs, extended)
    for r in res:
        so.assert_margin(r)
    pd, td = torch.from_numpy(noisy).to(dtype).cuda(), torch.from_numpy(clean).to(dtype).cuda()
    scores, frames = _op().stoi_scores(pd, td, fs, extended)
    assert scores.dtype == torch.float64 and frames.dtype == torch.int32 and scores.shape == frames.shape == (clean.shape[0],)
    assert frames.tolist() == [r.frames for r in res], (key, frames.tolist(), [r.frames for r in res])
    want = torch.tensor([r.score for r in res], dtype=torch.float64)
    err = float((scores.cpu() - want).abs().max())
    rel = 0.0
    if bands:
        xt, yt, fr = _op().stoi_bands(pd, td, fs)
        assert torch.equal(fr, frames) and xt.shape == yt.shape and xt.shape[:2] == (clean.shape[0], 15)
        for i, r in enumerate(res):
            for got, ref in ((xt[i], r.x_tob), (yt[i], r.y_tob)):
                assert bool((got[:, r.frames :] == 0).all())
                if r.frames:
                    scale = float(np.abs(ref).max())
                    this = float((got[:, : r.frames].cpu() - torch.from_numpy(ref)).abs().max()) / scale
                    rel = max(rel, this)
    print(f"stoi_err {key} fs={fs} ext={int(extended)} {str(dtype)[6:]}: score {err:.3e} bands {rel:.3e} frames {sorted(set(frames.tolist()))}")
    assert err <= 1e-9, (key, err)
    assert rel <= 1e-9, (key, rel)
    return scores, frames, res


def test_tile_is_what_the_shapes_assume():
    assert _op().stoi_tile() == (TILE_FRAMES, SEG_BLOCK, RESAMPLE_STRIP, KEEP_STRIP, ENERGY_FRAMES)


# ----------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("fs", [10000, 16000, 8000, 22050, 48000])
def test_values(fs, extended, dtype):
    clean, noisy = _speech_batch(fs, int(0.9 * fs), 100 + fs % 97)
    _, frames, res = _check(f"speech{fs}", clean, noisy, fs, extended, dtype, bands=not extended)
    assert min(frames.tolist()) >= 30 and not all(r.kept.all() for r in res)  # a score, and silent frames were removed


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fs", [10000, 16000])
def test_16_bit_inputs_are_their_upcast(dtype, fs):
    clean, noisy = _speech_batch(fs, int(0.9 * fs), 7)
    pd, td = torch.from_numpy(noisy).to(dtype).cuda(), torch.from_numpy(clean).to(dtype).cuda()
    for extended in (False, True):
        a, b = _op().stoi_scores(pd, td, fs, extended), _op().stoi_scores(pd.float(), td.float(), fs, extended)
        assert _same_bits(a[0], b[0]) and torch.equal(a[1], b[1]) and min(a[1].tolist()) >= 30
    for a, b in zip(_op().stoi_bands(pd, td, fs), _op().stoi_bands(pd.float(), td.float(), fs)):
        assert _same_bits(a, b)


def test_every_signal_has_its_own_kept_count():
    masks = [[True] * (42 - 2 * i) + [False] * (2 * i) for i in range(7)]  # 42, 40, ..., 30 kept of 42: the last one is too short
    pairs = [so.planted(30 + i, so.hops_for_frames(m)) for i, m in enumerate(masks)]
    clean, noisy = _f32(np.stack([c for c, _ in pairs])), _f32(np.stack([y for _, y in pairs]))
    for extended in (False, True):
        scores, frames, _ = _check("own_counts", clean, noisy, 10000, extended, bands=not extended)
        assert frames.tolist() == [41 - 2 * i for i in range(7)]
        assert float(scores[6]) == 1e-5 and all(float(s) != 1e-5 for s in scores[:6])


# -------------------------------------------------------------------------------------------------- edges of the algorithm
@pytest.mark.parametrize("t_len", [255, 256, 257, 4095, 4096, 4097, 4224])
def test_length_edges_at_10k(t_len):
    clean, noisy = _noise_batch(t_len, t_len)
    f = _functional()
    pd, td = torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda()
    if t_len < 4096:
        with pytest.warns(RuntimeWarning, match=WARNING):
            out = f(pd, td, 10000)
        assert out.tolist() == [1e-5] * 7
        _check(f"len{t_len}", clean, noisy, 10000)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out = f(pd, td, 10000)
        scores, frames, _ = _check(f"len{t_len}", clean, noisy, 10000)
        assert torch.equal(out, scores.cpu()) and frames.tolist() == [30 + (t_len - 4096) // 128] * 7


def test_length_edge_at_16k():
    """The 16 kHz lengths on each side of the 31-kept-frame boundary, found with the oracle: 4096 resampled samples."""
    rng = np.random.default_rng(16)
    clean = _f32(rng.standard_normal((7, 6600)))
    noisy = _f32(clean + 0.5 * rng.standard_normal((7, 6600)))
    first = next(t for t in range(6540, 6600) if so.stoi(clean[0, :t].astype(np.float64), noisy[0, :t].astype(np.float64), 16000).frames >= 30)
    assert -(-first * 5 // 8) == 4096 and -(-(first - 1) * 5 // 8) == 4095
    for t_len, want in ((first - 1, 29), (first, 30), (first + 1, 30)):
        scores, frames, _ = _check(f"len16k_{t_len}", np.ascontiguousarray(clean[:, :t_len]), np.ascontiguousarray(noisy[:, :t_len]), 16000)
        assert frames.tolist() == [want] * 7 and (scores.tolist() == [1e-5] * 7) == (want < 30)


_MASKS = {
    "all_kept": [True] * 40,
    "first_dropped": [False] + [True] * 39,
    "last_dropped": [True] * 39 + [False],
    "one_mid_dropped": [True] * 17 + [False] + [True] * 22,
    "alternating_runs": ([True] * 3 + [False] * 2) * 9,
    "31_kept_of_many": [True] * 10 + [False] * 25 + [True] * 21 + [False] * 9,
    "30_kept_too_short": [True] * 10 + [False] * 25 + [True] * 20 + [False] * 10,
}


@pytest.mark.parametrize("name", list(_MASKS))
def test_planted_masks(name):
    mask = _MASKS[name]
    clean, noisy = _planted_batch(mask, 200 + len(name), tail=37)
    for extended in (False, True):
        scores, frames, res = _check(f"mask_{name}", clean, noisy, 10000, extended, bands=not extended)
        assert all(r.kept.tolist() == mask for r in res) and frames.tolist() == [sum(mask) - 1] * 7
        assert (scores.tolist() == [1e-5] * 7) == (sum(mask) < 31)


def test_one_short_signal_among_long_ones():
    long_c, long_y = _planted_batch(_MASKS["all_kept"][:40] + [True] * 25, 300, b=6)
    short_c, short_y = _planted_batch(_MASKS["30_kept_too_short"], 310, b=1)
    assert long_c.shape[1] == short_c.shape[1]
    clean, noisy = np.concatenate([long_c[:3], short_c, long_c[3:]]), np.concatenate([long_y[:3], short_y, long_y[3:]])
    scores, frames, _ = _check("one_short", clean, noisy, 10000)
    assert [float(s) == 1e-5 for s in scores] == [False] * 3 + [True] + [False] * 3
    with pytest.warns(RuntimeWarning, match=WARNING) as rec:
        out = _functional()(torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda(), 10000)
    assert len([w for w in rec if WARNING in str(w.message)]) == 1 and torch.equal(out, scores.cpu())


# ---------------------------------------------------------------------------------------------------- edges of the tiles
@pytest.mark.parametrize("j", [2, 3, 4, TILE_FRAMES - 1, TILE_FRAMES, TILE_FRAMES + 1, 2 * TILE_FRAMES - 1, 2 * TILE_FRAMES, 2 * TILE_FRAMES + 1,
                               3 * TILE_FRAMES - 1, 3 * TILE_FRAMES, 3 * TILE_FRAMES + 1])
def test_frame_tile_edges(j):
    """``J`` STFT frames, all source frames kept: one below, at and one above the band kernel's tile (and the energy kernel's 4 frames)."""
    clean, noisy = _noise_batch(128 * j + 256, 400 + j)
    _, frames, _ = _check(f"tile_j{j}", clean, noisy, 10000)
    assert frames.tolist() == [j] * 7


@pytest.mark.parametrize("nseg", [SEG_BLOCK - 1, SEG_BLOCK, SEG_BLOCK + 1, 2 * SEG_BLOCK - 1, 2 * SEG_BLOCK, 2 * SEG_BLOCK + 1])
@pytest.mark.parametrize("extended", [False, True])
def test_segment_block_edges(nseg, extended):
    j = nseg + 29
    clean, noisy = _noise_batch(128 * j + 256 + 5, 500 + nseg)
    _, frames, _ = _check(f"seg{nseg}", clean, noisy, 10000, extended, bands=False)
    assert frames.tolist() == [j] * 7


@pytest.mark.parametrize("length", [17 * RESAMPLE_STRIP - 1, 17 * RESAMPLE_STRIP, 17 * RESAMPLE_STRIP + 1])
@pytest.mark.parametrize("fs", [16000, 22050])
def test_resampler_strip_edges(fs, length):
    """Resampled lengths one below, at and one above a multiple of the resampler's outputs per workgroup."""
    up, down = (5, 8) if fs == 16000 else (200, 441)
    t_len = next(t for t in range(length * down // up - 2, length * down // up + 4) if -(-t * up // down) == length)
    clean, noisy = _noise_batch(t_len, 600 + length)
    _, frames, _ = _check(f"strip{fs}_{length}", clean, noisy, fs)
    assert frames.tolist() == [(length - 256) // 128] * 7


@pytest.mark.parametrize("f", [KEEP_STRIP - 1, KEEP_STRIP, KEEP_STRIP + 1])
def test_keep_strip_edges(f):
    """``f`` source frames with dropped runs inside the first strip of the kept-frame scan and across its end."""
    mask = [True] * f
    for lo, hi in ((60, 64), (KEEP_STRIP - 3, KEEP_STRIP - 1)):
        mask[lo:hi] = [False] * (hi - lo)
    mask[-1] = True
    mask[-2] = True
    clean, noisy = _planted_batch(mask, 700 + f, b=3)  # three signals: the oracle walks 230 segments of each
    _, frames, res = _check(f"keep{f}", clean, noisy, 10000)
    assert all(r.kept.tolist() == mask for r in res) and frames.tolist() == [sum(mask) - 1] * 3


def test_more_signals_than_a_grid_axis():
    """66 000 signals: every kernel's grid is flat on x, so no axis limits the batch.  Two frames each: too short, but the envelopes are there."""
    clean, noisy = _noise_batch(384, 800, b=2)
    idx = torch.arange(66000) % 2
    pd, td = torch.from_numpy(noisy).cuda()[idx].contiguous(), torch.from_numpy(clean).cuda()[idx].contiguous()
    scores, frames = _op().stoi_scores(pd, td, 10000, False)
    assert bool((scores == 1e-5).all()) and bool((frames == 1).all())
    xt, yt, _ = _op().stoi_bands(pd, td, 10000)
    res = _oracle("many", clean, noisy, 10000, False)
    for i in (0, 1, 65534, 65535, 65536, 65999):
        ref = res[i % 2]
        assert float((xt[i, :, :1].cpu() - torch.from_numpy(ref.x_tob)).abs().max()) <= 1e-9 * float(np.abs(ref.x_tob).max())
        assert float((yt[i, :, :1].cpu() - torch.from_numpy(ref.y_tob)).abs().max()) <= 1e-9 * float(np.abs(ref.y_tob).max())
    assert _same_bits(xt[0], xt[65998]) and _same_bits(yt[1], yt[65999])


# ------------------------------------------------------------------------------------------------------ special values
def _special_base(n=4608):
    return _noise_batch(n, 900)


@pytest.mark.parametrize("fs", [10000, 16000])
def test_nan_or_inf_in_target_scores_1e_5_for_that_signal_only(fs):
    clean, noisy = _special_base(4608 if fs == 10000 else 7373)
    pd, td = torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda()
    _, base_frames = _op().stoi_scores(pd, td, fs, False)
    bad = td.clone()
    bad[2, 1000] = float("nan")
    bad[4, 3000] = float("inf")
    bad[5, 17] = float("-inf")
    for extended in (False, True):
        ref, _ = _op().stoi_scores(pd, td, fs, extended)
        scores, frames = _op().stoi_scores(pd, bad, fs, extended)
        assert frames[[2, 4, 5]].tolist() == [0, 0, 0] and scores[[2, 4, 5]].tolist() == [1e-5] * 3
        keep = [0, 1, 3, 6]
        assert _same_bits(scores[keep], ref[keep]) and torch.equal(frames[keep], base_frames[keep]) and min(base_frames.tolist()) >= 30


def test_nan_or_inf_in_preds_is_nan_for_that_signal_only():
    clean, noisy = _special_base()
    pd, td = torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda()
    bad = pd.clone()
    bad[1, 2000] = float("nan")
    bad[3, 77] = float("inf")
    for extended in (False, True):
        ref, ref_frames = _op().stoi_scores(pd, td, 10000, extended)
        scores, frames = _op().stoi_scores(bad, td, 10000, extended)
        assert torch.equal(frames, ref_frames) and bool(torch.isnan(scores[[1, 3]]).all())
        keep = [0, 2, 4, 5, 6]
        assert _same_bits(scores[keep], ref[keep])


def test_silent_signals_and_identity():
    clean, noisy = _special_base()
    pd, td = torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda()
    td[0] = 0.0  # silent target
    pd[1] = 0.0  # silent preds
    pd[2] = 0.0  # both
    td[2] = 0.0
    pd[3] = td[3]  # identity
    stoi, frames = _op().stoi_scores(pd, td, 10000, False)
    estoi, _ = _op().stoi_scores(pd, td, 10000, True)
    assert frames.tolist() == [34] * 7
    assert stoi[:3].tolist() == [0.0, 0.0, 0.0] and bool(torch.isnan(estoi[:3]).all())
    assert abs(float(stoi[3]) - 1.0) <= 1e-12 and abs(float(estoi[3]) - 1.0) <= 1e-12
    assert 0.0 < float(stoi[4]) < 1.0 and 0.0 < float(estoi[4]) < 1.0


# ------------------------------------------------------------------------------------------------ determinism and layout
def test_bit_equal_runs_batches_and_offsets():
    clean, noisy = _speech_batch(16000, 14400, 40)
    pd, td = torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda()
    for fs in (16000, 10000):
        for extended in (False, True):
            first = _op().stoi_scores(pd, td, fs, extended)
            again = _op().stoi_scores(pd, td, fs, extended)
            assert _same_bits(first[0], again[0]) and torch.equal(first[1], again[1])
            for i in (0, 3, 6):  # alone: the same bits as inside the batch
                alone = _op().stoi_scores(pd[i : i + 1], td[i : i + 1], fs, extended)
                assert _same_bits(alone[0], first[0][i : i + 1]) and torch.equal(alone[1], first[1][i : i + 1])
            buf_p, buf_t = torch.empty(pd.numel() + 1, device="cuda"), torch.empty(td.numel() + 1, device="cuda")
            buf_p[1:].copy_(pd.flatten())
            buf_t[1:].copy_(td.flatten())
            off_p, off_t = buf_p[1:].view(pd.shape), buf_t[1:].view(td.shape)
            assert off_p.is_contiguous() and off_p.data_ptr() % 8 != 0
            moved = _op().stoi_scores(off_p, off_t, fs, extended)
            assert _same_bits(moved[0], first[0]) and torch.equal(moved[1], first[1])
        for a, b in zip(_op().stoi_bands(pd, td, fs), _op().stoi_bands(pd, td, fs)):
            assert _same_bits(a, b)


def test_leading_dims_dtype_and_device():
    clean, noisy = _speech_batch(16000, 14400, 50, b=4)
    p, t = torch.from_numpy(noisy).reshape(2, 2, -1), torch.from_numpy(clean).reshape(2, 2, -1)
    f = _functional()
    out = f(p.cuda(), t.cuda(), 16000)
    assert out.shape == (2, 2) and out.dtype == torch.float64 and out.device.type == "cpu"
    same = f(p.cuda(), t.cuda(), 16000, keep_same_device=True)
    assert same.shape == (2, 2) and same.dtype == torch.float64 and same.is_cuda and torch.equal(same.cpu(), out)
    cpu = f(p, t, 16000)
    assert cpu.shape == (2, 2) and float((cpu - out).abs().max()) <= 1e-9
    one = f(p[0, 0].cuda(), t[0, 0].cuda(), 16000)
    assert one.shape == () and _same_bits(one, out[0, 0])


# ----------------------------------------------------------------------------------------------------------------- routes
def _route_inputs(b, n=16000):
    clean, noisy = _speech_batch(16000, n, 60, b=b)
    return torch.from_numpy(noisy).cuda(), torch.from_numpy(clean).cuda()


def test_routes(monkeypatch):
    f = _functional()
    pd, td = _route_inputs(7)
    for fs, extended in ((16000, False), (16000, True), (10000, False)):
        names = kernels_run(lambda: f(pd, td, fs, extended))
        assert_route(names, present=_NATIVE_MARKS + (("stoi_resample_kernel",) if fs != 10000 else ()))
        assert not [n for n in names if any(m in n.lower() for m in _FORBIDDEN)], sorted(set(names))
        assert ("stoi_resample_kernel" in " ".join(names)) == (fs != 10000)
        assert len(names) == len(kernels_run(lambda: f(pd[:1], td[:1], fs, extended)))  # as many launches for one signal as for seven
    # a dtype pair outside the gate reaches the composition, and the forbidden marks are live there
    names = kernels_run(lambda: f(pd[:1, :8000], td[:1, :8000].double(), 16000))
    assert_route(names, absent=("stoi_",))
    for mark in _FORBIDDEN:
        assert any(mark in n.lower() for n in names), (mark, sorted(set(names)))


def test_one_op_call_per_functional_call_and_per_update(monkeypatch):
    from torchmetrics_forked_amd.audio import ShortTimeObjectiveIntelligibility

    calls = count_calls(monkeypatch, torch.ops.tmx, "stoi_scores")
    pd, td = _route_inputs(7)
    _functional()(pd, td, 16000)
    assert len(calls) == 1 and calls[0][0][0].shape == (7, 16000)
    m = ShortTimeObjectiveIntelligibility(16000).cuda()
    m.update(pd, td)
    assert len(calls) == 2
    _functional()(pd.reshape(7, 1, -1), td.reshape(7, 1, -1), 16000, True)
    assert len(calls) == 3 and calls[2][0][-1] is True


def test_peak_memory():
    """7 x 16 000 at 16 kHz: the resampled signals (2 x 7 x 10 000 fp64, 1.1 MiB), energies, the kept list and the envelopes.  The composition's
    resampling gather alone is tens of MiB."""
    f = _functional()
    pd, td = _route_inputs(7)
    f(pd, td, 16000)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = f(pd, td, 16000)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print(f"stoi peak growth {grew} bytes")
    assert grew < 8 * 2**20 and out.shape == (7,)


def test_knob_keeps_the_composition():
    """``TMX_STOI_NATIVE=0`` is read once per process: a child process with it set runs no STOI kernel and gives this process's value."""
    code = (
        "import torch\n"
        "from tests.helpers.routes import kernels_run\n"
        "from torchmetrics_forked_amd.functional.audio.stoi import short_time_objective_intelligibility as f\n"
        "g = torch.Generator().manual_seed(0)\n"
        "t = torch.randn(1, 6000, generator=g).cuda()\n"
        "p = t + 0.5 * torch.randn(1, 6000, generator=g).cuda()\n"
        "names = kernels_run(lambda: f(p, t, 10000))\n"
        "print('STOI_KERNELS', sum('stoi_' in n for n in names), 'VALUE', repr(float(f(p, t, 10000))))\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TMX_STOI_NATIVE="0", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("STOI_KERNELS")][-1].split()
    assert int(line[1]) == 0
    g = torch.Generator().manual_seed(0)
    t = torch.randn(1, 6000, generator=g).cuda()
    p = t + 0.5 * torch.randn(1, 6000, generator=g).cuda()
    names = kernels_run(lambda: _functional()(p, t, 10000))
    assert sum("stoi_" in n for n in names) >= 5
    assert abs(float(line[3]) - float(_functional()(p, t, 10000))) <= 1e-9


# ----------------------------------------------------------------------------------------------------------------- module
def test_module_over_two_updates():
    from torchmetrics_forked_amd.audio import ShortTimeObjectiveIntelligibility

    pd, td = _route_inputs(7, 14400)
    for extended in (False, True):
        vals = _functional()(pd, td, 16000, extended)
        m = ShortTimeObjectiveIntelligibility(16000, extended).cuda().set_dtype(torch.float64)  # (an fp32 sum state cannot hold 1e-9)
        m.update(pd[:3], td[:3])
        m.update(pd[3:], td[3:])
        assert abs(float(m.compute().double()) - float(vals.mean())) <= 1e-9
