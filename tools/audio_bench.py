"""SI-SDR, SNR and speaker-wise PIT with SI-SDR, fp32, no autograd: the native route (``tmx::signal_pair_ratios``, ``csrc/signal_pairs.hip``) against
the composition in the same process.  The functionals' compositions are the private ``_si_sdr_composition`` / ``_snr_composition`` they keep;
PIT's is the same call with the gate's process flag (what ``TMX_AUDIO_NATIVE=0`` sets) switched off around it.  Alternating runs, device events
around the whole call including Python, median of ``--reps`` after ``--warmup`` warm-ups, peak allocated memory of one call.

    python tools/audio_bench.py --out profiles/audio_bench.json [--kernel-trace CSV]
    python tools/audio_bench.py --profile-run    # a few native calls per case, for a ``rocprofv3 --kernel-trace --stats`` run of its own

``--kernel-trace``: the ``kernel_trace`` CSV of such a run; adds each streaming pass's median time per case and its input GB/s against
``--hbm-tb-s`` (the read rate of ``profiles/stream_bw_mi355x_r4.json``).
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROW_SHAPES = ["16x2x64000", "64x1x160000", "4096x1x400", "4x2x8000"]
CASES = [(m, s) for s in ROW_SHAPES for m in ("si_sdr", "snr")] + [("pit_si_sdr", f"16x{s}x64000") for s in (2, 4, 8)]
PASSES = {"si_sdr": 2, "snr": 1, "pit_si_sdr": 2}  # streaming passes (reads of the inputs) per native call
PROFILE_CALLS = 5


def _parse_shape(s):
    return tuple(int(v) for v in s.split("x"))


def _inputs(shape):
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.randn(*shape, device="cuda", generator=g)
    p = t + 0.2 * torch.randn(*shape, device="cuda", generator=g)
    return p, t


def _steps(metric):
    """``(native, composition)`` callables of one case."""
    import torchmetrics_forked_amd.functional.audio.sdr as sdr
    import torchmetrics_forked_amd.functional.audio.snr as snr
    from torchmetrics_forked_amd.functional.audio.pit import permutation_invariant_training as pit

    if metric == "si_sdr":
        return sdr.scale_invariant_signal_distortion_ratio, sdr._si_sdr_composition
    if metric == "snr":
        return snr.signal_noise_ratio, snr._snr_composition

    def native(p, t):
        return pit(p, t, sdr.scale_invariant_signal_distortion_ratio)[0]

    def composition(p, t):
        keep = sdr._AUDIO_NATIVE
        sdr._AUDIO_NATIVE = False
        try:
            return pit(p, t, sdr.scale_invariant_signal_distortion_ratio)[0]
        finally:
            sdr._AUDIO_NATIVE = keep

    return native, composition


def _timed(fn, p, t):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn(p, t)
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def _peak_bytes(fn, p, t):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn(p, t)
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def bench(reps, warmup):
    import torch

    from torchmetrics_forked_amd import ops

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ops.require()
    rows = []
    for metric, shape in CASES:
        p, t = _inputs(_parse_shape(shape))
        native, composition = _steps(metric)
        times = {"native": [], "composition": []}
        outs = {}
        for i in range(warmup + reps):
            for route, fn in (("native", native), ("composition", composition)):  # alternating
                ms, outs[route] = _timed(fn, p, t)
                if i >= warmup:
                    times[route].append(ms)
        n, c = statistics.median(times["native"]), statistics.median(times["composition"])
        input_bytes = 2 * p.numel() * p.element_size()
        row = {"metric": metric, "shape": shape, "input_bytes": input_bytes, "native_ms": round(n, 4), "composition_ms": round(c, 4),
               "native_ms_min_max": [round(min(times["native"]), 4), round(max(times["native"]), 4)],
               "composition_ms_min_max": [round(min(times["composition"]), 4), round(max(times["composition"]), 4)],
               "native_peak_bytes": _peak_bytes(native, p, t), "composition_peak_bytes": _peak_bytes(composition, p, t),
               "speedup": round(c / n, 2), "native_below_composition": n < c,
               "native_input_gb_per_s": round(input_bytes / (n * 1e-3) / 1e9, 2),
               "native_read_gb_per_s": round(PASSES[metric] * input_bytes / (n * 1e-3) / 1e9, 2),
               "max_abs_diff_db": float((outs["native"].double() - outs["composition"].double()).abs().max())}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del p, t, outs
        torch.cuda.empty_cache()
    return rows, torch.cuda.get_device_name(0)


def profile_run():
    import torch

    from torchmetrics_forked_amd import ops

    ops.require()
    for metric, shape in CASES:
        p, t = _inputs(_parse_shape(shape))
        native, _ = _steps(metric)
        for _ in range(PROFILE_CALLS):
            native(p, t)
        torch.cuda.synchronize()


def kernel_times(path, hbm_tb_s):
    """Per case the streaming passes' median times of ``--profile-run``: the dispatches of ``signal_pairs_*`` appear in call order, ``PASSES`` per call."""
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    hits = [r for r in rows if "signal_pairs_" in r["Kernel_Name"]]
    folds = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "signal_fold_kernel" in r["Kernel_Name"]]
    out = {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} native calls per case, fp32), a run of its own; median time of "
                   "every streaming pass, input bytes / time against the HBM read rate (the calls re-read the same inputs, which the 256 MiB "
                   "Infinity Cache holds in full or in part: figures above the read rate are cache-assisted, not HBM rates)",
           "hbm_read_tb_per_s": hbm_tb_s, "fold_kernel_median_us": round(statistics.median(folds), 2) if folds else None, "kernels": []}
    want = sum(PASSES[m] for m, _ in CASES) * PROFILE_CALLS
    if len(hits) != want:
        out["error"] = f"expected {want} dispatches of signal_pairs_*, found {len(hits)}"
        return out
    at = 0
    for metric, shape in CASES:
        n = PASSES[metric]
        calls = [hits[at + i * n:at + (i + 1) * n] for i in range(PROFILE_CALLS)]
        at += n * PROFILE_CALLS
        g, s, t = _parse_shape(shape)
        requested = 2 * 4 * g * s * t
        for k in range(n):
            us = statistics.median((int(c[k]["End_Timestamp"]) - int(c[k]["Start_Timestamp"])) / 1e3 for c in calls)
            tb_s = requested / (us * 1e-6) / 1e12
            out["kernels"].append({"metric": metric, "shape": shape, "pass": k, "kernel": calls[0][k]["Kernel_Name"].split("(")[0], "median_us": round(us, 2),
                                   "input_bytes": requested, "input_tb_per_s": round(tb_s, 3), "fraction_of_hbm_read_rate": round(tb_s / hbm_tb_s, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-trace")
    ap.add_argument("--hbm-tb-s", type=float, default=5.649)
    ap.add_argument("--out")
    args = ap.parse_args()

    if args.profile_run:
        return profile_run()
    out = {"what": "scale_invariant_signal_distortion_ratio(p, t), signal_noise_ratio(p, t) on [G, S, T] and permutation_invariant_training(p, t, SI-SDR) "
                   "on [B, S, T], fp32, no autograd: the whole call, ms (median), native and composition alternating in one process",
           "reps": args.reps, "warmup": args.warmup}
    out["timings"], out["device"] = bench(args.reps, args.warmup)
    out["native_below_composition_at_every_shape"] = all(r["native_below_composition"] for r in out["timings"])
    if args.kernel_trace:
        out["kernel_times"] = kernel_times(args.kernel_trace, args.hbm_tb_s)
        for k in out["kernel_times"]["kernels"]:
            print(json.dumps(k), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
