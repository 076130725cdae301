"""``signal_distortion_ratio`` and speaker-wise PIT with it, fp32, no autograd: the native route (``tmx::sdr_scores``, ``csrc/sdr.hip``) against the
composition (fp64 copies, FFT correlations, ``tmx::toeplitz_solve``) in the same process.  The functional's composition is the private
``_sdr_composition`` it keeps; PIT's is the same call with the gate's process flag (what ``TMX_SDR_NATIVE=0`` sets) switched off around it.
Alternating runs, device events around the whole call including Python, median of ``--reps`` after ``--warmup`` warm-ups, peak allocated
memory of one call.

    python tools/sdr_bench.py --out profiles/sdr_bench.json [--trace-native CSV --trace-composition CSV]
    python tools/sdr_bench.py --profile-run native|composition   # a few calls at 16x2x64000, for a ``rocprofv3 --kernel-trace --stats`` run of its own

``--trace-*``: the ``kernel_trace`` CSVs of such runs; adds every kernel's time per call for both routes, and the correlation pass's
achieved fp64 rate (``2 · 2 L T`` flop per signal pair: the target's autocorrelation and the cross-correlation) against ``--fp64-tflops``.
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("sdr", "16x2x64000", 512), ("sdr", "64x1x160000", 512), ("sdr", "4x2x8000", 512), ("sdr", "4096x1x400", 64), ("sdr", "16x2x64000", 64),
         ("sdr", "16x2x64000", 2048), ("pit_sdr", "16x2x64000", 512), ("pit_sdr", "16x4x64000", 512)]
PROFILE_SHAPE, PROFILE_L, PROFILE_CALLS = "16x2x64000", 512, 5


def _parse_shape(s):
    return tuple(int(v) for v in s.split("x"))


def _inputs(shape):
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.randn(*shape, device="cuda", generator=g)
    p = t + 0.2 * torch.randn(*shape, device="cuda", generator=g)
    return p, t


def _steps(metric, length):
    """``(native, composition)`` callables of one case."""
    import torchmetrics_forked_amd.functional.audio.sdr as sdr
    from torchmetrics_forked_amd.functional.audio.pit import permutation_invariant_training as pit

    if metric == "sdr":
        return (lambda p, t: sdr.signal_distortion_ratio(p, t, filter_length=length)), (lambda p, t: sdr._sdr_composition(p, t, None, length))

    def native(p, t):
        return pit(p, t, sdr.signal_distortion_ratio, filter_length=length)[0]

    def composition(p, t):
        keep = sdr._SDR_NATIVE
        sdr._SDR_NATIVE = False
        try:
            return pit(p, t, sdr.signal_distortion_ratio, filter_length=length)[0]
        finally:
            sdr._SDR_NATIVE = keep

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
    for metric, shape, length in CASES:
        p, t = _inputs(_parse_shape(shape))
        native, composition = _steps(metric, length)
        times = {"native": [], "composition": []}
        outs = {}
        for i in range(warmup + reps):
            for route, fn in (("native", native), ("composition", composition)):  # alternating
                ms, outs[route] = _timed(fn, p, t)
                if i >= warmup:
                    times[route].append(ms)
        n, c = statistics.median(times["native"]), statistics.median(times["composition"])
        row = {"metric": metric, "shape": shape, "filter_length": length, "lags_x_samples": length * _parse_shape(shape)[-1],
               "native_ms": round(n, 4), "composition_ms": round(c, 4),
               "native_ms_min_max": [round(min(times["native"]), 4), round(max(times["native"]), 4)],
               "composition_ms_min_max": [round(min(times["composition"]), 4), round(max(times["composition"]), 4)],
               "native_peak_bytes": _peak_bytes(native, p, t), "composition_peak_bytes": _peak_bytes(composition, p, t),
               "speedup": round(c / n, 2), "native_below_composition": n < c,
               "max_abs_diff_db": float((outs["native"].double() - outs["composition"].double()).abs().max())}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del p, t, outs
        torch.cuda.empty_cache()
    return rows, torch.cuda.get_device_name(0)


FORM_CASES = [("16x2x64000", 512, 0), ("64x1x160000", 512, 0), ("16x4x64000", 512, 1), ("16x2x64000", 64, 0), ("16x2x64000", 2048, 0), ("4096x1x400", 64, 0),
              ("4x2x8000", 512, 0), ("16x2x64000", 128, 0), ("16x2x64000", 192, 0), ("16x2x64000", 320, 0), ("16x2x64000", 384, 0), ("16x2x16384", 512, 0)]


def _knob_ab(knob, values, cases, reps, warmup):
    """Pass C alone (``sdr_correlations``) under the two ``values`` of the per-call ``knob``, alternating in one process."""
    import torch

    from torchmetrics_forked_amd.ops import audio

    rows = []
    for shape, length, pairing in cases:
        p, t = _inputs(_parse_shape(shape))
        times = {v: [] for v in values}
        outs = {}
        for i in range(warmup + reps):
            for v in values:
                os.environ[knob] = v
                ms, outs[v] = _timed(lambda a, b: audio.sdr_correlations(a, b, length, False, pairing), p, t)
                if i >= warmup:
                    times[v].append(ms)
        os.environ.pop(knob, None)
        one, two = (statistics.median(times[v]) for v in values)
        r1, r2 = outs[values[0]], outs[values[1]]
        row = {"shape": shape, "filter_length": length, "pairing": pairing, f"{values[0]}_ms": round(one, 4), f"{values[1]}_ms": round(two, 4),
               f"{values[1]}_over_{values[0]}": round(two / one, 3), "bit_equal": all(torch.equal(a, b) for a, b in zip(r1, r2)),
               "max_rel_diff": max(float(((a - b).abs() / a.abs().clamp_min(1e-300)).max()) for a, b in zip(r1, r2))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def corr_form_ab(reps, warmup):
    """The plain-VALU form against the matrix-core form (``TMX_SDR_CORR_FORM``): other summation orders, so last-bit differences."""
    return _knob_ab("TMX_SDR_CORR_FORM", ("valu", "mfma"), FORM_CASES, reps, warmup)


def profile_run(route):
    import torch

    from torchmetrics_forked_amd import ops

    ops.require()
    p, t = _inputs(_parse_shape(PROFILE_SHAPE))
    fn = _steps("sdr", PROFILE_L)[0 if route == "native" else 1]
    for _ in range(PROFILE_CALLS):
        fn(p, t)
    torch.cuda.synchronize()


def kernel_times(path):
    """Every kernel of a ``--profile-run`` trace after the input generation: dispatches and microseconds per call, largest first."""
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    per = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        if "distribution" in name or "philox" in name.lower():  # the random inputs
            continue
        k = per.setdefault(name, [0, 0.0])
        k[0] += 1
        k[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    out = [{"kernel": name if len(name) <= 160 else name[:157] + "...", "dispatches_per_call": round(n / PROFILE_CALLS, 2),
            "us_per_call": round(us / PROFILE_CALLS, 2)} for name, (n, us) in per.items()]
    return sorted(out, key=lambda k: -k["us_per_call"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-run", choices=["native", "composition"])
    ap.add_argument("--trace-native")
    ap.add_argument("--trace-composition")
    ap.add_argument("--fp64-tflops", type=float, default=78.6, help="the chip's vector fp64 peak")
    ap.add_argument("--out")
    args = ap.parse_args()

    if args.profile_run:
        return profile_run(args.profile_run)
    out = {"what": "signal_distortion_ratio(p, t, filter_length=L) on [G, S, T] and permutation_invariant_training(p, t, SDR, filter_length=L) on "
                   "[B, S, T], fp32, no autograd: the whole call, ms (median), native and composition alternating in one process",
           "reps": args.reps, "warmup": args.warmup}
    out["timings"], out["device"] = bench(args.reps, args.warmup)
    out["corr_form_ab"] = {"what": "sdr_correlations alone, ms (median), TMX_SDR_CORR_FORM=valu (sdr_corr_kernel, 64-lag tiles) and mfma "
                                   "(sdr_corr_mfma_kernel, 256-lag tiles) alternating in one process", "cases": corr_form_ab(args.reps, args.warmup)}
    wins = [r["native_below_composition"] for r in out["timings"]]
    out["native_below_composition_at_every_shape"] = all(wins)
    out["crossover"] = ("none measured: the native route is below the composition at every shape, the largest at filter_length x samples = "
                        f"{max(r['lags_x_samples'] for r in out['timings'])}; the gate has no size condition") if all(wins) else \
        {"native_loses_at": [[r["metric"], r["shape"], r["filter_length"]] for r in out["timings"] if not r["native_below_composition"]]}
    if args.trace_native and args.trace_composition:
        g, s, t = _parse_shape(PROFILE_SHAPE)
        kt = {"what": f"rocprofv3 --kernel-trace --stats of --profile-run native / composition ({PROFILE_CALLS} calls of signal_distortion_ratio at "
                      f"{PROFILE_SHAPE}, filter_length {PROFILE_L}, fp32), each a run of its own: every kernel's dispatches and time per call",
              "native": kernel_times(args.trace_native), "composition": kernel_times(args.trace_composition)}
        for route in ("native", "composition"):
            kt[f"{route}_us_per_call"] = round(sum(k["us_per_call"] for k in kt[route]), 2)
        corr = [k for k in kt["native"] if "sdr_corr_" in k["kernel"]]  # whichever form the library picks at this shape
        if corr:
            flop = 2.0 * 2 * PROFILE_L * t * g * s
            tf = flop / (corr[0]["us_per_call"] * 1e-6) / 1e12
            kt["correlation_pass"] = {"kernel": corr[0]["kernel"], "flop": flop, "us": corr[0]["us_per_call"], "fp64_tflops": round(tf, 2), "vector_fp64_peak_tflops": args.fp64_tflops,
                                      "fraction_of_peak": round(tf / args.fp64_tflops, 3)}
        out["kernel_times"] = kt
        print(json.dumps({k: v for k, v in kt.items() if k not in ("native", "composition")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
