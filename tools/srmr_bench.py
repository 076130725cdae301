"""speech_reverberation_modulation_energy_ratio on [B, T] fp32 GPU batches: the native route (``tmx::srmr_gammatone``, ``tmx::srmr_energies``,
``tmx::srmr_scores``, ``csrc/srmr.hip``) against the composition (``TMX_SRMR_NATIVE=0``).  The knob is read once per process, so each route
runs in a child process of its own.  Device events around the whole call including Python, median of ``--reps`` after ``--warmup``
warm-ups, peak allocated memory of one call.  A shape whose composition does not fit in memory is recorded as such.

    python tools/srmr_bench.py --out profiles/srmr_bench.json [--kernel-stats CSV]
    python tools/srmr_bench.py --profile-run    # a few native calls at 16 x 64 000, for a ``rocprofv3 --kernel-trace --stats`` run of its own

``--kernel-stats``: the ``kernel_stats`` CSV of such a run; its rows go into the JSON.
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (signals, samples, fs)
CASES = [(1, 16000, 16000), (1, 64000, 16000), (16, 64000, 16000), (64, 32000, 16000), (8, 80000, 8000), (4, 132300, 44100)]
PROFILE_CASE = CASES[2]
PROFILE_CALLS = 5


def _inputs(b, n, fs):
    """Amplitude-modulated tones plus noise: the shape of ``tests/helpers/srmr_oracle.signals``."""
    import math

    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.arange(n, device="cuda", dtype=torch.float64) / fs
    rows = [0.3 * torch.sin(2 * math.pi * (300 - 7 * (i % 20)) * t) * (1 + torch.sin(2 * math.pi * (4 + i % 5) * t)) for i in range(b)]
    return (torch.stack(rows) + 0.05 * torch.randn(b, n, device="cuda", dtype=torch.float64, generator=g)).float()


def _timed(fn):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def _peak_bytes(fn):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def run_route(reps, warmup):
    """One route (this process's ``TMX_SRMR_NATIVE``) at every case: one JSON line per case."""
    import torch

    import torchmetrics_forked_amd.functional.audio.srmr as srmr
    from torchmetrics_forked_amd import ops

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ops.require()
    for b, n, fs in CASES:
        x = _inputs(b, n, fs)
        call = lambda: srmr.speech_reverberation_modulation_energy_ratio(x, fs)  # noqa: E731
        row = {"shape": f"{b}x{n}", "fs": fs, "native": srmr._native_srmr_ok(x, fs)}
        try:
            times = []
            for i in range(warmup + reps):
                ms, out = _timed(call)
                if i >= warmup:
                    times.append(ms)
            row.update(ms=round(statistics.median(times), 4), ms_min_max=[round(min(times), 4), round(max(times), 4)], values=out.tolist())
            del out
            row["peak_bytes"] = _peak_bytes(call)
        except torch.OutOfMemoryError:
            row.update(ms=None, ms_min_max=None, values=None, peak_bytes=None, out_of_memory=True)
        print("ROW " + json.dumps(row), flush=True)
        del x
        torch.cuda.empty_cache()
    print("DEVICE " + torch.cuda.get_device_name(0), flush=True)


def profile_run():
    import torch

    from torchmetrics_forked_amd import ops
    from torchmetrics_forked_amd.functional.audio.srmr import speech_reverberation_modulation_energy_ratio

    ops.require()
    b, n, fs = PROFILE_CASE
    x = _inputs(b, n, fs)
    for _ in range(PROFILE_CALLS):
        speech_reverberation_modulation_energy_ratio(x, fs)
    torch.cuda.synchronize()


def _child(knob, reps, warmup):
    env = dict(os.environ, TMX_SRMR_NATIVE=knob)
    cmd = [sys.executable, os.path.abspath(__file__), "--route", "--reps", str(reps), "--warmup", str(warmup)]
    proc = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"route TMX_SRMR_NATIVE={knob} failed:\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}")
    rows = [json.loads(ln[4:]) for ln in proc.stdout.splitlines() if ln.startswith("ROW ")]
    device = [ln[7:] for ln in proc.stdout.splitlines() if ln.startswith("DEVICE ")][-1]
    return rows, device


def kernel_stats(path):
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    b, n, fs = PROFILE_CASE
    return {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} native calls at {b}x{n} @ {fs} Hz), a run of its own; every kernel of the call",
            "kernels": [{"kernel": r["Name"].split("(")[0][:120], "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
                         "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)} for r in rows]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route", action="store_true", help="(child) time this process's route and print one line per case")
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out")
    args = ap.parse_args()

    if args.profile_run:
        return profile_run()
    if args.route:
        return run_route(args.reps, args.warmup)
    native, device = _child("1", args.reps, args.warmup)
    composition, _ = _child("0", args.reps, args.warmup)
    timings = []
    for nat, comp in zip(native, composition):
        assert nat["native"] and not comp["native"] and (nat["shape"], nat["fs"]) == (comp["shape"], comp["fs"])
        row = {"shape": nat["shape"], "fs": nat["fs"], "native_ms": nat["ms"], "composition_ms": comp["ms"], "native_ms_min_max": nat["ms_min_max"],
               "composition_ms_min_max": comp["ms_min_max"], "native_peak_bytes": nat["peak_bytes"], "composition_peak_bytes": comp["peak_bytes"]}
        if comp["ms"] is None:
            row.update(composition_out_of_memory=True, speedup=None, native_below_composition=True, max_rel_diff=None)
        else:
            row.update(speedup=round(comp["ms"] / nat["ms"], 1), native_below_composition=nat["ms"] < comp["ms"],
                       max_rel_diff=max(abs(a - b) / abs(b) for a, b in zip(nat["values"], comp["values"])))
        timings.append(row)
        print(json.dumps(row), flush=True)
    out = {"what": "speech_reverberation_modulation_energy_ratio(preds, fs) on [B, T] fp32 GPU tensors, the whole call, ms (median); native and "
                   "composition (TMX_SRMR_NATIVE=0) in a process each",
           "reps": args.reps, "warmup": args.warmup, "device": device, "timings": timings,
           "native_below_composition_at_every_shape": all(r["native_below_composition"] for r in timings)}
    if args.kernel_stats:
        out["kernel_stats"] = kernel_stats(args.kernel_stats)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
