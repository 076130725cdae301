"""short_time_objective_intelligibility on [B, T] fp32 GPU batches: the native route (``tmx::stoi_scores``, ``csrc/stoi.hip``) against the
composition (``TMX_STOI_NATIVE=0``).  The knob is read once per process, so each route runs in a child process of its own.  Device events
around the whole call including Python and the transfer of the scores, median of ``--reps`` after ``--warmup`` warm-ups, peak allocated
memory of one call.

    python tools/stoi_bench.py --out profiles/stoi_bench.json [--kernel-stats CSV]
    python tools/stoi_bench.py --profile-run    # a few native calls at the first shape, for a ``rocprofv3 --kernel-trace --stats`` run of its own

``--kernel-stats``: the ``kernel_stats`` CSV of such a run; its STOI rows go into the JSON.
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

# (signals, samples, fs, extended)
CASES = [(16, 64000, 16000, False), (16, 64000, 16000, True), (64, 32000, 16000, False), (8, 100000, 10000, False), (4, 132300, 44100, False),
         (1, 16000, 16000, False)]
PROFILE_CALLS = 5


def _inputs(b, n, fs):
    """Bursts of two tones plus noise with silent gaps, and a noisy copy: the shape of ``tests/helpers/stoi_oracle.speechlike``."""
    import math

    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.arange(n, device="cuda", dtype=torch.float64) / fs
    env = (torch.sin(2 * math.pi * 3 * t) > -0.3).double()
    tones = torch.sin(2 * math.pi * 220 * t) + 0.5 * torch.sin(2 * math.pi * 1230 * t)
    clean = (env * (tones + 0.2 * torch.randn(b, n, device="cuda", dtype=torch.float64, generator=g))).float()
    noisy = clean + 0.3 * torch.randn(b, n, device="cuda", generator=g)
    return noisy, clean


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
    """One route (this process's ``TMX_STOI_NATIVE``) at every case: one JSON line per case."""
    import warnings

    import torch

    import torchmetrics_forked_amd.functional.audio.stoi as stoi
    from torchmetrics_forked_amd import ops

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ops.require()
    warnings.simplefilter("ignore")
    for b, n, fs, extended in CASES:
        p, t = _inputs(b, n, fs)
        call = lambda: stoi.short_time_objective_intelligibility(p, t, fs, extended)  # noqa: E731
        times = []
        for i in range(warmup + reps):
            ms, out = _timed(call)
            if i >= warmup:
                times.append(ms)
        row = {"shape": f"{b}x{n}", "fs": fs, "extended": extended, "native": stoi._native_stoi_ok(p, t, fs), "ms": round(statistics.median(times), 4),
               "ms_min_max": [round(min(times), 4), round(max(times), 4)], "peak_bytes": _peak_bytes(call), "values": out.tolist()}
        print("ROW " + json.dumps(row), flush=True)
        del p, t
        torch.cuda.empty_cache()
    print("DEVICE " + torch.cuda.get_device_name(0), flush=True)


def profile_run():
    import torch

    from torchmetrics_forked_amd import ops
    from torchmetrics_forked_amd.functional.audio.stoi import short_time_objective_intelligibility

    ops.require()
    b, n, fs, extended = CASES[0]
    p, t = _inputs(b, n, fs)
    for _ in range(PROFILE_CALLS):
        short_time_objective_intelligibility(p, t, fs, extended)
    torch.cuda.synchronize()


def _child(knob, reps, warmup):
    env = dict(os.environ, TMX_STOI_NATIVE=knob)
    cmd = [sys.executable, os.path.abspath(__file__), "--route", "--reps", str(reps), "--warmup", str(warmup)]
    proc = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"route TMX_STOI_NATIVE={knob} failed:\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}")
    rows = [json.loads(ln[4:]) for ln in proc.stdout.splitlines() if ln.startswith("ROW ")]
    device = [ln[7:] for ln in proc.stdout.splitlines() if ln.startswith("DEVICE ")][-1]
    return rows, device


def kernel_stats(path):
    with open(path, newline="") as fh:
        rows = [r for r in csv.DictReader(fh) if "stoi_" in r["Name"]]
    return {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} native calls at {CASES[0][0]}x{CASES[0][1]} @ {CASES[0][2]} Hz), "
                    "a run of its own",
            "kernels": [{"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
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
        assert nat["native"] and not comp["native"] and (nat["shape"], nat["fs"], nat["extended"]) == (comp["shape"], comp["fs"], comp["extended"])
        diff = max(abs(a - b) for a, b in zip(nat["values"], comp["values"]))
        row = {"shape": nat["shape"], "fs": nat["fs"], "extended": nat["extended"], "native_ms": nat["ms"], "composition_ms": comp["ms"],
               "native_ms_min_max": nat["ms_min_max"], "composition_ms_min_max": comp["ms_min_max"], "native_peak_bytes": nat["peak_bytes"],
               "composition_peak_bytes": comp["peak_bytes"], "speedup": round(comp["ms"] / nat["ms"], 1), "native_below_composition": nat["ms"] < comp["ms"],
               "max_abs_diff": diff}
        timings.append(row)
        print(json.dumps(row), flush=True)
    out = {"what": "short_time_objective_intelligibility(preds, target, fs, extended) on [B, T] fp32 GPU tensors, the whole call including the transfer "
                   "of the scores, ms (median); native and composition (TMX_STOI_NATIVE=0) in a process each",
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
