"""SSIM forward + backward (``ssim(p, t, data_range=1.0).backward()``, fp32, gaussian 11x11): the native backward
(``tmx::ssim_sums_backward``) against the composition (``TMX_SSIM_NATIVE_GRAD=0``: reflect pad, 5·B stacked batch, grouped
conv, crop, autograd) in one process, alternating; device events, median of ``--reps`` repeats after a warm-up.

    python tools/ssim_grad_bench.py --out profiles/ssim_backward_r7.json          # timings + scratch-cap sweep
        [--test-log LOG]        # collect the ``ssim_grad_ratio`` lines of ``pytest -s tests/test_ssim_grad_gpu.py``
        [--kernel-stats CSV]    # collect the tmx kernels of a ``rocprofv3 --kernel-trace --stats`` run of ``--profile-run``
    python tools/ssim_grad_bench.py --profile-run                                 # a few native iterations, to be traced
    python tools/ssim_grad_bench.py --native-only --shapes 32x3x1024x1024          # one JSON line (a sweep child)
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ["16x3x256x256", "8x3x512x512", "4x3x1024x1024", "32x3x1024x1024"]
SWEEP_SHAPES = ["4x3x1024x1024", "32x3x1024x1024"]
SWEEP_MB = [64, 128, 512]


def _inputs(shape):
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.rand(*shape, device="cuda", generator=g)
    p = (t + 0.1 * torch.randn(*shape, device="cuda", generator=g)).clamp_(0, 1)
    return p.requires_grad_(), t


def _step(p, t, native):
    from torchmetrics_forked_amd.functional.image import structural_similarity_index_measure as ssim

    os.environ["TMX_SSIM_NATIVE_GRAD"] = "1" if native else "0"  # read on every differentiable call
    p.grad = None
    ssim(p, t, data_range=1.0).backward()
    return p.grad


def measure(shape, reps, warmup, routes):
    import torch

    p, t = _inputs(shape)
    times = {r: [] for r in routes}
    grads = {}
    for i in range(warmup + reps):
        for route in routes:  # alternate the routes inside every repeat
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            grads[route] = _step(p, t, route == "native")
            end.record()
            end.synchronize()
            if i >= warmup:
                times[route].append(start.elapsed_time(end))
    row = {"shape": list(shape), "reps": reps}
    for route in routes:
        row[f"{route}_ms"] = round(statistics.median(times[route]), 4)
        row[f"{route}_ms_min_max"] = [round(min(times[route]), 4), round(max(times[route]), 4)]
    if len(routes) == 2:
        row["speedup"] = round(row["composition_ms"] / row["native_ms"], 2)
        diff = float((grads["native"] - grads["composition"]).abs().max())
        row["max_abs_grad_diff_over_max_abs_grad"] = diff / float(grads["composition"].abs().max())
    return row


def _parse_shape(s):
    return tuple(int(v) for v in s.split("x"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=SHAPES)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--test-log")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from torchmetrics_forked_amd import ops

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ops.require()
    if args.profile_run:
        p, t = _inputs(_parse_shape("32x3x1024x1024"))
        for _ in range(5):
            _step(p, t, True)
        torch.cuda.synchronize()
        return
    if args.native_only:
        rows = [measure(_parse_shape(s), args.reps, args.warmup, ["native"]) for s in args.shapes]
        print(json.dumps({"scratch_mb": int(os.environ.get("TMX_SSIM_GRAD_SCRATCH_MB", 512)), "rows": rows}))
        return

    out = {"what": "ssim(p, t, data_range=1.0).backward(), fp32, gaussian 11x11: forward + backward, ms (median)",
           "device": torch.cuda.get_device_name(0),
           "scratch_mb": int(os.environ.get("TMX_SSIM_GRAD_SCRATCH_MB", 512)),
           "timings": [measure(_parse_shape(s), args.reps, args.warmup, ["native", "composition"]) for s in args.shapes]}
    for row in out["timings"]:
        print(json.dumps(row), flush=True)
    if not args.no_sweep:  # the cap is read once per process: one fresh child per value
        out["scratch_sweep"] = []
        for mb in SWEEP_MB:
            env = dict(os.environ, TMX_SSIM_GRAD_SCRATCH_MB=str(mb))
            proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--native-only", "--reps", str(args.reps), "--warmup",
                                   str(args.warmup), "--shapes", *SWEEP_SHAPES], env=env, capture_output=True, text=True, timeout=300)
            if proc.returncode != 0:
                raise RuntimeError(f"sweep child ({mb} MB) failed with {proc.returncode}:\n{proc.stderr[-2000:]}")
            out["scratch_sweep"].append(json.loads(proc.stdout.strip().splitlines()[-1]))
            print(json.dumps(out["scratch_sweep"][-1]), flush=True)
    if args.test_log:
        with open(args.test_log) as fh:
            lines = fh.read().splitlines()
        out["error_ratios"] = [json.loads(ln.split("ssim_grad_ratio ", 1)[1]) for ln in lines if "ssim_grad_ratio " in ln]
        out["error_16bit"] = [json.loads(ln.split("ssim_grad_16bit ", 1)[1]) for ln in lines if "ssim_grad_16bit " in ln]
    if args.kernel_stats:
        with open(args.kernel_stats, newline="") as fh:
            out["kernel_stats_32x3x1024x1024_5_iterations"] = [
                {"kernel": r["Name"].split("(")[0].replace("void ", ""), "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                 "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3)}
                for r in csv.DictReader(fh) if "tmx::ssim" in r["Name"]]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
