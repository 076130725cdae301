"""Spectral angle mapper (``spectral_angle_mapper(p, t, reduction)``) and ERGAS (``error_relative_global_dimensionless_synthesis(p, t)``)
on ``[B, C, H, W]``, fp32, no autograd: the native route (``tmx::sam_map`` / ``tmx::sam_sums`` / ``tmx::ergas_scores``) against the composition
(``TMX_SPECTRAL_NATIVE=0``) and against the native route held to its generic kernels (``TMX_SPECTRAL_GENERIC=1``, the A/B of the 16-byte
loads).  The knobs are read once per process, so every route runs in a process of its own, one after the other; device events
around the whole functional call, median of ``--reps`` repeats after ``--warmup`` warm-ups; peak allocated memory of one call.

    python tools/spectral_bench.py --out profiles/spectral_bench.json [--kernel-trace CSV] [--generic-kernel-trace CSV]
    python tools/spectral_bench.py --profile-run    # a few native op calls per shape, for a ``rocprofv3 --kernel-trace --stats`` run

``--kernel-trace``: the ``kernel_trace`` CSV of such a run; adds each streaming kernel's time per shape and its input GB/s against
``--hbm-tb-s`` (the read rate of ``profiles/stream_bw_mi355x_r4.json``).
``--generic-kernel-trace``: the same of a ``--profile-run`` under ``TMX_SPECTRAL_GENERIC=1``, for the kernel-level A/B.
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ["16x3x256x256", "8x4x512x512", "4x8x1024x1024", "2x200x256x256", "64x4x41x41"]
CASES = [("sam", "elementwise_mean"), ("sam", "none"), ("ergas", "elementwise_mean")]
ROUTES = {"native": {}, "composition": {"TMX_SPECTRAL_NATIVE": "0"}, "generic": {"TMX_SPECTRAL_GENERIC": "1"}}
PROFILE_CALLS = 5
PROFILE_OPS = ("sam_sums", "sam_map", "ergas_scores")
_PROFILE_MARKS = {"sam_sums": ("sam_vec_kernel", "false>"), "sam_map": ("sam_vec_kernel", "true>"), "ergas_scores": ("ergas_plane_vec_kernel", "")}


def _parse_shape(s):
    return tuple(int(v) for v in s.split("x"))


def _inputs(shape):
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.rand(*shape, device="cuda", generator=g) + 0.5
    p = t + 0.1 * torch.randn(*shape, device="cuda", generator=g)
    return p, t


def _step(metric, p, t, reduction):
    from torchmetrics_forked_amd.functional.image.ergas import error_relative_global_dimensionless_synthesis as ergas
    from torchmetrics_forked_amd.functional.image.sam import spectral_angle_mapper as sam

    return sam(p, t, reduction=reduction) if metric == "sam" else ergas(p, t, 4, reduction)


def _timed(metric, p, t, reduction):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = _step(metric, p, t, reduction)
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def _peak_bytes(metric, p, t, reduction):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = _step(metric, p, t, reduction)
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def run_route(reps, warmup):
    """One route (whatever the environment of this process selects): one JSON row per (metric, reduction, shape) on stdout."""
    import torch

    from torchmetrics_forked_amd import ops

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ops.require()
    for shape in SHAPES:
        p, t = _inputs(_parse_shape(shape))
        for metric, reduction in CASES:
            times = []
            for i in range(warmup + reps):
                ms, out = _timed(metric, p, t, reduction)
                if i >= warmup:
                    times.append(ms)
            row = {"metric": metric, "reduction": reduction, "shape": shape, "ms": round(statistics.median(times), 4),
                   "ms_min_max": [round(min(times), 4), round(max(times), 4)], "peak_bytes": _peak_bytes(metric, p, t, reduction),
                   "input_bytes": 2 * p.numel() * p.element_size(), "mean": float(out.double().mean())}
            print("ROW " + json.dumps(row), flush=True)
        del p, t
        torch.cuda.empty_cache()
    print("DEVICE " + json.dumps(torch.cuda.get_device_name(0)), flush=True)


def profile_run():
    import torch

    from torchmetrics_forked_amd import ops
    from torchmetrics_forked_amd.ops import image

    ops.require()
    for shape in SHAPES:
        p, t = _inputs(_parse_shape(shape))
        for op in PROFILE_OPS:
            for _ in range(PROFILE_CALLS):
                getattr(image, op)(p, t, 4.0) if op == "ergas_scores" else getattr(image, op)(p, t)
        torch.cuda.synchronize()


def kernel_times(path, hbm_tb_s, generic=False):
    """Per (op, shape) the streaming kernel's median time of ``--profile-run``: its dispatches appear in call order.  ``generic``: the
    trace of a run under ``TMX_SPECTRAL_GENERIC=1``, where every shape runs the generic kernels."""
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    out = {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} calls of each op per shape, fp32), a run of its own; "
                   "median kernel time, input bytes / time against the HBM read rate (the calls re-read the same inputs, which the 256 MiB Infinity Cache holds in full or in part: figures above the read rate are cache-assisted, not HBM rates)",
           "hbm_read_tb_per_s": hbm_tb_s, "kernels": []}
    for op in PROFILE_OPS:
        name, tag = _PROFILE_MARKS[op]
        name = name.replace("_vec_", "_generic_") if generic else name
        hits = [r for r in rows if name in r["Kernel_Name"] and tag in r["Kernel_Name"]]
        # without the knob the planes that are no multiple of four elements run the generic kernel
        vec_shapes = [s for s in SHAPES if generic or (_parse_shape(s)[2] * _parse_shape(s)[3]) % 4 == 0]
        if len(hits) != PROFILE_CALLS * len(vec_shapes):
            out["kernels"].append({"op": op, "error": f"expected {PROFILE_CALLS * len(vec_shapes)} dispatches of {name}, found {len(hits)}"})
            continue
        for i, shape in enumerate(vec_shapes):
            us = statistics.median((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in hits[i * PROFILE_CALLS:(i + 1) * PROFILE_CALLS])
            b, c, h, w = _parse_shape(shape)
            requested = 2 * 4 * b * c * h * w
            tb_s = requested / (us * 1e-6) / 1e12
            out["kernels"].append({"op": op, "kernel": name, "shape": shape, "median_us": round(us, 2), "input_bytes": requested,
                                   "input_tb_per_s": round(tb_s, 3), "fraction_of_hbm_read_rate": round(tb_s / hbm_tb_s, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--route", choices=sorted(ROUTES), help="run this one route in this process (the parent sets its environment)")
    ap.add_argument("--kernel-trace")
    ap.add_argument("--generic-kernel-trace", help="the same of a --profile-run under TMX_SPECTRAL_GENERIC=1")
    ap.add_argument("--hbm-tb-s", type=float, default=5.649)
    ap.add_argument("--out")
    args = ap.parse_args()

    if args.profile_run:
        return profile_run()
    if args.route:
        return run_route(args.reps, args.warmup)

    # the parent never touches the GPU: one child per route, one after the other
    rows, device = {}, None
    for route, env in ROUTES.items():
        child_env = {k: v for k, v in os.environ.items() if k not in ("TMX_SPECTRAL_NATIVE", "TMX_SPECTRAL_GENERIC")}
        child_env.update(env)
        cmd = [sys.executable, os.path.abspath(__file__), "--route", route, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        proc = subprocess.run(cmd, env=child_env, capture_output=True, text=True, timeout=600)
        if proc.returncode != 0:
            sys.stderr.write(proc.stdout + proc.stderr)
            raise SystemExit(f"route {route} failed with exit status {proc.returncode}")
        for line in proc.stdout.splitlines():
            if line.startswith("ROW "):
                r = json.loads(line[4:])
                rows.setdefault((r["metric"], r["reduction"], r["shape"]), {})[route] = r
            elif line.startswith("DEVICE "):
                device = json.loads(line[7:])

    out = {"what": "spectral_angle_mapper(p, t, reduction) and error_relative_global_dimensionless_synthesis(p, t), fp32, no autograd: the "
                   "whole functional call, ms (median); every route in a process of its own",
           "device": device, "reps": args.reps, "warmup": args.warmup, "timings": []}
    for (metric, reduction, shape), by_route in rows.items():
        n, c, g = by_route["native"], by_route["composition"], by_route["generic"]
        row = {"metric": metric, "reduction": reduction, "shape": shape, "input_bytes": n["input_bytes"]}
        for route, r in by_route.items():
            row[f"{route}_ms"], row[f"{route}_ms_min_max"], row[f"{route}_peak_bytes"] = r["ms"], r["ms_min_max"], r["peak_bytes"]
        row["native_input_gb_per_s"] = round(n["input_bytes"] / (n["ms"] * 1e-3) / 1e9, 2)
        row["speedup"] = round(c["ms"] / n["ms"], 2)
        row["native_below_composition"] = n["ms"] < c["ms"]
        row["generic_over_native"] = round(g["ms"] / n["ms"], 3)
        row["rel_diff"] = abs(n["mean"] - c["mean"]) / abs(c["mean"])
        out["timings"].append(row)
        print(json.dumps(row), flush=True)
    out["native_below_composition_at_every_shape"] = all(r["native_below_composition"] for r in out["timings"])
    if args.kernel_trace:
        out["kernel_times"] = kernel_times(args.kernel_trace, args.hbm_tb_s)
        for k in out["kernel_times"]["kernels"]:
            print(json.dumps(k), flush=True)
    if args.generic_kernel_trace:
        out["generic_kernel_times"] = kernel_times(args.generic_kernel_trace, args.hbm_tb_s, generic=True)
        for k in out["generic_kernel_times"]["kernels"]:
            print(json.dumps(k), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
