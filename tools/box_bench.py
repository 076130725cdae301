"""Sliding-window RMSE (``root_mean_squared_error_using_sliding_window(p, t, ws)``) and RASE
(``relative_average_spectral_error(p, t, ws)``) on ``[B, C, H, W]``, fp32, no autograd: the native route (``tmx::box_rmse_maps`` /
``tmx::rase_fold``) against the composition (what ``TMX_BOX_NATIVE=0`` selects: the gate's process-wide switch is flipped between
calls) in one process, alternating; device events around the whole functional call, median of ``--reps`` repeats after
``--warmup`` warm-ups; peak allocated memory of one call of each route; effective GB/s of the native call against the input bytes.

    python tools/box_bench.py --out profiles/box_bench.json [--kernel-stats CSV]
    python tools/box_bench.py --profile-run    # a few native calls of each metric at 1024 x 1024, for a ``rocprofv3 --kernel-trace --stats`` run

``--kernel-stats``: the ``kernel_stats`` CSV of such a run; adds the per-kernel table and the box kernels' effective bandwidth
(input bytes / average time) against ``--hbm-tb-s`` (the read rate of ``profiles/stream_bw_mi355x_r4.json``).
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (shape, window)
CASES = {"rmse_sw": [("16x3x256x256", 8), ("8x3x512x512", 8), ("4x3x1024x1024", 8), ("32x1x41x41", 8), ("4x3x1024x1024", 15)],
         "rase": [("16x3x256x256", 8), ("8x3x512x512", 8), ("4x3x1024x1024", 8), ("32x1x41x41", 8), ("4x8x512x512", 8),
                  ("4x3x1024x1024", 15)]}
PROFILE_SHAPE = "4x3x1024x1024"
PROFILE_CALLS = 5


def _inputs(shape):
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.rand(*shape, device="cuda", generator=g)
    p = (t + 0.1 * torch.randn(*shape, device="cuda", generator=g)).clamp_(0, 1)
    return p, t


def _step(metric, p, t, ws, native):
    import torchmetrics_forked_amd.functional.image.rase as rase_mod
    import torchmetrics_forked_amd.functional.image.rmse_sw as rmse_mod

    rmse_mod._BOX_NATIVE = native  # the one switch both metrics' gates read
    try:
        if metric == "rmse_sw":
            return rmse_mod.root_mean_squared_error_using_sliding_window(p, t, ws)
        return rase_mod.relative_average_spectral_error(p, t, ws)
    finally:
        rmse_mod._BOX_NATIVE = True


def _timed(metric, p, t, ws, native):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = _step(metric, p, t, ws, native)
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def _peak_bytes(metric, p, t, ws, native):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = _step(metric, p, t, ws, native)
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def measure(metric, shape, ws, reps, warmup):
    import torch

    p, t = _inputs(shape)
    routes = ("native", "composition")
    times = {r: [] for r in routes}
    outs = {}
    for i in range(warmup + reps):
        for route in routes:  # alternate the routes inside every repeat
            ms, outs[route] = _timed(metric, p, t, ws, route == "native")
            if i >= warmup:
                times[route].append(ms)
    row = {"metric": metric, "shape": list(shape), "window_size": ws, "reps": reps,
           "batch_chunks": int(torch.ops.tmx.box_batch_chunks(*shape))}
    for route in routes:
        row[f"{route}_ms"] = round(statistics.median(times[route]), 4)
        row[f"{route}_ms_min_max"] = [round(min(times[route]), 4), round(max(times[route]), 4)]
        row[f"{route}_peak_bytes"] = _peak_bytes(metric, p, t, ws, route == "native")
    input_bytes = 2 * p.numel() * p.element_size()
    row["input_bytes"] = input_bytes
    row["native_input_gb_per_s"] = round(input_bytes / (row["native_ms"] * 1e-3) / 1e9, 2)
    row["speedup"] = round(row["composition_ms"] / row["native_ms"], 2)
    row["native_below_composition"] = row["native_ms"] < row["composition_ms"]
    row["rel_diff"] = float(((outs["native"] - outs["composition"]).abs() / outs["composition"].abs()))
    del p, t
    torch.cuda.empty_cache()
    return row


def _parse_shape(s):
    return tuple(int(v) for v in s.split("x"))


def kernel_stats(path, hbm_tb_s):
    with open(path, newline="") as fh:
        rows = [{"kernel": r["Name"].split("(")[0].replace("void ", ""), "calls": int(r["Calls"]),
                 "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1),
                 "percent": round(float(r["Percentage"]), 1)} for r in csv.DictReader(fh)]
    out = {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} native calls of each metric at "
                   f"{PROFILE_SHAPE} fp32, window 8), a run of its own", "kernels": rows}
    shape = _parse_shape(PROFILE_SHAPE)
    requested = 2 * 4 * shape[0] * shape[1] * shape[2] * shape[3]
    for metric, mark in (("rmse_sw", "box_rmse_kernel<float, 8, false>"), ("rase", "box_rmse_kernel<float, 8, true>")):
        hit = [r for r in rows if mark in r["kernel"]]
        if hit:
            tb_s = requested / (hit[0]["avg_us"] * 1e-6) / 1e12
            out[f"{metric}_kernel"] = {"kernel": hit[0]["kernel"], "avg_us": hit[0]["avg_us"], "input_bytes": requested,
                                       "effective_tb_per_s": round(tb_s, 3), "hbm_read_tb_per_s": hbm_tb_s,
                                       "fraction_of_hbm": round(tb_s / hbm_tb_s, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--hbm-tb-s", type=float, default=5.649)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from torchmetrics_forked_amd import ops

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ops.require()
    if args.profile_run:
        p, t = _inputs(_parse_shape(PROFILE_SHAPE))
        for metric in ("rmse_sw", "rase"):
            for _ in range(PROFILE_CALLS):
                _step(metric, p, t, 8, True)
        torch.cuda.synchronize()
        return

    out = {"what": "root_mean_squared_error_using_sliding_window(p, t, ws) and relative_average_spectral_error(p, t, ws), fp32, no "
                   "autograd: the whole functional call, ms (median)",
           "device": torch.cuda.get_device_name(0), "tile": list(torch.ops.tmx.box_tile()), "timings": []}
    for metric in ("rmse_sw", "rase"):
        for shape, ws in CASES[metric]:
            out["timings"].append(measure(metric, _parse_shape(shape), ws, args.reps, args.warmup))
            print(json.dumps(out["timings"][-1]), flush=True)
    out["native_below_composition_at_every_shape"] = all(r["native_below_composition"] for r in out["timings"])
    if args.kernel_stats:
        out["kernel_stats"] = kernel_stats(args.kernel_stats, args.hbm_tb_s)
        print(json.dumps({k: v for k, v in out["kernel_stats"].items() if k.endswith("_kernel")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
