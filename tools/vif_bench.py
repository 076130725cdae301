"""VIF-p (``visual_information_fidelity(p, t)`` on ``[B, C, H, W]``, fp32, no autograd): the native route (``tmx::vif_sums``)
against the composition (what ``TMX_VIF_NATIVE=0`` selects: the gate's process-wide switch is flipped between calls) in
one process, alternating; device events around the whole functional call, median of ``--reps`` repeats after ``--warmup``
warm-ups; peak allocated memory of one call of each route; effective GB/s of the native call against the input bytes.

    python tools/vif_bench.py --out profiles/vif_bench.json [--kernel-stats CSV]
    python tools/vif_bench.py --profile-run    # a few native calls at 4x3x1024x1024, for a ``rocprofv3 --kernel-trace --stats`` run

``--kernel-stats``: the ``kernel_stats`` CSV of such a run; adds the per-kernel table and the scale-0 kernel's effective input
bandwidth (both inputs read once / its average time) against ``--hbm-tb-s`` (the read rate of
``profiles/stream_bw_mi355x_r4.json``).
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ["16x3x256x256", "8x3x512x512", "4x3x1024x1024", "32x1x41x41"]
PROFILE_SHAPE = "4x3x1024x1024"
PROFILE_CALLS = 5


def _inputs(shape):
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.rand(*shape, device="cuda", generator=g)
    p = (t + 0.1 * torch.randn(*shape, device="cuda", generator=g)).clamp_(0, 1)
    return p, t


def _step(p, t, native):
    import torchmetrics_forked_amd.functional.image.vif as vif_mod

    vif_mod._VIF_NATIVE = native
    try:
        return vif_mod.visual_information_fidelity(p, t)
    finally:
        vif_mod._VIF_NATIVE = True


def _timed(p, t, native):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = _step(p, t, native)
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def _peak_bytes(p, t, native):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = _step(p, t, native)
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def measure(shape, reps, warmup):
    import torch

    p, t = _inputs(shape)
    routes = ("native", "composition")
    times = {r: [] for r in routes}
    outs = {}
    for i in range(warmup + reps):
        for route in routes:  # alternate the routes inside every repeat
            ms, outs[route] = _timed(p, t, route == "native")
            if i >= warmup:
                times[route].append(ms)
    row = {"shape": list(shape), "reps": reps}
    for route in routes:
        row[f"{route}_ms"] = round(statistics.median(times[route]), 4)
        row[f"{route}_ms_min_max"] = [round(min(times[route]), 4), round(max(times[route]), 4)]
        row[f"{route}_peak_bytes"] = _peak_bytes(p, t, route == "native")
    input_bytes = 2 * p.numel() * p.element_size()
    row["input_bytes"] = input_bytes
    row["native_input_gb_per_s"] = round(input_bytes / (row["native_ms"] * 1e-3) / 1e9, 2)
    row["speedup"] = round(row["composition_ms"] / row["native_ms"], 2)
    row["native_below_composition"] = row["native_ms"] < row["composition_ms"]
    row["abs_diff"] = float((outs["native"] - outs["composition"]).abs())
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
    out = {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} native calls, {PROFILE_SHAPE} fp32), a run of its own",
           "kernels": rows}
    scale0 = [r for r in rows if "vif_scale_kernel<float, 17>" in r["kernel"]]
    if scale0:
        shape = _parse_shape(PROFILE_SHAPE)
        input_bytes = 2 * 4 * shape[0] * shape[1] * shape[2] * shape[3]
        tb_s = input_bytes / (scale0[0]["avg_us"] * 1e-6) / 1e12
        out["scale0_kernel"] = {"avg_us": scale0[0]["avg_us"], "input_bytes": input_bytes, "effective_input_tb_per_s": round(tb_s, 3),
                                "hbm_read_tb_per_s": hbm_tb_s, "fraction_of_hbm": round(tb_s / hbm_tb_s, 3)}
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
        for _ in range(PROFILE_CALLS):
            _step(p, t, True)
        torch.cuda.synchronize()
        return

    out = {"what": "visual_information_fidelity(p, t), fp32, no autograd: the whole functional call, ms (median)",
           "device": torch.cuda.get_device_name(0), "tile": list(torch.ops.tmx.vif_tile()), "timings": []}
    for shape in SHAPES:
        out["timings"].append(measure(_parse_shape(shape), args.reps, args.warmup))
        print(json.dumps(out["timings"][-1]), flush=True)
    out["native_below_composition_at_every_shape"] = all(r["native_below_composition"] for r in out["timings"])
    if args.kernel_stats:
        out["kernel_stats"] = kernel_stats(args.kernel_stats, args.hbm_tb_s)
        print(json.dumps(out["kernel_stats"].get("scale0_kernel")), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
