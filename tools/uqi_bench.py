"""UQI (``universal_image_quality_index(p, t)``) and D-lambda (``spectral_distortion_index(p, t)``) on ``[B, C, H, W]``, fp32, no
autograd: the native route (``tmx::uqi_sums`` / ``tmx::uqi_band_pair_sums``) against the composition (what ``TMX_UQI_NATIVE=0``
selects: the gate's process-wide switch is flipped between calls) in one process, alternating; device events around the
whole functional call, median of ``--reps`` repeats after ``--warmup`` warm-ups; peak allocated memory of one call of each
route; effective GB/s of the native call against the input bytes and, for D-lambda, against the pair traffic it requests
(every band is one of the two planes of ``L − 1`` pairs).

    python tools/uqi_bench.py --out profiles/uqi_bench.json [--kernel-stats CSV]
    python tools/uqi_bench.py --profile-run    # a few native calls of each metric at 1024 x 1024, for a ``rocprofv3 --kernel-trace --stats`` run
    TMX_UQI_V1=1 python tools/uqi_bench.py ... # the generic kernel where the fast fp32 one would run (read once per process)

``--kernel-stats``: the ``kernel_stats`` CSV of such a run; adds the per-kernel table and the two pairings' effective
bandwidth (bytes the kernel requests / its average time) against ``--hbm-tb-s`` (the read rate of
``profiles/stream_bw_mi355x_r4.json``).
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"uqi": ["16x3x256x256", "8x3x512x512", "4x3x1024x1024", "32x1x41x41"],
          "d_lambda": ["8x4x256x256", "4x8x512x512", "2x8x1024x1024"]}
PROFILE_SHAPES = {"uqi": "4x3x1024x1024", "d_lambda": "2x8x1024x1024"}
PROFILE_CALLS = 5


def _inputs(shape):
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.rand(*shape, device="cuda", generator=g)
    p = (t + 0.1 * torch.randn(*shape, device="cuda", generator=g)).clamp_(0, 1)
    return p, t


def _step(metric, p, t, native):
    import torchmetrics_forked_amd.functional.image.d_lambda as dl_mod
    import torchmetrics_forked_amd.functional.image.uqi as uqi_mod

    uqi_mod._UQI_NATIVE = native  # the one gate both metrics go through
    try:
        if metric == "uqi":
            return uqi_mod.universal_image_quality_index(p, t)
        return dl_mod.spectral_distortion_index(p, t)
    finally:
        uqi_mod._UQI_NATIVE = True


def _timed(metric, p, t, native):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = _step(metric, p, t, native)
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def _peak_bytes(metric, p, t, native):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = _step(metric, p, t, native)
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def _pair_bytes(metric, shape, element_size=4):
    """Bytes the native kernels request: both planes of every pair once (the KS − 1 halo rows and columns not counted)."""
    b, c, h, w = shape
    if metric == "uqi":
        return 2 * b * c * h * w * element_size
    return 2 * b * c * (c - 1) * h * w * element_size  # two tensors, L (L − 1) / 2 pairs of two planes each


def measure(metric, shape, reps, warmup):
    import torch

    p, t = _inputs(shape)
    routes = ("native", "composition")
    times = {r: [] for r in routes}
    outs = {}
    for i in range(warmup + reps):
        for route in routes:  # alternate the routes inside every repeat
            ms, outs[route] = _timed(metric, p, t, route == "native")
            if i >= warmup:
                times[route].append(ms)
    row = {"metric": metric, "shape": list(shape), "reps": reps}
    for route in routes:
        row[f"{route}_ms"] = round(statistics.median(times[route]), 4)
        row[f"{route}_ms_min_max"] = [round(min(times[route]), 4), round(max(times[route]), 4)]
        row[f"{route}_peak_bytes"] = _peak_bytes(metric, p, t, route == "native")
    input_bytes = 2 * p.numel() * p.element_size()
    row["input_bytes"] = input_bytes
    row["native_input_gb_per_s"] = round(input_bytes / (row["native_ms"] * 1e-3) / 1e9, 2)
    if metric == "d_lambda":
        row["pair_bytes"] = _pair_bytes(metric, shape)
        row["native_pair_gb_per_s"] = round(row["pair_bytes"] / (row["native_ms"] * 1e-3) / 1e9, 2)
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
    out = {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} native calls of each metric at "
                   f"{PROFILE_SHAPES['uqi']} / {PROFILE_SHAPES['d_lambda']} fp32), a run of its own", "kernels": rows}
    # the fast fp32 kernel, or the generic one under TMX_UQI_V1=1
    for metric, marks in (("uqi", ("uqi_pair_v2_kernel<11, false>", "uqi_pair_kernel<float, 11, false>")),
                          ("d_lambda", ("uqi_pair_v2_kernel<11, true>", "uqi_pair_kernel<float, 11, true>"))):
        hit = [r for r in rows if any(m in r["kernel"] for m in marks)]
        if hit:
            requested = _pair_bytes(metric, _parse_shape(PROFILE_SHAPES[metric]))
            if metric == "d_lambda":
                requested //= 2  # one launch per tensor
            tb_s = requested / (hit[0]["avg_us"] * 1e-6) / 1e12
            out[f"{metric}_kernel"] = {"kernel": hit[0]["kernel"], "avg_us": hit[0]["avg_us"], "requested_bytes": requested, "effective_tb_per_s": round(tb_s, 3),
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
        for metric in ("uqi", "d_lambda"):
            p, t = _inputs(_parse_shape(PROFILE_SHAPES[metric]))
            for _ in range(PROFILE_CALLS):
                _step(metric, p, t, True)
        torch.cuda.synchronize()
        return

    out = {"what": "universal_image_quality_index(p, t) and spectral_distortion_index(p, t), fp32, no autograd: the whole "
                   "functional call, ms (median)",
           "device": torch.cuda.get_device_name(0), "fp32_kernel": "generic (TMX_UQI_V1)" if os.environ.get("TMX_UQI_V1") else "fast",
           "tile": list(torch.ops.tmx.uqi_tile()), "timings": []}
    for metric in ("uqi", "d_lambda"):
        for shape in SHAPES[metric]:
            out["timings"].append(measure(metric, _parse_shape(shape), args.reps, args.warmup))
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
