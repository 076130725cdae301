"""3-D SSIM (``ssim(p, t, data_range=1.0)`` on ``[B, C, D, H, W]``, fp32, no autograd): the native kernel (``tmx::ssim3d_sums``)
against the composition (``TMX_SSIM3D_NATIVE=0``: 3-D reflect pad, 5·B stacked batch, dense grouped conv3d, crop) in one
process, alternating; device events, median of ``--reps`` repeats after ``--warmup`` warm-ups; peak allocated memory of
one call of each route; effective GB/s of the native call against the input bytes.

    python tools/ssim3d_bench.py --out profiles/ssim3d_bench.json
        [--no-sweep]            # skip the native-only sweep over TMX_SSIM3D_STRIP (output slices per workgroup)
    python tools/ssim3d_bench.py --profile-run    # a few native calls, for a ``rocprofv3 --kernel-trace --stats`` run
    python tools/ssim3d_bench.py --op-lib LIB.so  # the op alone from csrc/ssim3d.hip built on its own (footprint A/B)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (shape, kwargs)
CONFIGS = [
    ("4x1x64x64x64", {}),
    ("4x1x128x128x128", {}),
    ("1x1x256x256x256", {}),
    ("2x1x64x256x256", {}),
    ("4x1x128x128x128", {"sigma": (0.8, 1.5, 1.0)}),
    ("4x1x128x128x128", {"gaussian_kernel": False, "kernel_size": 7}),
]
SWEEP_SHAPES = ["4x1x64x64x64", "4x1x128x128x128", "1x1x256x256x256"]
SWEEP_STRIPS = [4, 8, 10, 16, 24, 32, 64, 1 << 20]  # (the last: one strip, no recomputed slice)


def _inputs(shape):
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.rand(*shape, device="cuda", generator=g)
    p = (t + 0.1 * torch.randn(*shape, device="cuda", generator=g)).clamp_(0, 1)
    return p, t


def _step(p, t, native, kw):
    from torchmetrics_forked_amd.functional.image import structural_similarity_index_measure as ssim

    os.environ["TMX_SSIM3D_NATIVE"] = "1" if native else "0"  # read on every 5-D call
    return ssim(p, t, data_range=1.0, reduction="none", **kw)


def _timed(p, t, native, kw):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = _step(p, t, native, kw)
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def _peak_bytes(p, t, native, kw):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = _step(p, t, native, kw)
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def measure(shape, kw, reps, warmup, routes=("native", "composition")):
    import torch

    p, t = _inputs(shape)
    times = {r: [] for r in routes}
    outs = {}
    for i in range(warmup + reps):
        for route in routes:  # alternate the routes inside every repeat
            ms, outs[route] = _timed(p, t, route == "native", kw)
            if i >= warmup:
                times[route].append(ms)
    row = {"shape": list(shape), "kwargs": {k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}, "reps": reps}
    for route in routes:
        row[f"{route}_ms"] = round(statistics.median(times[route]), 4)
        row[f"{route}_ms_min_max"] = [round(min(times[route]), 4), round(max(times[route]), 4)]
        row[f"{route}_peak_bytes"] = _peak_bytes(p, t, route == "native", kw)
    input_bytes = 2 * p.numel() * p.element_size()
    row["input_bytes"] = input_bytes
    row["native_input_gb_per_s"] = round(input_bytes / (row["native_ms"] * 1e-3) / 1e9, 2)
    if len(routes) == 2:
        row["speedup"] = round(row["composition_ms"] / row["native_ms"], 2)
        row["native_below_composition"] = row["native_ms"] < row["composition_ms"]
        row["peak_bytes_saved"] = row["composition_peak_bytes"] - row["native_peak_bytes"]
        row["max_abs_diff"] = float((outs["native"] - outs["composition"]).abs().max())
    del p, t
    torch.cuda.empty_cache()
    return row


def strip_sweep(shape, reps, warmup):
    """Native only: the default strip choice and fixed TMX_SSIM3D_STRIP values (read by the op on every call)."""
    import torch

    p, t = _inputs(shape)
    rows = []
    for strip in [None, *SWEEP_STRIPS]:
        if strip is None:
            os.environ.pop("TMX_SSIM3D_STRIP", None)
        else:
            os.environ["TMX_SSIM3D_STRIP"] = str(strip)
        ms = [_timed(p, t, True, {})[0] for _ in range(warmup + reps)][warmup:]
        rows.append({"strip": "default" if strip is None else ("all" if strip == SWEEP_STRIPS[-1] else strip),
                     "native_ms": round(statistics.median(ms), 4)})
    os.environ.pop("TMX_SSIM3D_STRIP", None)
    del p, t
    torch.cuda.empty_cache()
    return {"shape": list(shape), "reps": reps, "rows": rows}


def op_bench(lib, reps, warmup):
    """The op alone (``tmx::ssim3d_sums``, gaussian 11-tap windows) from a stand-alone library: ``csrc/ssim3d.hip`` compiled on
    its own, e.g. with ``-DTMX_SSIM3D_TH=16 -DTMX_SSIM3D_TW=16`` for another footprint.  The package's library is not loaded."""
    import torch

    torch.ops.load_library(os.path.abspath(lib))
    d = torch.arange(11, dtype=torch.float32, device="cuda") - 5
    w = torch.exp(-((d / 1.5) ** 2) / 2)
    w = w / w.sum()
    consts = torch.tensor([0.01**2, 0.03**2], device="cuda")
    rows = []
    for s in SWEEP_SHAPES:
        shape = _parse_shape(s)
        p, t = _inputs((shape[0] * shape[1], *shape[2:]))
        ms = []
        for _ in range(warmup + reps):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out = torch.ops.tmx.ssim3d_sums(p, t, w, w, w, consts)
            end.record()
            end.synchronize()
            ms.append(start.elapsed_time(end))
        rows.append({"shape": list(shape), "op_ms": round(statistics.median(ms[warmup:]), 4), "sum": float(out[0].sum())})
        del p, t
    print(json.dumps({"lib": os.path.basename(lib), "tile": list(torch.ops.tmx.ssim3d_tile()), "reps": reps, "rows": rows}), flush=True)


def _parse_shape(s):
    return tuple(int(v) for v in s.split("x"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--op-lib")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    torch.set_num_threads(min(16, torch.get_num_threads()))
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    if args.op_lib:
        op_bench(args.op_lib, args.reps, args.warmup)
        return
    from torchmetrics_forked_amd import ops

    ops.require()
    if args.profile_run:
        p, t = _inputs(_parse_shape("4x1x128x128x128"))
        for _ in range(5):
            _step(p, t, True, {})
        torch.cuda.synchronize()
        return

    out = {"what": "ssim(p, t, data_range=1.0, reduction='none') on 5-D fp32 volumes, no autograd, ms (median)",
           "device": torch.cuda.get_device_name(0), "tile": list(torch.ops.tmx.ssim3d_tile()), "timings": []}
    for shape, kw in CONFIGS:
        out["timings"].append(measure(_parse_shape(shape), kw, args.reps, args.warmup))
        print(json.dumps(out["timings"][-1]), flush=True)
    out["native_below_composition_at_every_shape"] = all(r["native_below_composition"] for r in out["timings"])
    if not args.no_sweep:
        out["strip_sweep"] = []
        for shape in SWEEP_SHAPES:
            out["strip_sweep"].append(strip_sweep(_parse_shape(shape), args.reps, args.warmup))
            print(json.dumps(out["strip_sweep"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
