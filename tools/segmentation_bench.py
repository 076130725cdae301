"""Per-sample mean IoU of segmentation maps, no autograd: the native route (``tmx::segment_overlap_index`` / ``tmx::segment_overlap_onehot`` and
``tmx::segment_scores``, ``csrc/segment_overlap.hip``) against the plain ATen composition a user has to write without this package, in the same
process.  The baseline is written here (``one_hot``, ``movedim``, ``&``, ``sum``, divide): it is not the package's own fallback.  Alternating runs,
device events around the whole call including Python, median of ``--reps`` after ``--warmup`` warm-ups, peak allocated memory of one call.
Every shape runs on two label kinds: uniformly random, and piecewise constant in 32 x 32 blocks (LDS contention differs between them).

    python tools/segmentation_bench.py --out profiles/segmentation_bench.json [--kernel-trace CSV]
    python tools/segmentation_bench.py --profile-run    # a few native calls per case, for a ``rocprofv3 --kernel-trace --stats`` run of its own

The index-form cases also time the overlap op alone under ``TMX_SEGMENT_MODE`` 0 (plain LDS atomics per pixel), 1 (wave-uniform fast path) and
2 (per-lane run merging, the default): the contention A/B.  ``--kernel-trace``: the ``kernel_trace`` CSV of a ``--profile-run``; adds each overlap
kernel's median time per case and its input bytes per second against ``--hbm-tb-s`` (the read rate of ``profiles/stream_bw_mi355x_r4.json``).
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (form, shape of the label map, classes, preds dtype, target dtype)
CASES = [
    ("index", "16x512x512", 21, "int64", "int64"),
    ("index", "8x1024x1024", 19, "int64", "int64"),
    ("index", "2x128x128x128", 14, "int64", "int64"),
    ("index", "32x64x64", 2, "int64", "int64"),
    ("index", "16x512x512", 21, "int64", "uint8"),
    ("one-hot", "16x512x512", 21, "bool", "bool"),
    ("one-hot", "16x512x512", 21, "int64", "int64"),
]
KINDS = ("random", "blocky32")
MODES = {"0": "plain", "1": "wave_uniform", "2": "run_merge"}
PROFILE_CALLS = 5


def _parse_shape(s):
    return tuple(int(v) for v in s.split("x"))


def _labels(shape, classes, kind, seed):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "random":
        return torch.randint(0, classes, shape, device="cuda", generator=g)
    lead, (h, w) = shape[:-2], shape[-2:]
    coarse = torch.randint(0, classes, (*lead, (h + 31) // 32, (w + 31) // 32), device="cuda", generator=g)
    return coarse.repeat_interleave(32, -2).repeat_interleave(32, -1)[..., :h, :w].contiguous()


def _inputs(form, shape, classes, dp, dt, kind):
    import torch

    p, t = _labels(shape, classes, kind, 1), _labels(shape, classes, kind, 2)
    if form == "one-hot":
        cls = torch.arange(classes, device="cuda").view(1, classes, *([1] * (len(shape) - 1)))
        p, t = p.unsqueeze(1) == cls, t.unsqueeze(1) == cls
    return p.to(getattr(torch, dp)), t.to(getattr(torch, dt))


def _steps(form, classes):
    """``(native, baseline)`` callables of one case."""
    import torch

    from torchmetrics_forked_amd.functional.segmentation import mean_iou

    def native(p, t):
        return mean_iou(p, t, classes, input_format=form)

    def baseline(p, t):
        if form == "index":
            p = torch.nn.functional.one_hot(p.long(), classes).movedim(-1, 1)
            t = torch.nn.functional.one_hot(t.long(), classes).movedim(-1, 1)
        dims = tuple(range(2, p.ndim))
        inter = (p & t).sum(dim=dims)
        union = p.sum(dim=dims) + t.sum(dim=dims) - inter
        iou = torch.where(union != 0, inter / union, torch.zeros((), device=p.device))
        return iou.mean(dim=1)

    return native, baseline


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


def _contention(p, t, classes, reps, warmup):
    """Median ms of the overlap op alone under each ``TMX_SEGMENT_MODE`` (read per call), alternating."""
    from torchmetrics_forked_amd.ops.segmentation import segment_overlap_index

    times = {m: [] for m in MODES}
    keep = os.environ.get("TMX_SEGMENT_MODE")
    try:
        for i in range(warmup + reps):
            for m in MODES:
                os.environ["TMX_SEGMENT_MODE"] = m
                ms, _ = _timed(lambda a, b: segment_overlap_index(a, b, classes), p, t)
                if i >= warmup:
                    times[m].append(ms)
    finally:
        if keep is None:
            os.environ.pop("TMX_SEGMENT_MODE", None)
        else:
            os.environ["TMX_SEGMENT_MODE"] = keep
    return {f"{MODES[m]}_ms": round(statistics.median(v), 4) for m, v in times.items()}


def bench(reps, warmup):
    import torch

    from torchmetrics_forked_amd import ops

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ops.require()
    rows = []
    for form, shape, classes, dp, dt in CASES:
        for kind in KINDS:
            p, t = _inputs(form, _parse_shape(shape), classes, dp, dt, kind)
            native, baseline = _steps(form, classes)
            times = {"native": [], "baseline": []}
            outs = {}
            for i in range(warmup + reps):
                for route, fn in (("native", native), ("baseline", baseline)):  # alternating
                    ms, outs[route] = _timed(fn, p, t)
                    if i >= warmup:
                        times[route].append(ms)
            n, c = statistics.median(times["native"]), statistics.median(times["baseline"])
            input_bytes = p.numel() * p.element_size() + t.numel() * t.element_size()
            row = {"form": form, "shape": shape, "classes": classes, "preds": dp, "target": dt, "labels": kind, "input_bytes": input_bytes,
                   "native_ms": round(n, 4), "baseline_ms": round(c, 4),
                   "native_ms_min_max": [round(min(times["native"]), 4), round(max(times["native"]), 4)],
                   "baseline_ms_min_max": [round(min(times["baseline"]), 4), round(max(times["baseline"]), 4)],
                   "native_peak_bytes": _peak_bytes(native, p, t), "baseline_peak_bytes": _peak_bytes(baseline, p, t),
                   "speedup": round(c / n, 2), "native_below_baseline": n < c,
                   "native_input_gb_per_s": round(input_bytes / (n * 1e-3) / 1e9, 2),
                   "max_abs_diff": float((outs["native"].double() - outs["baseline"].double()).abs().max())}
            if form == "index":
                row["overlap_op_by_mode"] = _contention(p, t, classes, reps, warmup)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del p, t, outs
            torch.cuda.empty_cache()
    return rows, torch.cuda.get_device_name(0)


def profile_run():
    import torch

    from torchmetrics_forked_amd import ops

    ops.require()
    for form, shape, classes, dp, dt in CASES:
        for kind in KINDS:
            p, t = _inputs(form, _parse_shape(shape), classes, dp, dt, kind)
            native, _ = _steps(form, classes)
            for _ in range(PROFILE_CALLS):
                native(p, t)
            torch.cuda.synchronize()


def kernel_times(path, hbm_tb_s):
    """Per case the overlap kernel's median time of ``--profile-run``: the dispatches of ``segment_overlap_*`` appear in call order, one per call."""
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    hits = [r for r in rows if "segment_overlap_" in r["Kernel_Name"]]
    scores = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "segment_scores_kernel" in r["Kernel_Name"]]
    out = {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} native mean_iou calls per case), a run of its own; median time of the "
                   "overlap kernel, input bytes / time against the HBM read rate (the calls re-read the same inputs, which the 256 MiB Infinity "
                   "Cache holds in full or in part: figures above the read rate are cache-assisted, not HBM rates)",
           "hbm_read_tb_per_s": hbm_tb_s, "scores_kernel_median_us": round(statistics.median(scores), 2) if scores else None, "kernels": []}
    want = len(CASES) * len(KINDS) * PROFILE_CALLS
    if len(hits) != want:
        out["error"] = f"expected {want} dispatches of segment_overlap_*, found {len(hits)}"
        return out
    at = 0
    sizes = {"bool": 1, "uint8": 1, "int16": 2, "int32": 4, "int64": 8}
    for form, shape, classes, dp, dt in CASES:
        for kind in KINDS:
            calls = hits[at:at + PROFILE_CALLS]
            at += PROFILE_CALLS
            pixels = 1
            for v in _parse_shape(shape):
                pixels *= v
            requested = pixels * (classes if form == "one-hot" else 1) * (sizes[dp] + sizes[dt])
            us = statistics.median((int(c["End_Timestamp"]) - int(c["Start_Timestamp"])) / 1e3 for c in calls)
            tb_s = requested / (us * 1e-6) / 1e12
            out["kernels"].append({"form": form, "shape": shape, "classes": classes, "preds": dp, "target": dt, "labels": kind,
                                   "kernel": calls[0]["Kernel_Name"].split("(")[0], "median_us": round(us, 2), "input_bytes": requested,
                                   "input_tb_per_s": round(tb_s, 3), "fraction_of_hbm_read_rate": round(tb_s / hbm_tb_s, 3)})
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
    out = {"what": "mean_iou(preds, target, C) per sample, no autograd: the whole call, ms (median), the native route and the plain ATen composition "
                   "(one_hot, movedim, &, sum, divide) alternating in one process; overlap_op_by_mode: the index-form overlap op alone under each "
                   "TMX_SEGMENT_MODE",
           "reps": args.reps, "warmup": args.warmup}
    out["timings"], out["device"] = bench(args.reps, args.warmup)
    out["native_below_baseline_at_every_shape"] = all(r["native_below_baseline"] for r in out["timings"])
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
