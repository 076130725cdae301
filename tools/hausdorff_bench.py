"""Hausdorff distance per (sample, class), no autograd: the native route (``tmx::hausdorff_index`` / ``tmx::hausdorff_onehot``, ``csrc/hausdorff.hip``)
against the package's tensor composition (what ``TMX_HAUSDORFF_NATIVE=0`` selects: edges by shifted comparisons, then per plane the distances
between the edge coordinates), in the same process.  Alternating runs, device events around the whole call including Python, median of
``--reps`` after ``--warmup`` warm-ups.

    python tools/hausdorff_bench.py --out profiles/hausdorff_bench.json [--kernel-trace CSV]
    python tools/hausdorff_bench.py --profile-run    # a few native calls per case, for a ``rocprofv3 --kernel-trace --stats`` run of its own

Masks are blob-like: a few discs per class.  ``outline_vs_pixel`` is the far-apart single pixel against the outline of the whole plane, and
``checkerboard_vs_pixel`` the bound of the file header: every pixel of the checkerboard is an edge pixel and scans most of its row.
``--kernel-trace``: the ``kernel_trace`` CSV of a ``--profile-run``; adds each kernel's median time per case.
"""
import argparse
import csv
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, form, B, C kept, H, W)
CASES = [
    ("blobs", "one-hot", 16, 3, 256, 256),
    ("blobs", "one-hot", 8, 3, 512, 512),
    ("blobs", "one-hot", 4, 3, 1024, 1024),
    ("blobs", "one-hot", 32, 1, 41, 41),
    ("blobs", "index", 8, 20, 512, 512),
    ("outline_vs_pixel", "one-hot", 1, 1, 1024, 1024),
    ("checkerboard_vs_pixel", "one-hot", 1, 1, 1024, 1024),
]
PROFILE_CALLS = 5
KERNELS = ("hausdorff_columns_kernel", "hausdorff_rows_kernel", "hausdorff_finish_kernel")


def _discs(shape, seed, discs=3):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    h, w = shape[-2:]
    yy = torch.arange(h, device="cuda").view(h, 1)
    xx = torch.arange(w, device="cuda").view(1, w)
    cy = torch.rand(*shape[:-2], discs, 1, 1, device="cuda", generator=g) * h
    cx = torch.rand(*shape[:-2], discs, 1, 1, device="cuda", generator=g) * w
    r = 1 + torch.rand(*shape[:-2], discs, 1, 1, device="cuda", generator=g) * (min(h, w) / 4)
    return (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r).any(dim=-3)


def _inputs(name, form, B, C, H, W):
    """``(preds, target, num_classes, kwargs)`` of one case."""
    import torch

    if name == "blobs" and form == "one-hot":
        return _discs((B, C, H, W), 1), _discs((B, C, H, W), 2), C, {"include_background": True}
    if name == "blobs":  # label maps: class c where its blob is, later classes on top, 0 elsewhere
        out = []
        for seed in (1, 2):
            m = _discs((B, C, H, W), seed, discs=2)
            lab = torch.zeros(B, H, W, dtype=torch.int64, device="cuda")
            for c in range(C):
                lab[m[:, c]] = c + 1
            out.append(lab)
        return out[0], out[1], C + 1, {"input_format": "index"}
    p = torch.zeros(B, C, H, W, dtype=torch.bool, device="cuda")
    t = torch.zeros_like(p)
    if name == "outline_vs_pixel":
        p[..., 0, :] = p[..., -1, :] = p[..., :, 0] = p[..., :, -1] = True
    else:
        p[..., ::2, ::2] = p[..., 1::2, 1::2] = True
    t[..., H // 2, W - 1] = True
    return p, t, C, {"include_background": True}


def _timed(fn):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def bench(reps, warmup):
    import torch

    from torchmetrics_forked_amd import ops
    from torchmetrics_forked_amd.functional.segmentation import hausdorff_distance

    hd = importlib.import_module("torchmetrics_forked_amd.functional.segmentation.hausdorff_distance")
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ops.require()
    assert hd._HAUSDORFF_NATIVE, "run without TMX_HAUSDORFF_NATIVE=0: the tool switches the route itself"
    rows = []
    for name, form, B, C, H, W in CASES:
        p, t, classes, kw = _inputs(name, form, B, C, H, W)
        times, outs = {"native": [], "composition": []}, {}
        for i in range(warmup + reps):
            for route in ("native", "composition"):  # alternating
                hd._HAUSDORFF_NATIVE = route == "native"  # what TMX_HAUSDORFF_NATIVE=0 sets at import
                ms, outs[route] = _timed(lambda: hausdorff_distance(p, t, classes, **kw))
                if i >= warmup:
                    times[route].append(ms)
        hd._HAUSDORFF_NATIVE = True
        n, c = statistics.median(times["native"]), statistics.median(times["composition"])
        row = {"case": name, "form": form, "shape": f"{B}x{C}x{H}x{W}", "planes": B * C, "native_ms": round(n, 4), "composition_ms": round(c, 4),
               "native_ms_min_max": [round(min(times["native"]), 4), round(max(times["native"]), 4)],
               "composition_ms_min_max": [round(min(times["composition"]), 4), round(max(times["composition"]), 4)],
               "speedup": round(c / n, 2), "native_below_composition": n < c, "bit_equal": bool(torch.equal(outs["native"], outs["composition"])),
               "largest_value": float(outs["native"].max())}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del p, t, outs
        torch.cuda.empty_cache()
    return rows, torch.cuda.get_device_name(0)


def profile_run():
    import torch

    from torchmetrics_forked_amd import ops
    from torchmetrics_forked_amd.functional.segmentation import hausdorff_distance

    ops.require()
    for case in CASES:
        p, t, classes, kw = _inputs(*case)
        for _ in range(PROFILE_CALLS):
            hausdorff_distance(p, t, classes, **kw)
        torch.cuda.synchronize()


def kernel_times(path):
    """Per case each kernel's median time of ``--profile-run``: a call is one dispatch of each of the three kernels (every case fits one
    plane chunk under the default scratch cap), in call order."""
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    out = {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} native calls per case), a run of its own; median microseconds "
                   "per kernel", "kernels": []}
    hits = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]] for k in KERNELS}
    if any(len(v) != len(CASES) * PROFILE_CALLS for v in hits.values()):
        out["error"] = f"expected {len(CASES) * PROFILE_CALLS} dispatches per kernel, found {({k: len(v) for k, v in hits.items()})}"
        return out
    for i, (name, form, B, C, H, W) in enumerate(CASES):
        us = {k: round(statistics.median(v[i * PROFILE_CALLS:(i + 1) * PROFILE_CALLS]), 2) for k, v in hits.items()}
        out["kernels"].append({"case": name, "form": form, "shape": f"{B}x{C}x{H}x{W}", **{k + "_us": v for k, v in us.items()}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-trace")
    ap.add_argument("--out")
    args = ap.parse_args()

    if args.profile_run:
        return profile_run()
    out = {"what": "hausdorff_distance(preds, target, C) per (sample, class), euclidean, both directions, no autograd: the whole call, ms (median), "
                   "the native route and the package's composition alternating in one process",
           "reps": args.reps, "warmup": args.warmup}
    out["timings"], out["device"] = bench(args.reps, args.warmup)
    out["native_below_composition_at_every_shape"] = all(r["native_below_composition"] for r in out["timings"])
    if args.kernel_trace:
        out["kernel_times"] = kernel_times(args.kernel_trace)
        for k in out["kernel_times"]["kernels"]:
            print(json.dumps(k), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
