"""cramers_v_matrix and theils_u_matrix on ``[N, V]`` int64 matrices and one two-column ``cramers_v`` pair call: the native route
(``csrc/nominal.hip``) against the composition (the per-pair host loop) in the same process.  The composition is the same call with the
gate's process flag (what ``TMX_NOMINAL_NATIVE=0`` sets) switched off around it.  Alternating runs, device events around the whole call
including Python, median of ``--reps`` after ``--warmup`` warm-ups, peak allocated memory of one call.  Also, at op level, the pair-table
kernel with the table extent 64 against the smallest extent that holds the labels (the extent the route could take from a host read).

    python tools/nominal_bench.py --out profiles/nominal_bench.json [--kernel-trace CSV]
    python tools/nominal_bench.py --profile-run    # a few native calls per case, for a ``rocprofv3 --kernel-trace --stats`` run of its own

``--kernel-trace``: the ``kernel_trace`` CSV of such a run; adds each native kernel's median time per case.
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MATRIX_SHAPES = [(10_000, 8), (100_000, 32), (1_000_000, 16)]
CATEGORIES = [4, 32]
PAIR_ROWS = 1_000_000
CASES = [(metric, n, v, k) for n, v in MATRIX_SHAPES for k in CATEGORIES for metric in ("cramers_v_matrix", "theils_u_matrix")]
CASES.append(("cramers_v", PAIR_ROWS, 2, 4))
PROFILE_CASES = [c for c in CASES if c[0] != "theils_u_matrix"]
KERNELS = ("nominal_labels_kernel", "nominal_pair_tables_kernel", "nominal_scores_kernel")  # per native call of a PROFILE_CASES entry, in order
PROFILE_CALLS = 5


def _inputs(n, v, k):
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    m = torch.randint(0, k, (n, v), device="cuda", generator=g)
    m[:, 1] = (m[:, 0] + (torch.rand(n, device="cuda", generator=g) < 0.3).long()) % k
    return m


def _steps(metric):
    """``(native, composition)`` callables of one case: the same functional, the gate's flag off around the second."""
    import torchmetrics_forked_amd.functional.nominal as FN
    import torchmetrics_forked_amd.functional.nominal.native as route

    fn = getattr(FN, metric)

    def native(m):
        return fn(m[:, 0], m[:, 1]) if metric == "cramers_v" else fn(m)

    def composition(m):
        keep = route._NOMINAL_NATIVE
        route._NOMINAL_NATIVE = False
        try:
            return native(m)
        finally:
            route._NOMINAL_NATIVE = keep

    return native, composition


def _timed(fn, *args):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn(*args)
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def _peak_bytes(fn, m):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn(m)
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def bench(reps, warmup):
    import torch

    from torchmetrics_forked_amd import ops

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ops.require()
    rows = []
    for metric, n, v, k in CASES:
        m = _inputs(n, v, k)
        native, composition = _steps(metric)
        times = {"native": [], "composition": []}
        outs = {}
        for i in range(warmup + reps):
            for route, fn in (("native", native), ("composition", composition)):  # alternating
                ms, outs[route] = _timed(fn, m)
                if i >= warmup:
                    times[route].append(ms)
        a, c = statistics.median(times["native"]), statistics.median(times["composition"])
        diff = (outs["native"].double() - outs["composition"].double()).abs()
        row = {"metric": metric, "rows": n, "columns": v, "categories": k, "native_ms": round(a, 4), "composition_ms": round(c, 4),
               "native_ms_min_max": [round(min(times["native"]), 4), round(max(times["native"]), 4)],
               "composition_ms_min_max": [round(min(times["composition"]), 4), round(max(times["composition"]), 4)],
               "native_peak_bytes": _peak_bytes(native, m), "composition_peak_bytes": _peak_bytes(composition, m),
               "speedup": round(c / a, 2), "native_below_composition": a < c, "max_abs_diff": float(diff[~diff.isnan()].max())}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del m, outs
        torch.cuda.empty_cache()
    return rows, torch.cuda.get_device_name(0)


def extent_bench(reps, warmup):
    """``nominal_pair_tables`` alone on the labels of every matrix case: the extent 64 the route always passes, and the smallest that holds the labels."""
    import torch

    from torchmetrics_forked_amd.ops import nominal as ops_nominal

    rows = []
    for n, v in MATRIX_SHAPES:
        for k in CATEGORIES:
            labels, masks, _ = ops_nominal.nominal_labels(_inputs(n, v, k), False, 0.0)
            times = {64: [], k: []}
            for i in range(warmup + reps):
                for extent in (64, k):
                    ms, _ = _timed(ops_nominal.nominal_pair_tables, labels, masks, extent)
                    if i >= warmup:
                        times[extent].append(ms)
            row = {"rows": n, "columns": v, "categories": k, "extent_64_ms": round(statistics.median(times[64]), 4),
                   "smallest_extent": k, "smallest_extent_ms": round(statistics.median(times[k]), 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del labels, masks
            torch.cuda.empty_cache()
    return rows


def profile_run():
    import torch

    from torchmetrics_forked_amd import ops

    ops.require()
    for metric, n, v, k in PROFILE_CASES:
        m = _inputs(n, v, k)
        native, _ = _steps(metric)
        for _ in range(PROFILE_CALLS):
            native(m)
        torch.cuda.synchronize()


def kernel_times(path):
    """Per case the native kernels' median times of ``--profile-run``: the dispatches of ``nominal_*`` appear in call order, ``len(KERNELS)`` per call."""
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    hits = [r for r in rows if "nominal_" in r["Kernel_Name"]]
    out = {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} native calls per case), a run of its own; median time of every "
                   "native kernel of a call", "kernels": []}
    want = len(PROFILE_CASES) * PROFILE_CALLS * len(KERNELS)
    if len(hits) != want:
        out["error"] = f"expected {want} dispatches of nominal_*, found {len(hits)}"
        return out
    at = 0
    for metric, n, v, k in PROFILE_CASES:
        calls = [hits[at + i * len(KERNELS):at + (i + 1) * len(KERNELS)] for i in range(PROFILE_CALLS)]
        at += len(KERNELS) * PROFILE_CALLS
        for j, name in enumerate(KERNELS):
            assert all(name in c[j]["Kernel_Name"] for c in calls), (name, calls[0][j]["Kernel_Name"])
            us = statistics.median((int(c[j]["End_Timestamp"]) - int(c[j]["Start_Timestamp"])) / 1e3 for c in calls)
            out["kernels"].append({"metric": metric, "rows": n, "columns": v, "categories": k, "kernel": name, "median_us": round(us, 2)})
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
    out = {"what": "cramers_v_matrix(m), theils_u_matrix(m) on int64 [rows, columns] with the given number of categories and cramers_v(p, t) on two "
                   "columns: the whole call, ms (median), native and composition alternating in one process",
           "reps": args.reps, "warmup": args.warmup}
    out["timings"], out["device"] = bench(args.reps, args.warmup)
    out["native_below_composition_at_every_shape"] = all(r["native_below_composition"] for r in out["timings"])
    out["pair_table_extent"] = {"what": "nominal_pair_tables alone, ms (median), extent 64 and the smallest extent alternating",
                                "timings": extent_bench(args.reps, args.warmup)}
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
