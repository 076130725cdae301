"""InfoLM's scoring side and the row-pair regression metrics, no autograd: the native route (``tmx::infolm_accumulate`` / ``tmx::row_pair_measure``,
``csrc/infolm.hip``) against the package's ATen composition (what ``TMX_INFOLM_NATIVE=0 TMX_ROWPAIR_NATIVE=0`` selects).  Each route runs in
a process of its own, twice, alternating (native, composition, native, composition); device events around the whole public call including
Python, median of ``--reps`` after ``--warmup`` warm-ups.

    python tools/infolm_bench.py --out profiles/infolm_bench.json [--kernel-trace CSV]
    python tools/infolm_bench.py --profile-run    # a few native calls per case, for a ``rocprofv3 --kernel-trace --stats`` run of its own
    python tools/infolm_bench.py --out profiles/infolm_bench.json --kernel-trace CSV --trace-only    # add the trace to an existing result, no GPU

``distribution``: ``_batch_distribution`` of 64 sentences of 32 tokens, 8 of them scored, on a stand-in model that returns fixed logits
``[512, 32, 30522]`` (one pass of 512 rows).  ``--kernel-trace``: the ``kernel_trace`` CSV of a ``--profile-run``; adds each kernel's median time
per case and the bytes/s it reaches on the bytes the algorithm needs, against the streaming read rate of ``profiles/stream_bw_mi355x_r4.json``.
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

V = 30522
# (path, label, N or rows, row length, dtype)
CASES = [
    ("distribution", "fp32", 512, V, "float32"),
    ("distribution", "bf16", 512, V, "bfloat16"),
    ("measure", "kl_divergence", 4096, V, "float32"),
    ("measure", "ab_divergence", 4096, V, "float32"),
    ("measure", "fisher_rao_distance", 4096, V, "float32"),
    ("kl", "prob", 1 << 20, 10, "float32"),
    ("kl", "log_prob", 1 << 20, 10, "float32"),
    ("kl", "prob", 65536, 1000, "float32"),
    ("cosine", "", 1 << 20, 128, "float32"),
]
PROFILE_CALLS = 5
SENTENCES, TOKENS, SCORED = 64, 32, 8
_SPECIAL = {"mask_token_id": 1, "pad_token_id": 0, "sep_token_id": 2, "cls_token_id": 3}


def _key(case):
    return f"{case[0]}{'/' + case[1] if case[1] else ''} {case[2]}x{case[3]} {case[4]}"


def _bytes(case):
    """Bytes the native route has to move: the logits twice and acc once each way, or both operands once."""
    path, _, n, v, dtype = case
    elt = 4 if dtype == "float32" else 2
    return 2 * n * v * elt + 2 * SENTENCES * v * 4 if path == "distribution" else 2 * n * v * elt


def _call(case):
    """The public call of one case as a closure over its device inputs."""
    import torch

    from torchmetrics_forked_amd.functional.regression.cosine_similarity import cosine_similarity
    from torchmetrics_forked_amd.functional.regression.kl_divergence import kl_divergence
    from torchmetrics_forked_amd.functional.text.infolm import _batch_distribution, _InformationMeasure

    path, label, n, v, dtype = case
    g = torch.Generator(device="cuda").manual_seed(7)
    if path == "distribution":
        logits = (torch.randn(n, TOKENS, v, device="cuda", generator=g) * 3).to(getattr(torch, dtype))
        ids = torch.zeros(SENTENCES, TOKENS, dtype=torch.int64, device="cuda")
        ids[:, :SCORED] = torch.randint(4, 1000, (SENTENCES, SCORED), device="cuda", generator=g)
        mask = (ids != 0).long()
        model = lambda i, m: SimpleNamespace(logits=logits)  # noqa: E731
        return lambda: _batch_distribution(model, ids, mask, None, 0.25, _SPECIAL, n)
    if path == "kl" and label == "log_prob":
        p, q = (torch.log_softmax(torch.randn(n, v, device="cuda", generator=g), -1) for _ in range(2))
    elif path == "cosine":
        p, q = (torch.randn(n, v, device="cuda", generator=g) for _ in range(2))
    else:
        p, q = (torch.softmax(torch.randn(n, v, device="cuda", generator=g), -1) for _ in range(2))
    if path == "measure":
        im = _InformationMeasure(label, 0.5, 0.7)
        return lambda: im(p, q)
    if path == "kl":
        return lambda: kl_divergence(p, q, log_prob=label == "log_prob", reduction="none")
    return lambda: cosine_similarity(p, q, reduction="none")


def worker(reps, warmup, calls_only):
    """Times every case in this process, on the route its environment selects; one JSON line per case."""
    import torch

    from torchmetrics_forked_amd import ops

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ops.require()
    for case in CASES:
        fn = _call(case)
        times = []
        with torch.no_grad():
            for i in range(PROFILE_CALLS if calls_only else warmup + reps):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                out = fn()
                end.record()
                end.synchronize()
                if i >= warmup:
                    times.append(start.elapsed_time(end))
        if not calls_only:
            fin = out.double()[torch.isfinite(out)]
            print(json.dumps({"case": _key(case), "ms": round(statistics.median(times), 4), "ms_min_max": [round(min(times), 4), round(max(times), 4)],
                              "mean_of_result": float(fin.mean())}), flush=True)
        del fn, out
        torch.cuda.empty_cache()


def _spawn(route, reps, warmup):
    env = dict(os.environ)
    if route == "composition":
        env.update(TMX_INFOLM_NATIVE="0", TMX_ROWPAIR_NATIVE="0")
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(reps), "--warmup", str(warmup)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=REPO)
    if res.returncode != 0:
        raise RuntimeError(f"{route} worker failed ({res.returncode}):\n{res.stdout}\n{res.stderr}")
    return {r["case"]: r for r in map(json.loads, filter(None, res.stdout.splitlines()))}


def bench(reps, warmup):
    runs = [(route, _spawn(route, reps, warmup)) for route in ("native", "composition", "native", "composition")]
    rows = []
    for case in CASES:
        k = _key(case)
        nat, comp = ([r[k] for route, r in runs if route == want] for want in ("native", "composition"))
        n, c = min(x["ms"] for x in nat), min(x["ms"] for x in comp)  # the better of each route's two processes
        rows.append({"case": k, "native_ms": n, "composition_ms": c, "native_ms_both_runs": [x["ms"] for x in nat],
                     "composition_ms_both_runs": [x["ms"] for x in comp], "speedup": round(c / n, 2), "native_below_composition": n < c,
                     "relative_difference_of_result_means": abs(nat[0]["mean_of_result"] - comp[0]["mean_of_result"]) / abs(comp[0]["mean_of_result"])})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def kernel_times(path):
    """Per case each kernel's median time in a ``--profile-run``: ``PROFILE_CALLS`` native calls per case, in case order."""
    with open(os.path.join(REPO, "profiles", "stream_bw_mi355x_r4.json")) as fh:
        read_rate = max(r["TB_s"] for r in json.load(fh)["results"] if r["op"] == "read" and r["operand_MB"] > 1000)
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    ours = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows
            if any(k in r["Kernel_Name"] for k in ("infolm_row_stats", "infolm_accumulate", "infolm_offsets", "row_pair_"))]
    per_call = {"distribution": 3}
    out = {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} native calls per case), a run of its own; median microseconds per "
                   "kernel; TB/s on the bytes the algorithm needs (distribution: logits twice and acc both ways; else both operands once)",
           "stream_read_TB_s": read_rate, "kernels": []}
    at = 0
    for case in CASES:
        k = per_call.get(case[0], 1)
        chunk = ours[at:at + k * PROFILE_CALLS]
        at += k * PROFILE_CALLS
        if len(chunk) != k * PROFILE_CALLS:
            out["error"] = f"trace ends inside {_key(case)}"
            break
        names = [n.split("<")[0].split("(")[0].replace("void tmx::", "").replace("tmx::", "") for n, _ in chunk[:k]]
        us = [round(statistics.median(t for _, t in chunk[j::k]), 2) for j in range(k)]
        tb_s = _bytes(case) / (sum(us) * 1e-6) / 1e12
        out["kernels"].append({"case": _key(case), "kernels_us": dict(zip(names, us)), "bytes": _bytes(case), "TB_s": round(tb_s, 3),
                               "share_of_stream_read": round(tb_s / read_rate, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--worker", action="store_true", help="time every case in this process on the route the environment selects")
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-trace")
    ap.add_argument("--trace-only", action="store_true", help="parse --kernel-trace into the existing --out file; runs nothing")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.worker or args.profile_run:
        return worker(args.reps, 0 if args.profile_run else args.warmup, args.profile_run)
    out = {"what": "whole public call, ms (median), no autograd: _batch_distribution, _InformationMeasure, kl_divergence, cosine_similarity; the native "
                   "route and the composition (TMX_INFOLM_NATIVE=0 TMX_ROWPAIR_NATIVE=0) each in processes of their own, alternating, two each",
           "reps": args.reps, "warmup": args.warmup}
    if args.trace_only:
        with open(args.out) as fh:
            out = json.load(fh)
    else:
        out["timings"] = bench(args.reps, args.warmup)
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
