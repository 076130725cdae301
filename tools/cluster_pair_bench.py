"""Extrinsic clustering scores: the native route (``csrc/cluster_pairs.hip``) against the torch composition.

Same process, alternating routes (``TMX_CLUSTER_NATIVE=0`` selects the composition), device events around the whole call,
median of 20 after 3 warm-ups; GB/s of input (both label vectors, read once, as int64) against the read rate of
``profiles/stream_bw_mi355x_r4.json``.  ``TMX_CLUSTER_PAIR_LDS_CELLS`` is read once per process: ``--ab`` reruns the native
side of the LDS-arm shapes in fresh child processes, one per value.  AMI is timed up to ``--ami-cells`` table cells times
``N`` (its EMI kernel, shared by both routes, walks every n_ij of every cluster pair).  Writes
``profiles/cluster_pair_bench.json`` (``--out``)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
SIZES = (65536, 1 << 20, 1 << 24)
CLUSTERS = ((8, 8), (100, 100), (1000, 1000))
METRICS = ("mutual_info_score", "adjusted_rand_score", "v_measure_score", "adjusted_mutual_info_score")


def _time(fn, preds, target, native, reps=20, warm=3):
    os.environ["TMX_CLUSTER_NATIVE"] = "1" if native else "0"
    times = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(preds, target)
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), float(out)


def _case(n, kp, kt, order, ami_work, routes=(True, False)):
    import torchmetrics_forked_amd.functional.clustering as FC

    g = torch.Generator().manual_seed(0)
    preds = torch.randint(0, kp, (n,), generator=g)
    target = torch.where(torch.rand(n, generator=g) < 0.7, preds % kt, torch.randint(0, kt, (n,), generator=g))
    if order == "sorted":
        target, idx = torch.sort(target)
        preds = preds[idx]
    preds, target, rows = preds.cuda(), target.cuda(), []
    for name in METRICS:
        if name == "adjusted_mutual_info_score" and n * kp * kt > ami_work:
            continue
        row = {"shape": [n, kp, kt], "order": order, "metric": name}
        for native in routes:
            us, value = _time(getattr(FC, name), preds, target, native)
            key = "native" if native else "composition"
            row.update({f"{key}_us": round(us, 1), f"{key}_value": value})
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "cluster_pair_bench.json"))
    ap.add_argument("--stream-bw", default=str(REPO / "profiles" / "stream_bw_mi355x_r4.json"))
    ap.add_argument("--ami-work", type=float, default=2e10, help="largest N * K_p * K_t at which AMI is timed")
    ap.add_argument("--ab", action="store_true", help="also run the LDS_CELLS A/B in child processes")
    ap.add_argument("--child", nargs=3, type=int, help="internal: print the native timings of one shape as JSON")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cluster_pair_bench needs a GPU"
    if args.child:
        print(json.dumps([r for o in ("shuffled", "sorted") for r in _case(*args.child, o, args.ami_work, routes=(True,))]))
        return
    read = None
    if Path(args.stream_bw).exists():
        read = next(r["TB_s"] for r in json.load(open(args.stream_bw))["results"] if r["op"] == "read" and r["variant"] == "rotating-4")
    out = {"device": torch.cuda.get_device_name(0), "method": "same process, alternating, device events, median of 20 after 3 warm-ups",
           "stream_read_TB_s": read, "timings": [], "ab": []}

    def save():
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")

    for n in SIZES:
        for kp, kt in CLUSTERS:
            for order in ("shuffled", "sorted"):
                for row in _case(n, kp, kt, order, args.ami_work):
                    row["speedup"] = round(row["composition_us"] / row["native_us"], 2)
                    row["native_input_GB_s"] = round(n * 16 / row["native_us"] / 1e3, 1)
                    row["share_of_stream_read"] = round(row["native_input_GB_s"] / (read * 1e3), 4) if read else None
                    out["timings"].append(row)
                    print(json.dumps(row), flush=True)
                save()
    if args.ab:
        for shape in ((1 << 20, 8, 8), (1 << 24, 8, 8), (1 << 24, 64, 64), (1 << 24, 100, 100)):
            for v in (4096, 8192, 16384):
                env = dict(os.environ, TMX_CLUSTER_PAIR_LDS_CELLS=str(v))
                proc = subprocess.run([sys.executable, __file__, "--child", *map(str, shape), "--ami-work", "0"], env=env, capture_output=True,
                                      text=True, timeout=300)
                assert proc.returncode == 0, proc.stderr[-2000:]
                rows = json.loads(proc.stdout.strip().splitlines()[-1])
                rec = {"knob": "TMX_CLUSTER_PAIR_LDS_CELLS", "value": v, "shape": list(shape),
                       "native_us": {f"{r['metric']}/{r['order']}": r["native_us"] for r in rows}}
                out["ab"].append(rec)
                print(json.dumps(rec), flush=True)
            save()


if __name__ == "__main__":
    main()
