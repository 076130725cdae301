"""Intrinsic clustering scores: the native route (``csrc/cluster_scatter.hip``) against the torch composition.

Same process, alternating routes (``TMX_CLUSTER_NATIVE=0`` selects the composition), device events around the whole call,
median of 20 after 3 warm-ups; peak allocated memory per route; GB/s of input (two reads of ``data`` are the least the native
route can do, one read is what the figure counts) against the read rate of ``profiles/stream_bw_mi355x_r4.json``.
``TMX_CLUSTER_KW`` and ``TMX_CLUSTER_TARGET_GROUPS`` are read once per process: ``--ab`` reruns the native side of two shapes
in fresh child processes, one per knob value.  Writes ``profiles/cluster_bench.json`` (``--out``)."""
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
SHAPES = [(1 << 20, 128, 16), (262144, 32, 100), (65536, 2, 8), (4096, 512, 10), (1 << 20, 16, 1000)]
METRICS = ("calinski_harabasz_score", "davies_bouldin_score", "dunn_index")


def _time(fn, data, labels, native, reps=20, warm=3):
    os.environ["TMX_CLUSTER_NATIVE"] = "1" if native else "0"
    torch.cuda.reset_peak_memory_stats()
    base, times = torch.cuda.memory_allocated(), []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(data, labels)
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), (torch.cuda.max_memory_allocated() - base) / 2**20, float(out)


def _case(n, d, k, routes=(True, False)):
    import torchmetrics_forked_amd.functional.clustering as FC

    g = torch.Generator().manual_seed(0)
    labels = torch.randint(0, k, (n,), generator=g).cuda()
    data = torch.randn(n, d, generator=g).cuda() + 3.0 * torch.randn(k, d, generator=g).cuda()[labels]
    rows = []
    for name in METRICS:
        row = {"shape": [n, d, k], "metric": name}
        for native in routes:
            us, mib, value = _time(getattr(FC, name), data, labels, native)
            key = "native" if native else "composition"
            row.update({f"{key}_us": round(us, 1), f"{key}_peak_MiB": round(mib, 1), f"{key}_value": value})
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "cluster_bench.json"))
    ap.add_argument("--stream-bw", default=str(REPO / "profiles" / "stream_bw_mi355x_r4.json"))
    ap.add_argument("--ab", action="store_true", help="also run the KW and chunk-target A/B in child processes")
    ap.add_argument("--child", nargs=3, type=int, help="internal: print the native timings of one shape as JSON")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cluster_bench needs a GPU"
    if args.child:
        print(json.dumps(_case(*args.child, routes=(True,))))
        return
    read = None
    if Path(args.stream_bw).exists():
        read = next(r["TB_s"] for r in json.load(open(args.stream_bw))["results"] if r["op"] == "read" and r["variant"] == "rotating-4")
    out = {"device": torch.cuda.get_device_name(0), "method": "same process, alternating, device events, median of 20 after 3 warm-ups",
           "stream_read_TB_s": read, "timings": [], "ab": []}
    for n, d, k in SHAPES:
        for row in _case(n, d, k):
            row["speedup"] = round(row["composition_us"] / row["native_us"], 2)
            row["native_input_GB_s"] = round(n * d * 4 / row["native_us"] / 1e3, 1)
            row["share_of_stream_read"] = round(row["native_input_GB_s"] / (read * 1e3), 3) if read else None
            out["timings"].append(row)
            print(json.dumps(row), flush=True)
    if args.ab:
        for knob, values in (("TMX_CLUSTER_KW", (8, 16, 24)), ("TMX_CLUSTER_TARGET_GROUPS", (512, 2048, 8192))):
            for shape in ((1 << 20, 128, 16), (1 << 20, 16, 1000)):
                for v in values:
                    env = dict(os.environ, **{knob: str(v)})
                    proc = subprocess.run([sys.executable, __file__, "--child", *map(str, shape)], env=env, capture_output=True, text=True, timeout=300)
                    assert proc.returncode == 0, proc.stderr[-2000:]
                    rows = json.loads(proc.stdout.strip().splitlines()[-1])
                    rec = {"knob": knob, "value": v, "shape": list(shape), "native_us": {r["metric"]: r["native_us"] for r in rows}}
                    out["ab"].append(rec)
                    print(json.dumps(rec), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
