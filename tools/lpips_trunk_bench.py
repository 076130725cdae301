"""LPIPS VGG16 trunk, layer by layer: ``tmx::conv3x3_relu`` (split-f16 matrix cores) against the channels_last ``nn.Conv2d`` + ReLU
of MIOpen, fp32, the 13 layer shapes of a 1024 x 1024 input at the batch ``_lpips_chunk`` picks for it.

Both routes run in one process, alternating; device events; median of ``--reps`` after ``--warmup``.  FLOP/s are the layer's
``2 · B · H · W · C_out · 9 · C_in`` over the median.  ``err_ratio`` is ``max|native − fp64| / max|MIOpen fp32 − fp64|`` at ``--err-size``.
Every run of the command appends one entry to ``runs`` of the output file, so running it twice shows the run-to-run spread.

    python tools/lpips_trunk_bench.py [--out profiles/lpips_trunk_bench.json] [--size 1024]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from torchmetrics_forked_amd import ops  # noqa: E402
from torchmetrics_forked_amd.functional.image.lpips import _LPIPS, _lpips_chunk  # noqa: E402
from torchmetrics_forked_amd.ops import image as image_ops  # noqa: E402

CL = torch.channels_last


def vgg_layers(size):
    """(name, C_in, C_out, H = W) of the 13 convolutions."""
    cfg = [(1, 3, 64), (1, 64, 64), (2, 64, 128), (2, 128, 128), (3, 128, 256), (3, 256, 256), (3, 256, 256),
           (4, 256, 512), (4, 512, 512), (4, 512, 512), (5, 512, 512), (5, 512, 512), (5, 512, 512)]
    seen = {}
    for stage, c_in, c_out in cfg:
        seen[stage] = seen.get(stage, 0) + 1
        yield f"conv{stage}_{seen[stage]}", c_in, c_out, size >> (stage - 1)


def median_ms(fn_a, fn_b, reps, warmup):
    """Median device time of two callables, run alternately."""
    times = ([], [])
    for i in range(warmup + reps):
        for k, fn in enumerate((fn_a, fn_b)):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            if i >= warmup:
                times[k].append(start.elapsed_time(end))
    return [sorted(t)[len(t) // 2] for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lpips_trunk_bench.json"))
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--err-size", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ops.require()
    torch.manual_seed(0)
    net = _LPIPS(net="vgg", pretrained=False).to(dev)
    batch = min(_lpips_chunk(torch.empty(1, 3, args.size, args.size), net), 256)
    convs = [m for s in net.net.slices for m in s if isinstance(m, torch.nn.Conv2d)]
    rows = []
    with torch.no_grad():
        for (name, c_in, c_out, hw), conv in zip(vgg_layers(args.size), convs):
            conv = conv.to(memory_format=CL)
            planes, shift = image_ops.pack_conv3x3_weights(conv.weight)
            # error against fp64 at a reduced plane (both signs in, the layer's own random weights)
            xs = torch.randn(2, c_in, args.err_size, args.err_size, device=dev).contiguous(memory_format=CL)
            oracle = F.relu(F.conv2d(xs.double(), conv.weight.double(), conv.bias.double(), padding=1))
            err_native = (image_ops.conv3x3_relu(xs, planes, shift, conv.bias)[0].double() - oracle).abs().max().item()
            err_comp32 = (F.relu(conv(xs)).double() - oracle).abs().max().item()
            x = torch.randn(batch, c_in, hw, hw, device=dev).contiguous(memory_format=CL)
            absmax = torch.ops.tmx.conv3x3_absmax(x)
            ms_native, ms_miopen = median_ms(lambda: image_ops.conv3x3_relu(x, planes, shift, conv.bias, absmax),
                                             lambda: conv(x).relu_(), args.reps, args.warmup)
            flop = 2.0 * batch * hw * hw * c_out * 9 * c_in
            rows.append({"layer": name, "c_in": c_in, "c_out": c_out, "hw": hw, "batch": batch,
                         "native_ms": round(ms_native, 3), "miopen_ms": round(ms_miopen, 3),
                         "native_tflops": round(flop / ms_native / 1e9, 1), "miopen_tflops": round(flop / ms_miopen / 1e9, 1),
                         "speedup": round(ms_miopen / ms_native, 3), "err_native": err_native, "err_comp32": err_comp32,
                         "err_ratio": round(err_native / err_comp32, 3) if err_comp32 else None})
            print(json.dumps(rows[-1]), flush=True)
            del x
    run = {"device": torch.cuda.get_device_name(0), "size": args.size, "reps": args.reps, "warmup": args.warmup, "layers": rows,
           "trunk_native_ms": round(sum(r["native_ms"] for r in rows), 2), "trunk_miopen_ms": round(sum(r["miopen_ms"] for r in rows), 2)}
    doc = {"runs": []}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc["runs"].append(run)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps({k: v for k, v in run.items() if k != "layers"}), flush=True)


if __name__ == "__main__":
    main()
