"""Inception-v3 trunk of FID / KID / IS / MiFID, layer class by layer class and as a whole: ``tmx::conv_bn_relu`` (split-f16 matrix cores,
folded batch norm) against the channels_last ``nn.Conv2d`` + ``BatchNorm2d`` + ``relu`` of MIOpen it replaces, fp32.

A layer class is one (taps, padding, C_in, C_out, plane) of the stride-1 convolutions; the planes are those of a 299 x 299 input, the
batch is ``--batch`` images (64: a realistic ``update``).  Both routes run in one process, alternating; device events; median of
``--reps`` after ``--warmup``.  ``err_ratio`` is ``max|native − fp64| / max|MIOpen fp32 − fp64|`` on two images of the class's shape.
The whole ``_taps`` call is timed native against the route of ``TMX_INCEPTION_TRUNK_NATIVE=0`` (the gate's flag set to that value here,
which is the parent commit's route) on a module whose weights are as its constructor makes them (contiguous, NCHW).  Every run of the
command appends one entry to ``runs`` of the output file, so running it twice shows the run-to-run spread.

    python tools/inception_trunk_bench.py [--out profiles/inception_trunk_bench.json] [--batch 64]
"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from torchmetrics_forked_amd import ops  # noqa: E402
from torchmetrics_forked_amd.models import inception  # noqa: E402
from torchmetrics_forked_amd.ops import image as image_ops  # noqa: E402

CL = torch.channels_last


def layer_classes(net):
    """{(taps, padding, C_in, C_out, H, W): (first module of the class, count)} of the stride-1 layers, from one forward on the CPU."""
    seen, hooks = {}, []

    def hook(m, args):
        c = m.conv
        if c.stride == (1, 1):
            key = (c.kernel_size, c.padding, c.in_channels, c.out_channels, args[0].shape[2], args[0].shape[3])
            seen[key] = (seen[key][0] if key in seen else m, seen.get(key, (None, 0))[1] + 1)

    for m in net.modules():
        if isinstance(m, inception.BasicConv2d):
            hooks.append(m.register_forward_pre_hook(hook))
    net(torch.zeros(1, 3, 299, 299, dtype=torch.uint8))
    for h in hooks:
        h.remove()
    return seen


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "inception_trunk_bench.json"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ops.require()
    torch.manual_seed(0)
    net = inception.FeatureExtractorInceptionV3(["2048"])
    for m in net.modules():  # statistics that keep a random trunk's activations near one
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_var.uniform_(0.1, 0.3)
            m.running_mean.normal_(0, 0.1)
    classes = layer_classes(net)
    net = net.to(dev)  # weights stay as the constructor makes them (contiguous): the whole-call rows time a user's module
    rows = []
    with torch.no_grad():
        for (taps, pad, c_in, c_out, h, w), (m, count) in classes.items():
            m = copy.deepcopy(m).to(memory_format=CL)  # the channels_last layer the native one replaces; the trunk's own stays as it is
            bn = m.bn
            packed = image_ops.pack_conv_bn_weights(m.conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
            xs = torch.randn(2, c_in, h, w, device=dev).contiguous(memory_format=CL)
            g = (bn.weight.double() / (bn.running_var.double() + bn.eps).sqrt()).reshape(1, -1, 1, 1)
            oracle = F.relu((F.conv2d(xs.double(), m.conv.weight.double(), padding=pad) - bn.running_mean.double().reshape(1, -1, 1, 1)) * g
                            + bn.bias.double().reshape(1, -1, 1, 1))
            err_native = (image_ops.conv_bn_relu(xs, *packed, taps, pad)[0].double() - oracle).abs().max().item()
            err_comp32 = (m(xs).double() - oracle).abs().max().item()
            x = torch.randn(args.batch, c_in, h, w, device=dev).contiguous(memory_format=CL)
            absmax = torch.ops.tmx.conv3x3_absmax(x)
            out = torch.empty_like(m(x))
            omax = torch.zeros(args.batch, device=dev)
            ms_native, ms_miopen = median_ms(lambda: image_ops.conv_bn_relu(x, *packed, taps, pad, absmax, out, omax), lambda: m(x),
                                             args.reps, args.warmup)
            flop = 2.0 * args.batch * out.shape[2] * out.shape[3] * c_out * taps[0] * taps[1] * c_in
            rows.append({"taps": list(taps), "pad": list(pad), "c_in": c_in, "c_out": c_out, "hw": [h, w], "layers": count, "batch": args.batch,
                         "native_ms": round(ms_native, 4), "miopen_ms": round(ms_miopen, 4),
                         "native_tflops": round(flop / ms_native / 1e9, 1), "miopen_tflops": round(flop / ms_miopen / 1e9, 1),
                         "speedup": round(ms_miopen / ms_native, 3), "err_native": err_native, "err_comp32": err_comp32,
                         "err_ratio": round(err_native / err_comp32, 3) if err_comp32 else None})
            print(json.dumps(rows[-1]), flush=True)
            del x, out
        imgs = torch.randint(0, 256, (args.batch, 3, 299, 299), dtype=torch.uint8, device=dev)

        def route(native):
            inception._TRUNK_NATIVE = native
            return net._taps(imgs)[0]

        diff = (route(True) - route(False)).abs().max().item()
        ms_native, ms_parent = median_ms(lambda: route(True), lambda: route(False), args.reps, args.warmup)
        inception._TRUNK_NATIVE = True
    run = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "reps": args.reps, "warmup": args.warmup, "classes": rows,
           "layers_native_ms": round(sum(r["native_ms"] * r["layers"] for r in rows), 2),
           "layers_miopen_ms": round(sum(r["miopen_ms"] * r["layers"] for r in rows), 2),
           "taps_native_ms": round(ms_native, 2), "taps_parent_route_ms": round(ms_parent, 2), "taps_speedup": round(ms_parent / ms_native, 3),
           "taps_max_abs_diff_2048": diff}
    doc = {"runs": []}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc["runs"].append(run)
    with open(args.out, "w") as fh:  # one layer class per line
        runs = []
        for r in doc["runs"]:
            head = json.dumps({k: v for k, v in r.items() if k != "classes"})
            runs.append(head[:-1] + ', "classes": [\n' + ",\n".join("  " + json.dumps(c) for c in r["classes"]) + "\n ]}")
        fh.write('{"runs": [\n ' + ",\n ".join(runs) + "\n]}\n")
    print(json.dumps({k: v for k, v in run.items() if k != "classes"}), flush=True)


if __name__ == "__main__":
    main()
