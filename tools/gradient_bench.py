"""``total_variation``, ``image_gradients`` and ``peak_signal_noise_ratio_with_blocked_effect`` (functional, and one ``update`` of the module) on
``[B, C, H, W]``, fp32, no autograd: the native route (``tmx::tv_sums`` / ``tmx::image_gradients`` / ``tmx::psnrb_sums``, ``csrc/neighbour_diff.hip``) against
the composition in the same process, alternating call by call (the gates' module flag ``_GRADIENT_NATIVE`` is switched between the
calls; ``TMX_GRADIENT_NATIVE=0`` sets it for a whole process).  Device events around the whole call, median of ``--reps`` repeats after
``--warmup`` warm-ups of each route; peak allocated memory of one call.

    python tools/gradient_bench.py --out profiles/gradient_bench.json [--kernel-trace CSV]
    python tools/gradient_bench.py --profile-run    # a few native op calls per shape, for a ``rocprofv3 --kernel-trace --stats`` run

``--kernel-trace``: the ``kernel_trace`` CSV of such a run; adds each streaming kernel's time per shape and its bytes over time against
``--hbm-tb-s`` (the read rate of ``profiles/stream_bw_mi355x_r4.json``).
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGE_SHAPES = ["16x3x256x256", "8x3x512x512", "4x3x1024x1024", "32x1x41x41"]
PSNRB_SHAPES = ["16x1x256x256", "4x1x1024x1024", "64x1x1024x1024", "32x1x41x41"]
BLOCK_SIZE = 8
CASES = [("tv", IMAGE_SHAPES), ("gradients", IMAGE_SHAPES), ("psnrb", PSNRB_SHAPES), ("psnrb_update", PSNRB_SHAPES)]
PROFILE_CALLS = 5
# op -> (kernel name, shapes, bytes read and written per element)
PROFILE_OPS = {"tv_sums": ("tv_vec_kernel", IMAGE_SHAPES, 4), "image_gradients": ("gradients_vec_kernel", IMAGE_SHAPES, 12),
               "psnrb_sums": ("psnrb_vec_kernel", PSNRB_SHAPES, 8)}


def _parse_shape(s):
    return tuple(int(v) for v in s.split("x"))


def _inputs(shape):
    import torch

    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.rand(*shape, device="cuda", generator=g)
    p = t + 0.1 * torch.randn(*shape, device="cuda", generator=g)
    return p, t


def _set_route(native):
    import torchmetrics_forked_amd.functional.image.gradients as grad_mod
    import torchmetrics_forked_amd.functional.image.psnrb as psnrb_mod
    import torchmetrics_forked_amd.functional.image.tv as tv_mod

    for mod in (grad_mod, psnrb_mod, tv_mod):
        mod._GRADIENT_NATIVE = native


def _make_step(case, p, t):
    from torchmetrics_forked_amd.functional.image.gradients import image_gradients
    from torchmetrics_forked_amd.functional.image.psnrb import peak_signal_noise_ratio_with_blocked_effect as psnrb
    from torchmetrics_forked_amd.functional.image.tv import total_variation
    from torchmetrics_forked_amd.image import PeakSignalNoiseRatioWithBlockedEffect

    if case == "tv":
        return lambda: total_variation(p)
    if case == "gradients":
        return lambda: image_gradients(p)[0]
    if case == "psnrb":
        return lambda: psnrb(p, t, block_size=BLOCK_SIZE)
    metric = PeakSignalNoiseRatioWithBlockedEffect(block_size=BLOCK_SIZE).cuda()

    def update():
        metric.update(p, t)
        return metric.sum_squared_error

    return update


def _timed(step):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = step()
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def _peak_bytes(step):
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = step()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def run(reps, warmup):
    import torch

    from torchmetrics_forked_amd import ops

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ops.require()
    rows = []
    for case, shapes in CASES:
        for shape in shapes:
            p, t = _inputs(_parse_shape(shape))
            steps = {"native": _make_step(case, p, t), "composition": _make_step(case, p, t)}
            times, value, peak = {"native": [], "composition": []}, {}, {}
            for i in range(warmup + reps):
                for route in ("native", "composition"):  # alternating, call by call
                    _set_route(route == "native")
                    ms, out = _timed(steps[route])
                    if i >= warmup:
                        times[route].append(ms)
                    if case != "psnrb_update":
                        value[route] = float(out.double().mean())
            for route in ("native", "composition"):
                _set_route(route == "native")
                peak[route] = _peak_bytes(steps[route])
            _set_route(True)
            n, c = statistics.median(times["native"]), statistics.median(times["composition"])
            row = {"case": case, "shape": shape, "input_bytes": (1 if case in ("tv", "gradients") else 2) * p.numel() * p.element_size(),
                   "native_ms": round(n, 4), "native_ms_min_max": [round(min(times["native"]), 4), round(max(times["native"]), 4)],
                   "composition_ms": round(c, 4), "composition_ms_min_max": [round(min(times["composition"]), 4), round(max(times["composition"]), 4)],
                   "native_peak_bytes": peak["native"], "composition_peak_bytes": peak["composition"], "speedup": round(c / n, 2),
                   "native_below_composition": n < c}
            if value:
                row["rel_diff"] = abs(value["native"] - value["composition"]) / max(abs(value["composition"]), 1e-30)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del p, t, steps
            torch.cuda.empty_cache()
    return rows, torch.cuda.get_device_name(0)


def profile_run():
    import torch

    from torchmetrics_forked_amd import ops
    from torchmetrics_forked_amd.ops import image

    ops.require()
    for op, (_, shapes, _) in PROFILE_OPS.items():
        for shape in shapes:
            p, t = _inputs(_parse_shape(shape))
            for _ in range(PROFILE_CALLS):
                image.psnrb_sums(p, t, BLOCK_SIZE) if op == "psnrb_sums" else getattr(image, op)(p)
            torch.cuda.synchronize()


def kernel_times(path, hbm_tb_s):
    """Per (op, shape) the streaming kernel's median time of ``--profile-run``: its dispatches appear in call order."""
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    out = {"what": f"rocprofv3 --kernel-trace --stats of --profile-run ({PROFILE_CALLS} calls of each op per shape, fp32), a run of its own; median "
                   "kernel time, bytes read and written / time against the HBM read rate (the calls re-read the same inputs, which the 256 MiB "
                   "Infinity Cache holds in full or in part: figures above the read rate are cache-assisted, not HBM rates)",
           "hbm_read_tb_per_s": hbm_tb_s, "kernels": []}
    for op, (name, shapes, bytes_per_element) in PROFILE_OPS.items():
        hits = [r for r in rows if name in r["Kernel_Name"]]
        vec_shapes = [s for s in shapes if _parse_shape(s)[3] % 4 == 0]  # the other planes run the generic kernel
        generic = [r for r in rows if name.replace("_vec_", "_generic_") in r["Kernel_Name"]]
        if len(hits) != PROFILE_CALLS * len(vec_shapes) or len(generic) != PROFILE_CALLS * (len(shapes) - len(vec_shapes)):
            out["kernels"].append({"op": op, "error": f"expected {PROFILE_CALLS * len(vec_shapes)} dispatches of {name}, found {len(hits)}"})
            continue
        for kernel, subset, found in ((name, vec_shapes, hits), (name.replace("_vec_", "_generic_"), [s for s in shapes if s not in vec_shapes], generic)):
            for i, shape in enumerate(subset):
                us = statistics.median((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in found[i * PROFILE_CALLS:(i + 1) * PROFILE_CALLS])
                b, c, h, w = _parse_shape(shape)
                moved = bytes_per_element * b * c * h * w
                tb_s = moved / (us * 1e-6) / 1e12
                out["kernels"].append({"op": op, "kernel": kernel, "shape": shape, "median_us": round(us, 2), "bytes": moved,
                                       "tb_per_s": round(tb_s, 3), "fraction_of_hbm_read_rate": round(tb_s / hbm_tb_s, 3)})
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
    rows, device = run(args.reps, args.warmup)
    out = {"what": "total_variation(img), image_gradients(img), peak_signal_noise_ratio_with_blocked_effect(p, t, 8) and one "
                   "PeakSignalNoiseRatioWithBlockedEffect(8).update(p, t), fp32, no autograd: the whole call, ms (median); native and "
                   "composition alternate call by call in one process",
           "device": device, "reps": args.reps, "warmup": args.warmup, "timings": rows,
           "native_below_composition_at_every_shape": all(r["native_below_composition"] for r in rows)}
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
