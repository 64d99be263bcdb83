#!/usr/bin/env python
"""Time the clip fit (wan_frames_u8_resample) on one GPU against what a user has today.  One process, the arms alternating,
medians of 5 runs, HIP events around each arm (arm c, which works on the host, by a host clock around a device synchronise).

    a  video_io.fit_frames: the kernel, one launch
    b  the same fit with torch's own kernels on the device: uint8 -> float, F.interpolate(mode="bilinear", antialias=True),
       crop, round, -> uint8
    c  Pillow per frame on the host (skipped where Pillow is not importable) + the host -> device copy of the result
    d  a plain device copy of as many bytes as the kernel reads + writes: the ceiling of a streaming kernel

Shapes: 81 and 33 frames of 1080 x 1920 -> fit_size, and of 480 x 854 -> 464 x 848.  Prints one JSON line per shape.
"""
import argparse
import json
import statistics
import sys
import time
import os

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videocof_amd import video_io  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="*", default=[81, 33])
    ap.add_argument("--no-pillow", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frame_fit needs a GPU"
    dev = torch.device("cuda", 0)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if args.no_pillow:
        Image = None
    for T in args.frames:
        for (h, w) in ((1080, 1920), (480, 854)):
            oh, ow = video_io.fit_size(h, w)
            plan = video_io.fit_plan(h, w, oh, ow)
            host = torch.randint(0, 256, (T, h, w, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
            fr = host.to(dev)
            moved = fr.numel() + T * oh * ow * 3                   # bytes the kernel reads + writes (each source byte once)
            cp_src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            cp_dst = torch.empty_like(cp_src)

            def arm_a():
                return video_io.fit_frames(fr, oh, ow)[0]

            def arm_b():
                x = fr.permute(0, 3, 1, 2).float()
                y = torch.nn.functional.interpolate(x, size=(plan.new_height, plan.new_width), mode="bilinear", antialias=True,
                                                    align_corners=False)
                y = y[:, :, plan.y0:plan.y0 + oh, plan.x0:plan.x0 + ow]
                return y.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

            def arm_c():
                a = host.numpy()
                out = np.stack([np.asarray(Image.fromarray(a[t]).resize((plan.new_width, plan.new_height), Image.BILINEAR))
                                [plan.y0:plan.y0 + oh, plan.x0:plan.x0 + ow] for t in range(T)])
                return torch.from_numpy(out).to(dev)

            def arm_d():
                return cp_dst.copy_(cp_src)

            arms = {"a_kernel": (event_ms, arm_a), "b_torch": (event_ms, arm_b), "d_copy": (event_ms, arm_d)}
            if Image is not None:
                arms["c_pillow_host"] = (host_ms, arm_c)
            times = {k: [] for k in arms}
            outs = {}
            for k, (_, fn) in arms.items():                        # warm up every arm at this shape
                if k != "c_pillow_host":
                    outs[k] = fn()
            torch.cuda.synchronize()
            for _ in range(args.runs):                             # alternate the arms
                for k, (clock, fn) in arms.items():
                    ms, outs[k] = clock(fn)
                    times[k].append(ms)
            med = {k: statistics.median(v) for k, v in times.items()}
            diff_b = (outs["a_kernel"].int() - outs["b_torch"].int()).abs()
            res = {"frames": T, "src": [h, w], "dst": [oh, ow], "taps": None, "runs": args.runs,
                   "ms_median": {k: round(v, 4) for k, v in med.items()},
                   "ms_all": {k: [round(x, 4) for x in v] for k, v in times.items()},
                   "bytes_moved": moved, "kernel_tbps": round(moved / med["a_kernel"] / 1e9, 3),
                   "copy_tbps": round(moved / med["d_copy"] / 1e9, 3),
                   "kernel_fraction_of_copy": round(med["d_copy"] / med["a_kernel"], 3),
                   "torch_over_kernel": round(med["b_torch"] / med["a_kernel"], 2),
                   "max_abs_diff_vs_torch_float": int(diff_b.max()), "differing_vs_torch_float": float((diff_b > 0).float().mean())}
            if "c_pillow_host" in outs:
                res["equal_to_pillow"] = bool(torch.equal(outs["a_kernel"], outs["c_pillow_host"]))
                res["pillow_over_kernel"] = round(med["c_pillow_host"] / med["a_kernel"], 1)
            del res["taps"]
            print(json.dumps(res), flush=True)
            del fr, cp_src, cp_dst, outs


if __name__ == "__main__":
    main()
