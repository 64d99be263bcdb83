#!/usr/bin/env python3
"""YCbCr 4:2:0 planes in and out on one MI355X against the host conversion, on the protocol of bench_e2e.py --io-only: one process,
the two arms alternating, medians of --reps repetitions, synchronised wall seconds per arm, each kernel alone with HIP events.

    python tools/bench_yuv_io.py [--frames 81 33] [--reps 5] [--in-size 1080 1920] [--out-size 480 832] [--log profiles/r07/yuv_io_ab.log]

  in   (a) the 4:2:0 planes of the clip in page-locked host memory -> one copy (1.5 bytes per pixel) -> yuv_to_frames on the device
       (b) reference_yuv_to_frames on the host (numpy, frame by frame) -> one copy of the RGB frames (3 bytes per pixel)
  out  (a) RGB frames on the device -> frames_to_yuv -> one copy of the planes into page-locked memory
       (b) one copy of the RGB frames into page-locked memory -> reference_frames_to_yuv on the host
Both arms of a pair end with the same bytes in the same place (asserted).  No time is fixed in advance: arm (b) in the same process is
the yardstick.  `kernel` reports the two kernels alone as (bytes read + written) per second next to a plain device copy that moves
the same number of bytes."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def kernel_seconds(fn, iters=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters / 1e3


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[81, 33])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--in-size", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--out-size", type=int, nargs=2, default=[480, 832])
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from videocof_amd.video_io import (_plane_views, frames_to_yuv, reference_frames_to_yuv, reference_yuv_to_frames, y4m_frame_bytes,
                                       yuv_to_frames)
    dev = torch.device("cuda:0")
    lines = []
    for T in args.frames:
        # ---------------------------------------------------------------- in
        H, W = args.in_size
        matrix = "bt709" if H >= 720 else "bt601"
        fb = y4m_frame_bytes(H, W, "420jpeg")
        planes_host = torch.empty(T, fb, dtype=torch.uint8, pin_memory=True)
        planes_host.random_(0, 256, generator=torch.Generator().manual_seed(T))
        rgb_host = torch.empty(T, H, W, 3, dtype=torch.uint8, pin_memory=True)
        hy, hcb, hcr = _plane_views(planes_host, H, W, "420jpeg")

        def in_a():
            y, cb, cr = _plane_views(planes_host.to(dev, non_blocking=True), H, W, "420jpeg")
            return yuv_to_frames(y, cb, cr, chroma="420jpeg", matrix=matrix)

        def in_b():
            for t in range(T):
                rgb_host[t] = reference_yuv_to_frames(hy[t:t + 1], hcb[t:t + 1], hcr[t:t + 1], chroma="420jpeg", matrix=matrix)[0]
            return rgb_host.to(dev, non_blocking=True)

        # ---------------------------------------------------------------- out
        Ho, Wo = args.out_size
        mo = "bt709" if Ho >= 720 else "bt601"
        fbo = y4m_frame_bytes(Ho, Wo, "420jpeg")
        edit = torch.randint(0, 256, (T, Ho, Wo, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(T + 1)).to(dev)
        out_planes = torch.empty(T, fbo, dtype=torch.uint8, pin_memory=True)
        out_rgb = torch.empty(T, Ho, Wo, 3, dtype=torch.uint8, pin_memory=True)
        out_ref = torch.empty(T, fbo, dtype=torch.uint8)

        def out_a():
            buf, _ = frames_to_yuv(edit, chroma="420jpeg", matrix=mo)
            out_planes.copy_(buf, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            return out_planes

        def out_b():
            out_rgb.copy_(edit, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            for t in range(T):
                out_ref[t] = torch.cat([p.reshape(-1) for p in reference_frames_to_yuv(out_rgb[t:t + 1], chroma="420jpeg", matrix=mo)])
            return out_ref

        arms = (("in_a", in_a), ("in_b", in_b), ("out_a", out_a), ("out_b", out_b))
        res = {k: [] for k, _ in arms}
        for _, fn in arms:
            fn()                                                 # warm-up: allocator, page-locked buffers
        for _ in range(args.reps):                               # alternating
            for name, fn in arms:
                res[name].append(round(wall(fn)[0], 5))
        assert torch.equal(in_a(), in_b()), "the two ways in disagree"
        assert torch.equal(out_a(), out_b()), "the two ways out disagree"

        # ---------------------------------------------------------------- the kernels alone
        pd = planes_host.to(dev)
        y, cb, cr = _plane_views(pd, H, W, "420jpeg")
        rgb_dev = torch.empty(T, H, W, 3, device=dev, dtype=torch.uint8)
        k_in = kernel_seconds(lambda: yuv_to_frames(y, cb, cr, chroma="420jpeg", matrix=matrix, out=rgb_dev))
        n_in = T * (fb + H * W * 3)
        a, b = torch.empty(n_in // 2, device=dev, dtype=torch.uint8), torch.empty(n_in // 2, device=dev, dtype=torch.uint8)
        c_in = kernel_seconds(lambda: b.copy_(a))
        k_out = kernel_seconds(lambda: frames_to_yuv(edit, chroma="420jpeg", matrix=mo))
        n_out = T * (fbo + Ho * Wo * 3)
        a, b = torch.empty(n_out // 2, device=dev, dtype=torch.uint8), torch.empty(n_out // 2, device=dev, dtype=torch.uint8)
        c_out = kernel_seconds(lambda: b.copy_(a))
        lines.append(json.dumps({
            "what": f"YCbCr 4:2:0 I/O, {T} frames, in {H}x{W} ({matrix}), out {Ho}x{Wo} ({mo}), {args.reps} alternating repetitions, "
                    "wall seconds", "seconds": res, "median": {k: med(v) for k, v in res.items()},
            "speedup_median": {"in": round(med(res["in_b"]) / med(res["in_a"]), 2), "out": round(med(res["out_b"]) / med(res["out_a"]), 2)},
            "link_bytes": {"in_a": T * fb, "in_b": T * H * W * 3, "out_a": T * fbo, "out_b": T * Ho * Wo * 3},
            "kernel": {"wan_yuv_to_frames_u8": {"seconds": round(k_in, 7), "tbps": round(n_in / k_in / 1e12, 3),
                                                "device_copy_same_bytes_tbps": round(n_in / c_in / 1e12, 3)},
                       "wan_frames_u8_to_yuv": {"seconds": round(k_out, 7), "tbps": round(n_out / k_out / 1e12, 3),
                                                "device_copy_same_bytes_tbps": round(n_out / c_out / 1e12, 3)}}}))
        print(lines[-1], flush=True)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
