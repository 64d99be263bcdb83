#!/usr/bin/env python3
"""clip_stats on one MI355X against its numpy definition on the host, on the protocol of bench_keep_unedited.py: one process, the arms
alternating, medians of --reps repetitions, every arm timed with HIP events on the stream it runs on.

    python tools/bench_clip_stats.py [--frames 81 33] [--reps 5] [--size 480 832] [--log profiles/r09/clip_stats_ab.log]

Every arm starts with the two clips (and alpha) on the device, where the pipeline, fit_frames / restore_frames and change_mask leave
them.
  (a)  clip_stats on the device, without and with alpha: four launches and one copy of T * 2 * 514 words to the host
  (b)  reference_clip_stats on the host with alpha, plus the copies of both clips and alpha over the link into page-locked memory
  (c)  one plain device copy of as many bytes as (a) has to read: both clips.  The traffic floor of (a) is the read half of it.
(a) and (b) end with the same words (asserted).  No time is fixed in advance; (c) is the yardstick of (a).  `launches` times the
device work of (a) without the copy to the host, and change_mask's three launches on the same clips beside it."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_seconds(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3, r


def kernel_seconds(fn, iters=10):
    for _ in range(2):
        fn()
    return event_seconds(lambda: [fn() for _ in range(iters)])[0] / iters


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[81, 33])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=[480, 832])
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clip_stats needs a GPU"
    from videocof_amd import ops
    from videocof_amd.video_io import change_mask, clip_stats, reference_clip_stats
    dev = torch.device("cuda:0")
    H, W = args.size
    fields = ("diff_hist", "smooth_hist", "ssim_sum", "ssim_windows")
    lines = []
    for T in args.frames:
        g = torch.Generator().manual_seed(T)
        src = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        edit = (src.int() + torch.randint(-3, 4, src.shape, generator=g).to(dev)).clamp(0, 255).to(torch.uint8)
        edit[:, H // 3:H // 2, W // 4:W // 2] = 255 - src[:, H // 3:H // 2, W // 4:W // 2]          # the "object": 1 / 24 of the frame
        alpha = change_mask(src, edit)
        host = [torch.empty(t.shape, dtype=torch.uint8, pin_memory=True) for t in (src, edit, alpha)]

        def arm_a():
            return clip_stats(src, edit)

        def arm_a_alpha():
            return clip_stats(src, edit, alpha)

        def arm_b(n=T):
            for h, d in zip(host, (src, edit, alpha)):
                h[:n].copy_(d[:n], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            return reference_clip_stats(host[0][:n], host[1][:n], host[2][:n])

        nbytes = 2 * src.numel()
        c_src, c_dst = (torch.empty(nbytes, device=dev, dtype=torch.uint8) for _ in range(2))

        def arm_c():
            return c_dst.copy_(c_src)

        arms = (("a_device", arm_a), ("a_device_alpha", arm_a_alpha), ("b_host_alpha", arm_b), ("c_copy", arm_c))
        arm_a(), arm_a_alpha(), arm_b(2), arm_c()                                    # warm-up: allocator, page-locked buffers
        res, last = {k: [] for k, _ in arms}, {}
        for rep in range(args.reps):                                                 # alternating
            for name, fn in arms:
                sec, last[name] = event_seconds(fn)
                res[name].append(round(sec, 6))
            print(f"# T={T} repetition {rep}: " + ", ".join(f"{k} {v[-1]}" for k, v in res.items()), flush=True)
        for f in fields:
            assert np.array_equal(getattr(last["a_device_alpha"], f), getattr(last["b_host_alpha"], f)), f"device and host disagree in {f}"

        s5, e5, a5 = src[None], edit[None], alpha[None]
        out = torch.empty(1, T, 2, ops.CLIP_STATS_WORDS, device=dev, dtype=torch.int64)
        launches = {"clip_stats": kernel_seconds(lambda: ops.clip_stats(s5, e5, None, 2, out=out)),
                    "clip_stats_alpha": kernel_seconds(lambda: ops.clip_stats(s5, e5, a5, 2, out=out)),
                    "change_mask": kernel_seconds(lambda: change_mask(src, edit)),
                    "copy": kernel_seconds(arm_c)}
        m = {k: med(v) for k, v in res.items()}
        st = last["a_device_alpha"]
        lines.append(json.dumps({
            "what": f"clip_stats, {T} frames of {H}x{W}, smooth 2, alpha = change_mask's defaults, {args.reps} alternating repetitions, "
                    f"seconds by HIP events",
            "seconds": res, "median": m, "a_over_b": round(m["a_device_alpha"] / m["b_host_alpha"], 6),
            "copy_over_a": round(m["c_copy"] / m["a_device"], 3), "input_bytes": nbytes,
            "a_read_tbps": round(nbytes / m["a_device"] / 1e12, 3), "c_read_plus_write_tbps": round(2 * nbytes / m["c_copy"] / 1e12, 3),
            "launches_only_seconds": {k: round(v, 6) for k, v in launches.items()},
            "launches_read_tbps": {k: round(nbytes / launches[k] / 1e12, 3) for k in ("clip_stats", "clip_stats_alpha")},
            "result": {"psnr_db": [round(float(st.psnr(r, False)), 3) for r in (0, 1)],
                       "ssim": [round(float(st.ssim(r, False)), 5) for r in (0, 1)], "threshold_for": st.threshold_for(region=0)}}))
        print(lines[-1], flush=True)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
