#!/usr/bin/env python3
"""keep_unedited on one MI355X against its numpy definition on the host, on the protocol of bench_yuv_io.py: one process, the arms
alternating, medians of --reps repetitions, every arm timed with HIP events on the stream it runs on.

    python tools/bench_keep_unedited.py [--frames 81 33] [--reps 5] [--orig-size 1080 1920] [--log profiles/r08/keep_unedited_ab.log]

Every arm starts with the original clip, the fitted source and the edit on the device (where fit_frames and the pipeline leave them)
and ends with the composited clip on the device.
  (a) keep_unedited on the device: change_mask (3 launches), the edit and alpha resampled to the source window (1 + 2 launches), the
      composite (1 launch)
  (b) the numpy definition on the host (reference_change_mask on the clip, reference_composite_frames frame by frame) plus both
      copies over the link: the three clips into page-locked memory, the result back to the device
  (c) one plain device copy of as many bytes as (a) has to read and write: source, edit and original in, the result out
(a) and (b) end with the same bytes (asserted).  No time is fixed in advance; (c) is the yardstick of (a), `stages` splits (a)."""
import argparse
import json
import os
import sys

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
    ap.add_argument("--orig-size", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_keep_unedited needs a GPU"
    from videocof_amd import ops
    from videocof_amd.video_io import (_device_table, _resize_plan, change_mask, fit_frames, keep_unedited,
                                       reference_change_mask, reference_composite_frames, restore_frames)
    dev = torch.device("cuda:0")
    Ho, Wo = args.orig_size
    lines = []
    for T in args.frames:
        g = torch.Generator().manual_seed(T)
        orig = torch.randint(0, 256, (T, Ho, Wo, 3), generator=g, dtype=torch.uint8).to(dev)
        src, plan = fit_frames(orig)                                                 # 1080 x 1920 runs at 464 x 848
        H, W = plan.out_height, plan.out_width
        edit = (src.int() + torch.randint(-3, 4, src.shape, generator=g).to(dev)).clamp(0, 255).to(torch.uint8)
        edit[:, H // 3:H // 2, W // 4:W // 2] = 255 - src[:, H // 3:H // 2, W // 4:W // 2]          # the "object": 1 / 24 of the frame
        host = [torch.empty(t.shape, dtype=torch.uint8, pin_memory=True) for t in (orig, src, edit)]
        res_host = torch.empty(orig.shape, dtype=torch.uint8, pin_memory=True)

        def arm_a():
            return keep_unedited(orig, src, edit, plan)

        def arm_b(n=T):
            for h, d in zip(host, (orig, src, edit)):
                h[:n].copy_(d[:n], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            alpha = reference_change_mask(host[1][:n], host[2][:n])
            for t in range(n):
                res_host[t] = reference_composite_frames(host[0][t:t + 1], host[2][t:t + 1], alpha[t:t + 1], plan)[0]
            return res_host[:n].to(dev, non_blocking=True)

        nbytes = 2 * src.numel() + 2 * orig.numel()
        c_src, c_dst = (torch.empty(nbytes // 2, device=dev, dtype=torch.uint8) for _ in range(2))

        def arm_c():
            return c_dst.copy_(c_src)

        arms = (("a_device", arm_a), ("b_host", arm_b), ("c_copy", arm_c))
        arm_a(), arm_b(2), arm_c()                                                   # warm-up: allocator, tables, page-locked buffers
        res, last = {k: [] for k, _ in arms}, {}
        for rep in range(args.reps):                                                 # alternating
            for name, fn in arms:
                sec, last[name] = event_seconds(fn)
                res[name].append(round(sec, 6))
            print(f"# T={T} repetition {rep}: " + ", ".join(f"{k} {v[-1]}" for k, v in res.items()), flush=True)
        assert torch.equal(last["a_device"], last["b_host"]), "device and host disagree"

        # ---------------------------------------------------------------- the stages of (a) alone
        y, x, wh, ww = plan.source_window
        alpha = change_mask(src, edit)
        rp = _resize_plan(H, W, wh, ww)
        xtab, kx = _device_table(rp.width, rp.new_width, 0, ww, str(dev))
        ytab, ky = _device_table(rp.height, rp.new_height, 0, wh, str(dev))
        e_up, a_up = restore_frames(edit, wh, ww), ops.plane_u8_resample(alpha, wh, ww, xtab, kx, ytab, ky)
        stages = {"change_mask": kernel_seconds(lambda: change_mask(src, edit)),
                  "restore_frames(edit)": kernel_seconds(lambda: restore_frames(edit, wh, ww)),
                  "plane_u8_resample(alpha)": kernel_seconds(lambda: ops.plane_u8_resample(alpha, wh, ww, xtab, kx, ytab, ky)),
                  "frames_u8_composite": kernel_seconds(lambda: ops.frames_u8_composite(orig, e_up, a_up, (y, x, wh, ww)))}
        ma, mb, mc = med(res["a_device"]), med(res["b_host"]), med(res["c_copy"])
        lines.append(json.dumps({
            "what": f"keep_unedited, {T} frames, original {Ho}x{Wo}, edit {H}x{W}, window {plan.source_window}, default mask arguments, "
                    f"{args.reps} alternating repetitions, seconds by HIP events",
            "seconds": res, "median": {"a_device": ma, "b_host": mb, "c_copy": mc},
            "a_over_b": round(ma / mb, 6), "copy_over_a": round(mc / ma, 3), "bytes_in_and_out": nbytes,
            "a_tbps": round(nbytes / ma / 1e12, 3), "c_tbps": round(nbytes / mc / 1e12, 3),
            "stages_of_a_seconds": {k: round(v, 6) for k, v in stages.items()}}))
        print(lines[-1], flush=True)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
