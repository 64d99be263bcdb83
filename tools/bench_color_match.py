#!/usr/bin/env python3
"""color_match's three kernels on one MI355X, on the protocol of bench_clip_stats.py: one process, warm, the arms alternating, every
arm timed with HIP events on the stream it runs on, the MINIMUM of --reps repetitions (each the mean of --iters back-to-back calls).

    python tools/bench_color_match.py [--frames 81] [--sizes 480x832 1080x1920] [--reps 7] [--log profiles/r19/color_match_ab.log]

Every arm starts with the source frames, the edit and alpha on the device, where the pipeline leaves them.
  stats, stats_alpha   wan_color_stats without and with alpha (two launches): both clips are read once
  coef                 wan_color_coef (one launch, T * 3 threads)
  affine, affine_inpl  wan_frames_u8_affine out of place and in place: the clip read once and written once
  affine_lut           the form that was not kept, a 256-entry table per channel in LDS (tools/color_affine_lut.hip, compiled here with
                       hipcc into build/ unless it is there already), asserted equal to `affine` byte for byte
  copy_2, copy_1       a plain device copy of both clips' bytes (the yardstick of stats: its read half is the traffic floor) and of
                       one clip's (the yardstick of affine: the same bytes read and written)
  host                 reference_color_match in numpy / Python ints on the host, with the copies of the clips over the link into
                       page-locked memory and of the result back (--host-reps repetitions, the first --host-frames frames only at
                       sizes above 480x832; asserted equal to the device's result on the same frames)
No ratio is fixed in advance."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_seconds(fn, iters=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / iters, r


def lut_library():
    so, src = os.path.join(ROOT, "build", "color_affine_lut.so"), os.path.join(ROOT, "tools", "color_affine_lut.hip")
    if not os.path.isfile(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-fno-honor-nans", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "videocof_amd", "csrc"), src,
                        "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.color_affine_lut.restype = ctypes.c_int
    lib.color_affine_lut.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=81)
    ap.add_argument("--sizes", nargs="+", default=["480x832", "1080x1920"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-frames", type=int, default=17, help="frames of the host arm at sizes above 480x832")
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_color_match needs a GPU"
    from videocof_amd import ops
    from videocof_amd.video_io import color_match, reference_color_match
    dev, T = torch.device("cuda:0"), args.frames
    lut = lut_library()
    lines = []
    for size in args.sizes:
        H, W = (int(v) for v in size.split("x"))
        g = torch.Generator().manual_seed(H)
        src = torch.randint(0, 256, (1, T, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        # the edit: the source under a gain and offset that wobble from frame to frame, +-2 of noise, one repainted block under alpha
        gain = (0.9 + 0.2 * torch.rand(T, 1, 1, 3, generator=g)).to(dev)
        edit = (src.float() * gain + 8 * torch.rand(T, 1, 1, 3, generator=g).to(dev) - 4).round_()
        edit = (edit + torch.randint(-2, 3, (T, H, W, 3), generator=g).to(dev)).clamp_(0, 255).to(torch.uint8)
        alpha = torch.zeros(1, T, H, W, dtype=torch.uint8, device=dev)
        alpha[:, :, H // 3:H // 2, W // 4:W // 2] = 255
        edit[:, :, H // 3:H // 2, W // 4:W // 2] = 255 - src[:, :, H // 3:H // 2, W // 4:W // 2]
        N, nbytes = T, src.numel()
        stats = torch.empty(1, T, ops.COLOR_STATS_WORDS, device=dev, dtype=torch.int64)
        coef = torch.empty(1, T, 3, 2, device=dev, dtype=torch.int32)
        flat, out, out_lut, inpl = edit.view(N, H, W, 3), torch.empty(N, H, W, 3, device=dev, dtype=torch.uint8), \
            torch.empty(N, H, W, 3, device=dev, dtype=torch.uint8), edit.view(N, H, W, 3).clone()
        c2_src, c2_dst = (torch.empty(2 * nbytes, device=dev, dtype=torch.uint8) for _ in range(2))
        stream = torch.cuda.current_stream().cuda_stream
        host = [torch.empty(t.shape, dtype=torch.uint8, pin_memory=True) for t in (src, edit, alpha)]
        back = torch.empty(edit.shape, dtype=torch.uint8, pin_memory=True)

        def arm_lut():
            assert lut.color_affine_lut(flat.data_ptr(), coef.data_ptr(), out_lut.data_ptr(), N, H, W, stream) == 0

        def arm_host(n=T):
            for h, d in zip(host, (src, edit, alpha)):
                h[:, :n].copy_(d[:, :n], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            res = reference_color_match(host[1][:, :n], host[0][:, :n], host[2][:, :n])
            back[:, :n].copy_(res)
            return res

        arms = (("stats", lambda: ops.color_stats(src, edit, None, out=stats)),
                ("stats_alpha", lambda: ops.color_stats(src, edit, alpha, out=stats)),
                ("coef", lambda: ops.color_coef(stats, 2, True, 1024, out=coef)),
                ("affine", lambda: ops.frames_u8_affine(flat, coef.view(N, 3, 2), out=out)),
                ("affine_inpl", lambda: ops.frames_u8_affine(inpl, coef.view(N, 3, 2), out=inpl)),
                ("affine_lut", arm_lut),
                ("copy_2", lambda: c2_dst.copy_(c2_src)),
                ("copy_1", lambda: c2_dst[:nbytes].copy_(c2_src[:nbytes])))
        for _, fn in arms:                                                           # warm-up: code objects, allocator
            fn(), fn()
        arm_host(2)
        assert torch.equal(out, out_lut), "the LDS-table form and the product kernel disagree"
        res = {k: [] for k, _ in arms}
        for rep in range(args.reps):                                                 # alternating
            for name, fn in arms:
                res[name].append(round(event_seconds(fn, args.iters)[0], 7))
            print(f"# {size} repetition {rep}: " + ", ".join(f"{k} {v[-1]}" for k, v in res.items()), flush=True)
        whole = [round(event_seconds(lambda: color_match(edit, src, alpha))[0], 6) for _ in range(args.reps)]
        host_s, want = [], None
        n_host = T if H * W <= 480 * 832 else min(T, args.host_frames)              # the definition holds the clip in int64 several times
        for _ in range(args.host_reps):
            sec, want = event_seconds(lambda: arm_host(n_host))
            host_s.append(round(sec, 4))
        assert torch.equal(color_match(edit[:, :n_host], src[:, :n_host], alpha[:, :n_host]).cpu(), want), "device and host disagree"
        m = {k: min(v) for k, v in res.items()}
        lines.append(json.dumps({
            "what": f"color_match, {T} frames of {H}x{W}, alpha = one block of 1/24 of the frame, pool_t 2; minimum of {args.reps} "
                    f"alternating repetitions of {args.iters} calls, seconds per call by HIP events",
            "seconds": res, "min": m, "clip_bytes": nbytes,
            "stats_over_copy_2": round(m["stats"] / m["copy_2"], 3), "stats_alpha_over_copy_2": round(m["stats_alpha"] / m["copy_2"], 3),
            "affine_over_copy_1": round(m["affine"] / m["copy_1"], 3), "affine_inpl_over_copy_1": round(m["affine_inpl"] / m["copy_1"], 3),
            "affine_lut_over_affine": round(m["affine_lut"] / m["affine"], 3),
            "stats_read_tbps": round(2 * nbytes / m["stats"] / 1e12, 3), "affine_read_plus_write_tbps": round(2 * nbytes / m["affine"] / 1e12, 3),
            "copy_1_read_plus_write_tbps": round(2 * nbytes / m["copy_1"] / 1e12, 3),
            "color_match_whole_call_seconds": whole, "host_frames": n_host, "host_definition_with_copies_seconds": host_s,
            "device_over_host_per_frame": round(min(whole) / T / (min(host_s) / n_host), 6)}))
        print(lines[-1], flush=True)
        del src, edit, alpha, out, out_lut, inpl, c2_src, c2_dst, host, back
        torch.cuda.empty_cache()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
