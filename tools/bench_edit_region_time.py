#!/usr/bin/env python3
"""What ``WanPipeline.__call__(edit_region=True, edit_region_time_margin=8)`` saves and what it adds, the time arm of
tools/bench_edit_region.py, at 321f@480x832: a mask of 321 x 480 x 832 pixels, the loop state 16 x 163 x 60 x 104 in bf16 ([source 81 |
grounding 1 | target 81] latent frames), Wan2.1-14B random-init weights, no guidance, ``temporal_window=81, temporal_overlap=16``.  The
mask is a rectangle on pixel frames 120..179; the spatial margin makes the region the whole frame, so only the time axis is cropped: the
rule gives the latent frames [28, 48), one whole-clip forward of 41 latent frames.

    python tools/bench_edit_region_time.py [--rounds 2] [--layers 40] [--kernels-only] [--steps 1] [--log PATH]

The protocol of tools/bench_edit_region.py: one process, warm, alternating, HIP-event time.  The two kernels are timed alone, each
beside ``Tensor.copy_`` over as many bytes as the kernel moves (read + written), minimum of 5; then the per-call overhead as the pipeline
runs it -- bounds, their copy to the host (the one synchronisation), the two crops, the restore -- in wall time, minimum of 5.  Then
``--steps`` denoise steps of the same ``WanPipeline`` call with the time crop against the call without ``edit_region`` (the five windows
of the whole clip, the parent commit's unchanged path), ``output_type='latent'``, alternating (range, windows, range, windows, ...),
minimum of ``--rounds``.  The expectation -- not asserted -- is that the cropped call costs about one headline step (81f@480x832).
Prints one JSON line and appends it to ``--log`` (default profiles/r15/edit_region_time_ab.log).  A protocol for a measurement, not a
pass criterion."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--kernels-only", action="store_true", help="time the two kernels and the per-call overhead only (no model)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r15", "edit_region_time_ab.log"))
    args = ap.parse_args()
    from videocof_amd import FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel, ops, region_plan, region_time_plan
    from videocof_amd.weights import random_dit_state_dict

    dev = torch.device("cuda", 0)
    dim, ffn, heads = 5120, 13824, 40
    T, H, W, C, Fs, G, h, w = 321, 480, 832, 16, 81, 1, 60, 104
    margin, time_margin, windows = (480, 832), 8, dict(temporal_window=81, temporal_overlap=16)
    g = torch.Generator(device=dev).manual_seed(0)
    alpha = torch.zeros(T, H, W, device=dev, dtype=torch.uint8)
    alpha[120:180, 100:380, 200:632] = 255                       # pixel frames 120..179: latent frames 30..45
    weights = ops.latent_mask(alpha[None], 1, 0, 1)
    lat = torch.randn(1, C, 2 * Fs + G, h, w, device=dev, generator=g).bfloat16()

    def plans():
        bounds = ops.mask_bounds(weights).cpu()
        return region_plan(bounds, (h, w), (margin[0] // 8, margin[1] // 8), None, 2), region_time_plan(bounds, Fs, time_margin // 4, G)
    plan, rng = plans()
    assert tuple(plan) == (0, 0, h, w) and tuple(rng) == (28, 20), (plan, rng)
    t0, n = rng
    runs = [(t0, n), (Fs, G), (Fs + G + t0, n)]
    es = lat.element_size()
    result = {"what": "edit_region_time_margin=8 at 321 x 480 x 832 / state 16 x 163 x 60 x 104 bf16, temporal_window 81 / overlap 16: the two "
                      "kernels beside a plain copy of the bytes they move (us, min of 5), the per-call overhead (us, wall, min of 5), and "
                      f"{args.steps} step(s) of a Wan2.1-14B call ({args.layers} layers, no guidance) with the time crop and without "
                      "edit_region (ms, HIP events)",
              "region_cells": list(plan), "range_latent_frames": list(rng), "range_pixel_frames": list(rng.pixels())}
    state_r = ops.region_crop_frames(lat, runs, plan)
    source = lat[:, :, :Fs].contiguous()
    full = torch.empty_like(lat)
    kern = {}
    for key, fn, nbytes in (("region_crop_frames_state", lambda: ops.region_crop_frames(lat, runs, plan, out=state_r), 2 * state_r.numel() * es),
                            ("region_restore_frames", lambda: ops.region_restore_frames(source, state_r, (plan.y0, plan.x0), rng, out=full),
                             2 * full.numel() * es)):
        src = torch.empty(max(nbytes // 4, 1), device=dev, dtype=torch.bfloat16)
        dst = torch.empty_like(src)
        fn(), dst.copy_(src)
        ks, cs = [], []
        for _ in range(5):
            ks.append(timed(fn)[0])
            cs.append(timed(lambda: dst.copy_(src))[0])
        kern[key] = {"bytes": nbytes, "kernel_us_min": round(min(ks) * 1e3, 1), "copy_us_min": round(min(cs) * 1e3, 1),
                     "kernel_tbps": round(nbytes / min(ks) / 1e9, 3), "copy_tbps": round(nbytes / min(cs) / 1e9, 3)}
        del src, dst
    result["kernels"] = kern

    def per_call():                                              # what the two stages of the pipeline run, in its order
        p, r = plans()
        s, _ = ops.region_crop_frames(lat, runs, p), ops.region_crop_frames(weights, [tuple(r)], p)
        return ops.region_restore_frames(lat[:, :, :Fs], s, (p.y0, p.x0), r)
    walls = []
    for _ in range(6):
        torch.cuda.synchronize()
        t_wall = time.perf_counter()
        per_call()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t_wall) * 1e6)
    result["per_call_overhead_us"] = {"wall_us_min": round(min(walls[1:]), 1), "wall_us": [round(v, 1) for v in walls[1:]]}
    if not args.kernels_only:
        model = WanTransformer3DModel(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=args.layers)
        model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=dim, ffn_dim=ffn, num_layers=args.layers), device=dev)
        pipe = WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))
        ctx = torch.randn(37, 4096, device=dev, generator=g).bfloat16()

        def call(**kw):
            return pipe(latents=lat, prompt_embeds=[ctx], source_frames=T, reasoning_frames=4, height=H, width=W,
                        num_inference_steps=args.steps, guidance_scale=1.0, cot=True, output_type="latent", return_dict=True,
                        edit_mask=alpha, **windows, **kw)
        forms = (("range", lambda: call(edit_region=True, edit_region_margin=margin, edit_region_time_margin=time_margin)),
                 ("windows", lambda: call()))
        times = {"range": [], "windows": []}
        for key, fn in forms:                                    # warm-up: workspaces, text K/V, kernel attributes
            ms, out = timed(fn)
            print(f"[warm] {key}: {ms:.0f} ms, edit_region_time={out.edit_region_time}", flush=True)
        for r in range(args.rounds):
            for key, fn in forms:
                ms, out = timed(fn)
                times[key].append(ms)
                print(f"[round {r}] {key}: {ms:.0f} ms", flush=True)
                assert bool(torch.isfinite(out.latents).all()) and tuple(out.latents.shape) == tuple(lat.shape)
        ra, wi = min(times["range"]), min(times["windows"])
        result["call"] = {"steps": args.steps, "range_ms": [round(v, 1) for v in times["range"]],
                          "windows_ms": [round(v, 1) for v in times["windows"]], "range_ms_min": round(ra, 1),
                          "windows_ms_min": round(wi, 1), "windows_over_range": round(wi / ra, 3)}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
