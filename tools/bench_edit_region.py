#!/usr/bin/env python3
"""What ``WanPipeline.__call__(edit_region=True)`` saves and what it adds, at 81f@1080x1920: a mask of 81 x 1080 x 1920
pixels, the loop state 16 x 43 x 135 x 240 in bf16 ([source 21 | grounding 1 | target 21] latent frames), Wan2.1-14B random-init weights,
no guidance, ``spatial_window=(480, 832)``.  The mask is a rectangle whose margined box fits one tile.

    python tools/bench_edit_region.py [--rounds 2] [--layers 40] [--kernels-only] [--steps 1] [--log PATH]

One process, warm, alternating, HIP-event time.  The three kernels are timed alone, each beside ``Tensor.copy_`` over as many bytes as
the kernel moves (read + written), minimum of 5; then the per-call overhead as the pipeline runs it -- bounds, their copy to the host
(the one synchronisation), the two crops, the restore -- in wall time, minimum of 5.  Then ``--steps`` denoise steps of the same
``WanPipeline`` call with ``edit_region=True`` against the call without it (the 3 x 3 tiles of every frame, the parent commit's unchanged
path), ``output_type='latent'``, alternating (region, tiles, region, tiles, ...), minimum of ``--rounds``.  The expectation -- not
asserted -- is that the region call costs about one headline step (81f@480x832).  Prints one JSON line and appends it to ``--log``
(default profiles/r14/edit_region_ab.log).  A protocol for a measurement, not a pass criterion."""
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
    ap.add_argument("--kernels-only", action="store_true", help="time the three kernels and the per-call overhead only (no model)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r14", "edit_region_ab.log"))
    args = ap.parse_args()
    from videocof_amd import FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel, ops, region_plan
    from videocof_amd.weights import random_dit_state_dict

    dev = torch.device("cuda", 0)
    dim, ffn, heads = 5120, 13824, 40
    T, H, W, C, Fs, G, h, w = 81, 1080, 1920, 16, 21, 1, 135, 240
    tile, margin = (480, 832), (64, 64)
    g = torch.Generator(device=dev).manual_seed(0)
    alpha = torch.zeros(T, H, W, device=dev, dtype=torch.uint8)
    alpha[:, 500:780, 900:1500] = 255                            # 280 x 600 pixels; with grow, feather and the margin: inside 480 x 832
    weights = ops.latent_mask(alpha[None], 1, 0, 1)
    lat = torch.randn(1, C, 2 * Fs + G, h, w, device=dev, generator=g).bfloat16()
    plan = region_plan(ops.mask_bounds(weights).cpu(), (h, w), (margin[0] // 8, margin[1] // 8), (tile[0] // 8, tile[1] // 8), 2)
    assert (plan.h, plan.w) == (tile[0] // 8, tile[1] // 8), plan
    es = lat.element_size()
    result = {"what": "edit_region at 81 x 1080 x 1920 / state 16 x 43 x 135 x 240 bf16, spatial_window 480 x 832: the three kernels beside a "
                      "plain copy of the bytes they move (us, min of 5), the per-call overhead (us, wall, min of 5), and "
                      f"{args.steps} step(s) of a Wan2.1-14B call ({args.layers} layers, no guidance) with the region and without it "
                      "(ms, HIP events)",
              "region_cells": list(plan), "region_pixels": list(plan.pixels())}
    state_r = ops.region_crop(lat, plan)
    source = lat[:, :, :Fs].contiguous()
    full = torch.empty_like(lat)
    bounds = torch.empty(Fs, 4, device=dev, dtype=torch.int32)
    kern = {}
    for key, fn, nbytes in (("mask_bounds", lambda: ops.mask_bounds(weights, out=bounds), weights.numel() + 16 * Fs),
                            ("region_crop_state", lambda: ops.region_crop(lat, plan, out=state_r), 2 * state_r.numel() * es),
                            ("region_restore", lambda: ops.region_restore(source, state_r, (plan.y0, plan.x0), out=full), 2 * full.numel() * es)):
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
        p = region_plan(ops.mask_bounds(weights).cpu(), (h, w), (margin[0] // 8, margin[1] // 8), (tile[0] // 8, tile[1] // 8), 2)
        s, _ = ops.region_crop(lat, p), ops.region_crop(weights, p)
        return ops.region_restore(lat[:, :, :Fs], s, (p.y0, p.x0))
    walls = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        per_call()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e6)
    result["per_call_overhead_us"] = {"wall_us_min": round(min(walls[1:]), 1), "wall_us": [round(v, 1) for v in walls[1:]]}
    if not args.kernels_only:
        model = WanTransformer3DModel(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=args.layers)
        model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=dim, ffn_dim=ffn, num_layers=args.layers), device=dev)
        pipe = WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))
        ctx = torch.randn(37, 4096, device=dev, generator=g).bfloat16()

        def call(**kw):
            return pipe(latents=lat, prompt_embeds=[ctx], source_frames=T, reasoning_frames=4, height=H, width=W,
                        num_inference_steps=args.steps, guidance_scale=1.0, cot=True, output_type="latent", return_dict=True,
                        edit_mask=alpha, spatial_window=tile, **kw)
        forms = (("region", lambda: call(edit_region=True, edit_region_margin=margin)), ("tiles", lambda: call()))
        times = {"region": [], "tiles": []}
        for key, fn in forms:                                    # warm-up: workspaces, text K/V, kernel attributes
            ms, out = timed(fn)
            print(f"[warm] {key}: {ms:.0f} ms, edit_region={out.edit_region}", flush=True)
        for r in range(args.rounds):
            for key, fn in forms:
                ms, out = timed(fn)
                times[key].append(ms)
                print(f"[round {r}] {key}: {ms:.0f} ms", flush=True)
                assert bool(torch.isfinite(out.latents).all()) and tuple(out.latents.shape) == tuple(lat.shape)
        re, ti = min(times["region"]), min(times["tiles"])
        result["call"] = {"steps": args.steps, "region_ms": [round(v, 1) for v in times["region"]], "tiles_ms": [round(v, 1) for v in times["tiles"]],
                          "region_ms_min": round(re, 1), "tiles_ms_min": round(ti, 1), "tiles_over_region": round(ti / re, 3)}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
