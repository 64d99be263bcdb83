#!/usr/bin/env python3
"""What ``WanPipeline.__call__(edit_region=True, edit_region_split=2)`` saves and what it adds, the two-objects arm of
tools/bench_edit_region.py, at 81f@1080x1920: a mask of 81 x 1080 x 1920 pixels, the loop state 16 x 43 x 135 x 240 in bf16 ([source 21
| grounding 1 | target 21] latent frames), Wan2.1-14B random-init weights, no guidance, ``spatial_window=(480, 832)``.  The mask is two
rectangles of 200 x 200 pixels in opposite corners of the frame: their union box is the whole frame and runs as 3 x 3 tiles, each one's
own box fits one tile of 60 x 104 cells.

    python tools/bench_edit_region_split.py [--rounds 2] [--layers 40] [--kernels-only] [--steps 1] [--log PATH]

The protocol of tools/bench_edit_region_follow.py: one process, warm, alternating, HIP-event time.  The three kernels are timed alone,
each beside ``Tensor.copy_`` over as many bytes as the kernel moves (read + written) and beside the form it extends on bytes of its own
(``mask_bounds`` for the spans; ``region_crop_frames`` / ``region_restore_frames`` of ONE box, so half the crop's bytes), in rotating
order, minimum of 8 (each sample is one call of the ``ops`` function between two HIP events, so it holds that call's host work as well
as the launch); then the per-call overhead as the pipeline runs it -- spans, their copy to the host (the one synchronisation), the
rule, the two crops, the restore -- in wall time, minimum of 5 (``edit_region=True`` alone crops nothing here: its rectangle is the
frame).  Then ``--steps``
denoise steps of the same ``WanPipeline`` call with ``edit_region_split=2`` against ``edit_region=True`` alone,
``output_type='latent'``, alternating (split, union, split, union, ...), minimum of ``--rounds``.  Nothing is asserted about a time.
Prints one JSON line and appends it to ``--log`` (default profiles/r18/edit_region_split_ab.log).  A protocol for a measurement, not a
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
    ap.add_argument("--kernels-only", action="store_true", help="time the three kernels and the per-call overhead only (no model)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r18", "edit_region_split_ab.log"))
    args = ap.parse_args()
    from videocof_amd import (FlowUniPCMultistepScheduler, SplitPlan, WanPipeline, WanTransformer3DModel, ops, region_plan,
                              region_split_plan)
    from videocof_amd.edit_region import spans_bounds
    from videocof_amd.weights import random_dit_state_dict

    dev = torch.device("cuda", 0)
    dim, ffn, heads = 5120, 13824, 40
    T, H, W, C, Fs, G, h, w = 81, 1080, 1920, 16, 21, 1, 135, 240
    margin, tile, windows = (64, 64), (60, 104), dict(spatial_window=(480, 832))
    g = torch.Generator(device=dev).manual_seed(0)
    alpha = torch.zeros(T, H, W, device=dev, dtype=torch.uint8)
    alpha[:, :200, :200] = 255                                   # two objects of 200 x 200 pixels in opposite corners
    alpha[:, H - 200:, W - 200:] = 255
    weights = ops.latent_mask(alpha[None], 1, 0, 1)
    lat = torch.randn(1, C, 2 * Fs + G, h, w, device=dev, generator=g).bfloat16()
    rule = (h, w), (margin[0] // 8, margin[1] // 8), tile, 2

    def plans():
        spans = ops.mask_spans(weights).cpu()
        return region_split_plan(spans, *rule, max_regions=2), spans
    split, spans = plans()
    union = region_plan(spans_bounds(spans, (h, w)), *rule)
    assert isinstance(split, SplitPlan) and (split.h, split.w) == tile and (union.h, union.w) == (h, w), (split, union)
    runs = [(0, 2 * Fs + G)]
    es = lat.element_size()
    boxes = split.origins, split.cuts, split.axis, tile
    result = {"what": "edit_region_split=2 at 81 x 1080 x 1920 / state 16 x 43 x 135 x 240 bf16, spatial_window (480, 832), two 200 x 200 "
                      "pixel objects in opposite corners: the three kernels beside a plain copy of the bytes they move and beside the form "
                      "each extends (us, min of 8), the per-call overhead (us, wall, min of 5), and "
                      f"{args.steps} step(s) of a Wan2.1-14B call ({args.layers} layers, no guidance) with two boxes and with the union box "
                      "(ms, HIP events)",
              "axis": split.axis, "box_cells": [split.h, split.w], "origins": split.origins.tolist(), "cuts": split.cuts.tolist(),
              "union_cells": list(union)}
    one = (int(split.origins[0][0]), int(split.origins[0][1]), split.h, split.w)
    state_r = ops.region_crop_split(lat, runs, *boxes)
    state_2 = state_r.flatten(0, 1)
    state_1 = ops.region_crop_frames(lat, runs, one)
    source = lat[:, :, :Fs].contiguous()
    full = torch.empty_like(lat)
    spans_d, bounds_d = ops.mask_spans(weights), ops.mask_bounds(weights)
    kern = {}
    for key, fn, same, nbytes, same_bytes in (
            ("mask_spans", lambda: ops.mask_spans(weights, out=spans_d), lambda: ops.mask_bounds(weights, out=bounds_d),
             2 * weights.numel() + spans_d.numel() * 2, weights.numel() + bounds_d.numel() * 4),
            ("region_crop_split_state", lambda: ops.region_crop_split(lat, runs, *boxes, out=state_r),
             lambda: ops.region_crop_frames(lat, runs, one, out=state_1), 2 * state_r.numel() * es, 2 * state_1.numel() * es),
            ("region_restore_split", lambda: ops.region_restore_split(source, state_2, *boxes[:3], (0, Fs), out=full),
             lambda: ops.region_restore_frames(source, state_1, one[:2], (0, Fs), out=full), 2 * full.numel() * es, 2 * full.numel() * es)):
        src = torch.empty(max(nbytes // 4, 1), device=dev, dtype=torch.bfloat16)
        dst = torch.empty_like(src)
        forms = [("kernel", fn), ("extended_form", same), ("copy", lambda: dst.copy_(src))]
        for _, f in forms:
            f()
        us = {name: [] for name, _ in forms}
        for r in range(8):                                       # every form after every other one: the order rotates
            for name, f in forms[r % 3:] + forms[:r % 3]:
                us[name].append(timed(f)[0] * 1e3)
        kern[key] = {"bytes": nbytes, "extended_form_bytes": same_bytes, **{f"{name}_us_min": round(min(v), 1) for name, v in us.items()},
                     "kernel_tbps": round(nbytes / min(us["kernel"]) / 1e6, 3), "copy_tbps": round(nbytes / min(us["copy"]) / 1e6, 3),
                     "extended_form_tbps": round(same_bytes / min(us["extended_form"]) / 1e6, 3)}
        del src, dst
    result["kernels"] = kern

    def per_call_split():                                        # what the two stages of the pipeline run, in its order
        p, _ = plans()
        b = p.origins, p.cuts, p.axis, (p.h, p.w)
        s, _ = ops.region_crop_split(lat, runs, *b), ops.region_crop_split(weights, [(0, Fs)], *b, clip=True)
        return ops.region_restore_split(lat[:, :, :Fs], s.flatten(0, 1), *b[:3], (0, Fs))

    for key, fn in (("per_call_overhead_us", per_call_split),):
        walls = []
        for _ in range(6):
            torch.cuda.synchronize()
            t_wall = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t_wall) * 1e6)
        result[key] = {"wall_us_min": round(min(walls[1:]), 1), "wall_us": [round(v, 1) for v in walls[1:]]}
    result["host_copy_bytes"] = {"spans": int(spans_d.numel() * 2), "bounds": int(bounds_d.numel() * 4)}
    if not args.kernels_only:
        model = WanTransformer3DModel(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=args.layers)
        model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=dim, ffn_dim=ffn, num_layers=args.layers), device=dev)
        pipe = WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))
        ctx = torch.randn(37, 4096, device=dev, generator=g).bfloat16()

        def call(**kw):
            return pipe(latents=lat, prompt_embeds=[ctx], source_frames=T, reasoning_frames=4, height=H, width=W,
                        num_inference_steps=args.steps, guidance_scale=1.0, cot=True, output_type="latent", return_dict=True,
                        edit_mask=alpha, edit_region=True, edit_region_margin=margin, **windows, **kw)
        forms = (("split", lambda: call(edit_region_split=2)), ("union", lambda: call()))
        times = {"split": [], "union": []}
        for key, fn in forms:                                    # warm-up: workspaces, text K/V, kernel attributes
            ms, out = timed(fn)
            print(f"[warm] {key}: {ms:.0f} ms, edit_region={out.edit_region}, edit_regions={out.edit_regions}", flush=True)
        for r in range(args.rounds):
            for key, fn in forms:
                ms, out = timed(fn)
                times[key].append(ms)
                print(f"[round {r}] {key}: {ms:.0f} ms", flush=True)
                assert bool(torch.isfinite(out.latents).all()) and tuple(out.latents.shape) == tuple(lat.shape)
        sp, un = min(times["split"]), min(times["union"])
        result["call"] = {"steps": args.steps, "split_ms": [round(v, 1) for v in times["split"]],
                          "union_ms": [round(v, 1) for v in times["union"]], "split_ms_min": round(sp, 1),
                          "union_ms_min": round(un, 1), "union_over_split": round(un / sp, 3)}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
