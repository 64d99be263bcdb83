#!/usr/bin/env python3
"""What ``WanPipeline.__call__(edit_region=True, edit_region_vae_halo=32)`` saves and what it adds, at 81f@1080x1920:
uint8 frames in, ``output_type="uint8"``, Wan2.1-14B random-init weights in bf16, the VAE with random weights, no guidance,
``spatial_window=(480, 832)``, the rectangle mask of tools/bench_edit_region.py (its margined region is one 480 x 832 tile; with the halo
the VAE's box is 544 x 896 of 1080 x 1920 pixels, 0.235 of the frame's area).

    python tools/bench_edit_region_vae.py [--rounds 2] [--layers 40] [--kernels-only] [--steps 1] [--log PATH]

One process, warm, alternating, HIP-event time.  The two kernels are timed alone, each beside ``Tensor.copy_`` over as many bytes as the
kernel moves (read + written), minimum of 5.  Then the same ``WanPipeline`` call with the switch ("box") against the call without it
("whole": today's ``edit_region=True`` path, the VAE on whole frames), alternating (box, whole, box, whole, ...), minimum of ``--rounds``:
the whole call in HIP-event time, and its ``vae_encode`` / ``vae_decode`` stages from ``pipeline.stage_seconds`` (synchronised wall
seconds; the decode stage holds the stitch and the copy of the frames to the host).  The expectation -- not asserted -- is that the VAE
stages fall roughly with the box's share of the frame's area, and by more where the mid-block attention (quadratic in the area)
dominates.  The ratio is against this run's own "whole" arm.  Prints one JSON line and appends it to ``--log`` (default
profiles/r16/edit_region_vae_ab.log).  A protocol for a measurement, not a pass criterion."""
from __future__ import annotations

import argparse
import json
import os
import sys

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
    ap.add_argument("--kernels-only", action="store_true", help="time the two kernels only (no model)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r16", "edit_region_vae_ab.log"))
    args = ap.parse_args()
    from videocof_amd import (AutoencoderKLWan, FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel, ops, region_plan,
                              region_vae_box)
    from videocof_amd.weights import random_dit_state_dict, random_vae_state_dict

    dev = torch.device("cuda", 0)
    dim, ffn, heads = 5120, 13824, 40
    T, H, W, h, w = 81, 1080, 1920, 135, 240
    tile, margin, halo = (480, 832), (64, 64), 32
    g = torch.Generator(device=dev).manual_seed(0)
    alpha = torch.zeros(T, H, W, device=dev, dtype=torch.uint8)
    alpha[:, 500:780, 900:1500] = 255                            # 280 x 600 pixels; with grow, feather and the margin: inside 480 x 832
    frames = torch.randint(0, 256, (1, T, H, W, 3), device=dev, generator=g, dtype=torch.uint8)
    plan = region_plan(ops.mask_bounds(ops.latent_mask(alpha[None], 1, 0, 1)).cpu(), (h, w), (margin[0] // 8, margin[1] // 8),
                       (tile[0] // 8, tile[1] // 8), 2)
    box = region_vae_box(plan, (h, w), (halo // 8, halo // 8))
    rect_px, box_px = plan.pixels(), box.pixels()
    assert (plan.h, plan.w) == (tile[0] // 8, tile[1] // 8) and box_px[2:] == (544, 896), (plan, box)
    result = {"what": "edit_region_vae_halo=32 at 81 x 1080 x 1920 uint8 frames, spatial_window 480 x 832: the two kernels beside a plain "
                      "copy of the bytes they move (us, min of 5), and the whole call (ms, HIP events) with its vae_encode / vae_decode "
                      f"stages (s, synchronised wall) with the switch (box) and without it (whole); {args.steps} step(s) of a "
                      f"Wan2.1-14B call ({args.layers} layers, bf16, no guidance)",
              "region_pixels": list(rect_px), "box_pixels": list(box_px), "box_share_of_area": round(box_px[2] * box_px[3] / (H * W), 3)}
    planes = torch.empty(1, 3, T, box_px[2], box_px[3], device=dev, dtype=torch.bfloat16)
    decoded = torch.randn(planes.shape, device=dev, generator=g).bfloat16()
    clip = torch.empty_like(frames)
    n_box, n_rect, n_frame = T * box_px[2] * box_px[3] * 3, T * rect_px[2] * rect_px[3] * 3, frames.numel()
    kern = {}
    for key, fn, nbytes in (("frames_u8_box_to_video", lambda: ops.frames_u8_box_to_video(frames, box_px, torch.bfloat16, out=planes),
                             n_box + 2 * n_box),
                            ("video_box_stitch_u8", lambda: ops.video_box_stitch_u8(decoded, frames, box_px, rect_px, 0, out=clip),
                             2 * n_frame + 2 * n_rect)):
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
    del planes, decoded, clip
    if not args.kernels_only:
        model = WanTransformer3DModel(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=args.layers)
        model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=dim, ffn_dim=ffn, num_layers=args.layers), device=dev)
        vae = AutoencoderKLWan()
        vae.load_state_dict(random_vae_state_dict(dev), device=dev)
        pipe = WanPipeline(vae=vae, transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))
        ctx = torch.randn(37, 4096, device=dev, generator=g).bfloat16()

        def call(**kw):
            pipe.stage_seconds = {}
            out = pipe(video=frames, prompt_embeds=[ctx], source_frames=T, reasoning_frames=4, height=H, width=W,
                       num_inference_steps=args.steps, guidance_scale=1.0, cot=True, output_type="uint8", return_dict=True,
                       generator=torch.Generator(device=dev).manual_seed(1), edit_mask=alpha, spatial_window=tile, edit_region=True,
                       edit_region_margin=margin, **kw)
            return out, dict(pipe.stage_seconds)
        forms = (("box", lambda: call(edit_region_vae_halo=halo)), ("whole", lambda: call()))
        times = {k: {"call_ms": [], "vae_encode_s": [], "vae_decode_s": [], "denoise_loop_s": []} for k, _ in forms}
        for key, fn in forms:                                    # warm-up: workspaces, text K/V, kernel attributes
            ms, (out, stages) = timed(fn)
            print(f"[warm] {key}: {ms:.0f} ms, edit_region={out.edit_region} edit_region_vae={out.edit_region_vae} {stages}", flush=True)
        for r in range(args.rounds):
            for key, fn in forms:
                ms, (out, stages) = timed(fn)
                times[key]["call_ms"].append(round(ms, 1))
                for name in ("vae_encode", "vae_decode", "denoise_loop"):
                    times[key][name + "_s"].append(round(stages[name], 4))
                print(f"[round {r}] {key}: {ms:.0f} ms {stages}", flush=True)
                assert out.videos.shape == (1, 1 + T, H, W, 3)
        best = {k: {name: min(v) for name, v in t.items()} for k, t in times.items()}
        result["call"] = {"steps": args.steps, "runs": times, "min": best,
                          "whole_over_box": {name: round(best["whole"][name] / best["box"][name], 3) for name in best["box"]}}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
