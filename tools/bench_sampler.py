#!/usr/bin/env python3
"""The 4-step CoF denoise loop at the headline shape (bench.py's 14b-cof workload: Wan2.1-14B random-init weights, latents
[1, 16, 43, 60, 104] bf16) through ``WanPipeline``, once with ``FlowUniPCMultistepScheduler`` and once with
``FlowDPMSolverMultistepScheduler`` on the same model, alternating: wall ms per denoise step for each sampler.

    python tools/bench_sampler.py [--rounds 2] [--layers N]

One warm-up call per sampler, then ``rounds`` timed calls of each (UniPC, DPM++, UniPC, DPM++, ...); prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=4)
    args = ap.parse_args()
    from videocof_amd import FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel
    from videocof_amd.weights import random_dit_state_dict

    dev = torch.device("cuda", 0)
    dim, ffn, heads = 5120, 13824, 40
    model = WanTransformer3DModel(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=args.layers)
    model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=dim, ffn_dim=ffn, num_layers=args.layers), device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    latents = torch.randn(1, 16, 43, 60, 104, device=dev, generator=g).bfloat16()
    ctx = [torch.randn(37, 4096, device=dev, generator=g).bfloat16()]
    pipes = {"unipc": WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1)),
             "dpm++": WanPipeline(transformer=model, scheduler=FlowDPMSolverMultistepScheduler(shift=1))}
    kw = dict(latents=latents, prompt_embeds=ctx, source_frames=81, reasoning_frames=4, num_inference_steps=args.steps,
              guidance_scale=1.0, shift=3, repeat_rope=True, cot=True, output_type="latent", weight_dtype=torch.bfloat16)
    times = {k: [] for k in pipes}
    finite = {}
    for k, p in pipes.items():
        p(**kw)                                   # warm-up
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, p in pipes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = p(**kw).latents
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
            finite[k] = bool(torch.isfinite(out).all())
    print(json.dumps({"what": f"WanPipeline {args.steps}-step CoF loop, 14B ({args.layers} layers), latents [1,16,43,60,104] bf16",
                      "ms_per_step": {k: [round(t, 1) for t in v] for k, v in times.items()},
                      "ms_per_step_min": {k: round(min(v), 1) for k, v in times.items()}, "finite": finite}))


if __name__ == "__main__":
    main()
