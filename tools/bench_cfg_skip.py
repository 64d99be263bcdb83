#!/usr/bin/env python3
"""A full classifier-free-guidance step against a cfg_skip step (``WanTransformer3DModel.enable_cfg_skip``), Wan2.1-14B
random-init weights, on the BASELINE configs[3] shape (bench.py's 14b-720p workload, latents [1, 16, 21, 90, 160]) and on the
headline CoF shape (14b-cof, latents [1, 16, 43, 60, 104]), guidance 5.0.

    python tools/bench_cfg_skip.py [--rounds 3] [--layers 40] [--shapes 720p,cof]

One process, warm, alternating (full, skipped, full, skipped, ...): a *full* step is what ``WanPipeline`` runs with guidance --
the doubled batch, one forward over [uncond, cond], the guidance arithmetic; a *skipped* step is what it runs while the model's
rule holds -- one forward of the conditional sample, no guidance arithmetic.  HIP-event time per step; prints one JSON line with
the minimum and every sample, and the 50-step loop time the two figures project for cfg_skip_ratio 0, 0.25 and 0.5 (the number
of skipped steps counted by the model's own rule)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"720p": dict(lat=(1, 16, 21, 90, 160), fsi=None, gfi=None, what="14b-720p (BASELINE configs[3])"),
          "cof": dict(lat=(1, 16, 43, 60, 104), fsi=21, gfi=(21, 22), what="14b-cof (headline)")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--shapes", default="720p,cof")
    ap.add_argument("--guidance", type=float, default=5.0)
    args = ap.parse_args()
    from videocof_amd import WanTransformer3DModel
    from videocof_amd.wan_transformer3d import cfg_skip_active
    from videocof_amd.weights import random_dit_state_dict

    dev = torch.device("cuda", 0)
    dim, ffn, heads = 5120, 13824, 40
    model = WanTransformer3DModel(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=args.layers)
    model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=dim, ffn_dim=ffn, num_layers=args.layers), device=dev)
    model.cache_context = True
    model.enable_cfg_skip(0.5, 50)                 # keeps the workspaces of both batch sizes alive, as in a real loop
    g = torch.Generator(device=dev).manual_seed(0)
    ctx = [torch.randn(9, 4096, device=dev, generator=g).bfloat16(), torch.randn(37, 4096, device=dev, generator=g).bfloat16()]
    result = {"what": f"Wan2.1-14B ({args.layers} layers), guidance {args.guidance}: full CFG step vs cfg_skip step, ms (HIP events)"}
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        lat = torch.randn(*sh["lat"], device=dev, generator=g).bfloat16()
        F, H, W = sh["lat"][2:]
        seq_len = F * (H // 2) * (W // 2)
        t = torch.tensor([500], device=dev)

        def kw(nb):
            return dict(frame_split_indices=[sh["fsi"]] * nb if sh["fsi"] is not None else None,
                        ground_frame_indices=[sh["gfi"]] * nb if sh["gfi"] is not None else None)

        def full():
            model.current_steps = 0
            v = model(torch.cat([lat] * 2), t.expand(2), ctx, seq_len, **kw(2))
            vu, vt = v.chunk(2)
            return vu + args.guidance * (vt - vu)

        def skipped():
            model.current_steps = 49
            model._cfg_skip_suspended = True        # the pipeline's short path: the call is the conditional half already
            try:
                return model(lat, t, ctx[1:], seq_len, **kw(1))
            finally:
                model._cfg_skip_suspended = False

        times = {"full": [], "skipped": []}
        for fn in (full, skipped):                  # warm-up: workspaces, text K/V, kernel attributes
            fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for key, fn in (("full", full), ("skipped", skipped)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = fn()
                b.record()
                torch.cuda.synchronize()
                times[key].append(a.elapsed_time(b))
                assert bool(torch.isfinite(out).all())
        f, s = min(times["full"]), min(times["skipped"])
        proj = {}
        for r in (0.0, 0.25, 0.5):
            k = sum(cfg_skip_active(2, r or None, i, 50) for i in range(50))
            proj[str(r)] = {"skipped_steps": k, "loop_s": round(((50 - k) * f + k * s) / 1e3, 1)}
        result[name] = {"shape": sh["what"], "tokens": seq_len, "full_ms": [round(x, 1) for x in times["full"]],
                        "skipped_ms": [round(x, 1) for x in times["skipped"]], "full_ms_min": round(f, 1), "skipped_ms_min": round(s, 1),
                        "skipped_over_full": round(s / f, 4),
                        "spread_full_pct": round(100 * (max(times["full"]) - f) / f, 2), "projected_50_step_loop": proj}
        model.release_workspaces()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
