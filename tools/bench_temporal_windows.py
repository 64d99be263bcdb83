#!/usr/bin/env python3
"""One denoise step of a long clip run whole against the same clip in temporal context windows (``temporal_window=81,
temporal_overlap=16``; DESIGN.md "Temporal context windows"), Wan2.1-14B random-init weights, bf16 latents at 480p
(60 x 104 latent pixels), 161 and 321 source frames, no guidance.

    python tools/bench_temporal_windows.py [--rounds 2] [--layers 40] [--frames 161,321] [--window-batch 0] [--log PATH]

One process, warm, alternating (whole, windows, whole, windows, ...), HIP-event time per step.  *whole* is the forward
``WanPipeline`` runs today over [source | grounding | target]; *windows* is what it runs with the option: wan_window_gather, ONE
forward over the K windows (``--window-batch`` windows per forward if set), wan_window_blend.  The sampler's step is the same
in both and left out.  The two new kernels are also timed alone, beside ``Tensor.copy_`` over as many bytes as the kernel moves
(read + written).  Prints one JSON line and writes it to ``--log`` (default profiles/r10/temporal_windows_ab.log).
A protocol for a measurement, not a pass criterion."""
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
    ap.add_argument("--frames", default="161,321")
    ap.add_argument("--window-batch", type=int, default=0, help="windows per forward (0 = all)")
    ap.add_argument("--kernels-only", action="store_true", help="time the two kernels only (no model, no log file)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r10", "temporal_windows_ab.log"))
    args = ap.parse_args()
    from videocof_amd import WanTransformer3DModel, ops, window_latent_frames, window_plan
    from videocof_amd.weights import random_dit_state_dict

    dev = torch.device("cuda", 0)
    dim, ffn, heads, G, h, w = 5120, 13824, 40, 1, 60, 104
    model = None
    if not args.kernels_only:
        model = WanTransformer3DModel(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=args.layers)
        model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=dim, ffn_dim=ffn, num_layers=args.layers), device=dev)
        model.cache_context = True
    g = torch.Generator(device=dev).manual_seed(0)
    ctx = torch.randn(37, 4096, device=dev, generator=g).bfloat16()
    t = torch.tensor([500], device=dev)
    n, o = window_latent_frames(81, 16)
    result = {"what": f"Wan2.1-14B ({args.layers} layers), bf16, 480p, no guidance: one step whole vs in windows of 81 frames "
                      "(overlap 16), ms (HIP events)"}
    for frames in (int(f) for f in args.frames.split(",")):
        Fs = (frames - 1) // 4 + 1
        plan = window_plan(Fs, n, o)
        K = plan.K
        per_call = args.window_batch or K
        alpha = torch.from_numpy(plan.alpha).to(dev)
        lat = torch.randn(1, 16, 2 * Fs + G, h, w, device=dev, generator=g).bfloat16()
        state = torch.cat([lat[:, :, :Fs]] + [lat[:, :, Fs:Fs + G]] * K + [lat[:, :, Fs + G:]], dim=2).contiguous()
        tokens = lambda f: f * (h // 2) * (w // 2)

        def whole():
            model.mask_source_frames = model.skip_source_frames = Fs
            return model(lat, t, [ctx], tokens(2 * Fs + G), frame_split_indices=[Fs], ground_frame_indices=[(Fs, Fs + G)])

        def windows():
            model.mask_source_frames = model.skip_source_frames = n
            preds = []
            for k0 in range(0, K, per_call):
                k1 = min(k0 + per_call, K)
                x = ops.window_gather(state, plan.starts, n, G, k0, k1)
                preds.append(model(x, t.expand(k1 - k0), [ctx] * (k1 - k0), tokens(2 * n + G), frame_split_indices=[n] * (k1 - k0),
                                   ground_frame_indices=[(n, n + G)] * (k1 - k0)))
            return ops.window_blend(preds[0] if len(preds) == 1 else torch.cat(preds), alpha, plan.starts, Fs, G)

        times = {"whole": [], "windows": []}
        for key, fn in (("whole", whole), ("windows", windows)) if model is not None else ():    # warm-up: workspaces, text K/V, kernel attributes
            ms, _ = timed(fn)
            print(f"[warm] {frames}f {key}: {ms:.0f} ms", flush=True)
        for r in range(args.rounds if model is not None else 0):
            for key, fn in (("whole", whole), ("windows", windows)):
                ms, out = timed(fn)
                times[key].append(ms)
                print(f"[round {r}] {frames}f {key}: {ms:.0f} ms", flush=True)
                assert bool(torch.isfinite(out).all())
        # the two kernels alone, beside a plain copy of the bytes they move
        x = ops.window_gather(state, plan.starts, n, G)
        pred = torch.randn(x.shape, device=dev, generator=g).bfloat16()
        gather_bytes = 2 * x.numel() * 2                                                  # every element read once, written once
        blend_bytes = (K * 16 * (n + G) * h * w + state.numel()) * 2                      # grounding + target frames read, the state written
        kern = {}
        for key, fn, nbytes in (("gather", lambda: ops.window_gather(state, plan.starts, n, G, out=x), gather_bytes),
                                ("blend", lambda: ops.window_blend(pred, alpha, plan.starts, Fs, G), blend_bytes)):
            src = torch.empty(nbytes // 4, device=dev, dtype=torch.bfloat16)
            dst = torch.empty_like(src)
            fn(), dst.copy_(src)
            ks, cs = [], []
            for _ in range(5):
                ks.append(timed(fn)[0])
                cs.append(timed(lambda: dst.copy_(src))[0])
            kern[key] = {"bytes": nbytes, "kernel_us_min": round(min(ks) * 1e3, 1), "copy_us_min": round(min(cs) * 1e3, 1),
                         "kernel_tbps": round(nbytes / min(ks) / 1e9, 3), "copy_tbps": round(nbytes / min(cs) / 1e9, 3)}
        if model is None:
            result[f"{frames}f"] = {"latent_frames": Fs, "windows": K, "kernels": kern}
            continue
        wh, wi = min(times["whole"]), min(times["windows"])
        result[f"{frames}f"] = {"latent_frames": Fs, "windows": K, "starts": list(plan.starts), "windows_per_forward": per_call,
                                "tokens_whole": tokens(2 * Fs + G), "tokens_window": tokens(2 * n + G),
                                "whole_ms": [round(v, 1) for v in times["whole"]], "windows_ms": [round(v, 1) for v in times["windows"]],
                                "whole_ms_min": round(wh, 1), "windows_ms_min": round(wi, 1), "windows_over_whole": round(wi / wh, 4),
                                "spread_whole_pct": round(100 * (max(times["whole"]) - wh) / wh, 2), "kernels": kern}
        del x, pred, lat, state
        model.release_workspaces()
    line = json.dumps(result)
    print(line)
    if model is None:
        return
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
