#!/usr/bin/env python3
"""One denoise step of a large-frame clip run whole against the same clip in spatial context windows (``spatial_window=(480, 832),
spatial_overlap=(96, 128)``), Wan2.1-14B random-init weights, bf16 latents, no guidance.

    python tools/bench_spatial_windows.py [--rounds 2] [--layers 40] [--arms 81x720x1280,33x1088x1920,81x1080x1920:tiles]
                                          [--window-batch 0] [--kernels-only] [--log PATH]

An arm is FRAMESxHEIGHTxWIDTH in pixels; ``:tiles`` runs the tiled side only (the whole frame at that size is not attempted).
One process, warm, alternating (whole, tiles, whole, tiles, ...), HIP-event time per step, minimum of ``--rounds``.  *whole* is the
forward ``WanPipeline`` runs today over [source | grounding | target] at the clip's own size; *tiles* is what it runs with the
option: wan_tile_gather, ONE forward over the K tiles (``--window-batch`` tiles per forward if set), wan_tile_blend.  The sampler's
step is the same in both and left out.  The two new kernels are also timed alone, beside ``Tensor.copy_`` over as many bytes as the
kernel moves (read + written).  Prints one JSON line and writes it to ``--log`` (default profiles/r11/spatial_windows_ab.log).
A protocol for a measurement, not a pass criterion."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAX_ROWS = 5 * 67080        # tokens of one forward unless --window-batch says otherwise: the largest batch this model has been run at


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
    ap.add_argument("--arms", default="81x720x1280,33x1088x1920,81x1080x1920:tiles")
    ap.add_argument("--window-batch", type=int, default=0,
                    help=f"tiles per forward (0 = all, as long as one forward stays within {MAX_ROWS} tokens)")
    ap.add_argument("--kernels-only", action="store_true", help="time the two kernels only (no model, no log file)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r11", "spatial_windows_ab.log"))
    args = ap.parse_args()
    from videocof_amd import TilePlan, WanTransformer3DModel, ops, spatial_window_cells, window_plan
    from videocof_amd.weights import random_dit_state_dict

    dev = torch.device("cuda", 0)
    dim, ffn, heads, G, C = 5120, 13824, 40, 1, 16
    model = None
    if not args.kernels_only:
        model = WanTransformer3DModel(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=args.layers)
        model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=dim, ffn_dim=ffn, num_layers=args.layers), device=dev)
        model.cache_context = True
    g = torch.Generator(device=dev).manual_seed(0)
    ctx = torch.randn(37, 4096, device=dev, generator=g).bfloat16()
    t = torch.tensor([500], device=dev)
    (th, tw), (oy, ox) = spatial_window_cells((480, 832), (96, 128))
    result = {"what": f"Wan2.1-14B ({args.layers} layers), bf16, no guidance: one step whole vs in tiles of 480 x 832 (overlap 96 x 128), "
                      "ms (HIP events)"}
    for arm in args.arms.split(","):
        spec, _, mode = arm.partition(":")
        frames, height, width = (int(v) for v in spec.split("x"))
        Fs, H, W = (frames - 1) // 4 + 1, height // 8, width // 8
        plan = TilePlan(window_plan(Fs, max(Fs, 2), 0), window_plan(H, th, oy), window_plan(W, tw, ox))
        K, (n, ph, pw) = plan.K, plan.shape
        tokens = lambda f, h, w: f * -(-h // 2) * -(-w // 2)
        # all tiles in one forward, as long as that forward stays within the largest batch of rows this model has been run at
        # (five windows of 67 080 tokens: tools/bench_temporal_windows.py at 321 frames)
        per_call = args.window_batch or min(K, max(1, MAX_ROWS // tokens(2 * n + G, ph, pw)))
        starts = (plan.t.starts, plan.y.starts, plan.x.starts)
        tables = tuple(torch.from_numpy(a.alpha).to(dev) for a in (plan.t, plan.y, plan.x))
        state = torch.randn(1, C, 2 * Fs + G, H, W, device=dev, generator=g).bfloat16()       # Kt = 1: the state is the clip's latents
        run_whole = model is not None and mode != "tiles" and H % 2 == 0 and W % 2 == 0           # (135 rows: not patchifiable whole)

        def whole():
            model.mask_source_frames = model.skip_source_frames = Fs
            return model(state, t, [ctx], tokens(2 * Fs + G, H, W), frame_split_indices=[Fs], ground_frame_indices=[(Fs, Fs + G)])

        def tiles():
            model.mask_source_frames = model.skip_source_frames = n
            preds = []
            for k0 in range(0, K, per_call):
                k1 = min(k0 + per_call, K)
                x = ops.tile_gather(state, starts, plan.shape, G, k0, k1)
                preds.append(model(x, t.expand(k1 - k0), [ctx] * (k1 - k0), tokens(2 * n + G, ph, pw), frame_split_indices=[n] * (k1 - k0),
                                   ground_frame_indices=[(n, n + G)] * (k1 - k0)))
            return ops.tile_blend(preds[0] if len(preds) == 1 else torch.cat(preds), tables, starts, plan.extent, G)

        sides = ([("whole", whole)] if run_whole else []) + ([("tiles", tiles)] if model is not None else [])
        times = {key: [] for key, _ in sides}
        for key, fn in sides:                                   # warm-up: workspaces, text K/V, kernel attributes
            ms, _ = timed(fn)
            print(f"[warm] {arm} {key}: {ms:.0f} ms", flush=True)
        for r in range(args.rounds):
            for key, fn in sides:
                ms, out = timed(fn)
                times[key].append(ms)
                print(f"[round {r}] {arm} {key}: {ms:.0f} ms", flush=True)
                assert bool(torch.isfinite(out).all())
        # the two kernels alone, beside a plain copy of the bytes they move
        x = ops.tile_gather(state, starts, plan.shape, G)
        pred = torch.randn(x.shape, device=dev, generator=g).bfloat16()
        gather_bytes = 2 * x.numel() * 2                                                  # every tile element read once, written once
        blend_bytes = (K * C * (n + G) * ph * pw + state.numel()) * 2                     # grounding + target frames read, the state written
        kern = {}
        for key, fn, nbytes in (("gather", lambda: ops.tile_gather(state, starts, plan.shape, G, out=x), gather_bytes),
                                ("blend", lambda: ops.tile_blend(pred, tables, starts, plan.extent, G), blend_bytes)):
            src = torch.empty(nbytes // 4, device=dev, dtype=torch.bfloat16)
            dst = torch.empty_like(src)
            fn(), dst.copy_(src)
            ks, cs = [], []
            for _ in range(5):
                ks.append(timed(fn)[0])
                cs.append(timed(lambda: dst.copy_(src))[0])
            kern[key] = {"bytes": nbytes, "kernel_us_min": round(min(ks) * 1e3, 1), "copy_us_min": round(min(cs) * 1e3, 1),
                         "kernel_tbps": round(nbytes / min(ks) / 1e9, 3), "copy_tbps": round(nbytes / min(cs) / 1e9, 3)}
        entry = {"latent": [Fs, H, W], "tiles": [plan.Ky, plan.Kx], "tile": [n, ph, pw], "y_starts": list(plan.y.starts),
                 "x_starts": list(plan.x.starts), "tokens_whole": tokens(2 * Fs + G, H, W), "tokens_tile": tokens(2 * n + G, ph, pw),
                 "kernels": kern}
        if times.get("tiles"):
            entry.update(tiles_per_forward=per_call, tiles_ms=[round(v, 1) for v in times["tiles"]],
                         tiles_ms_min=round(min(times["tiles"]), 1))
        if times.get("whole"):
            wh = min(times["whole"])
            entry.update(whole_ms=[round(v, 1) for v in times["whole"]], whole_ms_min=round(wh, 1),
                         tiles_over_whole=round(min(times["tiles"]) / wh, 4),
                         spread_whole_pct=round(100 * (max(times["whole"]) - wh) / wh, 2))
        elif model is not None:
            entry["whole"] = "not run"
        result[arm] = entry
        del x, pred, state
        if model is not None:
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
