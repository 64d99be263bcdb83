#!/usr/bin/env python3
"""What ``WanPipeline.__call__(edit_mask=...)`` adds, at the headline shape: a mask of 81 x 480 x 832 pixels, the
loop state 16 x 43 x 60 x 104 in bf16 ([source 21 | grounding 1 | target 21] latent frames), Wan2.1-14B random-init weights, no guidance.

    python tools/bench_edit_mask.py [--rounds 2] [--layers 40] [--kernels-only] [--log PATH]

One process, warm, alternating, HIP-event time.  The two kernels are timed alone, each beside ``Tensor.copy_`` over as many bytes as the
kernel moves (read + written), minimum of 5: ``wan_latent_mask_u8`` runs once per call, ``wan_masked_prediction`` once per step.  Then
one denoise step without the mask (the forward ``WanPipeline`` runs today) against the same step with it (the forward, then
``ops.masked_prediction_`` on its prediction; the mask is a rectangle over a quarter of the frame, so three quarters of the target are
rewritten), alternating (plain, masked, plain, masked, ...), minimum of ``--rounds``.  The sampler's step is the same in both and left
out.  The expectation -- not asserted -- is that the difference is inside the spread of two identical steps.  Prints one JSON line and
appends it to ``--log`` (default profiles/r13/edit_mask_ab.log).  A protocol for a measurement, not a pass criterion."""
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
    ap.add_argument("--kernels-only", action="store_true", help="time the two kernels only (no model)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r13", "edit_mask_ab.log"))
    args = ap.parse_args()
    from videocof_amd import WanTransformer3DModel, ops
    from videocof_amd.weights import random_dit_state_dict

    dev = torch.device("cuda", 0)
    dim, ffn, heads = 5120, 13824, 40
    T, H, W, C, Fs, G, h, w = 81, 480, 832, 16, 21, 1, 60, 104
    g = torch.Generator(device=dev).manual_seed(0)
    alpha = torch.zeros(1, T, H, W, device=dev, dtype=torch.uint8)
    alpha[:, :, H // 4:3 * H // 4, W // 4:3 * W // 4] = 255
    weights = ops.latent_mask(alpha, 1, 0, 1)
    lat = torch.randn(1, C, 2 * Fs + G, h, w, device=dev, generator=g).bfloat16()
    pred = torch.randn(lat.shape, device=dev, generator=g).bfloat16()
    sigma = 0.75
    result = {"what": "edit_mask at 81 x 480 x 832 / state 16 x 43 x 60 x 104 bf16: the two kernels beside a plain copy of the bytes they "
                      f"move (us, min of 5), and one Wan2.1-14B step ({args.layers} layers, no guidance) without and with the mask "
                      "(ms, HIP events)",
              "mask_cells_inside": int((weights == 255).sum()), "mask_cells_outside": int((weights == 0).sum()),
              "mask_cells_feathered": int(((weights > 0) & (weights < 255)).sum())}
    cells = weights.numel()
    mask_bytes = alpha.numel() + 5 * cells                       # the pixel mask read once; the p and g planes written and read, the weights written
    pred_bytes = C * Fs * h * w * (4 * 2 + 1)                    # per (channel, cell): v, x_t, s read, the result written (bf16), one weight byte
    kern = {}
    for key, fn, nbytes in (("latent_mask", lambda: ops.latent_mask(alpha, 1, 0, 1, out=weights), mask_bytes),
                            ("masked_prediction", lambda: ops.masked_prediction_(pred, lat, weights, Fs, Fs + G, sigma), pred_bytes)):
        src = torch.empty(nbytes // 4, device=dev, dtype=torch.bfloat16)
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
    if not args.kernels_only:
        model = WanTransformer3DModel(dim=dim, ffn_dim=ffn, num_heads=heads, num_layers=args.layers)
        model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=dim, ffn_dim=ffn, num_layers=args.layers), device=dev)
        model.cache_context = True
        model.mask_source_frames = model.skip_source_frames = Fs
        ctx = torch.randn(37, 4096, device=dev, generator=g).bfloat16()
        t = torch.tensor([500], device=dev)
        tokens = (2 * Fs + G) * (h // 2) * (w // 2)

        def plain():
            return model(lat, t, [ctx], tokens, frame_split_indices=[Fs], ground_frame_indices=[(Fs, Fs + G)])

        def masked():
            return ops.masked_prediction_(plain().contiguous(), lat, weights, Fs, Fs + G, sigma)

        times = {"plain": [], "masked": []}
        for key, fn in (("plain", plain), ("masked", masked)):   # warm-up: workspaces, text K/V, kernel attributes
            ms, _ = timed(fn)
            print(f"[warm] {key}: {ms:.0f} ms", flush=True)
        for r in range(args.rounds):
            for key, fn in (("plain", plain), ("masked", masked)):
                ms, out = timed(fn)
                times[key].append(ms)
                print(f"[round {r}] {key}: {ms:.0f} ms", flush=True)
                assert bool(torch.isfinite(out).all())
        pl, ma = min(times["plain"]), min(times["masked"])
        result["step"] = {"tokens": tokens, "plain_ms": [round(v, 1) for v in times["plain"]],
                          "masked_ms": [round(v, 1) for v in times["masked"]], "plain_ms_min": round(pl, 1), "masked_ms_min": round(ma, 1),
                          "masked_over_plain": round(ma / pl, 5), "spread_plain_pct": round(100 * (max(times["plain"]) - pl) / pl, 3)}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
