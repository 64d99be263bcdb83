#!/usr/bin/env python3
"""Local self-attention (key tiles listed per query block) against the dense kernel, at the headline CoF shape
(grid 43 x 30 x 52 = 67 080 tokens, 21 source + 1 grounding + 21 target frames, 40 heads).

    python tools/bench_local_attention.py [--rounds 2] [--layers 40] [--windows 2x8,3x10,4x10] [--step-window 3x10]
                                          [--launch-only] [--log PATH]

One process, warm, dense and sparse alternating, HIP-event time, minimum of ``--rounds``:

(a) the self-attention launch alone at B = 1, H = 40, L = 67 080 on random pre-scaled q / k / v^T: the dense lazy launch
    (``workspace`` too small for the max-free attempt and the split tail: ONE launch of the kernel the sparse form instantiates), the
    dense call as the model makes it (with its scratch), the sparse launch with EVERY tile listed, and one sparse launch per window.
    Per plan: its density, the time ratio to the dense lazy launch and the efficiency t_sparse / (density x t_dense_lazy)
    (1 = the time per listed tile is the dense kernel's);
(b) one Wan2.1-14B denoise step (random-init weights, bf16 latents, no guidance), dense against ``--step-window``.

Prints one JSON line and writes it to ``--log`` (default profiles/r12/local_attention_ab.log).  A protocol for a measurement, not a
pass criterion; the option is lossy and no quality claim rides on these numbers."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRID, N_SRC, G = (43, 30, 52), 21, 1


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def alternate(sides, rounds, tag):
    """{name: [ms per round]} of the callables in `sides`, one warm-up each, then `rounds` passes over all of them in turn."""
    times = {key: [] for key, _ in sides}
    for key, fn in sides:
        ms, _ = timed(fn)
        print(f"[warm] {tag} {key}: {ms:.2f} ms", flush=True)
    for r in range(rounds):
        for key, fn in sides:
            ms, out = timed(fn)
            times[key].append(ms)
            print(f"[round {r}] {tag} {key}: {ms:.2f} ms", flush=True)
            assert bool(torch.isfinite(out.float()).all())
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--windows", default="2x8,3x10,4x10", help="(window_frames x window_rows) plans of the launch-alone part")
    ap.add_argument("--step-window", default="3x10", help="the window of the one-step part")
    ap.add_argument("--launch-only", action="store_true", help="part (a) only: no model")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r12", "local_attention_ab.log"))
    args = ap.parse_args()
    from videocof_amd import WanTransformer3DModel, _lib, local_attention_plan, ops
    from videocof_amd.local_attention import plan_from_blocks
    from videocof_amd.weights import random_dit_state_dict

    dev = torch.device("cuda", 0)
    H, L = 40, GRID[0] * GRID[1] * GRID[2]
    C = H * 128
    fsi, gfi = [N_SRC], [(N_SRC, N_SRC + G)]
    windows = [tuple(int(v) for v in w.split("x")) for w in args.windows.split(",")]
    result = {"what": f"self-attention at B = 1, H = {H}, L = {L} (grid {GRID}, n = {N_SRC}, G = {G}): dense vs listed key tiles; ms (HIP "
                      f"events), minimum of {args.rounds} alternating rounds, one process", "measured": True}

    # ---- (a) the launch alone
    g = torch.Generator(device=dev).manual_seed(0)
    q = (torch.randn(1, L, C, device=dev, generator=g) * ops.q_prescale(128)).bfloat16()      # N(0, 1) scores in the log2 domain's scale
    k = torch.randn(1, L, C, device=dev, generator=g).bfloat16()
    ldv = ops.round_up(L, 64)
    vt = torch.zeros(1, C, ldv, device=dev, dtype=torch.bfloat16)
    vt[:, :, :L] = torch.randn(1, C, L, device=dev, generator=g).bfloat16()
    out = torch.empty(1, L, C, device=dev, dtype=torch.bfloat16)
    lib = _lib.load()
    scratch = ops.AttentionWorkspace()

    def dense_lazy():           # no scratch: ONE launch of the lazy-reference form
        _lib.check(lib.wan_attention_fwd(q.data_ptr(), C, 0, k.data_ptr(), C, 0, vt.data_ptr(), ldv, 0, out.data_ptr(), C, 0, 1, L, L, H, 128,
                                         0.0, _lib.ATTN_Q_PRESCALED, None, 0, torch.cuda.current_stream().cuda_stream), "wan_attention_fwd")
        return out

    def dense_default():        # what the model's block enqueues: the max-free attempt, its fix-up launch, the split tail round
        return ops.attention_fwd(q, k, vt, H, k_len=L, out=out, q_prescaled=True, workspace=scratch)

    hosts = {"full": plan_from_blocks(np.ones((-(-L // 256), -(-L // 64)), dtype=bool), L, L)}
    for wf, wr in windows:
        hosts[f"{wf}x{wr}"] = local_attention_plan(GRID, fsi, gfi, wf, wr)
    plans = {key: ops.AttnSparsePlan(h.row_ptr, h.tiles, L, L, dev) for key, h in hosts.items()}
    sides = [("dense_lazy", dense_lazy), ("dense_default", dense_default)]
    sides += [(key, (lambda p: lambda: ops.attention_fwd_sparse(q, k, vt, H, p, k_len=L, out=out, q_prescaled=True))(p)) for key, p in plans.items()]
    times = alternate(sides, args.rounds, "launch")
    dense_lazy()
    lazy_variant = ops.get_tuning("last_attn_variant")
    dense_default()
    default_variant = ops.get_tuning("last_attn_variant")
    t_lazy = min(times["dense_lazy"])
    flops = 4.0 * L * L * C
    launch = {"dense_lazy_ms": round(t_lazy, 3), "dense_lazy_variant": _lib.attn_variant_name(lazy_variant),
              "dense_lazy_pflops": round(flops / t_lazy / 1e12, 3),
              "dense_default_ms": round(min(times["dense_default"]), 3), "dense_default_variant": _lib.attn_variant_name(default_variant),
              "spread_dense_lazy_pct": round(100 * (max(times["dense_lazy"]) - t_lazy) / t_lazy, 2), "plans": {}}
    for key, h in hosts.items():
        ts = min(times[key])
        per_block = np.diff(h.row_ptr)
        launch["plans"][key] = {"density": round(h.density, 5), "tiles_per_block_min": int(per_block.min()), "tiles_per_block_max": int(per_block.max()),
                                "ms": round(ts, 3), "ms_rounds": [round(v, 3) for v in times[key]],
                                "over_dense_lazy": round(ts / t_lazy, 4), "over_dense_default": round(ts / min(times["dense_default"]), 4),
                                "efficiency": round(ts / (h.density * t_lazy), 4)}
    result["launch"] = launch
    del q, k, vt, out, plans

    # ---- (b) one 14B step
    if not args.launch_only:
        dim, ffn = 5120, 13824
        model = WanTransformer3DModel(dim=dim, ffn_dim=ffn, num_heads=H, num_layers=args.layers)
        model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=dim, ffn_dim=ffn, num_layers=args.layers), device=dev)
        model.cache_context = True
        model.mask_source_frames = model.skip_source_frames = N_SRC
        ctx = torch.randn(37, 4096, device=dev, generator=g).bfloat16()
        t = torch.tensor([500], device=dev)
        lat = torch.randn(1, 16, GRID[0], 2 * GRID[1], 2 * GRID[2], device=dev, generator=g).bfloat16()
        wf, wr = (int(v) for v in args.step_window.split("x"))

        def step(local):
            if local:
                model.enable_local_attention(wf, wr)
            else:
                model.disable_local_attention()
            return model(lat, t, [ctx], L, frame_split_indices=fsi, ground_frame_indices=gfi)

        times = alternate([("dense", lambda: step(False)), ("local", lambda: step(True))], args.rounds, "step")
        d, s = min(times["dense"]), min(times["local"])
        result["step"] = {"layers": args.layers, "window": [wf, wr], "density": round(model._local_plan_last.density, 5),
                          "dense_ms": [round(v, 1) for v in times["dense"]], "local_ms": [round(v, 1) for v in times["local"]],
                          "dense_ms_min": round(d, 1), "local_ms_min": round(s, 1), "local_over_dense": round(s / d, 4),
                          "spread_dense_pct": round(100 * (max(times["dense"]) - d) / d, 2),
                          "note": "the last block's suffix form (skip_source_frames) stays dense in both arms"}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    with open(args.log, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
