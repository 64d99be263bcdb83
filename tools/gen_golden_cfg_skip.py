#!/usr/bin/env python3
"""Generate tests/golden/dit_g16_cfg_skip_*.npz from the REFERENCE model with ``enable_cfg_skip``
(``videox_fun/models/wan_transformer3d.py:752-771``, the ``@cfg_skip()`` decorator of ``videox_fun/utils/cfg_optimization.py``),
where the reference tree is available.

    python tools/gen_golden_cfg_skip.py

The reference is loaded through ``oracle/ref_import.py``; the model is the tiny fixture model of ``oracle/gen_golden.py``
(integer-hash weights).  How many samples a forward really computed is observed, not derived: a pre-hook on the first block
records the batch size of the token stream.  Fixtures:

- ``dit_g16_cfg_skip_fwd_b{2,3}``: one CoF forward at B = 2 / B = 3 with ``enable_cfg_skip(r, 8)`` for r in 0.25, 0.5, 1.0 at
  ``current_steps`` on both sides of each boundary (r = 1.0: the first and the last step -- every step is inside).  Per case:
  ratio, n, step, batch, ``halved`` (the blocks saw fewer samples than the call had), ``halves_equal`` (the two halves of the
  result are the same bits), the result's sample count.  The results themselves are stored once: every not-halved case returned
  the bits of ``out_full``, every halved case ``cat([out_half, out_half])`` (asserted here before anything is written).
- ``dit_g16_cfg_skip_loop_{unipc_r25,unipc_r50,dpm_r25}``: 8-step CFG denoise loops (guidance 5, shift 5, CoF layout, the inputs
  of ``dit_g8_cof_loop`` / ``dit_g8b_cfg_loop`` by name) in the glue of pipeline_wan.py:694-740 -- ``current_steps = i``, the
  doubled batch, guidance, the CoF mask, the scheduler step -- with the latents after every step and the steps in which the
  blocks saw one sample.
- ``dit_g16_cfg_skip_teacache``: 8 forwards at B = 2 with TeaCache AND cfg_skip (ratio 0.625) on a smaller latent: the outputs
  (conditional half only where the step was halved), ``should_calc`` and the accumulated distance per step.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import TINY, build_ref_model, save  # noqa: E402
from tools.gen_golden_dpm import load_dpm  # noqa: E402
from videocof_amd.weights import deterministic_dit_state_dict, det_uniform  # noqa: E402

N = 8
FWD_CASES = ((0.25, 5), (0.25, 6), (0.5, 3), (0.5, 4), (1.0, 0), (1.0, 7))
CTX_LEN = (9, 37, 21)
TEA_COEFF = [0.5, -0.25, 1.0, 0.01]          # the mild cubic of oracle/gen_golden_teacache.py (same reason)
TEA_TS = [999, 937, 857, 749, 599, 374, 250, 120]


class Seen:
    """Batch size of the token stream entering the first block, per forward."""

    def __init__(self, model):
        self.sizes = []
        model.blocks[0].register_forward_pre_hook(self._hook, with_kwargs=True)

    def _hook(self, module, args, kwargs):
        x = args[0] if args else kwargs["x"]
        self.sizes.append(int(x.shape[0]))


@torch.no_grad()
def main():
    torch.set_num_threads(8)
    ns = load_dpm()
    sd = deterministic_dit_state_dict(**TINY)
    model = build_ref_model(ns, sd)
    seen = Seen(model)
    seq_len, cc, G = 7 * 6 * 10, 3, 1

    # ---- single forwards
    lat = det_uniform("g16.lat", (3, 16, 7, 12, 20), 1.0)
    ctx = [det_uniform(f"g16.ctx{b}", (CTX_LEN[b], TINY["text_dim"]), 1.0) for b in range(3)]
    for B in (2, 3):
        def fwd():
            seen.sizes.clear()
            out = model(lat[:B], torch.tensor([749] * B), ctx[:B], seq_len, frame_split_indices=[cc] * B,
                        ground_frame_indices=[(cc, cc + G)] * B)
            return out, seen.sizes[-1]
        model.disable_cfg_skip()
        out_full, nb = fwd()
        assert nb == B and out_full.shape[0] == B
        out_half, meta = None, []
        for r, step in FWD_CASES:
            model.enable_cfg_skip(r, N)
            model.current_steps = step
            out, nb = fwd()
            halved = nb < B
            if halved:
                h = out.shape[0] // 2
                eq = bool(torch.equal(out[:h], out[h:]))
                if out_half is None:
                    out_half = out[:h].clone()
                assert eq and torch.equal(out[:h], out_half) and nb == h
            else:
                eq = bool(out.shape[0] % 2 == 0 and torch.equal(out[:out.shape[0] // 2], out[out.shape[0] // 2:]))
                assert torch.equal(out, out_full)
            meta.append((r, N, step, B, int(halved), int(eq), out.shape[0]))
            print(f"B={B} ratio={r} step={step}: blocks saw {nb}, result {tuple(out.shape)}, halved={halved}, halves_equal={eq}")
        model.disable_cfg_skip()
        save(f"dit_g16_cfg_skip_fwd_b{B}", t=np.array([749] * B), ctx_len=np.array(CTX_LEN[:B]),
             cases=np.array(meta, dtype=np.float64), case_fields=np.array(["ratio", "n", "step", "batch", "halved", "halves_equal", "rows"]),
             out_full=out_full, out_half=out_half)

    # ---- CFG denoise loops
    src = det_uniform("g8.src", (1, 16, 3, 12, 20), 1.0)
    noise = det_uniform("g8.noise", (1, 16, 4, 12, 20), 1.7)
    pos = [det_uniform("g6.ctx", (37, TINY["text_dim"]), 1.0)]
    neg = [det_uniform("g8.neg", (9, TINY["text_dim"]), 1.0)]

    def loop(kind, ratio, scale=5.0, shift=5.0):
        if kind == "unipc":
            sch = ns.unipc.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, solver_order=2, prediction_type="flow_prediction")
            sch.set_timesteps(N, device="cpu", shift=shift)
            timesteps = sch.timesteps
        else:
            sch = ns.dpm.FlowDPMSolverMultistepScheduler(shift=1.0, solver_order=2, algorithm_type="dpmsolver++")
            timesteps, _ = ns.dpm.retrieve_timesteps(sch, device="cpu", sigmas=ns.dpm.get_sampling_sigmas(N, shift))
        model.enable_cfg_skip(ratio, N)
        latents = torch.cat([src, noise], dim=2)
        steps, halved = [], []
        for i, tt in enumerate(timesteps):
            model.current_steps = i                                           # pipeline_wan.py:695
            seen.sizes.clear()
            v = model(x=torch.cat([latents] * 2), context=neg + pos, t=tt.expand(2), seq_len=seq_len,
                      frame_split_indices=[cc] * 2, ground_frame_indices=[(cc, cc + G)] * 2)
            if seen.sizes[-1] == 1:
                halved.append(i)
            vu, vt = v.chunk(2)
            v = vu + scale * (vt - vu)
            v[:, :, :cc] = 0
            latents = sch.step(v, tt, latents, return_dict=False)[0]
            steps.append(latents)
        model.disable_cfg_skip()
        print(f"loop {kind} ratio={ratio}: halved steps {halved}")
        return dict(steps=torch.stack(steps), timesteps=timesteps, halved_steps=np.array(halved, dtype=np.int64),
                    ratio=ratio, n=N, guidance=scale, shift=shift)

    save("dit_g16_cfg_skip_loop_unipc_r25", **loop("unipc", 0.25))
    save("dit_g16_cfg_skip_loop_unipc_r50", **loop("unipc", 0.5))
    save("dit_g16_cfg_skip_loop_dpm_r25", **loop("dpm", 0.25))

    # ---- TeaCache together with cfg_skip (wan_transformer3d.py:956-1031 on a halved batch)
    lat0 = det_uniform("g16.tea.lat", (2, 16, 5, 8, 12), 1.0)
    dl = det_uniform("g16.tea.dlat", (2, 16, 5, 8, 12), 0.15)
    tea_ratio = 0.625          # boundary at step 3: a step TeaCache skips, so the halved batch meets a full-batch residual

    def tea_run(thresh):
        model.enable_teacache(TEA_COEFF, len(TEA_TS), thresh, num_skip_start_steps=1, offload=False)
        model.enable_cfg_skip(tea_ratio, len(TEA_TS))
        outs, calc, acc, halved = [], [], [], []
        for i, t in enumerate(TEA_TS):
            model.current_steps = i
            out = model(lat0 + i * dl, t=torch.tensor([t, t]), context=ctx[:2], seq_len=5 * 4 * 6, frame_split_indices=[2, 2],
                        ground_frame_indices=[(2, 3), (2, 3)])
            assert out.shape[0] == 2
            calc.append(bool(model.should_calc))
            acc.append(float(model.teacache.accumulated_rel_l1_distance) if model.teacache.cnt else -1.0)
            # (a step whose blocks TeaCache skipped never reaches the hook: the rule is read off the result instead)
            is_half = bool(torch.equal(out[0], out[1]))
            halved.append(is_half)
            outs.append(out[1:] if is_half else out)
        model.disable_teacache()
        model.disable_cfg_skip()
        print(f"teacache({thresh}) + cfg_skip: calc", calc, "halved", halved, "acc", [round(a, 4) for a in acc])
        return outs, calc, acc, halved

    for th in (0.05, 0.2, 0.6, 2.0):
        tea_run(th)
    # the threshold must leave a step that re-applies, on the halved batch, a residual taken at the full batch
    thresh = float(os.environ.get("G16_THRESH", "2.0"))
    outs, calc, acc, halved = tea_run(thresh)
    arrs = {f"out{i}": o for i, o in enumerate(outs)}
    save("dit_g16_cfg_skip_teacache", ts=np.array(TEA_TS), coeff=np.array(TEA_COEFF), thresh=thresh, ratio=tea_ratio,
         calc=np.array(calc), acc=np.array(acc), halved=np.array(halved), **arrs)


if __name__ == "__main__":
    main()
