#!/usr/bin/env python3
"""Generate tests/golden/dit_g15_*.npz + tests/golden/dit_g15_dpm_surface.json from the REFERENCE's
``FlowDPMSolverMultistepScheduler`` (``videox_fun/utils/fm_solvers.py``), where the reference tree is available.

    python tools/gen_golden_dpm.py

The reference is loaded through ``oracle/ref_import.py`` (diffusers stubs + load-by-path).  ``fm_solvers.py`` also
imports ``diffusers.utils.torch_utils.randn_tensor``; the stub installed here is diffusers' behaviour (draw on the
generator's device, then move).  Fixtures:

- ``dit_g15_sched``: timesteps / sigmas of ``retrieve_timesteps(s, sigmas=get_sampling_sigmas(n, shift))`` per (steps, shift).
- ``dit_g15_sweep_<algo>_o<order>``: the per-step trajectory of every configuration of the sweep below, on a 32-element latent
  with fixed model outputs ``det_uniform("g15.v<i>")``; the step at which the reference raised (-1: never) or first went
  non-finite (-1: never); SDE noise from ``torch.Generator().manual_seed(SEED0 + k)`` and, after the loop, 4 draws from it.
- ``dit_g15_loop_{det,sde,cfg}``: the 4-step CoF denoise loop of ``dit_g8_cof_loop`` (same inputs, by name) with the DPM++
  scheduler (``solver_order=2``, shift 3): ``dpmsolver++``, ``sde-dpmsolver++`` under ``torch.Generator().manual_seed(LOOP_SEED)``,
  and a 3-step CFG variant (guidance 5, shift 5, the negative prompt of ``dit_g8b_cfg_loop``).
- ``dit_g15_dpm_surface.json``: parameter names and default reprs of the class's methods the mirror implements and of the two
  module functions (names only).
"""
from __future__ import annotations

import inspect
import itertools
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from oracle.gen_golden import TINY, build_ref_model, save  # noqa: E402
from videocof_amd.weights import deterministic_dit_state_dict, det_uniform  # noqa: E402

SHAPE = (1, 2, 2, 2, 4)
STEPS = (1, 2, 3, 4, 5, 7, 20, 50)
SHIFTS = (1.0, 3.0, 5.0)
ORDERS = (1, 2, 3)
SOLVER_TYPES = ("midpoint", "heun")
ALGOS = ("dpmsolver++", "sde-dpmsolver++")
SEED0 = 1500
LOOP_SEED = 15


def sweep_configs():
    """Every configuration of the sweep, in a fixed order: (algo, order, steps, shift, solver_type, lower_order_final, euler_at_final)."""
    return list(itertools.product(ALGOS, ORDERS, STEPS, SHIFTS, SOLVER_TYPES, (True, False), (False, True)))


def _randn_tensor(shape, generator=None, device=None, dtype=None, layout=None):
    """diffusers.utils.torch_utils.randn_tensor: draw on the generator's device (a list: one generator per batch entry), then move."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    layout = layout or torch.strided
    rand_device = device
    batch = shape[0]
    if generator is not None:
        gen_type = generator[0].device.type if isinstance(generator, list) else generator.device.type
        if gen_type != device.type and gen_type == "cpu":
            rand_device = torch.device("cpu")
        elif gen_type != device.type and gen_type == "cuda":
            raise ValueError(f"Cannot generate a {device} tensor from a generator of type {gen_type}.")
    if isinstance(generator, list) and len(generator) == 1:
        generator = generator[0]
    if isinstance(generator, list):
        shape = (1,) + tuple(shape[1:])
        out = [torch.randn(shape, generator=generator[i], device=rand_device, dtype=dtype, layout=layout) for i in range(batch)]
        return torch.cat(out, dim=0).to(device)
    return torch.randn(shape, generator=generator, device=rand_device, dtype=dtype, layout=layout).to(device)


def load_dpm():
    ns = ref_import.load_reference()          # installs the diffusers stubs
    if "diffusers.utils.torch_utils" not in sys.modules:
        m = types.ModuleType("diffusers.utils.torch_utils")
        m.randn_tensor = _randn_tensor
        sys.modules["diffusers.utils.torch_utils"] = m
    ns.dpm = ref_import._load_by_path("videox_fun.utils.fm_solvers", "videox_fun/utils/fm_solvers.py")
    return ns


def _sig(fn):
    ps = [p for p in inspect.signature(fn).parameters.values() if p.kind not in (p.VAR_POSITIONAL, p.VAR_KEYWORD)]
    return [[p.name, None if p.default is p.empty else repr(p.default)] for p in ps]


def main():
    torch.set_num_threads(8)
    ns = load_dpm()
    D = ns.dpm
    Cls = D.FlowDPMSolverMultistepScheduler

    # ---- surface (names and default reprs only)
    surface = {f"FlowDPMSolverMultistepScheduler.{m}": _sig(getattr(Cls, m)) for m in
               ("__init__", "set_timesteps", "step", "scale_model_input", "add_noise", "index_for_timestep", "set_begin_index")}
    surface["get_sampling_sigmas"] = _sig(D.get_sampling_sigmas)
    surface["retrieve_timesteps"] = _sig(D.retrieve_timesteps)
    with open(os.path.join(ROOT, "tests", "golden", "dit_g15_dpm_surface.json"), "w") as f:
        json.dump(surface, f, indent=1, sort_keys=True)
        f.write("\n")

    # ---- schedules per (steps, shift)
    sched = {}
    for n, shift in itertools.product(STEPS, SHIFTS):
        s = Cls(shift=1.0)
        ts, _ = D.retrieve_timesteps(s, device="cpu", sigmas=D.get_sampling_sigmas(n, shift))
        sched[f"n{n}_s{int(shift)}_timesteps"] = ts
        sched[f"n{n}_s{int(shift)}_sigmas"] = s.sigmas
    save("dit_g15_sched", **sched)

    # ---- sweep
    x = det_uniform("g15.x", SHAPE, 1.0)
    vs = [det_uniform(f"g15.v{i}", SHAPE, 1.0) for i in range(max(STEPS))]
    files = {}
    n_raise = n_ok = 0
    for k, (algo, order, n, shift, st, lof, eaf) in enumerate(sweep_configs()):
        s = Cls(shift=1.0, solver_order=order, solver_type=st, algorithm_type=algo, lower_order_final=lof, euler_at_final=eaf)
        D.retrieve_timesteps(s, device="cpu", sigmas=D.get_sampling_sigmas(n, shift))
        gen = torch.Generator().manual_seed(SEED0 + k) if algo.startswith("sde") else None
        cur, traj, raised, nonfinite = x.clone(), [], -1, -1
        for i, t in enumerate(s.timesteps):
            try:
                cur = s.step(vs[i], t, cur, generator=gen, return_dict=False)[0]
            except UnboundLocalError:
                raised = i
                break
            traj.append(cur)
            if nonfinite < 0 and not bool(torch.isfinite(cur).all()):
                nonfinite = i
        n_raise += raised >= 0
        n_ok += raised < 0 and nonfinite < 0
        d = files.setdefault(f"dit_g15_sweep_{algo.replace('-', '_').replace('+', 'p')}_o{order}", {})
        d[f"c{k}_traj"] = torch.stack(traj) if traj else torch.zeros((0,) + SHAPE)
        d[f"c{k}_raised"] = np.int64(raised)
        d[f"c{k}_nonfinite"] = np.int64(nonfinite)
        if gen is not None:
            d[f"c{k}_gen_after"] = torch.rand(4, generator=gen)
    for name, d in files.items():
        save(name, **d)
    print(f"sweep: {len(sweep_configs())} configurations, {n_ok} finite, {n_raise} raised")

    # ---- the CoF denoise loop on the tiny reference model (inputs of dit_g8_cof_loop, by name)
    sd = deterministic_dit_state_dict(**TINY)
    model = build_ref_model(ns, sd)
    src = det_uniform("g8.src", (1, 16, 3, 12, 20), 1.0)
    noise = det_uniform("g8.noise", (1, 16, 4, 12, 20), 1.7)
    ctx = [det_uniform("g6.ctx", (37, TINY["text_dim"]), 1.0)]
    neg = [det_uniform("g8.neg", (9, TINY["text_dim"]), 1.0)]
    seq_len, cc, G = 7 * 6 * 10, 3, 1

    @torch.no_grad()
    def loop(algo, n, shift, scale):
        sch = Cls(shift=1.0, solver_order=2, algorithm_type=algo)
        timesteps, _ = D.retrieve_timesteps(sch, device="cpu", sigmas=D.get_sampling_sigmas(n, shift))
        gen = torch.Generator().manual_seed(LOOP_SEED) if algo.startswith("sde") else None
        latents = torch.cat([src, noise], dim=2)
        steps = []
        for tt in timesteps:
            if scale > 1.0:
                v = model(x=torch.cat([latents] * 2), context=neg + ctx, t=tt.expand(2), seq_len=seq_len,
                          frame_split_indices=[cc] * 2, ground_frame_indices=[(cc, cc + G)] * 2)
                vu, vt = v.chunk(2)
                v = vu + scale * (vt - vu)
            else:
                v = model(x=latents, context=ctx, t=tt.expand(1), seq_len=seq_len,
                          frame_split_indices=[cc], ground_frame_indices=[(cc, cc + G)])
            v[:, :, :cc] = 0
            latents = sch.step(v, tt, latents, generator=gen, return_dict=False)[0]
            steps.append(latents)
        return torch.stack(steps), timesteps

    det, ts4 = loop("dpmsolver++", 4, 3.0, 1.0)
    sde, _ = loop("sde-dpmsolver++", 4, 3.0, 1.0)
    cfg, ts3 = loop("dpmsolver++", 3, 5.0, 5.0)
    save("dit_g15_loop_det", steps=det, timesteps=ts4)
    save("dit_g15_loop_sde", steps=sde, timesteps=ts4, seed=np.int64(LOOP_SEED))
    save("dit_g15_loop_cfg", steps=cfg, timesteps=ts3)


if __name__ == "__main__":
    main()
