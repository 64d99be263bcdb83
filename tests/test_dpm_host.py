"""FlowDPMSolverMultistepScheduler (videocof_amd/fm_solvers.py), host path (CPU tensors), against what the reference's
``FlowDPMSolverMultistepScheduler`` computed (tests/golden/dit_g15_*, tools/gen_golden_dpm.py): schedules, per-step
trajectories of 1 152 configurations, the steps where the reference cannot go on, seeded SDE noise, and the call surface."""
import inspect
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch

from videocof_amd import FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, get_sampling_sigmas, retrieve_timesteps
from videocof_amd.weights import det_uniform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the sweep of tools/gen_golden_dpm.py, in its order (the fixtures key configuration k as c<k>_*)
SHAPE = (1, 2, 2, 2, 4)
STEPS = (1, 2, 3, 4, 5, 7, 20, 50)
SHIFTS = (1.0, 3.0, 5.0)
ALGOS = ("dpmsolver++", "sde-dpmsolver++")
SEED0 = 1500
CONFIGS = list(itertools.product(ALGOS, (1, 2, 3), STEPS, SHIFTS, ("midpoint", "heun"), (True, False), (False, True)))


def sweep_file(algo, order):
    return f"dit_g15_sweep_{algo.replace('-', '_').replace('+', 'p')}_o{order}"


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def inputs():
    return det_uniform("g15.x", SHAPE, 1.0), [det_uniform(f"g15.v{i}", SHAPE, 1.0) for i in range(max(STEPS))]


def make(algo, order, n, shift, st, lof, eaf):
    s = FlowDPMSolverMultistepScheduler(shift=1.0, solver_order=order, solver_type=st, algorithm_type=algo,
                                        lower_order_final=lof, euler_at_final=eaf)
    retrieve_timesteps(s, device="cpu", sigmas=get_sampling_sigmas(n, shift))
    return s


def test_schedules_equal_the_references(golden):
    g = golden("dit_g15_sched")
    for k, cfg in enumerate(CONFIGS):
        _, _, n, shift = cfg[:4]
        s = make(*cfg)
        assert s.timesteps.dtype == torch.int64 and s.sigmas.dtype == torch.float32 and s.sigmas.device.type == "cpu"
        assert torch.equal(s.timesteps, torch.from_numpy(g[f"n{n}_s{int(shift)}_timesteps"])), cfg
        assert torch.equal(s.sigmas, torch.from_numpy(g[f"n{n}_s{int(shift)}_sigmas"])), cfg
    s = make("dpmsolver++", 2, 4, 3.0, "midpoint", True, False)
    assert s.timesteps.tolist() == [1000, 900, 750, 500] and s.sigmas.tolist() == [1.0, 0.8999999761581421, 0.75, 0.5, 0.0]


@pytest.mark.parametrize("algo,order", list(itertools.product(ALGOS, (1, 2, 3))))
def test_sweep_trajectories_match_the_reference(golden, inputs, algo, order):
    """Every configuration of the sweep: rel-L2 <= 1e-5 per step wherever the reference's trajectory is finite; the mirror
    raises NotImplementedError exactly where the reference raised (sde-dpmsolver++ at its first third-order step) and nowhere
    else; seeded SDE runs leave the generator in the reference's state."""
    g = golden(sweep_file(algo, order))
    x, vs = inputs
    compared = raised = 0
    for k, cfg in enumerate(CONFIGS):
        if cfg[:2] != (algo, order):
            continue
        want, ref_raised, ref_nonfinite = g[f"c{k}_traj"], int(g[f"c{k}_raised"]), int(g[f"c{k}_nonfinite"])
        s = make(*cfg)
        gen = torch.Generator().manual_seed(SEED0 + k) if algo.startswith("sde") else None
        cur, got_raised = x.clone(), -1
        for i, t in enumerate(s.timesteps):
            try:
                cur = s.step(vs[i], t, cur, generator=gen, return_dict=False)[0]
            except NotImplementedError as e:
                assert "third-order" in str(e)
                got_raised = i
                break
            assert cur.dtype == torch.float32
            if ref_nonfinite < 0 or i < ref_nonfinite:
                assert rel_l2(cur, want[i]) <= 1e-5, (cfg, i, rel_l2(cur, want[i]))
        assert got_raised == ref_raised, (cfg, got_raised, ref_raised)
        if gen is not None:
            assert torch.equal(torch.rand(4, generator=gen), torch.from_numpy(g[f"c{k}_gen_after"])), cfg
        compared += 1
        raised += got_raised >= 0
    assert compared == 192
    assert raised == (108 if (algo, order) == ("sde-dpmsolver++", 3) else 0)


def test_four_step_cli_setting_runs_with_sde_order_3(inputs):
    """With 4 steps and lower_order_final (the default) the third-order update is never reached: the SDE order-3 run completes."""
    x, vs = inputs
    s = make("sde-dpmsolver++", 3, 4, 3.0, "midpoint", True, False)
    cur = x
    for i, t in enumerate(s.timesteps):
        cur = s.step(vs[i], t, cur, generator=torch.Generator().manual_seed(i), return_dict=False)[0]
    assert torch.isfinite(cur).all()


def test_variance_noise_equals_the_generator_draws(inputs):
    x, vs = inputs
    a, b = make("sde-dpmsolver++", 2, 5, 3.0, "heun", True, False), make("sde-dpmsolver++", 2, 5, 3.0, "heun", True, False)
    gen = torch.Generator().manual_seed(7)
    ca = cb = x
    for i, t in enumerate(a.timesteps):
        ca = a.step(vs[i], t, ca, generator=gen).prev_sample
    gen = torch.Generator().manual_seed(7)
    for i, t in enumerate(b.timesteps):
        cb = b.step(vs[i], t, cb, variance_noise=torch.randn(SHAPE, generator=gen, dtype=torch.float32)).prev_sample
    assert torch.equal(ca, cb)


def test_bf16_dtypes_follow_the_reference(inputs):
    """x0 (the history) in the promoted dtype of sample and model output, prev_sample in the model output's dtype."""
    x, vs = inputs
    s = make("dpmsolver++", 2, 4, 3.0, "midpoint", True, False)
    out = s.step(vs[0].bfloat16(), s.timesteps[0], x.bfloat16(), return_dict=False)[0]
    assert out.dtype == torch.bfloat16 and s.model_outputs[-1].dtype == torch.bfloat16
    out = s.step(vs[1].bfloat16(), s.timesteps[1], x, return_dict=False)[0]
    assert out.dtype == torch.bfloat16 and s.model_outputs[-1].dtype == torch.float32


def test_signatures_equal_the_references():
    with open(os.path.join(GOLDEN, "dit_g15_dpm_surface.json")) as f:
        ref = json.load(f)

    def sig(fn):
        ps = [p for p in inspect.signature(fn).parameters.values() if p.kind not in (p.VAR_POSITIONAL, p.VAR_KEYWORD)]
        return [[p.name, None if p.default is p.empty else repr(p.default)] for p in ps]

    C = FlowDPMSolverMultistepScheduler
    mine = {f"FlowDPMSolverMultistepScheduler.{m}": sig(getattr(C, m)) for m in
            ("__init__", "set_timesteps", "step", "scale_model_input", "add_noise", "index_for_timestep", "set_begin_index")}
    mine["get_sampling_sigmas"] = sig(get_sampling_sigmas)
    mine["retrieve_timesteps"] = sig(retrieve_timesteps)
    assert mine == ref


def test_config_remapping_and_from_unipc_config():
    s = FlowDPMSolverMultistepScheduler(solver_type="bh1", algorithm_type="deis")
    assert s.config.solver_type == "midpoint" and s.config["algorithm_type"] == "dpmsolver++"
    assert s.config.lambda_min_clipped == -math.inf and len(s.config) == 16 and s.order == 1 and len(s) == 1000
    u = FlowUniPCMultistepScheduler(shift=1, solver_order=3)
    d = FlowDPMSolverMultistepScheduler.from_config(u.config)
    assert isinstance(d, FlowDPMSolverMultistepScheduler)
    assert d.config.solver_type == "midpoint" and d.config.solver_order == 3 and d.config.shift == 1
    d = FlowDPMSolverMultistepScheduler.from_config(u.config, algorithm_type="sde-dpmsolver++", solver_order=2)
    assert d.config.algorithm_type == "sde-dpmsolver++" and d.config.solver_order == 2


@pytest.mark.parametrize("kw,exc", [
    (dict(final_sigmas_type="sigma_min"), NotImplementedError),
    (dict(algorithm_type="dpmsolver", final_sigmas_type="sigma_min"), NotImplementedError),
    (dict(algorithm_type="sde-dpmsolver", final_sigmas_type="sigma_min"), NotImplementedError),
    (dict(algorithm_type="dpmsolver"), ValueError),
    (dict(algorithm_type="sde-dpmsolver"), ValueError),
    (dict(thresholding=True), NotImplementedError),
    (dict(use_dynamic_shifting=True), NotImplementedError),
    (dict(prediction_type="epsilon"), ValueError),
    (dict(solver_order=4), ValueError),
    (dict(algorithm_type="ddim"), NotImplementedError),
    (dict(solver_type="euler"), NotImplementedError),
    (dict(final_sigmas_type="other"), ValueError),
])
def test_refused_configurations_raise(kw, exc):
    with pytest.raises(exc):
        FlowDPMSolverMultistepScheduler(**kw)


def test_step_index_rules_and_add_noise(inputs):
    x, vs = inputs
    s = make("dpmsolver++", 2, 4, 3.0, "midpoint", True, False)
    with pytest.raises(ValueError, match="set_timesteps"):
        FlowDPMSolverMultistepScheduler().step(vs[0], 1000, x)
    assert s.index_for_timestep(900) == 1
    assert s.index_for_timestep(5, torch.tensor([9, 5, 5, 1])) == 2          # second position
    noisy = s.add_noise(x, vs[0], torch.tensor([750]))
    assert torch.allclose(noisy, 0.25 * x + 0.75 * vs[0])
    s.set_begin_index(0)
    assert s.begin_index == 0 and s.step_index is None
    s.step(vs[0], s.timesteps[0], x)
    assert s.step_index == 1
    s._reset()
    assert s.step_index is None and s.begin_index is None and s.lower_order_nums == 0
    assert s.scale_model_input(x, 3) is x
