"""-m gpu: the flow DPM-Solver++ sampler on the MI355X -- the fused step kernel (wan_solver_step) against an fp64 composition of
its inputs, the scheduler's device path against its host path and against the trajectories captured from the reference
(tests/golden/dit_g15_*, tools/gen_golden_dpm.py), one launch per step, and WanPipeline with the DPM++ scheduler on the tiny
model against the reference's denoise loops (deterministic, SDE, CFG), eager and under graph capture."""
import itertools

import numpy as np
import pytest
import torch

from videocof_amd import (FlowDPMSolverMultistepScheduler, WanPipeline, WanTransformer3DModel, _lib, get_sampling_sigmas, ops,
                          retrieve_timesteps)
from videocof_amd.weights import deterministic_dit_state_dict, det_uniform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(dim=256, ffn_dim=512, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)

# the sweep of tools/gen_golden_dpm.py, in its order (the fixtures key configuration k as c<k>_*)
SHAPE = (1, 2, 2, 2, 4)
STEPS = (1, 2, 3, 4, 5, 7, 20, 50)
ALGOS = ("dpmsolver++", "sde-dpmsolver++")
SEED0 = 1500
CONFIGS = list(itertools.product(ALGOS, (1, 2, 3), STEPS, (1.0, 3.0, 5.0), ("midpoint", "heun"), (True, False), (False, True)))
HEADLINE_N = 16 * 43 * 60 * 104 + 7          # the headline latent [1, 16, 43, 60, 104] (4.3 M elements) and a tail that is not a whole packet


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def cosine(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm()))


def sweep_file(algo, order):
    return f"dit_g15_sweep_{algo.replace('-', '_').replace('+', 'p')}_o{order}"


def make(algo, order, n, shift, st, lof, eaf, device):
    s = FlowDPMSolverMultistepScheduler(shift=1.0, solver_order=order, solver_type=st, algorithm_type=algo,
                                        lower_order_final=lof, euler_at_final=eaf)
    retrieve_timesteps(s, device=device, sigmas=get_sampling_sigmas(n, shift))
    return s


# ------------------------------------------------------------------ the kernel
COEF = dict(a_s=1.0, a_v=-0.7310585786, c_s=0.3127, c_0=0.6891, c_1=-0.2517, c_2=0.0843, c_n=0.4219)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("hist", [0, 1, 2])
@pytest.mark.parametrize("n", [0, 1, 7, 4097, HEADLINE_N])
def test_solver_step_kernel_vs_fp64(dtype, with_noise, hist, n):
    g = torch.Generator().manual_seed(n * 7 + hist * 2 + int(with_noise))
    ts = [torch.randn(n, generator=g).to(dtype) for _ in range(4)]
    s, v = ts[0], ts[1]
    m1 = ts[2] if hist >= 1 else None
    m2 = ts[3] if hist >= 2 else None
    noise = torch.randn(n, generator=g) if with_noise else None
    d = lambda t: None if t is None else t.to(DEV)
    x0, prev = ops.solver_step(d(s), d(v), COEF["a_s"], COEF["a_v"], d(m1), d(m2), d(noise),
                               COEF["c_s"], COEF["c_0"], COEF["c_1"], COEF["c_2"], COEF["c_n"])
    assert x0.dtype == prev.dtype == dtype and x0.shape == prev.shape == (n,)
    if n == 0:
        return
    # the x0 output: bitwise wan_lincomb's on the same two terms
    assert torch.equal(x0, ops.lincomb([(COEF["a_s"], d(s)), (COEF["a_v"], d(v))], dtype))
    x0c, prevc = x0.cpu().double(), prev.cpu().double()
    f = lambda c: float(np.float32(c))                    # the coefficients as the kernel receives them
    x0_64 = f(COEF["a_s"]) * s.double() + f(COEF["a_v"]) * v.double()
    terms = [f(COEF["c_s"]) * s.double(), f(COEF["c_0"]) * x0c]           # the update reads x0 AS STORED
    terms += [f(COEF["c_1"]) * m1.double()] if m1 is not None else []
    terms += [f(COEF["c_2"]) * m2.double()] if m2 is not None else []
    terms += [f(COEF["c_n"]) * noise.double()] if noise is not None else []
    prev_64 = sum(terms)
    mag = sum(t.abs() for t in terms)
    if dtype == torch.float32:
        assert float(((x0c - x0_64).abs() - 1e-6 * (s.double().abs() + v.double().abs())).max()) <= 0
        assert float(((prevc - prev_64).abs() - 1e-6 * mag).max()) <= 0
        if n >= 7:
            assert rel_l2(x0c, x0_64) <= 1e-6 and rel_l2(prevc, prev_64) <= 1e-6
    else:
        # within one rounding to bf16 (half an ulp: 2^-8 relative) of the fp64 value, plus the fp32 accumulation
        assert float(((x0c - x0_64).abs() - 2.0 ** -8 * x0_64.abs() - 1e-6 * (s.double().abs() + v.double().abs())).max()) <= 0
        assert float(((prevc - prev_64).abs() - 2.0 ** -8 * prev_64.abs() - 1e-6 * mag).max()) <= 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_solver_step_unaligned_views_take_the_element_loop(dtype):
    """Operands that are not 16-byte aligned (a view one element in) give the same values as aligned copies."""
    g = torch.Generator().manual_seed(3)
    n = 4099
    base = [torch.randn(n + 1, generator=g).to(dtype).to(DEV) for _ in range(4)]
    nz = torch.randn(n + 1, generator=g).to(DEV)
    views = [b[1:] for b in base] + [nz[1:]]
    copies = [t.clone() for t in views]
    a = ops.solver_step(views[0], views[1], 1.0, -0.4, views[2], views[3], views[4], 0.2, 0.5, -0.1, 0.05, 0.3)
    b = ops.solver_step(copies[0], copies[1], 1.0, -0.4, copies[2], copies[3], copies[4], 0.2, 0.5, -0.1, 0.05, 0.3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_solver_step_bad_arguments_raise():
    lib = _lib.load()
    st = lib.wan_solver_step(None, None, 0, None, None, None, None, None, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 16, None)
    assert st == _lib.WAN_ERR_INVALID
    with pytest.raises(ValueError, match="null tensor"):
        _lib.check(st, "wan_solver_step")
    x = torch.zeros(16, device=DEV)
    p = lambda t: t.data_ptr()
    st = lib.wan_solver_step(p(x), p(x), 2, p(x), p(x), None, None, None, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 16, None)
    with pytest.raises(ValueError, match="dtype"):
        _lib.check(st, "wan_solver_step")
    st = lib.wan_solver_step(p(x), p(x), 0, p(x), p(x), None, None, None, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1, None)
    with pytest.raises(ValueError, match="n=-1"):
        _lib.check(st, "wan_solver_step")
    st = lib.wan_solver_step(p(x), p(x), 0, p(x), p(x), None, p(x), None, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 16, None)
    with pytest.raises(ValueError, match="m2 without m1"):
        _lib.check(st, "wan_solver_step")
    assert lib.wan_solver_step(p(x), p(x), 0, p(x), p(x), None, None, None, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0, None) == _lib.WAN_OK
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.solver_step(x.cpu(), x.cpu(), 1, 1, None, None, None, 1, 1, 0, 0, 0)
    with pytest.raises(ValueError, match="expected"):
        ops.solver_step(x, x.bfloat16(), 1, 1, None, None, None, 1, 1, 0, 0, 0)
    with pytest.raises(ValueError, match="expected"):
        ops.solver_step(x, x, 1, 1, None, None, x.bfloat16(), 1, 1, 0, 0, 0)
    with pytest.raises(ValueError, match="not supported"):
        ops.solver_step(x.half(), x.half(), 1, 1, None, None, None, 1, 1, 0, 0, 0)
    with pytest.raises(ValueError, match="shape"):
        ops.solver_step(x, x[:8], 1, 1, None, None, None, 1, 1, 0, 0, 0)


# ------------------------------------------------------------------ the scheduler on the device
@pytest.fixture(scope="module")
def inputs():
    return det_uniform("g15.x", SHAPE, 1.0), [det_uniform(f"g15.v{i}", SHAPE, 1.0) for i in range(max(STEPS))]


@pytest.mark.parametrize("algo,order", list(itertools.product(ALGOS, (1, 2, 3))))
def test_device_scheduler_equals_host_and_reference(golden, inputs, algo, order):
    """Every configuration of the sweep, fp32 latents: the device path (one wan_solver_step per step) equals the host path
    (rel-L2 <= 1e-5) and the reference's captured trajectory (rel-L2 <= 1e-5); both draw the SDE noise from the same seeded
    CPU generator and leave it in the reference's state; both refuse at the reference's step."""
    gf = golden(sweep_file(algo, order))
    x, vs = inputs
    compared = 0
    for k, cfg in enumerate(CONFIGS):
        if cfg[:2] != (algo, order):
            continue
        host, dev = make(*cfg, device="cpu"), make(*cfg, device=DEV)
        sde = algo.startswith("sde")
        gh = torch.Generator().manual_seed(SEED0 + k) if sde else None
        gd = torch.Generator().manual_seed(SEED0 + k) if sde else None
        a, b, raised = x.clone(), x.to(DEV), -1
        for i, (th, td) in enumerate(zip(host.timesteps, dev.timesteps)):
            try:
                a = host.step(vs[i], th, a, generator=gh, return_dict=False)[0]
            except NotImplementedError:
                with pytest.raises(NotImplementedError):
                    dev.step(vs[i].to(DEV), td, b, generator=gd)
                raised = i
                break
            b = dev.step(vs[i].to(DEV), td, b, generator=gd, return_dict=False)[0]
            assert b.is_cuda and b.dtype == torch.float32
            assert rel_l2(b, a) <= 1e-5, (cfg, i)
            assert rel_l2(b, gf[f"c{k}_traj"][i]) <= 1e-5, (cfg, i)
        assert raised == int(gf[f"c{k}_raised"]), cfg
        if sde:
            want = torch.from_numpy(gf[f"c{k}_gen_after"])
            assert torch.equal(torch.rand(4, generator=gh), want) and torch.equal(torch.rand(4, generator=gd), want), cfg
        compared += 1
    assert compared == 192


@pytest.mark.parametrize("algo,order,st", [("sde-dpmsolver++", 2, "midpoint"), ("sde-dpmsolver++", 2, "heun"),
                                           ("dpmsolver++", 3, "heun")])
def test_device_variance_noise_equals_host(inputs, algo, order, st):
    x, vs = inputs
    host, dev = make(algo, order, 7, 3.0, st, True, False, "cpu"), make(algo, order, 7, 3.0, st, True, False, DEV)
    g = torch.Generator().manual_seed(11)
    a, b = x.clone(), x.to(DEV)
    for i, (th, td) in enumerate(zip(host.timesteps, dev.timesteps)):
        nz = torch.randn(SHAPE, generator=g)
        a = host.step(vs[i], th, a, variance_noise=nz).prev_sample
        b = dev.step(vs[i].to(DEV), td, b, variance_noise=nz.to(DEV)).prev_sample
        assert rel_l2(b, a) <= 1e-5, i


def test_bf16_latents_stay_bf16_and_close(golden, inputs):
    x, vs = inputs
    for k, cfg in enumerate(CONFIGS):
        if cfg[2] not in (4, 7) or cfg[3] != 3.0 or cfg[0:2] == ("sde-dpmsolver++", 3):
            continue
        gf = golden(sweep_file(*cfg[:2]))
        s = make(*cfg, device=DEV)
        gen = torch.Generator().manual_seed(SEED0 + k) if cfg[0].startswith("sde") else None
        cur = x.to(DEV, torch.bfloat16)
        for i, t in enumerate(s.timesteps):
            cur = s.step(vs[i].to(DEV, torch.bfloat16), t, cur, generator=gen, return_dict=False)[0]
            assert cur.dtype == torch.bfloat16 and s.model_outputs[-1].dtype == torch.bfloat16
        assert rel_l2(cur.float(), gf[f"c{k}_traj"][-1]) < 2e-2, cfg


@pytest.mark.parametrize("algo,order", [("dpmsolver++", 1), ("dpmsolver++", 2), ("dpmsolver++", 3), ("sde-dpmsolver++", 2)])
def test_one_kernel_launch_per_step(algo, order):
    """Each step() on CUDA tensors is ONE kernel on the device (wan_solver_step), the SDE variant included (noise drawn from a
    CPU generator arrives by a copy, not a kernel)."""
    from torch.profiler import ProfilerActivity, profile
    shape = (1, 16, 5, 12, 20)
    s = make(algo, order, 7, 3.0, "midpoint", True, False, DEV)
    s.set_begin_index(0)
    gen = torch.Generator().manual_seed(0) if algo.startswith("sde") else None
    cur = det_uniform("g15.launch.x", shape).to(DEV)
    vs = [det_uniform(f"g15.launch.v{i}", shape).to(DEV) for i in range(7)]
    torch.cuda.synchronize()
    for i, t in enumerate(s.timesteps):
        before = ops.solver_step_launches
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            cur = s.step(vs[i], t, cur, generator=gen, return_dict=False)[0]
            torch.cuda.synchronize()
        kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        assert ops.solver_step_launches == before + 1, i
        assert len(kernels) == 1 and "solver_step" in kernels[0], (i, kernels)


# ------------------------------------------------------------------ WanPipeline with the DPM++ scheduler
@pytest.fixture(scope="module")
def model():
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    m.load_state_dict(deterministic_dit_state_dict(**TINY), device=DEV)
    return m


def _loop_inputs(golden):
    g = golden("dit_g8_cof_loop")
    lat = torch.cat([torch.from_numpy(g["src"]), torch.from_numpy(g["noise"])], dim=2).to(DEV)
    return g, lat, torch.from_numpy(g["ctx"]).to(DEV)


KW = dict(source_frames=9, reasoning_frames=4, guidance_scale=1.0, repeat_rope=True, cot=True, output_type="latent",
          weight_dtype=torch.float32)


@pytest.mark.parametrize("algo,fixture", [("dpmsolver++", "dit_g15_loop_det"), ("sde-dpmsolver++", "dit_g15_loop_sde")])
def test_pipeline_dpm_cof_loop_matches_the_reference(golden, model, algo, fixture):
    g, lat, ctx = _loop_inputs(golden)
    want = golden(fixture)
    pipe = WanPipeline(transformer=model, scheduler=FlowDPMSolverMultistepScheduler(shift=1.0, solver_order=2, algorithm_type=algo))
    gen = torch.Generator().manual_seed(int(want["seed"])) if "seed" in want else None
    seen = []
    out = pipe(latents=lat, prompt_embeds=[ctx], num_inference_steps=4, shift=3, generator=gen,
               callback_on_step_end=lambda p, i, t, kw: seen.append(kw["latents"].clone()) or {}, **KW)
    assert pipe.scheduler.timesteps.cpu().tolist() == want["timesteps"].tolist() == [1000, 900, 750, 500]
    for i in range(4):
        assert rel_l2(seen[i], want["steps"][i]) < 2e-2, i
    assert cosine(out.latents, want["steps"][3]) > 0.9998
    if algo == "dpmsolver++":
        # source frames: algebraically fixed (v = 0 there and sigma_t + alpha_t = 1); the SDE noise moves them, in the reference too
        assert float((out.latents[:, :, :3].cpu() - torch.from_numpy(g["src"])).abs().max()) < 1e-5


def test_pipeline_dpm_cfg_loop_matches_the_reference(golden, model):
    g, lat, ctx = _loop_inputs(golden)
    want = golden("dit_g15_loop_cfg")
    neg = torch.from_numpy(golden("dit_g8b_cfg_loop")["neg"]).to(DEV)
    pipe = WanPipeline(transformer=model, scheduler=FlowDPMSolverMultistepScheduler(shift=1.0, solver_order=2))
    kw = dict(KW, guidance_scale=5.0)
    out = pipe(latents=lat, prompt_embeds=[ctx], negative_prompt_embeds=[neg], num_inference_steps=3, shift=5.0, **kw)
    assert pipe.scheduler.timesteps.cpu().tolist() == want["timesteps"].tolist()
    assert rel_l2(out.latents, want["steps"][2]) < 5e-2 and cosine(out.latents, want["steps"][2]) > 0.999
    assert float((out.latents[:, :, :3].cpu() - torch.from_numpy(g["src"])).abs().max()) < 1e-5


@pytest.mark.parametrize("graph", ["step", "loop"])
def test_pipeline_dpm_graph_capture_is_bit_identical(golden, model, graph):
    """capture_graph 'step' (the scheduler eager between replays) and 'loop' (the scheduler's launches recorded with the loop):
    first call, capturing call and replaying call all give the eager loop's bits, with and without CFG."""
    g, lat, ctx = _loop_inputs(golden)
    neg = (ctx[:9] * 0.5).contiguous()
    mk = lambda: WanPipeline(transformer=model, scheduler=FlowDPMSolverMultistepScheduler(shift=1.0, solver_order=2, solver_type="heun"))

    def run(pipe, capture, scale=1.0):
        return pipe(latents=lat, prompt_embeds=[ctx], negative_prompt_embeds=[neg] if scale > 1 else None, num_inference_steps=4,
                    shift=3, capture_graph=capture, **dict(KW, guidance_scale=scale)).latents

    eager = mk()
    want, want_cfg = run(eager, False), run(eager, False, 3.0)
    graphed = mk()
    for _ in range(3):
        assert torch.equal(run(graphed, graph), want)
    for _ in range(2):
        assert torch.equal(run(graphed, graph, 3.0), want_cfg)
    assert not torch.equal(want, want_cfg)


def test_pipeline_sde_under_loop_capture_raises_and_other_schedulers_are_refused(golden, model):
    _, lat, ctx = _loop_inputs(golden)
    pipe = WanPipeline(transformer=model, scheduler=FlowDPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++"))
    with pytest.raises(NotImplementedError, match="sde-dpmsolver"):
        pipe(latents=lat, prompt_embeds=[ctx], num_inference_steps=2, shift=3, capture_graph="loop",
             generator=torch.Generator().manual_seed(0), **KW)

    class Other:
        config = {}

        def step(self, *a, **k):
            raise AssertionError

    with pytest.raises(NotImplementedError, match="FlowDPMSolverMultistepScheduler"):
        WanPipeline(transformer=model, scheduler=Other())(latents=lat, prompt_embeds=[ctx], num_inference_steps=2, shift=3, **KW)
