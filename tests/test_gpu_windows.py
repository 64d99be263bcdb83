"""-m gpu: temporal context windows -- wan_window_gather / wan_window_blend against their torch float32 definitions (bit for bit,
with guard bands), and the windowed denoise loop of WanPipeline against a loop composed from the CPU oracle, against a loop
composed from the model's own single-window forwards, and against today's path where the clip fits one window.
Bounds and observed values: docs/TEST_BOUNDS.md, "Temporal context windows"."""
import math

import numpy as np
import pytest
import torch

from oracle import wan_oracle as O
from videocof_amd import (FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel, _lib, ops,
                          reference_window_blend, reference_window_gather, window_plan)
from videocof_amd.weights import deterministic_dit_state_dict, det_uniform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(dim=256, ffn_dim=512, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)
CFG = O.DiTConfig(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
POISON = 7.0
PLAN = window_plan(7, 4, 2)            # starts (0, 2, 3): frame 3 is covered by all three windows


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def cosine(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm()))


# ------------------------------------------------------------------------------------------------ kernels
class Guarded:
    """A contiguous tensor of `shape` inside a poisoned flat buffer, `pad` elements of guard band on either side."""

    def __init__(self, shape, dtype, pad=64, fill=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * pad,), POISON, device=DEV, dtype=dtype)
        self.view = self.buf[pad:pad + n].view(shape)
        self.pad, self.n = pad, n
        if fill is not None:
            self.view.copy_(fill)

    def intact(self):
        return bool((self.buf[:self.pad] == POISON).all()) and bool((self.buf[self.pad + self.n:] == POISON).all())


def _values(tag, shape, dtype):
    return det_uniform(tag, shape, 2.0).to(dtype)      # (bf16: rounded once, both sides then hold the same values)


SHAPES = [(3, 5, 64), (4, 8, 64), (4, 8, 3), (24, 44, 64)]      # (h, w, guard elements): 15-element frames are never 16-byte
                                                                  # aligned; (4, 8) is; (4, 8) behind a 3-element band is not
                                                                  # (element-wise form); 24 x 44 needs several workgroups per row


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("h,w,pad", SHAPES)
def test_window_gather_equals_the_torch_definition(h, w, pad, dtype):
    K, n, Fs, C = PLAN.K, PLAN.window, PLAN.frames, 16
    big = h * w > 64
    for B in ((1,) if big else (1, 2)):
        for G in ((1,) if big else (0, 1)):
            state = Guarded((B, C, 2 * Fs + K * G, h, w), dtype, pad, _values(f"win.state{B}{G}", (B, C, 2 * Fs + K * G, h, w), dtype))
            for k0, k1 in ((0, K), (1, K), (1, 2)):
                for rep in (1, 2):
                    want = reference_window_gather(state.view, PLAN, n, G, k0, k1, rep)
                    out = Guarded(want.shape, dtype, pad)
                    got = ops.window_gather(state.view, PLAN.starts, n, G, k0, k1, rep, out=out.view)
                    assert got.data_ptr() == out.view.data_ptr()
                    assert torch.equal(out.view, want), (B, G, k0, k1, rep)
                    assert out.intact() and state.intact()
            # the default arguments: every window, once, into a fresh tensor
            assert torch.equal(ops.window_gather(state.view, PLAN.starts, n, G), reference_window_gather(state.view, PLAN, n, G))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("h,w,pad", SHAPES)
def test_window_blend_equals_the_torch_definition(h, w, pad, dtype):
    K, n, Fs, C = PLAN.K, PLAN.window, PLAN.frames, 16
    alpha = torch.from_numpy(PLAN.alpha).to(DEV)
    big = h * w > 64
    for B in ((1,) if big else (1, 2)):
        for G in ((1,) if big else (0, 1)):
            pred = Guarded((K * B, C, 2 * n + G, h, w), dtype, pad, _values(f"win.pred{B}{G}", (K * B, C, 2 * n + G, h, w), dtype))
            want = reference_window_blend(pred.view, PLAN, G)
            out = Guarded(want.shape, dtype, pad)
            ops.window_blend(pred.view, alpha, PLAN.starts, Fs, G, out=out.view)
            assert torch.equal(out.view, want), (B, G)
            assert out.intact() and pred.intact()
            p = pred.view.view(K, B, C, 2 * n + G, h, w)
            assert not bool(out.view[:, :, :Fs].any())                                     # source frames: the CoF mask
            for k in range(K):                                                             # ground_k: window k's own block
                assert torch.equal(out.view[:, :, Fs + k * G:Fs + (k + 1) * G], p[k][:, :, n:n + G])
            singles = [f for f in range(Fs) if len(PLAN.covering(f)) == 1]
            assert singles == [0, 1, 6] and PLAN.covering(3) == (0, 1, 2)
            for f in singles:                                                              # one window: its prediction unchanged
                k = PLAN.covering(f)[0]
                assert torch.equal(out.view[:, :, Fs + K * G + f], p[k][:, :, n + G + f - PLAN.starts[k]])
            if dtype == torch.float32:
                # and the definition itself is the weighted sum: float64 yardstick, float32 rounding of three terms
                f64 = sum(float(PLAN.alpha[k, 3]) * p[k][:, :, n + G + 3 - PLAN.starts[k]].double() for k in range(K))
                assert float((out.view[:, :, Fs + K * G + 3].double() - f64).abs().max()) <= 6 * 2.0 ** -24 * 2.0


def test_invalid_arguments_return_wan_err_invalid():
    import ctypes
    lib = _lib.load()
    buf = torch.zeros(16 * 9 * 15, device=DEV)
    ok, gap = (ctypes.c_int * 3)(0, 2, 3), (ctypes.c_int * 2)(0, 5)
    p = ctypes.c_void_p(buf.data_ptr())
    # two windows of 4 frames at 0 and 5 leave frame 4 of 9 uncovered; nothing is launched
    assert lib.wan_window_gather(p, p, 0, gap, 2, 0, 2, 1, 1, 9, 4, 0, 15, 1, 0, None) == _lib.WAN_ERR_INVALID
    assert lib.wan_window_blend(p, p, 0, p, gap, 2, 1, 1, 9, 4, 0, 15, None) == _lib.WAN_ERR_INVALID
    assert lib.wan_window_gather(p, p, 0, ok, 3, 2, 2, 1, 1, 7, 4, 0, 15, 1, 0, None) == _lib.WAN_ERR_INVALID      # empty range
    assert lib.wan_window_gather(p, p, 0, ok, 3, 0, 3, 1, 1, 7, 4, 0, 15, 3, 0, None) == _lib.WAN_ERR_INVALID      # rep = 3
    assert lib.wan_window_blend(p, p, 2, p, ok, 3, 1, 1, 7, 4, 0, 15, None) == _lib.WAN_ERR_INVALID                # dtype
    assert lib.wan_window_blend(p, None, 0, p, ok, 3, 1, 1, 7, 4, 0, 15, None) == _lib.WAN_ERR_INVALID
    with pytest.raises(ValueError, match="leave no gap"):
        ops.window_gather(torch.zeros(1, 1, 18, 3, 5, device=DEV), (0, 5), 4, 0)
    with pytest.raises(ValueError, match="leave no gap"):
        ops.window_blend(torch.zeros(2, 1, 8, 3, 5, device=DEV), torch.zeros(2, 9, device=DEV), (0, 5), 9, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.window_gather(torch.zeros(1, 1, 14, 3, 5), PLAN.starts, 4, 0)


# ------------------------------------------------------------------------------------------------ loop
STEPS, SHIFT = 3, 3.0
N, G, FS, K = 4, 1, 7, 3               # temporal_window=13, temporal_overlap=8, source_frames=25 in latent frames
SEQ = math.ceil(4 * 4 / 4 * (2 * N + G))


@pytest.fixture(scope="module")
def sd():
    return deterministic_dit_state_dict(**TINY)


@pytest.fixture()
def model(sd):
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    m.load_state_dict(sd, device=DEV)
    yield m
    m.disable_cfg_skip()
    m.disable_teacache()


def _inputs(fs=FS):
    lat = torch.cat([det_uniform("win.src", (1, 16, 7, 4, 4), 1.0)[:, :, :fs], det_uniform("win.noise", (1, 16, 8, 4, 4), 1.0)[:, :, :fs + G]],
                    dim=2)
    return lat, det_uniform("win.ctx", (37, 64), 1.0), det_uniform("win.neg", (9, 64), 1.0)


def _pipe(model, kind="unipc"):
    if kind == "unipc":
        return WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))
    return WanPipeline(transformer=model, scheduler=FlowDPMSolverMultistepScheduler(shift=1.0, solver_order=2, algorithm_type=kind))


def _run(pipe, scale=1.0, steps_out=None, source_frames=25, shift=SHIFT, dtype=torch.float32, windows=True, fs=FS, **kw):
    lat, ctx, neg = _inputs(fs)
    cb = None
    if steps_out is not None:
        cb = lambda p, i, t, d: steps_out.append(d["latents"].clone()) or {}
    if windows:
        kw = {"temporal_window": 13, "temporal_overlap": 8, **kw}
    return pipe(latents=lat.to(DEV), prompt_embeds=[ctx.to(DEV)], negative_prompt_embeds=[neg.to(DEV)] if scale > 1 else None,
                source_frames=source_frames, reasoning_frames=4, num_inference_steps=STEPS, guidance_scale=scale, shift=shift,
                repeat_rope=True, cot=True, output_type="latent", weight_dtype=dtype, callback_on_step_end=cb, **kw).latents


def _windowed(lat):
    return torch.cat([lat[:, :, :FS]] + [lat[:, :, FS:FS + G]] * K + [lat[:, :, FS + G:]], dim=2)


def _unwindowed(state):
    return torch.cat([state[:, :, :FS + G], state[:, :, FS + K * G:]], dim=2)


def _blend64(preds):
    """The K window predictions [1, 16, 2n + G, 4, 4] (float32, CPU) as the state's prediction, every sum in float64."""
    out = torch.zeros(1, 16, 2 * FS + K * G, 4, 4, dtype=torch.float64)
    for k in range(K):
        out[:, :, FS + k * G:FS + (k + 1) * G] = preds[k][:, :, N:N + G].double()
    for f in range(FS):
        out[:, :, FS + K * G + f] = sum(float(PLAN.alpha[k, f]) * preds[k][:, :, N + G + f - PLAN.starts[k]].double()
                                        for k in PLAN.covering(f))
    return out.float()


_oracle_cache = {}


def _oracle_loop(sd, scale, shift):
    """The windowed loop composed from the fp32 CPU oracle: per step and window one dit_forward (two with guidance), the float64
    blend, one UniPC step on the whole state.  Computed once per (scale, shift) and shared."""
    if (scale, shift) in _oracle_cache:
        return _oracle_cache[(scale, shift)]
    lat, ctx, neg = _inputs()
    state = _windowed(lat)
    sched = O.UniPCOracle()
    sched.set_timesteps(STEPS, shift)
    steps = []
    for t in sched.timesteps:
        preds = []
        for k in range(K):
            x = reference_window_gather(state, PLAN, N, G, k, k + 1)
            v = O.dit_forward(sd, CFG, x, t.expand(1), [ctx], SEQ, [N], [(N, N + G)])
            if scale > 1:
                vu = O.dit_forward(sd, CFG, x, t.expand(1), [neg], SEQ, [N], [(N, N + G)])
                v = vu + scale * (v - vu)
            preds.append(v)
        state = sched.step(_blend64(preds), state)
        steps.append(state)
    _oracle_cache[(scale, shift)] = steps
    return steps


def test_a_windowed_loop_against_the_oracle_composition(sd, model):
    """Bound: tests/test_gpu_dit.py::test_g8_cof_denoise_loop's -- rel-L2 < 2e-2 per step, cosine > 0.9998 at the end.
    Observed on an MI355X: see docs/TEST_BOUNDS.md."""
    want = _oracle_loop(sd, 1.0, SHIFT)
    seen = []
    out = _run(_pipe(model), steps_out=seen)
    assert len(seen) == STEPS and seen[0].shape == (1, 16, 2 * FS + K * G, 4, 4)       # the callback sees the windowed layout
    rels = [rel_l2(seen[i], want[i]) for i in range(STEPS)]
    cos = cosine(out, _unwindowed(want[-1]))
    print(f"windowed loop vs oracle: rel-L2 per step {['%.3e' % r for r in rels]}, final cosine {cos:.6f}")
    assert all(r < 2e-2 for r in rels) and cos > 0.9998
    assert out.shape == (1, 16, 2 * FS + G, 4, 4) and torch.equal(out, _unwindowed(seen[-1]))
    # source frames: the prediction there is 0, the sampler leaves them alone (to rounding, as test_g8_cof_denoise_loop)
    assert float((out[:, :, :FS].cpu() - _inputs()[0][:, :, :FS]).abs().max()) < 1e-5


def _model_loop(model):
    """The windowed loop composed from the model's own B = 1 forwards, torch slices for the gather, ops.window_blend and
    scheduler.step: what the pipeline must reproduce bit for bit with window_batch=1."""
    lat, ctx, _ = _inputs()
    state, ctx = _windowed(lat).to(DEV), ctx.to(DEV)
    sched = FlowUniPCMultistepScheduler(shift=1)
    sched.set_timesteps(STEPS, device=DEV, shift=SHIFT)
    alpha = torch.from_numpy(PLAN.alpha).to(DEV)
    keep = model.cache_context, model.skip_source_frames, model.mask_source_frames
    model.cache_context, model.skip_source_frames, model.mask_source_frames = True, N, N
    model.clear_context_cache()
    steps = []
    try:
        for t in sched.timesteps:
            preds = [model(reference_window_gather(state, PLAN, N, G, k, k + 1), t.expand(1), [ctx], SEQ, frame_split_indices=[N],
                           ground_frame_indices=[(N, N + G)]) for k in range(K)]
            pred = ops.window_blend(torch.cat(preds), alpha, PLAN.starts, FS, G)
            state = sched.step(pred, t, state, return_dict=False)[0]
            steps.append(state.clone())
    finally:
        model.cache_context, model.skip_source_frames, model.mask_source_frames = keep
        model.clear_context_cache()
    return steps


def test_b_c_window_batch(model):
    """(b) window_batch=1 is the composed loop, bit for bit: the pipeline's wiring adds nothing of its own.
    (c) all windows in one forward: the same kernels at another batch size -- rel-L2 within 1e-5 of (b)
    (tests/test_gpu_dit.py bounds the batch-size difference of rows at 1e-6; three steps and a sampler sit on top here).
    Observed on an MI355X: 0.0 at every step, i.e. bit-identical at this shape; the bound stays 1e-5 because the GEMM plan
    depends on the row count and promises no bit-identity across batch sizes (docs/TEST_BOUNDS.md)."""
    want = _model_loop(model)
    one, seen = [], []
    out1 = _run(_pipe(model), steps_out=one, window_batch=1)
    assert all(torch.equal(a, b) for a, b in zip(one, want)) and torch.equal(out1, _unwindowed(want[-1]))
    out = _run(_pipe(model), steps_out=seen)
    rels = [rel_l2(a, b) for a, b in zip(seen, one)]
    print(f"window_batch default vs 1: rel-L2 per step {['%.3e' % r for r in rels]}")
    assert max(rels) < WINDOW_BATCH_BOUND
    two = _run(_pipe(model), window_batch=2)               # forwards of 2 and 1 windows
    r2 = rel_l2(two, out1)
    print(f"window_batch 2 vs 1: rel-L2 {r2:.3e}")
    assert r2 < WINDOW_BATCH_BOUND
    assert torch.equal(_run(_pipe(model), window_batch=5), out)      # more than K: all windows


WINDOW_BATCH_BOUND = 1e-5


@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_d_a_clip_that_fits_one_window_takes_todays_path(model, kind, scale):
    plain = _run(_pipe(model, kind), scale=scale, source_frames=9, fs=3, windows=False)
    opted = _run(_pipe(model, kind), scale=scale, source_frames=9, fs=3)
    assert plain.shape == (1, 16, 7, 4, 4) and torch.equal(opted, plain)
    assert torch.equal(_run(_pipe(model, kind), scale=scale, source_frames=9, fs=3, temporal_window=None), plain)


def test_e_guidance_against_the_oracle_composition(sd, model):
    """Bound: test_g8b_cfg_loop's (guidance 5.0, shift 5.0, 3 steps) -- rel-L2 < 5e-2, cosine > 0.999."""
    want = _unwindowed(_oracle_loop(sd, 5.0, 5.0)[-1])
    out = _run(_pipe(model), scale=5.0, shift=5.0)
    r, c = rel_l2(out, want), cosine(out, want)
    print(f"windowed CFG loop vs oracle: rel-L2 {r:.3e} cosine {c:.6f}")
    assert r < 5e-2 and c > 0.999


def test_e_bf16_runs_and_is_close(sd, model):
    """Bound: test_pipeline_bf16_mode_runs_and_is_close's -- rel-L2 < 4e-2 against the fp32 oracle loop."""
    out = _run(_pipe(model), dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16
    r = rel_l2(out.float(), _unwindowed(_oracle_loop(sd, 1.0, SHIFT)[-1]))
    print(f"windowed bf16 loop vs oracle: rel-L2 {r:.3e}")
    assert r < 4e-2


@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_e_step_graph_is_bit_identical_to_eager(model, scale):
    eager, graphed = [], []
    a = _run(_pipe(model), scale=scale, steps_out=eager)
    pipe = _pipe(model)
    b = _run(pipe, scale=scale, steps_out=graphed, capture_graph="step")
    assert pipe._graphed.replays >= 1
    assert all(torch.equal(x, y) for x, y in zip(eager, graphed)) and torch.equal(a, b)


def test_e_cfg_skip_halves_the_windows_batch(model):
    """enable_cfg_skip: late steps run the conditional windows only -- the same latents as the reference's literal order (doubled
    batch through the model's rule, then guidance); and without guidance the model's rule (which halves ANY batch >= 2) stays off."""
    plain = _run(_pipe(model), scale=1.0)
    model.enable_cfg_skip(0.5, STEPS)
    short, literal = _pipe(model), _pipe(model)
    literal._cfg_skip_literal = True
    sizes, inner = [], model._forward

    def counted(x, *a, **kw):
        sizes.append(len(x))
        return inner(x, *a, **kw)
    model._forward = counted
    try:
        s = _run(short, scale=5.0)
    finally:
        del model._forward
    assert sizes == [2 * K, 2 * K, K]                         # ratio 0.5 of 3 steps: the rule holds from step 1.5 on
    assert torch.equal(s, _run(literal, scale=5.0))
    assert torch.equal(_run(_pipe(model), scale=1.0), plain)
    model.disable_cfg_skip()
    assert not torch.equal(_run(_pipe(model), scale=5.0), s)


def test_e_sde_sampler_draws_noise_of_the_states_shape(model):
    outs = []
    for seed in (3, 3, 4):
        gen = torch.Generator(device=DEV).manual_seed(seed)
        steps = []
        outs.append(_run(_pipe(model, "sde-dpmsolver++"), steps_out=steps, generator=gen))
        assert steps[0].shape == (1, 16, 2 * FS + K * G, 4, 4) and bool(torch.isfinite(outs[-1]).all())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    assert not torch.equal(steps[-1][:, :, FS], steps[-1][:, :, FS + 1])       # every window's grounding block goes its own way


def test_e_unsupported_combinations_raise(model):
    with pytest.raises(NotImplementedError, match="capture_graph='loop'"):
        _run(_pipe(model), capture_graph="loop")
    model.enable_teacache([1.0, 0.0], STEPS, 0.1, offload=False)
    with pytest.raises(NotImplementedError, match="TeaCache"):
        _run(_pipe(model))
    model.disable_teacache()
    with pytest.raises(ValueError, match="has none"):          # a T2V call has no source segment
        _pipe(model)(prompt_embeds=[_inputs()[1].to(DEV)], source_frames=25, num_inference_steps=STEPS, guidance_scale=1.0, cot=True,
                     output_type="latent", temporal_window=13, temporal_overlap=8)
    with pytest.raises(ValueError, match="temporal_window=14"):
        _run(_pipe(model), windows=False, temporal_window=14)


def test_e_decoded_clip_covers_every_target_frame():
    """With the VAE: edit_videos has all 1 + 4 * (Fs - 1) = 25 frames, window 0's grounding is ground_videos, and
    output_type='uint8' returns the same frames as the writer's bytes."""
    from videocof_amd import AutoencoderKLWan
    from videocof_amd.weights import deterministic_vae_state_dict
    vae = AutoencoderKLWan()
    vae.load_state_dict(deterministic_vae_state_dict(), device=DEV)
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    m.load_state_dict(deterministic_dit_state_dict(**TINY), device=DEV)
    lat, ctx, _ = _inputs()
    pipe = WanPipeline(vae=vae, transformer=m, scheduler=FlowUniPCMultistepScheduler(shift=1))
    kw = dict(latents=lat.to(DEV), prompt_embeds=[ctx.to(DEV)], height=32, width=32, source_frames=25, reasoning_frames=4,
              num_inference_steps=2, guidance_scale=1.0, shift=SHIFT, cot=True, weight_dtype=torch.float32, return_dict=True,
              temporal_window=13, temporal_overlap=8)
    f = pipe(output_type="numpy", **kw)
    assert f.edit_videos.shape == (1, 3, 25, 32, 32) and f.ground_videos.shape == (1, 3, 1, 32, 32)
    assert f.videos.shape == (1, 3, 26, 32, 32) and f.latents.shape == (1, 16, 2 * FS + G, 4, 4)
    u = pipe(output_type="uint8", **kw)
    assert u.edit_videos.shape == (1, 25, 32, 32, 3) and u.edit_videos.dtype == np.uint8
    assert torch.equal(u.latents, f.latents)
    want = (np.transpose(f.videos, (0, 2, 3, 4, 1)) * 255).astype(np.uint8)             # the writer's conversion
    assert np.array_equal(u.videos, want)
