"""-m gpu: spatial context windows -- wan_tile_gather / wan_tile_blend against their torch float32 definitions (bit for bit, with
guard bands) and, where every frame is one tile, against the temporal pair and the temporal definition, and the tiled denoise
loop of WanPipeline against a loop composed from the CPU oracle, against a loop composed from the model's own single-tile forwards,
and against today's paths where the frame fits one tile.  Bounds and observed values: docs/TEST_BOUNDS.md, "Spatial context windows"."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import wan_oracle as O
from videocof_amd import (FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, TilePlan, WanPipeline, WanTransformer3DModel, _lib,
                          ops, reference_tile_blend, reference_tile_gather, reference_window_blend, reference_window_gather, window_plan)
from videocof_amd.weights import deterministic_dit_state_dict, det_uniform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(dim=256, ffn_dim=512, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)
CFG = O.DiTConfig(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
POISON = 7.0
T_PLAN = window_plan(7, 4, 2)          # starts (0, 2, 3): frame 3 is covered by all three windows


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


# (H, W, th, tw, oy, ox, guard elements)
SHAPES = [(5, 7, 4, 4, 2, 2, 64),        # odd pitch: element form
          (6, 8, 4, 4, 2, 2, 64),        # x starts (0, 2, 4): 8-byte form in fp32, 4-byte in bf16
          (8, 16, 4, 8, 2, 4, 64),       # 16-byte form in fp32, 8-byte in bf16
          (8, 32, 4, 16, 2, 8, 64),      # 16-byte form in both dtypes
          (8, 32, 4, 16, 2, 8, 3),       # the same behind a 3-element guard band: misaligned base, the form falls back
          (24, 88, 16, 48, 4, 8, 64),    # several workgroups per row
          # an axis with ONE window (weight 1.0f everywhere) beside a tiled one
          (6, 8, 4, 8, 2, 0, 64),        # y tiled, x whole: the rows of a tile are contiguous in the state
          (6, 7, 4, 7, 2, 0, 64),        # the same at an odd pitch
          (4, 8, 4, 4, 0, 2, 64),        # x tiled, y whole
          (24, 88, 16, 88, 4, 0, 3)]     # y tiled, x whole, behind a misaligned base, several row passes
B, C = 2, 3


def _tile_plan(H, W, th, tw, oy, ox):
    return TilePlan(T_PLAN, window_plan(H, th, oy), window_plan(W, tw, ox))


def _starts(p):
    return p.t.starts, p.y.starts, p.x.starts


def _tables(p):
    return tuple(torch.from_numpy(a.alpha).to(DEV) for a in (p.t, p.y, p.x))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W,th,tw,oy,ox,pad", SHAPES)
def test_a_tile_gather_equals_the_torch_definition(H, W, th, tw, oy, ox, pad, dtype):
    p = _tile_plan(H, W, th, tw, oy, ox)
    if (H, W, tw) == (6, 8, 4):
        assert p.x.starts == (0, 2, 4)
    if ox == 0:
        assert (p.Ky, p.Kx) == (2, 1) and bool((p.x.alpha == 1).all())         # y tiled, x whole
    if oy == 0:
        assert (p.Ky, p.Kx) == (1, 3) and bool((p.y.alpha == 1).all())         # x tiled, y whole
    K, (n, _, _), Fs = p.K, p.shape, p.extent[0]
    for G in (0, 1):
        shape = (B, C, 2 * Fs + p.Kt * G, H, W)
        state = Guarded(shape, dtype, pad, _values(f"tile.state{G}", shape, dtype))
        for k0, k1 in ((0, K), (1, K), (K // 2, K // 2 + 2)):
            for rep in (1, 2):
                want = reference_tile_gather(state.view, p, G, k0, k1, rep)
                out = Guarded(want.shape, dtype, pad)
                got = ops.tile_gather(state.view, _starts(p), p.shape, G, k0, k1, rep, out=out.view)
                assert got.data_ptr() == out.view.data_ptr()
                assert torch.equal(out.view, want), (G, k0, k1, rep)
                assert out.intact() and state.intact()
        # the default arguments: every tile, once, into a fresh tensor
        assert torch.equal(ops.tile_gather(state.view, _starts(p), p.shape, G), reference_tile_gather(state.view, p, G))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W,th,tw,oy,ox,pad", SHAPES)
def test_a_tile_blend_equals_the_torch_definition(H, W, th, tw, oy, ox, pad, dtype):
    p = _tile_plan(H, W, th, tw, oy, ox)
    K, (n, _, _), Fs, Kt = p.K, p.shape, p.extent[0], p.Kt
    tables = _tables(p)
    for G in (0, 1):
        shape = (K * B, C, 2 * n + G, th, tw)
        pred = Guarded(shape, dtype, pad, _values(f"tile.pred{G}", shape, dtype))
        want = reference_tile_blend(pred.view, p, G)
        out = Guarded(want.shape, dtype, pad)
        got = ops.tile_blend(pred.view, tables, _starts(p), p.extent, G, out=out.view)
        assert got.data_ptr() == out.view.data_ptr()
        assert torch.equal(out.view, want), G
        assert out.intact() and pred.intact()
        assert not bool(out.view[:, :, :Fs].any())                                         # source frames: the CoF mask
        # one tile covers the corner (0, 0, 0): its prediction unchanged, and its grounding block's corner too
        q = pred.view.view(K, B, C, 2 * n + G, th, tw)
        assert torch.equal(out.view[:, :, Fs + Kt * G, 0, 0], q[0][:, :, n + G, 0, 0])
        if G:
            assert torch.equal(out.view[:, :, Fs, 0, 0], q[0][:, :, n, 0, 0])
        assert torch.equal(ops.tile_blend(pred.view, tables, _starts(p), p.extent, G), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(3, 5), (4, 8)])
def test_b_one_tile_per_spatial_axis_equals_the_window_kernels(H, W, dtype):
    p = TilePlan(T_PLAN, window_plan(H, H + 1, 1), window_plan(W, W, 2))
    assert (p.Ky, p.Kx) == (1, 1) and p.shape == (4, H, W)
    K, n, Fs = p.K, 4, 7
    alpha = torch.from_numpy(T_PLAN.alpha).to(DEV)
    bits = lambda t: t.view(torch.int32 if dtype == torch.float32 else torch.int16)        # signed zeros included
    for G in (0, 1):
        state = _values(f"tile.one.state{G}", (B, C, 2 * Fs + K * G, H, W), dtype).to(DEV)
        for k0, k1, rep in ((0, K, 1), (1, K, 2), (1, 2, 2)):
            got = ops.tile_gather(state, _starts(p), p.shape, G, k0, k1, rep)
            assert torch.equal(got, ops.window_gather(state, T_PLAN.starts, n, G, k0, k1, rep))
            assert torch.equal(bits(got), bits(reference_window_gather(state, T_PLAN, n, G, k0, k1, rep)))      # the temporal definition
        pred = _values(f"tile.one.pred{G}", (K * B, C, 2 * n + G, H, W), dtype).to(DEV)
        got, want = ops.tile_blend(pred, _tables(p), _starts(p), p.extent, G), ops.window_blend(pred, alpha, T_PLAN.starts, Fs, G)
        assert torch.equal(bits(got), bits(want))
        assert torch.equal(bits(got), bits(reference_window_blend(pred, T_PLAN, G)))                             # the temporal definition


def test_c_invalid_arguments_return_wan_err_invalid():
    lib = _lib.load()
    buf = torch.zeros(8192, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    ok = dict(out=p, src=p, dtype=0, at=p, ay=p, ax=p, ts=ints(0, 2, 3), ys=ints(0, 2), xs=ints(0, 2, 4), Kt=3, Ky=2, Kx=3, k0=0, k1=18,
              B=1, C=1, Fs=7, H=6, W=8, n=4, th=4, tw=4, G=0, rep=1, rep_stride=0)

    def gather(**kw):
        a = {**ok, **kw}
        return lib.wan_tile_gather(a["out"], a["src"], a["dtype"], a["ts"], a["ys"], a["xs"], a["Kt"], a["Ky"], a["Kx"], a["k0"], a["k1"],
                                   a["B"], a["C"], a["Fs"], a["H"], a["W"], a["n"], a["th"], a["tw"], a["G"], a["rep"], a["rep_stride"],
                                   None)

    def blend(**kw):
        a = {**ok, **kw}
        return lib.wan_tile_blend(a["out"], a["src"], a["dtype"], a["at"], a["ay"], a["ax"], a["ts"], a["ys"], a["xs"], a["Kt"], a["Ky"],
                                  a["Kx"], a["B"], a["C"], a["Fs"], a["H"], a["W"], a["n"], a["th"], a["tw"], a["G"], None)

    both = [dict(out=None), dict(src=None), dict(dtype=2), dict(B=0), dict(C=0), dict(G=-1),
            dict(ts=ints(0, 5), Kt=2, Fs=9),                    # two windows of 4 frames at 0 and 5 leave frame 4 of 9 uncovered
            dict(ts=ints(0, 3, 2)), dict(ts=ints(1, 2, 3)), dict(ts=None), dict(Kt=0), dict(Kt=65),
            dict(ys=ints(0, 5), H=9),                           # a gap in y
            dict(ys=ints(0, 3)),                                # the last tile does not end at H
            dict(ys=ints(0,), Ky=1, th=7),                      # th > H
            dict(th=0), dict(ys=None),
            dict(xs=ints(0, 5), Kx=2, W=9),                     # a gap in x
            dict(xs=ints(0, 2, 5)), dict(xs=ints(0,), Kx=1, tw=9), dict(tw=0), dict(xs=None),
            dict(ys=ints(0,), Ky=1, H=1 << 30, th=1 << 30)]     # 2^30 rows per frame: more than 2^31 rows in all
    for kw in both:
        assert gather(**kw) == _lib.WAN_ERR_INVALID, kw
        assert blend(**kw) == _lib.WAN_ERR_INVALID, kw
    for kw in (dict(k0=2, k1=2), dict(k0=-1), dict(k1=19), dict(rep=0), dict(rep=3), dict(rep=2, rep_stride=18 * 8 * 16 - 1)):
        assert gather(**kw) == _lib.WAN_ERR_INVALID, kw
    for kw in (dict(at=None), dict(ay=None), dict(ax=None)):
        assert blend(**kw) == _lib.WAN_ERR_INVALID, kw
    assert bool((buf == 0).all())                               # nothing was launched
    plan = _tile_plan(6, 8, 4, 4, 2, 2)
    state, pred = torch.zeros(1, 1, 14, 6, 8, device=DEV), torch.zeros(18, 1, 8, 4, 4, device=DEV)
    with pytest.raises(ValueError, match="leave no gap"):
        ops.tile_gather(state, ((0, 2, 3), (0, 2), (0, 2, 5)), (4, 4, 4), 0)
    with pytest.raises(ValueError, match="tile range"):
        ops.tile_gather(state, _starts(plan), plan.shape, 0, 3, 19)
    with pytest.raises(ValueError, match="leave no gap"):
        ops.tile_blend(pred, _tables(plan), ((0, 2, 3), (0, 1), (0, 2, 4)), (7, 6, 8), 0)
    with pytest.raises(ValueError, match="tile_blend.ay"):
        ops.tile_blend(pred, (_tables(plan)[0], _tables(plan)[2], _tables(plan)[2]), _starts(plan), (7, 6, 8), 0)
    with pytest.raises(ValueError, match="samples for"):
        ops.tile_blend(pred[:17], _tables(plan), _starts(plan), (7, 6, 8), 0)
    with pytest.raises(ValueError, match="not supported"):
        ops.tile_gather(state.half(), _starts(plan), plan.shape, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tile_gather(state.cpu(), _starts(plan), plan.shape, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tile_blend(pred.cpu(), _tables(plan), _starts(plan), (7, 6, 8), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tile_blend(pred, tuple(t.cpu() for t in _tables(plan)), _starts(plan), (7, 6, 8), 0)


# ------------------------------------------------------------------------------------------------ loop
STEPS, SHIFT = 3, 3.0
G, FS, H, W = 1, 7, 6, 8
SPACE = dict(spatial_window=(32, 32), spatial_overlap=(16, 16))                    # tiles of 4 x 4 cells, overlap 2
TIME = dict(temporal_window=13, temporal_overlap=8)                                # windows of 4 latent frames, overlap 2
PLAN_TS = TilePlan(T_PLAN, window_plan(H, 4, 2), window_plan(W, 4, 2))             # K = 3 * 2 * 3 = 18 tiles of [16, 9, 4, 4]
PLAN_S = TilePlan(window_plan(FS, FS, 0), window_plan(H, 4, 2), window_plan(W, 4, 2))      # space alone: 6 tiles of [16, 15, 4, 4]


def _seq(plan):
    n, th, tw = plan.shape
    return math.ceil(th * tw / 4 * (2 * n + G))


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


def _inputs(fs=FS, h=H, w=W):
    lat = torch.cat([det_uniform("tile.src", (1, 16, 7, H, W), 1.0)[:, :, :fs, :h, :w],
                     det_uniform("tile.noise", (1, 16, 8, H, W), 1.0)[:, :, :fs + G, :h, :w]], dim=2).contiguous()
    return lat, det_uniform("tile.ctx", (37, 64), 1.0), det_uniform("tile.neg", (9, 64), 1.0)


def _pipe(model, kind="unipc"):
    if kind == "unipc":
        return WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))
    return WanPipeline(transformer=model, scheduler=FlowDPMSolverMultistepScheduler(shift=1.0, solver_order=2, algorithm_type=kind))


def _run(pipe, scale=1.0, steps_out=None, source_frames=25, shift=SHIFT, dtype=torch.float32, fs=FS, h=H, w=W, **kw):
    lat, ctx, neg = _inputs(fs, h, w)
    cb = None
    if steps_out is not None:
        cb = lambda p, i, t, d: steps_out.append(d["latents"].clone()) or {}
    return pipe(latents=lat.to(DEV), prompt_embeds=[ctx.to(DEV)], negative_prompt_embeds=[neg.to(DEV)] if scale > 1 else None,
                source_frames=source_frames, reasoning_frames=4, num_inference_steps=STEPS, guidance_scale=scale, shift=shift,
                repeat_rope=True, cot=True, output_type="latent", weight_dtype=dtype, callback_on_step_end=cb, **kw).latents


def _windowed(lat, plan):
    return torch.cat([lat[:, :, :FS]] + [lat[:, :, FS:FS + G]] * plan.Kt + [lat[:, :, FS + G:]], dim=2)


def _unwindowed(state, plan):
    return torch.cat([state[:, :, :FS + G], state[:, :, FS + plan.Kt * G:]], dim=2)


def _blend64(preds, plan):
    """The K tile predictions [1, 16, 2n + G, th, tw] (float32, CPU) as the state's prediction, every product and sum in float64."""
    (n, th, tw), Kt = plan.shape, plan.Kt
    out = torch.zeros(1, 16, 2 * FS + Kt * G, H, W, dtype=torch.float64)
    for k, v in enumerate(preds):
        kt = plan.split(k)[0]
        a, y0, x0 = plan.origin(k)
        ys, xs = slice(y0, y0 + th), slice(x0, x0 + tw)
        wg = torch.from_numpy(plan.weights(k, ground=True)[ys, xs]).double()
        w = torch.from_numpy(plan.weights(k)[a:a + n, ys, xs]).double()
        out[:, :, FS + kt * G:FS + (kt + 1) * G, ys, xs] += wg * v[:, :, n:n + G].double()
        out[:, :, FS + Kt * G + a:FS + Kt * G + a + n, ys, xs] += w * v[:, :, n + G:].double()
    return out.float()


_oracle_cache = {}


def _oracle_loop(sd, plan, scale, shift):
    """The tiled loop composed from the fp32 CPU oracle: per step and tile one dit_forward (two with guidance), the float64 blend,
    one UniPC step on the whole state.  Computed once per (plan, scale, shift) and shared."""
    key = (plan.K, scale, shift)
    if key in _oracle_cache:
        return _oracle_cache[key]
    lat, ctx, neg = _inputs()
    state = _windowed(lat, plan)
    n, seq = plan.shape[0], _seq(plan)
    sched = O.UniPCOracle()
    sched.set_timesteps(STEPS, shift)
    steps = []
    for t in sched.timesteps:
        preds = []
        for k in range(plan.K):
            x = reference_tile_gather(state, plan, G, k, k + 1)
            v = O.dit_forward(sd, CFG, x, t.expand(1), [ctx], seq, [n], [(n, n + G)])
            if scale > 1:
                vu = O.dit_forward(sd, CFG, x, t.expand(1), [neg], seq, [n], [(n, n + G)])
                v = vu + scale * (v - vu)
            preds.append(v)
        state = sched.step(_blend64(preds, plan), state)
        steps.append(state)
    _oracle_cache[key] = steps
    return steps


PLANS = {"time+space": (PLAN_TS, {**TIME, **SPACE}), "space": (PLAN_S, SPACE)}


@pytest.mark.parametrize("which", list(PLANS))
def test_d_tiled_loop_against_the_oracle_composition(sd, model, which):
    """Bound: tests/test_gpu_dit.py::test_g8_cof_denoise_loop's -- rel-L2 < 2e-2 per step, cosine > 0.9998 at the end.
    Observed on an MI355X: see docs/TEST_BOUNDS.md."""
    plan, opts = PLANS[which]
    assert plan.K == (18 if which == "time+space" else 6)
    want = _oracle_loop(sd, plan, 1.0, SHIFT)
    seen = []
    out = _run(_pipe(model), steps_out=seen, **opts)
    assert len(seen) == STEPS and seen[0].shape == (1, 16, 2 * FS + plan.Kt * G, H, W)        # the callback sees the windowed layout
    rels = [rel_l2(seen[i], want[i]) for i in range(STEPS)]
    cos = cosine(out, _unwindowed(want[-1], plan))
    print(f"tiled loop ({which}) vs oracle: rel-L2 per step {['%.3e' % r for r in rels]}, final cosine {cos:.6f}")
    assert all(r < 2e-2 for r in rels) and cos > 0.9998
    assert out.shape == (1, 16, 2 * FS + G, H, W) and torch.equal(out, _unwindowed(seen[-1], plan))
    assert float((out[:, :, :FS].cpu() - _inputs()[0][:, :, :FS]).abs().max()) < 1e-5        # source frames stay


@pytest.mark.parametrize("which", list(PLANS))
def test_d_guidance_against_the_oracle_composition(sd, model, which):
    """Bound: test_g8b_cfg_loop's (guidance 5.0, shift 5.0, 3 steps) -- rel-L2 < 5e-2, cosine > 0.999."""
    plan, opts = PLANS[which]
    want = _unwindowed(_oracle_loop(sd, plan, 5.0, 5.0)[-1], plan)
    out = _run(_pipe(model), scale=5.0, shift=5.0, **opts)
    r, c = rel_l2(out, want), cosine(out, want)
    print(f"tiled CFG loop ({which}) vs oracle: rel-L2 {r:.3e} cosine {c:.6f}")
    assert r < 5e-2 and c > 0.999


@pytest.mark.parametrize("which", list(PLANS))
def test_d_bf16_runs_and_is_close(sd, model, which):
    """Bound: test_pipeline_bf16_mode_runs_and_is_close's -- rel-L2 < 4e-2 against the fp32 oracle loop."""
    plan, opts = PLANS[which]
    out = _run(_pipe(model), dtype=torch.bfloat16, **opts)
    assert out.dtype == torch.bfloat16
    r = rel_l2(out.float(), _unwindowed(_oracle_loop(sd, plan, 1.0, SHIFT)[-1], plan))
    print(f"tiled bf16 loop ({which}) vs oracle: rel-L2 {r:.3e}")
    assert r < 4e-2


WINDOW_BATCH_BOUND = 1e-5


def _model_loop(model, plan):
    """The tiled loop composed from the model's own B = 1 forwards, torch slices for the gather, ops.tile_blend and
    scheduler.step: what the pipeline must reproduce bit for bit with window_batch=1."""
    lat, ctx, _ = _inputs()
    state, ctx = _windowed(lat, plan).to(DEV), ctx.to(DEV)
    n, seq = plan.shape[0], _seq(plan)
    sched = FlowUniPCMultistepScheduler(shift=1)
    sched.set_timesteps(STEPS, device=DEV, shift=SHIFT)
    keep = model.cache_context, model.skip_source_frames, model.mask_source_frames
    model.cache_context, model.skip_source_frames, model.mask_source_frames = True, n, n
    model.clear_context_cache()
    steps = []
    try:
        for t in sched.timesteps:
            preds = [model(reference_tile_gather(state, plan, G, k, k + 1).contiguous(), t.expand(1), [ctx], seq, frame_split_indices=[n],
                           ground_frame_indices=[(n, n + G)]) for k in range(plan.K)]
            pred = ops.tile_blend(torch.cat(preds), _tables(plan), _starts(plan), plan.extent, G)
            state = sched.step(pred, t, state, return_dict=False)[0]
            steps.append(state.clone())
    finally:
        model.cache_context, model.skip_source_frames, model.mask_source_frames = keep
        model.clear_context_cache()
    return steps


def test_e_window_batch(model):
    """window_batch=1 is the composed loop, bit for bit: the pipeline's wiring adds nothing of its own.  All tiles in one forward,
    or four per forward: the same kernels at another batch size -- rel-L2 within 1e-5, for the reason given in
    tests/test_gpu_windows.py::test_b_c_window_batch (the GEMM plan depends on the row count and promises no bit-identity across
    batch sizes).
    Observed on an MI355X: 0.0 at every step, for all 18 tiles in one forward and for four per forward.  Before the model's time
    embedding went through torch.addmm in groups of at most 16 rows it was 2.4e-4, 9.3e-4, 1.5e-3: one addmm over 17 or more rows
    gives a row other last fp32 bits than over 1 .. 16 (docs/TEST_BOUNDS.md, "Spatial context windows")."""
    plan, opts = PLANS["time+space"]
    want = _model_loop(model, plan)
    one, seen = [], []
    out1 = _run(_pipe(model), steps_out=one, window_batch=1, **opts)
    assert all(torch.equal(a, b) for a, b in zip(one, want)) and torch.equal(out1, _unwindowed(want[-1], plan))
    out = _run(_pipe(model), steps_out=seen, **opts)
    rels = [rel_l2(a, b) for a, b in zip(seen, one)]
    print(f"tiles: window_batch default vs 1: rel-L2 per step {['%.3e' % r for r in rels]}")
    assert max(rels) < WINDOW_BATCH_BOUND
    four = _run(_pipe(model), window_batch=4, **opts)              # forwards of 4, 4, 4, 4 and 2 tiles
    r4 = rel_l2(four, out1)
    print(f"tiles: window_batch 4 vs 1: rel-L2 {r4:.3e}")
    assert r4 < WINDOW_BATCH_BOUND
    assert torch.equal(_run(_pipe(model), window_batch=40, **opts), out)       # more than K: all tiles


@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_f_a_clip_and_frame_that_fit_one_tile_take_todays_path(model, kind, scale):
    small = dict(source_frames=9, fs=3, h=4, w=4)
    plain = _run(_pipe(model, kind), scale=scale, **small)
    assert plain.shape == (1, 16, 7, 4, 4)
    assert torch.equal(_run(_pipe(model, kind), scale=scale, **small, **SPACE), plain)
    assert torch.equal(_run(_pipe(model, kind), scale=scale, **small, **SPACE, **TIME), plain)
    assert torch.equal(_run(_pipe(model, kind), scale=scale, **small, spatial_window=None), plain)


def test_f_a_frame_that_fits_one_tile_takes_the_temporal_path(model):
    a, b = [], []
    temporal = _run(_pipe(model), steps_out=a, h=4, w=4, **TIME)
    both = _run(_pipe(model), steps_out=b, h=4, w=4, **TIME, **SPACE)
    assert a[0].shape == (1, 16, 2 * FS + 3 * G, 4, 4)
    assert torch.equal(both, temporal) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_g_step_graph_is_bit_identical_to_eager(model, scale):
    opts = PLANS["time+space"][1]
    eager, graphed = [], []
    a = _run(_pipe(model), scale=scale, steps_out=eager, **opts)
    pipe = _pipe(model)
    b = _run(pipe, scale=scale, steps_out=graphed, capture_graph="step", **opts)
    assert pipe._graphed.replays >= 1
    assert all(torch.equal(x, y) for x, y in zip(eager, graphed)) and torch.equal(a, b)


def test_g_unsupported_combinations_raise(model):
    for opts in (SPACE, {**SPACE, **TIME}):
        with pytest.raises(NotImplementedError, match="capture_graph='loop'"):
            _run(_pipe(model), capture_graph="loop", **opts)
    model.enable_teacache([1.0, 0.0], STEPS, 0.1, offload=False)
    with pytest.raises(NotImplementedError, match="TeaCache"):
        _run(_pipe(model), **SPACE)
    model.disable_teacache()
    with pytest.raises(ValueError, match="has none"):          # a T2V call has no source segment
        _pipe(model)(prompt_embeds=[_inputs()[1].to(DEV)], source_frames=25, num_inference_steps=STEPS, guidance_scale=1.0, cot=True,
                     output_type="latent", **SPACE)
    with pytest.raises(ValueError, match="spatial_window="):
        _run(_pipe(model), spatial_window=(32, 40))
    with pytest.raises(ValueError, match="spatial_overlap="):
        _run(_pipe(model), spatial_window=(32, 32), spatial_overlap=(32, 16))
    with pytest.raises(ValueError, match="window_batch"):
        _run(_pipe(model), window_batch=0, **SPACE)
    seen = []
    _run(_pipe(model), steps_out=seen, **SPACE)
    assert seen[0].shape == (1, 16, 2 * FS + 1 * G, H, W)       # space alone: one temporal window, one grounding block
