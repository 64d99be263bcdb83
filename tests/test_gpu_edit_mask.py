"""-m gpu: edit inside a mask -- wan_latent_mask_u8 / wan_masked_prediction against their host definitions (bit for bit, with guard
bands), fit_mask against its definition, and WanPipeline(edit_mask=...) against the call without a mask, against a loop composed from
the model's own forwards, and against the zero-mask bound of tests/edit_mask_bounds.py.  docs/TEST_BOUNDS.md, "Edit inside a mask"."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from videocof_amd import (FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel, _lib, fit_mask,
                          latent_edit_mask, ops, reference_fit_mask, reference_latent_edit_mask, reference_masked_prediction)
from videocof_amd.video_io import fit_plan
from videocof_amd.weights import deterministic_dit_state_dict, det_uniform

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_mask_bounds as EB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(dim=256, ffn_dim=512, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)
POISON = 7


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


def bits(t):
    return t.view({torch.float32: torch.int32, torch.bfloat16: torch.int16}[t.dtype])


MASK_SHAPES = [(1, 16, 16), (5, 24, 40), (6, 16, 24), (9, 32, 72), (13, 64, 136)]      # T = 6: a short last group; 136 = 17 cells
EVERY = [(g, gt, f) for g in range(5) for gt in range(3) for f in range(g + 1)]


def _masks(B, T, H, W):
    """Random sparse masks with grey values, and single pixels at the corners of the clip (first and last frame, sample, row, column)."""
    rng = np.random.default_rng(B * 1000 + T * H + W)
    sparse = (rng.integers(1, 256, (B, T, H, W)) * (rng.random((B, T, H, W)) < 0.003)).astype(np.uint8)
    sparse[rng.random((B, T, H, W)) < 0.0005] = 255
    corners = np.zeros((B, T, H, W), np.uint8)
    corners[0, 0, 0, 0], corners[-1, -1, -1, -1], corners[0, -1, 0, -1], corners[-1, 0, -1, 0] = 255, 255, 200, 1
    return {"sparse": sparse, "corners": corners}


@pytest.mark.parametrize("T,H,W", MASK_SHAPES)
def test_latent_mask_equals_the_numpy_definition(T, H, W):
    small = (T, H, W) == MASK_SHAPES[0]
    for B in (1, 2):
        for name, a in _masks(B, T, H, W).items():
            for pad in ((64, 3) if name == "sparse" else (64,)):            # 3: a base that is not 8-byte aligned (byte loads)
                alpha = Guarded(a.shape, torch.uint8, pad, torch.from_numpy(a))
                for g, gt, f in (EVERY if small else ((1, 0, 1), (4, 2, 4))):
                    want = reference_latent_edit_mask(a, grow=g, grow_t=gt, feather=f)
                    out = Guarded(want.shape, torch.uint8, pad)
                    got = ops.latent_mask(alpha.view, g, gt, f, out=out.view)
                    assert got.data_ptr() == out.view.data_ptr()
                    assert torch.equal(out.view.cpu(), want), (B, name, pad, g, gt, f)
                    assert out.intact() and alpha.intact()
                    assert torch.equal(alpha.view.cpu(), torch.from_numpy(a))
    # the front end: host or device input, with or without the batch axis, the defaults
    a = _masks(1, T, H, W)["sparse"][0]
    want = reference_latent_edit_mask(a)
    assert torch.equal(latent_edit_mask(a).cpu(), want) and torch.equal(latent_edit_mask(torch.from_numpy(a).to(DEV)[None]).cpu(), want[None])
    assert torch.equal(want, reference_latent_edit_mask(a, grow=1, grow_t=0, feather=1))


# (h, w, guard elements).  The issue's four: 15-element frames are never 16-byte aligned; (4, 8) is; (4, 8) behind a 3-element band is not
# (element-wise form, and a mask base that is no multiple of the unit); 24 x 44 needs several workgroups per row.  (2, 3) and (3, 4) with
# Fs = 1 are the 8-byte (fp32) and 4- / 8-byte (bf16) units, which none of the four reaches.
PRED_SHAPES = [(3, 5, 64), (4, 8, 64), (4, 8, 3), (24, 44, 64), (2, 3, 64), (3, 4, 64)]
LEVELS = torch.tensor([0, 1, 127, 254, 255], dtype=torch.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("h,w,pad", PRED_SHAPES)
def test_masked_prediction_equals_the_torch_definition(h, w, pad, dtype):
    C, big = 5, h * w > 64
    gen = torch.Generator().manual_seed(h * 100 + w)
    for Fs in (1, 7):
        for G in ((1,) if big else (0, 1, 3)):
            for B in ((2,) if big else (1, 2)):
                for Bm in sorted({1, B}):
                    shape, sigma = (B, C, 2 * Fs + G, h, w), (0.9375, 0.31, 1.0)[G % 3]
                    tag = f"em.{h}.{Fs}.{G}.{B}"
                    p0 = det_uniform(tag + ".pred", shape, 2.0).to(dtype)
                    p0[0, 0, Fs + G, 0, 0] = -0.0
                    x0 = det_uniform(tag + ".sample", shape, 2.0).to(dtype)
                    for kind in ("levels", "random"):
                        if kind == "levels":
                            a = LEVELS[torch.randint(0, 5, (Bm, Fs, h, w), generator=gen)]
                            a[0, 0, 0, :2] = 255                                         # (a pair of 255s, and the -0.0 under one)
                        else:
                            a = torch.randint(0, 256, (Bm, Fs, h, w), generator=gen, dtype=torch.uint8)
                        want = reference_masked_prediction(p0, x0, a, Fs, Fs + G, sigma)
                        pred, sample = Guarded(shape, dtype, pad, p0), Guarded(shape, dtype, pad, x0)
                        wts = Guarded(a.shape, torch.uint8, pad, a)
                        got = ops.masked_prediction_(pred.view, sample.view, wts.view, Fs, Fs + G, sigma)
                        assert got.data_ptr() == pred.view.data_ptr()
                        res = pred.view.cpu()
                        assert torch.equal(bits(res), bits(want)), (Fs, G, B, Bm, kind)
                        assert pred.intact() and sample.intact() and wts.intact()
                        assert torch.equal(bits(sample.view.cpu()), bits(x0)) and torch.equal(wts.view.cpu(), a)
                        assert torch.equal(bits(res[:, :, :Fs + G]), bits(p0[:, :, :Fs + G]))       # source and grounding: their bits
                        keep = (a == 255)[:, None].expand(B, C, Fs, h, w)
                        assert torch.equal(bits(res[:, :, Fs + G:])[keep], bits(p0[:, :, Fs + G:])[keep])
                        zero = (a == 0)[:, None].expand(B, C, Fs, h, w)
                        r = ((x0[:, :, Fs + G:].float() - x0[:, :, :Fs].float()) / torch.tensor(sigma)).to(dtype)
                        assert torch.equal(res[:, :, Fs + G:][zero], r[zero])


def test_invalid_arguments_raise_and_launch_nothing():
    p = torch.zeros(2, 3, 5, 3, 5, device=DEV)
    w = torch.zeros(1, 2, 3, 5, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="sigma"):
        ops.masked_prediction_(p, p.clone(), w, 2, 3, 0.0)
    with pytest.raises(ValueError, match="do not fit"):
        ops.masked_prediction_(p, p.clone(), w, 2, 4, 0.5)
    with pytest.raises(ValueError, match="weights"):
        ops.masked_prediction_(p, p.clone(), w[:, :1], 2, 3, 0.5)
    with pytest.raises(ValueError, match="weights"):
        ops.masked_prediction_(p, p.clone(), w.expand(3, 2, 3, 5), 2, 3, 0.5)
    with pytest.raises(ValueError, match="expected"):
        ops.masked_prediction_(p, p.clone().bfloat16(), w, 2, 3, 0.5)
    with pytest.raises(ValueError, match="in place"):
        ops.masked_prediction_(p.transpose(0, 1), p.clone().transpose(0, 1), w, 2, 3, 0.5)
    with pytest.raises(ValueError, match="feather=2"):
        ops.latent_mask(torch.zeros(1, 5, 16, 16, device=DEV, dtype=torch.uint8), 1, 0, 2)
    with pytest.raises(ValueError, match="latent cells"):
        ops.latent_mask(torch.zeros(1, 5, 16, 20, device=DEV, dtype=torch.uint8), 1, 0, 1)
    assert not bool(p.any())


@pytest.mark.parametrize("orig,fit", [((54, 100), (32, 48)), ((37, 29), (48, 32))])
def test_fit_mask_equals_its_definition(orig, fit):
    a = np.random.default_rng(orig[1]).integers(0, 256, (2, 3) + orig).astype(np.uint8)
    plan = fit_plan(*orig, *fit)
    assert torch.equal(fit_mask(a, plan).cpu(), reference_fit_mask(a, plan))
    assert torch.equal(fit_mask(torch.from_numpy(a[0]).to(DEV), plan).cpu(), reference_fit_mask(a[0], plan))
    same = fit_plan(*fit, *fit)
    m = torch.zeros((3,) + fit, dtype=torch.uint8, device=DEV)
    assert fit_mask(m, same).data_ptr() == m.data_ptr()                     # already at the target: nothing is launched


# ------------------------------------------------------------------------------------------------ pipeline
STEPS, SHIFT = 3, 3.0
G, FS, K = 1, 7, 3                     # source_frames=25 -> 7 latent frames; temporal_window=13, temporal_overlap=8 -> 3 windows
SEQ = math.ceil(4 * 4 / 4 * (2 * FS + G))
SIZE = dict(source_frames=25, height=32, width=32)
FULL = np.full((25, 32, 32), 255, np.uint8)
NONE = np.zeros((25, 32, 32), np.uint8)
HALF = FULL.copy()
HALF[:, :, 16:] = 0                    # latent columns 0, 1 edit freely, columns 2, 3 keep the source


@pytest.fixture()
def model():
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    m.load_state_dict(deterministic_dit_state_dict(**TINY), device=DEV)
    return m


def _inputs():
    lat = torch.cat([det_uniform("win.src", (1, 16, 7, 4, 4), 1.0), det_uniform("win.noise", (1, 16, 8, 4, 4), 1.0)], dim=2)
    return lat, det_uniform("win.ctx", (37, 64), 1.0), det_uniform("win.neg", (9, 64), 1.0)


def _pipe(model, kind="unipc"):
    if kind == "unipc":
        return WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))
    return WanPipeline(transformer=model, scheduler=FlowDPMSolverMultistepScheduler(shift=1.0, solver_order=2, algorithm_type=kind))


def _run(pipe, scale=1.0, steps_out=None, dtype=torch.float32, **kw):
    lat, ctx, neg = _inputs()
    cb = None
    if steps_out is not None:
        cb = lambda p, i, t, d: steps_out.append(d["latents"].clone()) or {}
    return pipe(latents=lat.to(DEV), prompt_embeds=[ctx.to(DEV)], negative_prompt_embeds=[neg.to(DEV)] if scale > 1 else None,
                reasoning_frames=4, num_inference_steps=STEPS, guidance_scale=scale, shift=SHIFT, repeat_rope=True, cot=True,
                output_type="latent", weight_dtype=dtype, callback_on_step_end=cb, **SIZE, **kw).latents


WINDOWS = dict(temporal_window=13, temporal_overlap=8)


@pytest.mark.parametrize("case", ["plain", "windows", "guidance"])
def test_a_full_mask_changes_nothing(model, case):
    kw = dict(WINDOWS) if case == "windows" else dict(scale=3.0) if case == "guidance" else {}
    plain = _run(_pipe(model), **kw)
    masked = _run(_pipe(model), edit_mask=FULL, **kw)
    assert torch.equal(bits(masked), bits(plain))
    assert torch.equal(bits(_run(_pipe(model), edit_mask=torch.from_numpy(FULL).to(DEV)[None], edit_mask_grow=(4, 2), edit_mask_feather=4,
                                 **kw)), bits(plain))


def _excess(out, seen, target0=FS + G, cells=slice(None)):
    """The zero-mask bound's quantity on the cells `cells` (latent columns): the result's target against its source block, in ulps of the
    larger of the source and the target that entered the last step (`seen[-2]`, in the loop's own layout)."""
    return EB.zero_mask_excess(out[:, :, FS + G:][..., cells], out[:, :, :FS][..., cells], seen[-2][:, :, target0:][..., cells])


@pytest.mark.parametrize("kind,dtype", [("unipc", torch.float32), ("unipc", torch.bfloat16), ("sde-dpmsolver++", torch.float32)])
def test_b_an_empty_mask_returns_the_source(model, kind, dtype):
    """Bound: ZERO_MASK_ULPS of tests/edit_mask_bounds.py (derived from the rounding count, checked on the CPU in
    tests/test_edit_mask_host.py).  Observed on an MI355X: docs/TEST_BOUNDS.md."""
    seen = []
    gen = torch.Generator(device=DEV).manual_seed(3) if kind.startswith("sde") else None
    out = _run(_pipe(model, kind), steps_out=seen, dtype=dtype, edit_mask=NONE, generator=gen)
    assert out.dtype == dtype and len(seen) == STEPS
    ulps = _excess(out, seen)
    src = _inputs()[0][:, :, :FS]
    away = float((seen[-2][:, :, FS + G:].float().cpu() - src).abs().max())
    drift = float((out[:, :, :FS].float().cpu() - src).abs().max())
    print(f"empty mask {kind} {dtype}: {ulps:.2f} ulps (bound {EB.ZERO_MASK_ULPS}); the target entered the last step {away:.3f} away; "
          f"the source block itself moved {drift:.2e}")
    assert ulps <= EB.ZERO_MASK_ULPS and away > 0.05
    assert not torch.equal(out[:, :, FS:FS + G], seen[0][:, :, FS:FS + G])          # the grounding block is denoised as ever


def _composed_loop(model, weights):
    """The masked loop composed from the model's own forwards, ops.masked_prediction_ and scheduler.step: what the pipeline must
    reproduce bit for bit."""
    lat, ctx, _ = _inputs()
    state, ctx = lat.to(DEV), ctx.to(DEV)
    sched = FlowUniPCMultistepScheduler(shift=1)
    sched.set_timesteps(STEPS, device=DEV, shift=SHIFT)
    keep = model.cache_context, model.skip_source_frames, model.mask_source_frames
    model.cache_context, model.skip_source_frames, model.mask_source_frames = True, FS, FS
    model.clear_context_cache()
    try:
        for i, t in enumerate(sched.timesteps):
            pred = model(state, t.expand(1), [ctx], SEQ, frame_split_indices=[FS], ground_frame_indices=[(FS, FS + G)])
            pred = ops.masked_prediction_(pred.contiguous(), state, weights, FS, FS + G, float(sched.sigmas[i]))
            state = sched.step(pred, t, state, return_dict=False)[0]
    finally:
        model.cache_context, model.skip_source_frames, model.mask_source_frames = keep
        model.clear_context_cache()
    return state


def test_c_half_a_mask(model):
    """Left half 255, right half 0, grow = feather = 0: the right half meets the empty mask's bound, and the whole result -- the left
    half in particular -- is the composed loop bit for bit: the pipeline's wiring adds nothing of its own."""
    weights = latent_edit_mask(HALF, grow=0, grow_t=0, feather=0)[None]
    assert weights.shape == (1, FS, 4, 4) and bool((weights[..., :2] == 255).all()) and not bool(weights[..., 2:].any())
    seen = []
    out = _run(_pipe(model), steps_out=seen, edit_mask=HALF, edit_mask_grow=(0, 0), edit_mask_feather=0)
    ulps = _excess(out, seen, cells=slice(2, 4))
    print(f"half mask, right half: {ulps:.2f} ulps (bound {EB.ZERO_MASK_ULPS})")
    assert ulps <= EB.ZERO_MASK_ULPS
    want = _composed_loop(model, weights)
    assert torch.equal(bits(out[..., :2]), bits(want[..., :2])) and torch.equal(bits(out), bits(want))
    plain = _run(_pipe(model))
    assert not torch.equal(out[:, :, FS + G:][..., :2], plain[:, :, FS + G:][..., :2])      # attention sees the pinned half


def test_d_step_graph_is_bit_identical_to_eager(model):
    eager, graphed = [], []
    a = _run(_pipe(model), steps_out=eager, edit_mask=HALF)
    pipe = _pipe(model)
    b = _run(pipe, steps_out=graphed, edit_mask=HALF, capture_graph="step")
    assert pipe._graphed.replays >= 1
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(eager, graphed)) and torch.equal(bits(a), bits(b))
    assert not torch.equal(a, _run(_pipe(model)))


def test_e_unsupported_and_malformed_calls_raise(model):
    with pytest.raises(NotImplementedError, match="capture_graph='loop'"):
        _run(_pipe(model), edit_mask=HALF, capture_graph="loop")
    with pytest.raises(ValueError, match=r"expected uint8 \[25, 32, 32\]"):
        _run(_pipe(model), edit_mask=HALF[:24])
    with pytest.raises(ValueError, match="1 or 1 samples"):
        _run(_pipe(model), edit_mask=np.stack([HALF, HALF]))
    with pytest.raises(ValueError, match="has none"):
        _pipe(model)(prompt_embeds=[_inputs()[1].to(DEV)], num_inference_steps=STEPS, guidance_scale=1.0, cot=True, output_type="latent",
                     edit_mask=HALF, **SIZE)


def test_f_windows_with_an_empty_mask(model):
    """The windowed loop (one sampler step on the whole state, the replacement after the blend) meets the same bound on the un-windowed
    result; the callback sees the windowed layout, whose target starts at Fs + K * G."""
    seen = []
    out = _run(_pipe(model), steps_out=seen, edit_mask=NONE, **WINDOWS)
    assert out.shape == (1, 16, 2 * FS + G, 4, 4) and seen[-1].shape == (1, 16, 2 * FS + K * G, 4, 4)
    ulps = _excess(out, seen, target0=FS + K * G)
    print(f"windows, empty mask: {ulps:.2f} ulps (bound {EB.ZERO_MASK_ULPS})")
    assert ulps <= EB.ZERO_MASK_ULPS
