"""Edit inside a mask on the CPU (no GPU, unmarked): the two definitions the kernels are tested against (reference_latent_edit_mask,
reference_masked_prediction), the zero-mask bound of tests/edit_mask_bounds.py on the host schedulers with a float64 yardstick,
fit_mask's definition, the argument errors and the entry points' host-side validation.  docs/TEST_BOUNDS.md, "Edit inside a mask"."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from videocof_amd import (FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, WanPipeline, _lib, fit_mask, get_sampling_sigmas,
                          latent_edit_mask, ops, reference_fit_mask, reference_latent_edit_mask, reference_masked_prediction,
                          retrieve_timesteps)
from videocof_amd.video_io import _resample_axis, fit_plan, resample_axis_table
from videocof_amd.weights import det_uniform

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_mask_bounds as EB  # noqa: E402

LEGAL = [(g, gt, f) for g in range(5) for gt in range(3) for f in range(g + 1)]          # every (grow, grow_t, feather) the limits allow


def _single(T, H, W, t, y, x, value=255):
    a = np.zeros((T, H, W), dtype=np.uint8)
    a[t, y, x] = value
    return a


# ------------------------------------------------------------------------------------------------ reference_latent_edit_mask
def test_empty_and_full_masks_stay_empty_and_full():
    for g, gt, f in LEGAL:
        for T in (1, 6, 9):
            assert not reference_latent_edit_mask(np.zeros((T, 16, 24), np.uint8), grow=g, grow_t=gt, feather=f).any()
            full = reference_latent_edit_mask(np.full((2, T, 16, 24), 255, np.uint8), grow=g, grow_t=gt, feather=f)
            assert full.shape == (2, 1 + (T + 2) // 4, 2, 3) and bool((full == 255).all())


@pytest.mark.parametrize("frame,latent", [(0, 0), (1, 1), (4, 1), (5, 2), (8, 2)])
def test_a_pixel_lands_in_its_latent_frame_and_cell(frame, latent):
    """Latent frame 0 is pixel frame 0; latent frame j >= 1 is frames 4j-3 .. 4j.  The pixel's cell has weight 255 for every legal
    (grow, feather): feather <= grow keeps the whole feather window inside the grown region."""
    a = _single(9, 32, 40, frame, 19, 33)                    # cell (2, 4)
    w = reference_latent_edit_mask(a, grow=0, grow_t=0, feather=0)
    assert w.shape == (3, 4, 5)
    assert sorted(map(tuple, w.nonzero().tolist())) == [(latent, 2, 4)] and int(w[latent, 2, 4]) == 255
    for g, gt, f in LEGAL:
        w = reference_latent_edit_mask(a, grow=g, grow_t=gt, feather=f)
        assert int(w[latent, 2, 4]) == 255, (g, gt, f)
        hit = w.nonzero()
        assert int((hit[:, 0] - latent).abs().max()) <= gt                                     # grow_t latent frames, no further
        assert int(torch.maximum((hit[:, 1] - 2).abs(), (hit[:, 2] - 4).abs()).max()) <= g + f  # grow + feather cells, no further


def test_a_short_last_group():
    """T = 6: latent frames {0}, {1..4}, {5} -- three of them, the last one of a single pixel frame."""
    for frame, latent in ((0, 0), (4, 1), (5, 2)):
        w = reference_latent_edit_mask(_single(6, 8, 8, frame, 3, 3, 200), grow=0, grow_t=0, feather=0)
        assert w.shape == (3, 1, 1) and w[:, 0, 0].tolist() == [200 if j == latent else 0 for j in range(3)]


def test_weights_are_monotone_in_the_mask_and_in_grow():
    rng = np.random.default_rng(5)
    a = (rng.integers(0, 256, (2, 9, 32, 40)) * (rng.random((2, 9, 32, 40)) < 0.01)).astype(np.uint8)
    more = np.maximum(a, (rng.integers(0, 256, a.shape) * (rng.random(a.shape) < 0.01)).astype(np.uint8))
    for g, gt, f in ((0, 0, 0), (1, 0, 1), (2, 1, 1), (4, 2, 4)):
        w = reference_latent_edit_mask(a, grow=g, grow_t=gt, feather=f)
        assert bool((reference_latent_edit_mask(more, grow=g, grow_t=gt, feather=f) >= w).all())
        if g < 4:
            assert bool((reference_latent_edit_mask(a, grow=g + 1, grow_t=gt, feather=f) >= w).all())
        if gt < 2:
            assert bool((reference_latent_edit_mask(a, grow=g, grow_t=gt + 1, feather=f) >= w).all())


def test_the_definition_against_a_slow_statement():
    """The vectorised numpy against three nested loops, grey values and a batch: the dilation never crosses from one sample to the next."""
    rng = np.random.default_rng(7)
    a = (rng.integers(1, 256, (2, 6, 24, 32)) * (rng.random((2, 6, 24, 32)) < 0.004)).astype(np.uint8)
    g, gt, f = 2, 1, 1
    B, T, H, W = a.shape
    Fl, h, w = 3, H // 8, W // 8
    p = np.zeros((B, Fl, h, w), np.int64)
    for b, t, y, x in itertools.product(range(B), range(T), range(H), range(W)):
        j = 0 if t == 0 else (t + 3) // 4
        p[b, j, y // 8, x // 8] = max(p[b, j, y // 8, x // 8], a[b, t, y, x])
    grown = np.zeros_like(p)
    for b, j, y, x in itertools.product(range(B), range(Fl), range(h), range(w)):
        grown[b, j, y, x] = p[b, max(j - gt, 0):j + gt + 1, max(y - g, 0):y + g + 1, max(x - g, 0):x + g + 1].max()
    want = np.zeros_like(p)
    for b, j, y, x in itertools.product(range(B), range(Fl), range(h), range(w)):
        s = sum(grown[b, j, min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)] for dy in range(-f, f + 1) for dx in range(-f, f + 1))
        want[b, j, y, x] = (2 * s + 9) // 18
    assert np.array_equal(reference_latent_edit_mask(a, grow=g, grow_t=gt, feather=f).numpy(), want.astype(np.uint8))


# ------------------------------------------------------------------------------------------------ reference_masked_prediction
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_masked_prediction_exact_cases_and_untouched_frames(dtype):
    B, C, Fs, G, h, w = 2, 3, 2, 1, 3, 5
    pred = det_uniform("em.pred", (B, C, 2 * Fs + G, h, w), 2.0).to(dtype)
    sample = det_uniform("em.sample", (B, C, 2 * Fs + G, h, w), 2.0).to(dtype)
    pred[0, 0, Fs + G, 0, 0] = -0.0                                                 # weight 255 keeps even the sign of a zero
    orig, bits = pred.clone(), torch.int16 if dtype == torch.bfloat16 else torch.int32
    sigma = 0.7371
    keep = reference_masked_prediction(pred, sample, torch.full((1, Fs, h, w), 255, dtype=torch.uint8), Fs, Fs + G, sigma)
    assert torch.equal(keep.view(bits), pred.view(bits))
    zero = reference_masked_prediction(pred, sample, torch.zeros((B, Fs, h, w), dtype=torch.uint8), Fs, Fs + G, sigma)
    # a == 0: round((x_t - s) / sigma), the division as numpy's float32 (IEEE) does it
    d = sample[:, :, Fs + G:].float().numpy() - sample[:, :, :Fs].float().numpy()
    r = torch.from_numpy(d / np.float32(sigma)).to(dtype)
    assert torch.equal(zero[:, :, Fs + G:], r)
    assert torch.equal(zero[:, :, :Fs + G], pred[:, :, :Fs + G])                    # source and grounding frames: never written
    # a grey weight, every operation in numpy float32
    a = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (B, Fs, h, w)).astype(np.uint8))
    got = reference_masked_prediction(pred, sample, a, Fs, Fs + G, sigma)
    wgt = (a.numpy().astype(np.float32) / np.float32(255.0))[:, None]
    v = pred[:, :, Fs + G:].float().numpy()
    want = torch.from_numpy((wgt * v) + ((np.float32(1.0) - wgt) * (d / np.float32(sigma)))).to(dtype)
    want = torch.where((a == 255)[:, None], pred[:, :, Fs + G:], want)
    assert torch.equal(got[:, :, Fs + G:], want)
    assert torch.equal(pred.view(bits), orig.view(bits))                           # the definition changes nothing in place


def _scheduler(kind, steps=3, shift=3.0):
    if kind == "unipc":
        s = FlowUniPCMultistepScheduler(shift=1)
        s.set_timesteps(steps, device="cpu", shift=shift)
    else:
        s = FlowDPMSolverMultistepScheduler(shift=1.0, solver_order=2, algorithm_type=kind)
        retrieve_timesteps(s, device="cpu", sigmas=get_sampling_sigmas(steps, shift))
    return s


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++", "sde-dpmsolver++"])
def test_a_zero_mask_loop_lands_on_the_source(kind, dtype):
    """w = 0 everywhere, a random v, three steps of the host schedulers: the target ends within ZERO_MASK_ULPS ulps of the source block
    (the bound of tests/edit_mask_bounds.py, derived from the rounding count of x0 = x - sigma * round((x - s) / sigma); nothing here is
    calibrated on a kernel).  The float64 yardstick: the same x0 in float64 is the source to a few 1e-16, so all of the distance is
    rounding in the tensors' dtype."""
    Fs, G, shape = 3, 1, (1, 4, 7, 3, 5)
    weights = torch.zeros((1, Fs, 3, 5), dtype=torch.uint8)
    sched = _scheduler(kind)
    gen = torch.Generator().manual_seed(11)
    state = det_uniform("em.loop", shape, 1.0).to(dtype)
    before = state
    for i, t in enumerate(sched.timesteps):
        v = det_uniform(f"em.loop.v{i}", shape, 2.0).to(dtype)
        v[:, :, :Fs] = 0                                                        # the CoF mask
        v = reference_masked_prediction(v, state, weights, Fs, Fs + G, float(sched.sigmas[i]))
        before = state
        state = sched.step(v, t, state, return_dict=False, **({"generator": gen} if kind.startswith("sde") else {}))[0]
    src, tgt = state[:, :, :Fs], state[:, :, Fs + G:]
    assert state.dtype == dtype
    assert torch.equal(src, before[:, :, :Fs])                                  # the last step returns x0, and the source's x0 is itself
    far = float((before[:, :, Fs + G:].double() - src.double()).abs().max())
    assert far > 0.05                                                           # (the target was not there yet: two steps of a random v)
    x, s, sigma = before[:, :, Fs + G:].double(), src.double(), float(sched.sigmas[len(sched.timesteps) - 1])
    assert float((x - sigma * ((x - s) / sigma) - s).abs().max()) < 1e-14       # the yardstick
    ulps = EB.zero_mask_excess(tgt, src, before[:, :, Fs + G:])
    print(f"zero-mask host loop {kind} {dtype}: {ulps:.2f} ulps (bound {EB.ZERO_MASK_ULPS}); the target entered the last step {far:.3f} away")
    assert ulps <= EB.ZERO_MASK_ULPS


def test_ulp_of():
    assert EB.ulp_of(torch.tensor([1.0, 1.5, 2.0, 0.75]), torch.float32).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24]
    assert EB.ulp_of(torch.tensor([1.0, 3.0]), torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -6]


# ------------------------------------------------------------------------------------------------ argument errors
@pytest.mark.parametrize("bad", [dict(grow=5), dict(grow=-1), dict(grow_t=3), dict(feather=2), dict(grow=2, feather=3), dict(feather=-1),
                                 dict(grow=1.5)])
def test_the_limits_raise(bad):
    a = np.zeros((5, 16, 16), np.uint8)
    with pytest.raises(ValueError, match="grow"):
        reference_latent_edit_mask(a, **bad)
    with pytest.raises(ValueError, match="grow"):
        latent_edit_mask(a, **bad)                      # before anything touches a device


def test_bad_masks_raise_before_any_device_work():
    for fn in (reference_latent_edit_mask, latent_edit_mask):
        with pytest.raises(ValueError, match="uint8"):
            fn(np.zeros((5, 16, 16), np.float32))
        with pytest.raises(ValueError, match="uint8"):
            fn(np.zeros((16, 16), np.uint8))
        with pytest.raises(ValueError, match="latent cells"):
            fn(np.zeros((5, 16, 20), np.uint8))
    plan = fit_plan(54, 100, 32, 48)
    for fn in (reference_fit_mask, fit_mask):
        with pytest.raises(ValueError, match="54 x 100"):
            fn(np.zeros((5, 32, 48), np.uint8), plan)
        with pytest.raises(ValueError, match="FitPlan"):
            fn(np.zeros((5, 54, 100), np.uint8), None)
    p, s, w = torch.zeros(1, 2, 5, 3, 5), torch.zeros(1, 2, 5, 3, 5), torch.zeros(1, 2, 3, 5, dtype=torch.uint8)
    with pytest.raises(ValueError, match="sigma"):
        reference_masked_prediction(p, s, w, 2, 3, 0.0)
    with pytest.raises(ValueError, match="do not fit"):
        reference_masked_prediction(p, s, w, 2, 4, 0.5)
    with pytest.raises(ValueError, match="weights"):
        reference_masked_prediction(p, s, w[:, :1], 2, 3, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.masked_prediction_(p, s, w, 2, 3, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.latent_mask(torch.zeros(1, 5, 16, 16, dtype=torch.uint8), 1, 0, 1)


def test_the_pipeline_validates_the_mask_before_any_device_work():
    """Every refusal comes before the text encoder, the VAE or the transformer is touched: a pipeline whose transformer is a bare object
    (any use of it is an AttributeError) and that has neither of the other two gets there."""
    pipe = WanPipeline(transformer=object(), scheduler=FlowUniPCMultistepScheduler(shift=1))
    lat = torch.zeros(1, 16, 15, 4, 4)
    kw = dict(latents=lat, source_frames=25, height=32, width=32, cot=True, output_type="latent")
    ok = np.zeros((25, 32, 32), np.uint8)
    with pytest.raises(ValueError, match="has none"):
        pipe(edit_mask=ok, source_frames=25, height=32, width=32)
    with pytest.raises(ValueError, match=r"expected uint8 \[25, 32, 32\]"):
        pipe(edit_mask=ok.astype(np.float32), **kw)
    with pytest.raises(ValueError, match=r"expected uint8 \[25, 32, 32\]"):
        pipe(edit_mask=ok[0], **kw)
    with pytest.raises(ValueError, match=r"expected uint8 \[25, 32, 32\]"):
        pipe(edit_mask=np.zeros((24, 32, 32), np.uint8), **kw)
    with pytest.raises(ValueError, match=r"expected uint8 \[25, 32, 32\]"):
        pipe(edit_mask=np.zeros((2, 25, 32, 40), np.uint8), **kw)
    with pytest.raises(ValueError, match="grow=5"):
        pipe(edit_mask=ok, edit_mask_grow=(5, 0), **kw)
    with pytest.raises(ValueError, match="feather=2"):
        pipe(edit_mask=ok, edit_mask_feather=2, **kw)
    with pytest.raises(ValueError, match="pair"):
        pipe(edit_mask=ok, edit_mask_grow=1, **kw)
    with pytest.raises(NotImplementedError, match="capture_graph='loop'"):
        pipe(edit_mask=ok, capture_graph="loop", **kw)
    with pytest.raises(TypeError, match="edit_masks"):
        pipe(edit_masks=ok, **kw)


# ------------------------------------------------------------------------------------------------ fit_mask
@pytest.mark.parametrize("orig,fit", [((54, 100), (32, 48)), ((37, 29), (48, 32)), ((64, 64), (32, 32))])
def test_fit_mask_is_the_plans_two_passes(orig, fit):
    """reference_fit_mask = _resample_axis with the plan's tables (its crop window included), horizontal first -- and, channel by channel,
    what reference_fit_frames makes of the same bytes."""
    from videocof_amd import reference_fit_frames
    rng = np.random.default_rng(orig[0])
    a = rng.integers(0, 256, (2, 3) + orig).astype(np.uint8)
    plan = fit_plan(*orig, *fit)
    want = _resample_axis(a.astype(np.int64), -1, resample_axis_table(plan.width, plan.new_width, plan.x0, plan.out_width))
    want = _resample_axis(want, -2, resample_axis_table(plan.height, plan.new_height, plan.y0, plan.out_height)).astype(np.uint8)
    got = reference_fit_mask(a, plan)
    assert got.shape == (2, 3) + fit and np.array_equal(got.numpy(), want)
    frames = reference_fit_frames(np.repeat(a[..., None], 3, axis=-1), *fit, plan)
    assert all(torch.equal(frames[..., c], got) for c in range(3))
    assert torch.equal(reference_fit_mask(a[0], plan), got[0])


# ------------------------------------------------------------------------------------------------ the entry points, without a GPU
def test_entry_points_refuse_bad_arguments_before_launching():
    lib = _lib.load()
    inv = _lib.WAN_ERR_INVALID
    ws = lib.wan_latent_mask_workspace_bytes(1, 9, 32, 72)
    assert ws == 2 * 3 * 4 * 9 and lib.wan_latent_mask_workspace_bytes(2, 6, 16, 24) == 2 * 2 * 3 * 2 * 3
    mask = lambda *a, ws=ws: lib.wan_latent_mask_u8(*a, 8, ws, None)
    assert mask(None, 8, 1, 9, 32, 72, 8, 4, 1, 0, 1) == inv
    with pytest.raises(ValueError, match="null tensor"):
        _lib.check(inv, "wan_latent_mask_u8")
    assert mask(8, None, 1, 9, 32, 72, 8, 4, 1, 0, 1) == inv
    assert lib.wan_latent_mask_u8(8, 8, 1, 9, 32, 72, 8, 4, 1, 0, 1, None, ws, None) == inv             # no workspace
    assert mask(8, 8, 1, 9, 36, 72, 8, 4, 1, 0, 1) == inv                                               # H % 8
    with pytest.raises(ValueError, match="latent cells"):
        _lib.check(inv, "wan_latent_mask_u8")
    assert mask(8, 8, 1, 9, 32, 76, 8, 4, 1, 0, 1) == inv                                               # W % 8
    assert mask(8, 8, 1, 9, 32, 72, 8, 4, 1, 0, 2) == inv                                               # feather > grow
    with pytest.raises(ValueError, match="feather=2"):
        _lib.check(inv, "wan_latent_mask_u8")
    assert mask(8, 8, 1, 9, 32, 72, 8, 4, 5, 0, 1) == inv and mask(8, 8, 1, 9, 32, 72, 8, 4, 1, 3, 1) == inv
    assert mask(8, 8, 1, 9, 32, 72, 8, 4, -1, 0, -1) == inv
    assert mask(8, 8, 1, 9, 32, 72, 16, 4, 1, 0, 1) == inv and mask(8, 8, 1, 9, 32, 72, 8, 8, 1, 0, 1) == inv      # other ratios
    assert mask(8, 8, 1, 9, 32, 72, 8, 4, 1, 0, 1, ws=ws - 1) == inv                                    # workspace too small
    assert mask(8, 8, 0, 9, 32, 72, 8, 4, 1, 0, 1) == inv
    assert mask(8, 8, 64, 1024, 4096, 4096, 8, 4, 1, 0, 1, ws=1 << 40) == inv                           # 2^40 mask bytes
    with pytest.raises(ValueError, match="mask bytes"):
        _lib.check(inv, "wan_latent_mask_u8")

    pred = lambda *a: lib.wan_masked_prediction(*a, None)
    good = (8, 8, 0, 8, 1, 1, 16, 15, 7, 8, 16, 0.5)             # pred, sample, dtype, weights, B, Bm, C, F, Fs, target_frame0, hw, sigma
    for k in (0, 1, 3):
        assert pred(*good[:k], None, *good[k + 1:]) == inv
    with pytest.raises(ValueError, match="null tensor"):
        _lib.check(inv, "wan_masked_prediction")
    for sigma in (0.0, -0.5, float("inf"), float("nan")):
        assert pred(*good[:11], sigma) == inv
    with pytest.raises(ValueError, match="sigma"):
        _lib.check(inv, "wan_masked_prediction")
    assert pred(*good[:2], 2, *good[3:]) == inv                                                          # dtype
    assert pred(*good[:5], 2, *good[6:]) == inv                                                          # Bm not in {1, B}
    assert pred(*good[:9], 6, *good[10:]) == inv                                                         # the target overlaps the source
    assert pred(*good[:9], 9, *good[10:]) == inv                                                         # the target leaves the state
    with pytest.raises(ValueError, match="do not fit"):
        _lib.check(inv, "wan_masked_prediction")
    assert pred(*good[:10], 1 << 31, 0.5) == inv and pred(*good[:4], 1 << 16, 1, 1 << 16, *good[7:]) == inv      # counts of 2^31 or more
