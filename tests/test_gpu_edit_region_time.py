"""-m gpu: edit region, the time axis -- wan_region_crop_frames / wan_region_restore_frames against their torch definitions (bit for
bit, with guard bands) and against their spatial siblings, and WanPipeline(edit_region=True, edit_region_time_margin=...) against the
same pipeline WITHOUT the option run on the cropped latents with the cropped mask (call B of the issue): inside the range and the box
the two agree bit for bit, everywhere else the target is the source latents.  docs/TEST_BOUNDS.md, "Edit region: the time axis"."""
import ctypes

import numpy as np
import pytest
import torch

from videocof_amd import (FlowUniPCMultistepScheduler, RegionPlan, TimeRegion, WanPipeline, WanTransformer3DModel, _lib, latent_edit_mask,
                          ops, reference_region_crop_frames, reference_region_restore_frames, region_plan, region_time_plan)
from videocof_amd.weights import deterministic_dit_state_dict, det_uniform

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
    return t.view({torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}[t.dtype])


def _values(name, shape, dtype):
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(sum(map(ord, name))), dtype=torch.uint8)
    return det_uniform(name, shape, 2.0).to(dtype)


# (H, W, the region's x0 and width, guard elements).  The access unit: (6, 8) at 0 -- 16 bytes in fp32 and bf16, 8 in uint8; (6, 12) at 4
# -- 16 bytes in fp32, 8 in bf16, 4 in uint8; (5, 6) at 2 -- 8, 4, 2 bytes; (5, 7) at 1 -- one element; (6, 8) behind a 3-element band --
# one element through the bases alone; (3, 300) at 1 -- rows longer than 256 units.
FRAMES = [(6, 8, 0, 8, 64), (6, 12, 4, 8, 64), (5, 6, 2, 4, 64), (5, 7, 1, 5, 64), (6, 8, 0, 8, 3), (3, 300, 1, 290, 64)]
# (cc, G, t0, n): the range at either end of the clip, a single frame, G = 0, G = cc
RANGES = [(3, 1, 0, 3), (3, 1, 1, 2), (3, 1, 2, 1), (4, 2, 1, 2), (4, 0, 3, 1), (2, 2, 0, 2)]


def _runs(cc, G, t0, n):
    return [(t0, n)] + ([(cc, G)] if G else []) + [(cc + G + t0, n)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8], ids=["fp32", "bf16", "u8"])
@pytest.mark.parametrize("H,W,x0,wr,pad", FRAMES)
def test_crop_and_restore_equal_the_torch_definitions(H, W, x0, wr, pad, dtype):
    C = 2
    regions = [(1, x0, H - 2, wr), (0, 0, H, W)]
    for B in (1, 2):
        for cc, G, t0, n in RANGES:
            Ft = 2 * cc + G
            full = _values(f"ert.{H}.{W}.{B}.{cc}.{G}", (B, C, Ft, H, W), dtype)
            state = Guarded(full.shape, dtype, pad, full)
            source = Guarded((B, C, cc, H, W), dtype, pad, full[:, :, :cc])
            runs = _runs(cc, G, t0, n)
            for region in regions:
                y0, rx, hr, rw = region
                want = reference_region_crop_frames(full, runs, region)
                crop = Guarded(want.shape, dtype, pad)
                got = ops.region_crop_frames(state.view, runs, region, out=crop.view)
                assert got.data_ptr() == crop.view.data_ptr()
                assert torch.equal(bits(crop.view.cpu()), bits(want)), (B, runs, region)
                assert crop.intact() and state.intact()
                # the restore: a region-sized state of other values, so that every element shows where it came from
                final = _values(f"ert.final.{H}.{W}.{B}.{t0}.{n}.{y0}", want.shape, dtype)
                fin = Guarded(final.shape, dtype, pad, final)
                want_full = reference_region_restore_frames(full[:, :, :cc], final, (y0, rx), (t0, n))
                out = Guarded(full.shape, dtype, pad)
                got = ops.region_restore_frames(source.view, fin.view, (y0, rx), (t0, n), out=out.view)
                assert got.data_ptr() == out.view.data_ptr()
                res = out.view.cpu()
                assert torch.equal(bits(res), bits(want_full)), (B, runs, region)
                assert out.intact() and fin.intact() and source.intact()
                inside = torch.zeros(H, W, dtype=torch.bool)
                inside[y0:y0 + hr, rx:rx + rw] = True
                in_range = torch.zeros(cc, dtype=torch.bool)
                in_range[t0:t0 + n] = True
                src, target = full[:, :, :cc], res[:, :, cc + G:]
                assert torch.equal(bits(target[:, :, ~in_range]), bits(src[:, :, ~in_range]))        # outside the range: the source's bits
                assert torch.equal(bits(target[..., ~inside]), bits(src[..., ~inside]))              # outside the box: the source's bits
                assert torch.equal(bits(res[:, :, cc:cc + G][..., ~inside]), bits(src[:, :, :G][..., ~inside]))
                assert torch.equal(bits(res[:, :, :cc]), bits(src))
                assert torch.equal(bits(target[:, :, t0:t0 + n, y0:y0 + hr, rx:rx + rw]), bits(final[:, :, n + G:]))
                # the siblings: (0, cc) is wan_region_restore, one run (0, F) is wan_region_crop
                whole = _values(f"ert.whole.{H}.{W}.{B}.{cc}.{G}.{y0}", (B, C, Ft, hr, rw), dtype).to(DEV)
                assert torch.equal(bits(ops.region_restore_frames(source.view, whole, (y0, rx), (0, cc))),
                                   bits(ops.region_restore(source.view, whole, (y0, rx))))
                assert torch.equal(bits(ops.region_crop_frames(state.view, [(0, Ft)], region)), bits(ops.region_crop(state.view, region)))
            assert torch.equal(bits(state.view.cpu()), bits(full)) and torch.equal(bits(source.view.cpu()), bits(full[:, :, :cc]))


@pytest.mark.parametrize("H,W,x0,wr,pad", FRAMES[:5])
def test_the_weights_are_cropped_in_one_run(H, W, x0, wr, pad):
    for Bm in (1, 2):
        a = torch.randint(0, 256, (Bm, 5, H, W), generator=torch.Generator().manual_seed(H * W + Bm), dtype=torch.uint8)
        wts = Guarded(a.shape, torch.uint8, pad, a)
        for t0, n in ((0, 5), (0, 2), (1, 3), (4, 1)):
            region = (1, x0, H - 2, wr)
            want = reference_region_crop_frames(a, [(t0, n)], region)
            out = Guarded(want.shape, torch.uint8, pad)
            ops.region_crop_frames(wts.view, [(t0, n)], region, out=out.view)
            assert torch.equal(out.view.cpu(), want), (Bm, t0, n)
            assert out.intact() and wts.intact()
        assert torch.equal(wts.view.cpu(), a)


def test_invalid_arguments_raise_and_launch_nothing():
    src = Guarded((1, 2, 3, 6, 8), torch.float32)
    out = Guarded((1, 2, 7, 6, 8), torch.float32)
    small = Guarded((1, 2, 5, 2, 4), torch.float32)                             # n = 2, G = 1
    lib = _lib.load()
    for frames in ((2, 2), (-1, 2), (0, 4)):
        with pytest.raises(ValueError):
            ops.region_restore_frames(src.view, small.view, (0, 0), frames, out=out.view if frames != (0, 4) else None)
    with pytest.raises(ValueError, match="do not lie inside the 3 source frames"):
        ops.region_restore_frames(src.view, small.view, (0, 0), (2, 2), out=out.view)
    with pytest.raises(ValueError, match="G=5"):                               # 7 = 1 + 5 + 1 region frames: G > cc
        ops.region_restore_frames(src.view, torch.zeros(1, 2, 7, 2, 4, device=DEV), (0, 0), (0, 1))
    for origin in ((5, 0), (0, 5), (-1, 0)):
        with pytest.raises(ValueError, match="does not lie inside"):
            ops.region_restore_frames(src.view, small.view, origin, (0, 2), out=out.view)
    with pytest.raises(ValueError, match="region_restore_frames.out"):
        ops.region_restore_frames(src.view, small.view, (0, 0), (0, 2), out=out.view[:, :, :6])
    with pytest.raises(ValueError, match="one dtype"):
        ops.region_restore_frames(src.view, small.view.bfloat16(), (0, 0), (0, 2))
    for runs in ([], [(0, 1)] * 4, [(0, 2), (1, 2)], [(2, 1), (0, 1)], [(6, 2)], [(0, 0)], [(-1, 2)]):
        with pytest.raises(ValueError, match="run"):
            ops.region_crop_frames(out.view, runs, (0, 0, 2, 4))
    with pytest.raises(ValueError, match="pairs"):
        ops.region_crop_frames(out.view, [(0, 1, 2)], (0, 0, 2, 4))
    for region in ((0, 0, 7, 8), (0, 0, 6, 9), (5, 0, 2, 4), (0, 5, 2, 4), (-1, 0, 2, 4), (0, 0, 0, 4)):
        with pytest.raises(ValueError, match="does not lie inside"):
            ops.region_crop_frames(out.view, [(0, 2)], region)
    with pytest.raises(ValueError, match="region_crop_frames.out"):
        ops.region_crop_frames(out.view, [(0, 2), (3, 1), (4, 2)], (0, 0, 2, 4), out=small.view[:, :, :4])
    with pytest.raises(ValueError, match="contiguous"):
        ops.region_crop_frames(out.view.transpose(-1, -2), [(0, 2)], (0, 0, 2, 4))
    with pytest.raises(ValueError, match="1, 2 or 4"):
        ops.region_crop_frames(torch.zeros(2, 4, 4, device=DEV, dtype=torch.float64), [(0, 1)], (0, 0, 2, 2))
    p = lambda g: g.view.data_ptr()
    inv = _lib.WAN_ERR_INVALID
    runs = (ctypes.c_int * 6)(0, 2, 3, 1, 4, 2)
    assert lib.wan_region_restore_frames(None, p(src), p(small), 4, 1, 2, 3, 1, 6, 8, 0, 2, 0, 0, 2, 4, None) == inv             # null pointers
    assert lib.wan_region_restore_frames(p(out), None, p(small), 4, 1, 2, 3, 1, 6, 8, 0, 2, 0, 0, 2, 4, None) == inv
    assert lib.wan_region_restore_frames(p(out), p(src), None, 4, 1, 2, 3, 1, 6, 8, 0, 2, 0, 0, 2, 4, None) == inv
    assert lib.wan_region_restore_frames(p(out), p(src), p(small), 4, 1, 2, 3, 4, 6, 8, 0, 2, 0, 0, 2, 4, None) == inv           # G > cc
    assert lib.wan_region_restore_frames(p(out), p(src), p(small), 4, 1, 2, 3, 1, 6, 8, 2, 2, 0, 0, 2, 4, None) == inv           # t0 + n > cc
    assert lib.wan_region_crop_frames(None, p(out), 4, 2, 7, 6, 8, runs, 3, 0, 0, 2, 4, None) == inv
    assert lib.wan_region_crop_frames(p(small), None, 4, 2, 7, 6, 8, runs, 3, 0, 0, 2, 4, None) == inv
    assert lib.wan_region_crop_frames(p(small), p(out), 4, 2, 7, 6, 8, None, 3, 0, 0, 2, 4, None) == inv
    assert lib.wan_region_crop_frames(p(small), p(out), 4, 2, 7, 6, 8, runs, 0, 0, 0, 2, 4, None) == inv
    assert lib.wan_region_crop_frames(p(small), p(out), 4, 2, 5, 6, 8, runs, 3, 0, 0, 2, 4, None) == inv                          # a run leaves F = 5
    torch.cuda.synchronize()
    for g in (src, out, small):                                                # nothing was launched: every element is still the poison
        assert bool((g.buf == POISON).all())


# ------------------------------------------------------------------------------------------------ pipeline
STEPS, SHIFT = 3, 3.0
G, FS, HL, WL = 1, 5, 12, 16           # source_frames=17 -> 5 latent frames; 96 x 128 pixels -> 12 x 16 cells
SIZE = dict(source_frames=17, height=96, width=128)
WHOLE_FRAME = RegionPlan(0, 0, HL, WL)
SMALL = RegionPlan(0, 2, 10, 10)       # the existing file's region: the cell (5, 7), grow 1, feather 1 and a margin of 2 cells
MARGIN = (16, 16)
WIDE = (96, 128)                       # a spatial margin that makes the region the whole frame


def _mask(frames, box=(slice(40, 48), slice(56, 64))):
    """255 on the pixel frames `frames` (whole latent-frame groups: constant within each) and the pixel box (the cell (5, 7))."""
    m = np.zeros((17, 96, 128), np.uint8)
    m[(frames,) + box] = 255
    return m


MASK = _mask(slice(5, 13))             # pixel frames 5..12: latent frames 2..3
WINDOWS = dict(temporal_window=9, temporal_overlap=4)                          # 3 latent frames, 1 of overlap: two windows in 4 frames


@pytest.fixture(scope="module")
def sd():
    return deterministic_dit_state_dict(**TINY)


@pytest.fixture()
def model(sd):
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    m.load_state_dict(sd, device=DEV)
    return m


@pytest.fixture(scope="module")
def inputs():
    lat = torch.cat([det_uniform("ert.src", (1, 16, FS, HL, WL), 1.0), det_uniform("ert.noise", (1, 16, FS + G, HL, WL), 1.0)], dim=2)
    return lat.to(DEV), det_uniform("ert.ctx", (37, 64), 1.0).to(DEV), det_uniform("ert.neg", (9, 64), 1.0).to(DEV)


def _pipe(model):
    return WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))         # the deterministic sampler


def _call(pipe, inputs, lat=None, scale=1.0, steps_out=None, **kw):
    full, ctx, neg = inputs
    cb = None
    if steps_out is not None:
        cb = lambda p, i, t, d: steps_out.append(d["latents"].clone()) or {}
    kw = {**SIZE, **kw}
    return pipe(latents=(full if lat is None else lat).clone(), prompt_embeds=[ctx], negative_prompt_embeds=[neg] if scale > 1 else None,
                reasoning_frames=4, num_inference_steps=STEPS, guidance_scale=scale, shift=SHIFT, repeat_rope=True, cot=True,
                output_type="latent", weight_dtype=torch.float32, callback_on_step_end=cb, return_dict=True, **kw)


def _cropped_mask(mask, region, time):
    y, x, h, w = region.pixels()
    t0, n = time
    return np.ascontiguousarray(mask[4 * t0:4 * (t0 + n - 1) + 1, y:y + h, x:x + w])


def _call_b(pipe, inputs, region, time, mask=MASK, **kw):
    """Call B: the same pipeline WITHOUT the option on the cropped latents, with the mask cropped in pixel frames and pixels and the
    range's and the region's sizes."""
    t0, n = time
    lat = ops.region_crop_frames(inputs[0], [(t0, n), (FS, G), (FS + G + t0, n)], region)
    _, _, h, w = region.pixels()
    return _call(pipe, inputs, lat=lat, edit_mask=_cropped_mask(mask, region, time), source_frames=1 + 4 * (n - 1), height=h, width=w, **kw)


def _weights_agree(mask, region, time, **grow):
    """Call B's latent weights are call A's cropped ones (the masks are constant within each latent frame's pixel frames), and the
    planners give `region` and `time` for A's."""
    weights = latent_edit_mask(mask, **grow)[None]
    t0, n = time
    assert torch.equal(ops.region_crop_frames(weights, [(t0, n)], region), latent_edit_mask(_cropped_mask(mask, region, time), **grow)[None])
    return ops.mask_bounds(weights)


def _check_a_against_b(a, b, inputs, region, time):
    y0, x0, h, w = region
    t0, n = time
    full = inputs[0]
    assert a.edit_region == region.pixels() and a.edit_region_time == TimeRegion(t0, n).pixels()
    assert b.edit_region is None and b.edit_region_time is None
    assert a.latents.shape == full.shape and b.latents.shape == full.shape[:2] + (2 * n + G, h, w)
    inside = torch.zeros(HL, WL, dtype=torch.bool, device=DEV)
    inside[y0:y0 + h, x0:x0 + w] = True
    in_range = torch.zeros(FS, dtype=torch.bool, device=DEV)
    in_range[t0:t0 + n] = True
    src, ground, target = full[:, :, :FS], a.latents[:, :, FS:FS + G], a.latents[:, :, FS + G:]
    assert torch.equal(bits(ground[..., y0:y0 + h, x0:x0 + w]), bits(b.latents[:, :, n:n + G]))                  # grounding and target inside:
    assert torch.equal(bits(target[:, :, t0:t0 + n, y0:y0 + h, x0:x0 + w]), bits(b.latents[:, :, n + G:]))       # call B's bits
    assert torch.equal(bits(target[:, :, ~in_range]), bits(src[:, :, ~in_range]))                                # outside the range: the source's
    assert torch.equal(bits(target[..., ~inside]), bits(src[..., ~inside]))                                      # outside the box: the source's
    assert torch.equal(bits(ground[..., ~inside]), bits(src[:, :, :G][..., ~inside]))
    assert torch.equal(bits(a.latents[:, :, :FS]), bits(src))
    assert not torch.equal(b.latents[:, :, n + G:], ops.region_crop_frames(full, [(FS + G + t0, n)], region))    # the loop did run


def test_cropping_the_pixel_mask_and_cropping_the_weights_agree():
    bounds = _weights_agree(MASK, WHOLE_FRAME, (1, 4))
    assert bounds.tolist() == [[HL, -1, WL, -1]] * 2 + [[3, 7, 5, 9]] * 2 + [[HL, -1, WL, -1]]
    assert region_time_plan(bounds, FS, 1, G) == (1, 4) and region_time_plan(bounds, FS, 0, G) == (2, 2)
    assert region_plan(bounds, (HL, WL), (2, 2), None, 2) == SMALL
    _weights_agree(MASK, SMALL, (2, 2))


def test_a_time_only_equals_the_cropped_call(model, inputs):
    """The decisive case: without the feature the keyword is a TypeError.  The callback sees the range-sized state."""
    seen = []
    a = _call(_pipe(model), inputs, steps_out=seen, edit_mask=MASK, edit_region=True, edit_region_margin=WIDE, edit_region_time_margin=4)
    b = _call_b(_pipe(model), inputs, WHOLE_FRAME, (1, 4))
    _check_a_against_b(a, b, inputs, WHOLE_FRAME, (1, 4))
    assert a.edit_region_time == (1, 16)
    assert len(seen) == STEPS and all(s.shape == b.latents.shape for s in seen) and torch.equal(bits(seen[-1]), bits(b.latents))
    whole = _call(_pipe(model), inputs, edit_mask=MASK, edit_region=True, edit_region_margin=WIDE)       # the whole clip sees other context
    assert whole.edit_region_time is None and not torch.equal(whole.latents[:, :, FS + G + 1:], a.latents[:, :, FS + G + 1:])


def test_b_both_crops_at_once(model, inputs):
    a = _call(_pipe(model), inputs, edit_mask=MASK, edit_region=True, edit_region_margin=MARGIN, edit_region_time_margin=0)
    b = _call_b(_pipe(model), inputs, SMALL, (2, 2))
    _check_a_against_b(a, b, inputs, SMALL, (2, 2))
    assert a.edit_region_time == (5, 8) and a.edit_region == SMALL.pixels()


def test_c_a_range_longer_than_the_temporal_window_runs_as_windows(model, inputs):
    seen = []
    a = _call(_pipe(model), inputs, steps_out=seen, edit_mask=MASK, edit_region=True, edit_region_margin=WIDE, edit_region_time_margin=4,
              **WINDOWS)
    b = _call_b(_pipe(model), inputs, WHOLE_FRAME, (1, 4), **WINDOWS)
    _check_a_against_b(a, b, inputs, WHOLE_FRAME, (1, 4))
    plain = _call_b(_pipe(model), inputs, WHOLE_FRAME, (1, 4))
    assert not torch.equal(b.latents, plain.latents)                           # the windows did run: two of 3 frames over the 4
    assert seen[0].shape == b.latents.shape[:2] + (4 + 2 * G + 4,) + b.latents.shape[3:]       # the windowed state: a grounding block per window


def test_d_with_guidance(model, inputs):
    a = _call(_pipe(model), inputs, scale=3.0, edit_mask=MASK, edit_region=True, edit_region_margin=WIDE, edit_region_time_margin=4)
    b = _call_b(_pipe(model), inputs, WHOLE_FRAME, (1, 4), scale=3.0)
    _check_a_against_b(a, b, inputs, WHOLE_FRAME, (1, 4))
    assert not torch.equal(b.latents, _call_b(_pipe(model), inputs, WHOLE_FRAME, (1, 4)).latents)


def test_e_with_a_step_graph(model, inputs):
    pipe = _pipe(model)
    a = _call(pipe, inputs, edit_mask=MASK, edit_region=True, edit_region_margin=WIDE, edit_region_time_margin=4, capture_graph="step")
    assert pipe._graphed.replays >= 1
    _check_a_against_b(a, _call_b(_pipe(model), inputs, WHOLE_FRAME, (1, 4)), inputs, WHOLE_FRAME, (1, 4))


@pytest.mark.parametrize("frames,time", [(slice(0, 1), (0, 2)), (slice(13, 17), (3, 2))], ids=["first", "last"])
def test_f_a_mask_on_the_first_or_the_last_frame_only(model, inputs, frames, time):
    """Margin 0 and one marked latent frame: the floor of 2 frames, pushed inside the clip at either end."""
    mask = _mask(frames)
    bounds = _weights_agree(mask, WHOLE_FRAME, time)
    assert region_time_plan(bounds, FS, 0, G) == time
    a = _call(_pipe(model), inputs, edit_mask=mask, edit_region=True, edit_region_margin=WIDE, edit_region_time_margin=0)
    _check_a_against_b(a, _call_b(_pipe(model), inputs, WHOLE_FRAME, time, mask=mask), inputs, WHOLE_FRAME, time)


def test_g_a_range_that_is_the_whole_clip_changes_nothing(model, inputs):
    plain = _call(_pipe(model), inputs, edit_mask=MASK)
    a = _call(_pipe(model), inputs, edit_mask=MASK, edit_region=True, edit_region_margin=WIDE, edit_region_time_margin=8)
    assert a.edit_region == (0, 0, 96, 128) and a.edit_region_time == (0, 17) and torch.equal(bits(a.latents), bits(plain.latents))
    # the whole clip in time with a small region in space is the call with edit_region alone
    space = _call(_pipe(model), inputs, edit_mask=MASK, edit_region=True, edit_region_margin=MARGIN)
    a = _call(_pipe(model), inputs, edit_mask=MASK, edit_region=True, edit_region_margin=MARGIN, edit_region_time_margin=8)
    assert a.edit_region == SMALL.pixels() == space.edit_region and a.edit_region_time == (0, 17) and space.edit_region_time is None
    assert torch.equal(bits(a.latents), bits(space.latents))


def test_h_video_in_frames_out_keeps_the_shapes(model):
    """With the VAE on both sides: the source is encoded whole, the noise is drawn for the whole clip, the decode stays whole -- the
    outputs have the shapes of the call without the option, and outside the range the target latents are the encoded source."""
    from videocof_amd import AutoencoderKLWan
    from videocof_amd.weights import deterministic_vae_state_dict
    vae = AutoencoderKLWan()
    vae.load_state_dict(deterministic_vae_state_dict(), device=DEV)
    video = det_uniform("ert.video", (1, 3, 17, 64, 96), 0.8).to(DEV)           # 5 latent frames of 8 x 12 cells
    ctx = [det_uniform("ert.ctx", (37, 64), 1.0).to(DEV)]
    mask = np.zeros((17, 64, 96), np.uint8)
    mask[5:13, 24:32, 40:48] = 255                                             # latent frames 2..3, the cell (3, 5)
    pipe = WanPipeline(vae=vae, transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))

    def call(**kw):
        return pipe(video=video, prompt_embeds=ctx, height=64, width=96, source_frames=17, reasoning_frames=4, num_inference_steps=STEPS,
                    guidance_scale=1.0, shift=SHIFT, repeat_rope=True, cot=True, generator=torch.Generator(device=DEV).manual_seed(7),
                    weight_dtype=torch.float32, output_type="uint8", return_dict=True, edit_mask=mask, **kw)
    whole, a = call(), call(edit_region=True, edit_region_margin=(0, 0), edit_region_time_margin=0)
    assert a.edit_region == (0, 16, 48, 48) and a.edit_region_time == (5, 8) and whole.edit_region_time is None
    for name in ("videos", "ground_videos", "edit_videos"):
        assert getattr(a, name).shape == getattr(whole, name).shape and getattr(a, name).dtype == np.uint8
    assert a.videos.shape == (1, 18, 64, 96, 3) and a.latents.shape == whole.latents.shape == (1, 16, 11, 8, 12)
    source = a.latents[:, :, :FS]
    assert torch.equal(bits(source), bits(pipe._encode_modes(video, torch.device(DEV), torch.float32)))          # the source, encoded whole
    target = a.latents[:, :, FS + G:]
    assert torch.equal(bits(target[:, :, [0, 1, 4]]), bits(source[:, :, [0, 1, 4]]))                               # outside the range: its bits
    inside = torch.zeros(8, 12, dtype=torch.bool, device=DEV)
    inside[0:6, 2:8] = True
    assert torch.equal(bits(target[..., ~inside]), bits(source[..., ~inside]))
    assert not torch.equal(target[:, :, 2:4][..., inside], source[:, :, 2:4][..., inside])


def test_i_a_mask_grown_in_time_stays_inside_the_range(model, inputs):
    """edit_mask_grow=(1, 1) spreads the weights one latent frame to either side.  The bounds are those of the GROWN weights, so the
    range holds every frame with a weight and nothing outside it could dilate in: B's weights are still A's cropped ones."""
    grow = dict(grow=1, grow_t=1)
    bounds = _weights_agree(MASK, WHOLE_FRAME, (0, 5), **grow)
    assert [b[1] >= b[0] for b in bounds.tolist()] == [False, True, True, True, True]       # frames 2..3 grown to 1..4
    assert region_time_plan(bounds, FS, 1, G) == (0, 5)
    one = _mask(slice(13, 17))                                                 # latent frame 4 only: grown to 3..4, margin 4 -> [1, 5)
    bounds = _weights_agree(one, WHOLE_FRAME, (1, 4), **grow)
    assert [b[1] >= b[0] for b in bounds.tolist()] == [False, False, False, True, True]
    assert region_time_plan(bounds, FS, 1, G) == (1, 4)
    a = _call(_pipe(model), inputs, edit_mask=one, edit_mask_grow=(1, 1), edit_region=True, edit_region_margin=WIDE, edit_region_time_margin=4)
    b = _call_b(_pipe(model), inputs, WHOLE_FRAME, (1, 4), mask=one, edit_mask_grow=(1, 1))
    _check_a_against_b(a, b, inputs, WHOLE_FRAME, (1, 4))
