"""-m gpu: edit region -- wan_mask_bounds / wan_region_crop / wan_region_restore against their torch definitions (bit for bit, with
guard bands), and WanPipeline(edit_region=True) against the same pipeline run on the cropped latents with the cropped mask (call B of
the issue): inside the region the two agree bit for bit, outside it the target is the source latents.  docs/TEST_BOUNDS.md, "Edit region"."""
import numpy as np
import pytest
import torch

from videocof_amd import (FlowUniPCMultistepScheduler, RegionPlan, WanPipeline, WanTransformer3DModel, _lib, latent_edit_mask, ops,
                          reference_mask_bounds, reference_region_crop, reference_region_restore, region_plan)
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
    return t.view({torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8, torch.int32: torch.int32}[t.dtype])


# (H, W, the region's x0 and width, a corner's width, guard elements).  With the region at x0 the access unit is: (6, 8) at 0 -- 16 bytes
# in fp32 and bf16 (width 8); (6, 12) at 4 -- 16 bytes in fp32, 8 in bf16; (5, 6) at 2 -- 8 bytes in fp32, 4 in bf16; (5, 7) at 1 -- one
# element; (6, 8) behind a 3-element band -- one element through the bases alone; (3, 300) at 1 -- rows longer than 256 units; (135,
# 240), the 1080p frame with one 60 x 104 tile at its lower edge -- several workgroups per frame.
FRAMES = [(6, 8, 0, 8, 4, 64), (6, 12, 4, 8, 4, 64), (5, 6, 2, 4, 2, 64), (5, 7, 1, 5, 3, 64), (6, 8, 0, 8, 4, 3), (3, 300, 1, 290, 7, 64),
          (135, 240, 0, 104, 8, 64)]


def _regions(H, W, x0, wr, cw):
    """(y0, x0, h, w): the shape's own region, one in each corner, the whole frame, a single cell."""
    ch = min(2, H)
    own = (75, x0, 60, wr) if H == 135 else (1, x0, H - 2, wr)
    return [own, (0, 0, ch, cw), (0, W - cw, ch, cw), (H - ch, 0, ch, cw), (H - ch, W - cw, ch, cw), (0, 0, H, W), (H // 2, W // 2, 1, 1)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W,x0,wr,cw,pad", FRAMES)
def test_crop_and_restore_equal_the_torch_definitions(H, W, x0, wr, cw, pad, dtype):
    C, cc, G = 2, 2, 1
    for B in ((1,) if H * W > 1000 else (1, 2)):
        full = det_uniform(f"er.{H}.{W}.{B}", (B, C, 2 * cc + G, H, W), 2.0).to(dtype)
        full[0, 0, cc, 0, 0] = -0.0
        state = Guarded(full.shape, dtype, pad, full)
        source = Guarded((B, C, cc, H, W), dtype, pad, full[:, :, :cc])
        for region in _regions(H, W, x0, wr, cw):
            y0, rx, hr, rw = region
            want = reference_region_crop(full, region)
            crop = Guarded(want.shape, dtype, pad)
            got = ops.region_crop(state.view, region, out=crop.view)
            assert got.data_ptr() == crop.view.data_ptr()
            assert torch.equal(bits(crop.view.cpu()), bits(want)), (B, region)
            assert crop.intact() and state.intact()
            # the restore: a region-sized state of other values, so that every element shows where it came from
            final = det_uniform(f"er.final.{H}.{W}.{B}.{y0}.{rx}", want.shape, 2.0).to(dtype)
            fin = Guarded(final.shape, dtype, pad, final)
            want_full = reference_region_restore(full[:, :, :cc], final, (y0, rx))
            out = Guarded(full.shape, dtype, pad)
            got = ops.region_restore(source.view, fin.view, (y0, rx), out=out.view)
            assert got.data_ptr() == out.view.data_ptr()
            res = out.view.cpu()
            assert torch.equal(bits(res), bits(want_full)), (B, region)
            assert out.intact() and fin.intact() and source.intact()
            inside = torch.zeros(H, W, dtype=torch.bool)
            inside[y0:y0 + hr, rx:rx + rw] = True
            assert torch.equal(bits(res[:, :, cc + G:][..., ~inside]), bits(full[:, :, :cc][..., ~inside]))      # outside: the source's bits
            assert torch.equal(bits(res[:, :, :cc]), bits(full[:, :, :cc]))
        assert torch.equal(bits(state.view.cpu()), bits(full)) and torch.equal(bits(source.view.cpu()), bits(full[:, :, :cc]))
    # without `out`, and G = 0 and G = cc
    assert torch.equal(ops.region_crop(state.view, (0, 0, 1, W)).cpu(), full[..., :1, :])
    for g in (0, cc):
        st = det_uniform(f"er.g{g}", (1, C, 2 * cc + g, 1, 1), 2.0).to(dtype)
        got = ops.region_restore(source.view[:1], st.to(DEV), (H - 1, W - 1)).cpu()
        assert torch.equal(bits(got), bits(reference_region_restore(full[:1, :, :cc], st, (H - 1, W - 1))))


@pytest.mark.parametrize("H,W,x0,wr,cw,pad", FRAMES[:5])
def test_the_weights_are_cropped_as_bytes(H, W, x0, wr, cw, pad):
    for Bm in (1, 2):
        a = torch.randint(0, 256, (Bm, 3, H, W), generator=torch.Generator().manual_seed(H * W + Bm), dtype=torch.uint8)
        wts = Guarded(a.shape, torch.uint8, pad, a)
        for region in _regions(H, W, x0, wr, cw):
            want = reference_region_crop(a, region)
            out = Guarded(want.shape, torch.uint8, pad)
            ops.region_crop(wts.view, region, out=out.view)
            assert torch.equal(out.view.cpu(), want), (Bm, region)
            assert out.intact() and wts.intact()


# (h, w): rows of 16-, 8-, 4-, 2- and 1-byte units, a row longer than 256 units, the 1080p frame
BOUND_FRAMES = [(6, 16), (6, 8), (6, 12), (5, 6), (5, 7), (3, 259), (135, 240)]


@pytest.mark.parametrize("h,w", BOUND_FRAMES)
def test_bounds_equal_the_torch_definition(h, w):
    Fs = 5
    gen = torch.Generator().manual_seed(h * 1000 + w)
    for Bm in (1, 2):
        sparse = (torch.randint(1, 256, (Bm, Fs, h, w), generator=gen) * (torch.rand((Bm, Fs, h, w), generator=gen) < 4.0 / (h * w))).to(torch.uint8)
        some = sparse.clone()
        some[:, 1], some[:, 4] = 0, 0                                      # empty in some frames
        corners = torch.zeros((Bm, Fs, h, w), dtype=torch.uint8)
        corners[0, 0, 0, 0], corners[-1, 0, -1, -1] = 1, 255               # the whole frame from two cells (of two samples, if there are)
        corners[-1, 1, 0, -1], corners[0, 2, -1, 0], corners[0, 3, h // 2, w // 2] = 9, 9, 9
        for name, a in (("sparse", sparse), ("some", some), ("corners", corners), ("empty", torch.zeros_like(sparse)),
                        ("full", torch.full_like(sparse, 255))):
            for pad in (64, 3):                                                # 3: a base that only byte loads reach
                wts = Guarded(a.shape, torch.uint8, pad, a)
                out = Guarded((Fs, 4), torch.int32, 4)
                got = ops.mask_bounds(wts.view, out=out.view)
                assert got.data_ptr() == out.view.data_ptr()
                assert torch.equal(out.view.cpu(), reference_mask_bounds(a)), (Bm, name, pad)
                assert out.intact() and wts.intact() and torch.equal(wts.view.cpu(), a)
        assert ops.mask_bounds(torch.zeros_like(sparse).to(DEV)).tolist() == [[h, -1, w, -1]] * Fs
        assert ops.mask_bounds(corners.to(DEV)).tolist()[0] == [0, h - 1, 0, w - 1]


def test_invalid_arguments_raise_and_launch_nothing():
    src = Guarded((1, 2, 2, 6, 8), torch.float32)
    out = Guarded((1, 2, 5, 6, 8), torch.float32)
    small = Guarded((1, 2, 5, 2, 4), torch.float32)
    lib = _lib.load()
    with pytest.raises(ValueError, match="G=3"):                               # 7 = 2 + 3 + 2 state frames: G > cc
        ops.region_restore(src.view, torch.zeros(1, 2, 7, 2, 4, device=DEV), (0, 0))
    with pytest.raises(ValueError, match="does not lie inside"):
        ops.region_restore(src.view, small.view, (5, 0), out=out.view)
    with pytest.raises(ValueError, match="does not lie inside"):
        ops.region_restore(src.view, small.view, (0, 5), out=out.view)
    with pytest.raises(ValueError, match="does not lie inside"):
        ops.region_restore(src.view, small.view, (-1, 0), out=out.view)
    with pytest.raises(ValueError, match="region_restore.out"):
        ops.region_restore(src.view, small.view, (0, 0), out=out.view[:, :, :4])
    with pytest.raises(ValueError, match="one dtype"):
        ops.region_restore(src.view, small.view.bfloat16(), (0, 0))
    for region in ((0, 0, 7, 8), (0, 0, 6, 9), (5, 0, 2, 4), (0, 5, 2, 4), (-1, 0, 2, 4), (0, 0, 0, 4)):
        with pytest.raises(ValueError, match="does not lie inside"):
            ops.region_crop(out.view, region)
    with pytest.raises(ValueError, match="region_crop.out"):
        ops.region_crop(out.view, (0, 0, 2, 4), out=small.view[:, :, :4])
    with pytest.raises(ValueError, match="contiguous"):
        ops.region_crop(out.view.transpose(-1, -2), (0, 0, 2, 4))
    with pytest.raises(ValueError, match="1, 2 or 4"):
        ops.region_crop(torch.zeros(2, 4, 4, device=DEV, dtype=torch.float64), (0, 0, 2, 2))
    with pytest.raises(ValueError, match="uint8"):
        ops.mask_bounds(torch.zeros(1, 2, 4, 4, device=DEV))
    with pytest.raises(ValueError, match="mask_bounds.out"):
        ops.mask_bounds(torch.zeros(1, 2, 4, 4, device=DEV, dtype=torch.uint8), out=torch.zeros(3, 4, device=DEV, dtype=torch.int32))
    p = lambda g: g.view.data_ptr()
    inv = _lib.WAN_ERR_INVALID
    assert lib.wan_region_restore(None, p(src), p(small), 4, 1, 2, 2, 1, 6, 8, 0, 0, 2, 4, None) == inv             # null pointers
    assert lib.wan_region_restore(p(out), None, p(small), 4, 1, 2, 2, 1, 6, 8, 0, 0, 2, 4, None) == inv
    assert lib.wan_region_restore(p(out), p(src), None, 4, 1, 2, 2, 1, 6, 8, 0, 0, 2, 4, None) == inv
    assert lib.wan_region_restore(p(out), p(src), p(small), 4, 1, 2, 2, 3, 6, 8, 0, 0, 2, 4, None) == inv           # G > cc
    assert lib.wan_region_crop(None, p(out), 4, 10, 6, 8, 0, 0, 2, 4, None) == inv
    assert lib.wan_region_crop(p(small), None, 4, 10, 6, 8, 0, 0, 2, 4, None) == inv
    assert lib.wan_mask_bounds(None, p(out), 1, 2, 4, 4, None) == inv and lib.wan_mask_bounds(p(out), None, 1, 2, 4, 4, None) == inv
    torch.cuda.synchronize()
    for g in (src, out, small):                                                # nothing was launched: every element is still the poison
        assert bool((g.buf == POISON).all())


# ------------------------------------------------------------------------------------------------ pipeline
STEPS, SHIFT = 3, 3.0
G, FS, HL, WL = 1, 3, 12, 16           # source_frames=9 -> 3 latent frames; 96 x 128 pixels -> 12 x 16 cells
SIZE = dict(source_frames=9, height=96, width=128)
MASK = np.zeros((9, 96, 128), np.uint8)
MASK[:, 40:48, 56:64] = 255            # the cell (5, 7); grow 1 and feather 1 spread the weights over rows 3..7, columns 5..9
MARGIN = (16, 16)                      # 2 cells = edit_mask_grow + edit_mask_feather
REGION = RegionPlan(0, 2, 10, 10)      # rows: [2, 8) and the margin = [0, 10); columns: [4, 10) and the margin = [2, 12)
TILES = dict(spatial_window=(32, 32), spatial_overlap=(16, 16))             # tiles of 4 x 4 cells: the region is larger


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
    lat = torch.cat([det_uniform("er.src", (1, 16, FS, HL, WL), 1.0), det_uniform("er.noise", (1, 16, FS + G, HL, WL), 1.0)], dim=2)
    return lat.to(DEV), det_uniform("er.ctx", (37, 64), 1.0).to(DEV), det_uniform("er.neg", (9, 64), 1.0).to(DEV)


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


def _call_b(pipe, inputs, region, mask=MASK, **kw):
    """Call B: the same pipeline without the option on the cropped latents, with the mask cropped in pixels and the region's size."""
    y, x, h, w = region.pixels()
    lat = ops.region_crop(inputs[0], region)
    return _call(pipe, inputs, lat=lat, edit_mask=np.ascontiguousarray(mask[:, y:y + h, x:x + w]), height=h, width=w, **kw)


def _check_a_against_b(a, b, inputs, region):
    y0, x0, h, w = region
    full = inputs[0]
    assert a.edit_region == region.pixels() and b.edit_region is None
    assert a.latents.shape == full.shape and b.latents.shape == full.shape[:3] + (h, w)
    inside = torch.zeros(HL, WL, dtype=torch.bool, device=DEV)
    inside[y0:y0 + h, x0:x0 + w] = True
    assert torch.equal(bits(a.latents[:, :, FS:, y0:y0 + h, x0:x0 + w]), bits(b.latents[:, :, FS:]))         # grounding and target: call B's bits
    assert torch.equal(bits(a.latents[:, :, FS + G:][..., ~inside]), bits(full[:, :, :FS][..., ~inside]))     # outside: the source latents' bits
    assert torch.equal(bits(a.latents[:, :, FS:FS + G][..., ~inside]), bits(full[:, :, :G][..., ~inside]))
    assert torch.equal(bits(a.latents[:, :, :FS]), bits(full[:, :, :FS]))
    assert not torch.equal(b.latents[:, :, FS + G:], ops.region_crop(full, region)[:, :, FS + G:])            # the loop did run


def test_cropping_the_pixel_mask_and_cropping_the_weights_agree():
    """The margin is grow + feather cells, so the region's border is further from every marked cell than the dilation and the feather
    reach, and the feather clamps at borders: call B's weights are call A's."""
    weights = latent_edit_mask(MASK)[None]
    bounds = ops.mask_bounds(weights)
    assert torch.equal(bounds.cpu(), reference_mask_bounds(weights.cpu())) and bounds.tolist() == [[3, 7, 5, 9]] * FS
    assert region_plan(bounds, (HL, WL), (2, 2), None, 2) == REGION == region_plan(bounds, (HL, WL), (2, 2), (4, 4), 2)
    y, x, h, w = REGION.pixels()
    assert torch.equal(ops.region_crop(weights, REGION), latent_edit_mask(np.ascontiguousarray(MASK[:, y:y + h, x:x + w]))[None])


def test_a_the_region_equals_the_cropped_call(model, inputs):
    """The decisive case: without the option the call does not exist.  The callback sees the region-sized state."""
    seen = []
    a = _call(_pipe(model), inputs, steps_out=seen, edit_mask=MASK, edit_region=True, edit_region_margin=MARGIN)
    b = _call_b(_pipe(model), inputs, REGION)
    _check_a_against_b(a, b, inputs, REGION)
    assert len(seen) == STEPS and all(s.shape == b.latents.shape for s in seen) and torch.equal(bits(seen[-1]), bits(b.latents))
    whole = _call(_pipe(model), inputs, edit_mask=MASK)                       # the full-frame masked loop sees other context
    assert whole.edit_region is None and not torch.equal(whole.latents[:, :, FS + G:, :10, 2:12], a.latents[:, :, FS + G:, :10, 2:12])


def test_b_a_whole_frame_mask_changes_nothing(model, inputs):
    full = np.full((9, 96, 128), 255, np.uint8)
    plain = _call(_pipe(model), inputs, edit_mask=full)
    a = _call(_pipe(model), inputs, edit_mask=full, edit_region=True)
    assert a.edit_region == (0, 0, 96, 128) and torch.equal(bits(a.latents), bits(plain.latents))
    wide = MASK.copy()
    wide[:, 8:88, 8:120] = 255                                                 # cells 1..10 x 1..14: with the margin, the whole frame
    a = _call(_pipe(model), inputs, edit_mask=wide, edit_region=True, edit_region_margin=MARGIN)
    assert a.edit_region == (0, 0, 96, 128) and torch.equal(bits(a.latents), bits(_call(_pipe(model), inputs, edit_mask=wide).latents))


def test_c_a_region_larger_than_the_spatial_window_runs_as_tiles(model, inputs):
    seen = []
    a = _call(_pipe(model), inputs, steps_out=seen, edit_mask=MASK, edit_region=True, edit_region_margin=MARGIN, **TILES)
    b = _call_b(_pipe(model), inputs, REGION, **TILES)
    _check_a_against_b(a, b, inputs, REGION)
    plain = _call_b(_pipe(model), inputs, REGION)
    assert not torch.equal(b.latents, plain.latents)                           # the tiles did run: 4 x 4 of them over 10 x 10 cells
    assert seen[0].shape == b.latents.shape


def test_d_a_region_that_fits_one_tile_is_one_whole_clip(model, inputs):
    """spatial_window = 80 x 80 pixels = the region's 10 x 10 cells: one tile, the whole-clip form -- call B without windows at all."""
    a = _call(_pipe(model), inputs, edit_mask=MASK, edit_region=True, edit_region_margin=(0, 0), spatial_window=(80, 80), spatial_overlap=(16, 16))
    # margin 0: want = 6 <= 10 cells, so the tile's size, centred on the grid: rows [2, 8) less (10 - 6) // 4 * 2 = 2 -> 0; columns 4 - 2 -> 2
    assert a.edit_region == REGION.pixels()
    _check_a_against_b(a, _call_b(_pipe(model), inputs, REGION), inputs, REGION)


def test_e_with_guidance(model, inputs):
    a = _call(_pipe(model), inputs, scale=3.0, edit_mask=MASK, edit_region=True, edit_region_margin=MARGIN)
    b = _call_b(_pipe(model), inputs, REGION, scale=3.0)
    _check_a_against_b(a, b, inputs, REGION)
    assert not torch.equal(b.latents, _call_b(_pipe(model), inputs, REGION).latents)


def test_f_with_a_step_graph(model, inputs):
    pipe = _pipe(model)
    a = _call(pipe, inputs, edit_mask=MASK, edit_region=True, edit_region_margin=MARGIN, capture_graph="step")
    assert pipe._graphed.replays >= 1
    _check_a_against_b(a, _call_b(_pipe(model), inputs, REGION), inputs, REGION)


def test_h_video_in_frames_out_keeps_the_shapes(model):
    """With the VAE on both sides: the source is encoded whole, the noise is drawn for the whole frame, the decode stays full-frame --
    the outputs have the shapes of the call without the option, and outside the region the target latents are the encoded source."""
    from videocof_amd import AutoencoderKLWan
    from videocof_amd.weights import deterministic_vae_state_dict
    vae = AutoencoderKLWan()
    vae.load_state_dict(deterministic_vae_state_dict(), device=DEV)
    video = det_uniform("er.video", (1, 3, 9, 64, 96), 0.8).to(DEV)             # 8 x 12 cells
    ctx = [det_uniform("er.ctx", (37, 64), 1.0).to(DEV)]
    mask = np.zeros((9, 64, 96), np.uint8)
    mask[:, 24:32, 40:48] = 255                                                # the cell (3, 5); weights over rows 1..5, columns 3..7
    pipe = WanPipeline(vae=vae, transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))

    def call(**kw):
        return pipe(video=video, prompt_embeds=ctx, height=64, width=96, source_frames=9, reasoning_frames=4, num_inference_steps=STEPS,
                    guidance_scale=1.0, shift=SHIFT, repeat_rope=True, cot=True, generator=torch.Generator(device=DEV).manual_seed(7),
                    weight_dtype=torch.float32, output_type="uint8", return_dict=True, edit_mask=mask, **kw)
    whole, a = call(), call(edit_region=True, edit_region_margin=(0, 0))
    assert a.edit_region == (0, 16, 48, 48) and whole.edit_region is None      # rows [0, 6), columns [2, 8): the bounds on the patch grid
    for name in ("videos", "ground_videos", "edit_videos"):
        assert getattr(a, name).shape == getattr(whole, name).shape and getattr(a, name).dtype == np.uint8
    assert a.videos.shape == (1, 10, 64, 96, 3) and a.latents.shape == whole.latents.shape == (1, 16, 7, 8, 12)
    inside = torch.zeros(8, 12, dtype=torch.bool, device=DEV)
    inside[0:6, 2:8] = True
    assert torch.equal(bits(a.latents[:, :, :FS]), bits(pipe._encode_modes(video, torch.device(DEV), torch.float32)))   # the source, encoded whole
    assert torch.equal(bits(a.latents[:, :, FS + G:][..., ~inside]), bits(a.latents[:, :, :FS][..., ~inside]))   # outside: its bits
    assert not torch.equal(a.latents[:, :, FS + G:][..., inside], a.latents[:, :, :FS][..., inside])


def test_g_an_empty_mask_and_malformed_calls_raise(model, inputs):
    with pytest.raises(ValueError, match="edit_mask is empty"):
        _call(_pipe(model), inputs, edit_mask=np.zeros((9, 96, 128), np.uint8), edit_region=True)
    with pytest.raises(ValueError, match="no edit_mask"):
        _call(_pipe(model), inputs, edit_region=True)
    with pytest.raises(ValueError, match="edit_region_margin"):
        _call(_pipe(model), inputs, edit_mask=MASK, edit_region=True, edit_region_margin=(8, 16))
    with pytest.raises(NotImplementedError, match="capture_graph='loop'"):
        _call(_pipe(model), inputs, edit_mask=MASK, edit_region=True, capture_graph="loop")
