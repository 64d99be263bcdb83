"""-m gpu: edit region, the VAE on the box only (`edit_region_vae_halo`) -- wan_frames_u8_box_to_video / wan_video_box_stitch_u8 against
their definitions (bit for bit and byte for byte, with guard bands), and WanPipeline(edit_region=True, edit_region_vae_halo=16) against
the same pipeline without the switch on the clip cropped in pixels to the box (call B): the latents agree bit for bit, the frames are
call B's stitched into the source's bytes.  docs/TEST_BOUNDS.md, "Edit region: the VAE on the box"."""
import numpy as np
import pytest
import torch

from videocof_amd import (AutoencoderKLWan, FlowUniPCMultistepScheduler, RegionPlan, WanPipeline, WanTransformer3DModel, _lib,
                          latent_edit_mask, ops, reference_frames_box_to_video, reference_video_box_stitch, region_vae_box)
from videocof_amd.video_io import reference_frames_to_video, reference_video_to_frames
from videocof_amd.weights import deterministic_dit_state_dict, deterministic_vae_state_dict, det_uniform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
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


def _bytes(name, shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(sum(map(ord, name))), dtype=torch.uint8)


# (H, W, box (y, x, h, w), rectangle (y, x, h, w), guard elements).  The access unit in pixels follows W, the box's x origin and width
# and the bases: 16 at x 0 and 16 with widths 32 and 16; 8 at x 8, width 24; 4 at x 4, width 12; 2 at x 2, width 6; 1 at x 1, width 7;
# 1 through the bases alone behind a 3-element band.  The boxes touch every border of the frame between them, one touches none; the
# rectangles have 0 (the whole frame), 2 (a corner), 3 and 4 edges that are not the frame's border.
CASES = [(24, 32, (0, 0, 24, 32), (0, 0, 24, 32), 64),
         (24, 32, (8, 16, 16, 16), (10, 18, 14, 14), 64),
         (24, 40, (4, 8, 16, 24), (6, 10, 10, 19), 64),
         (24, 40, (0, 4, 12, 12), (0, 5, 9, 10), 64),
         (24, 40, (1, 2, 6, 6), (1, 2, 6, 6), 64),
         (24, 40, (2, 1, 9, 7), (3, 2, 6, 5), 64),
         (24, 32, (8, 16, 16, 16), (10, 18, 14, 14), 3),
         (24, 32, (0, 0, 13, 32), (0, 0, 13, 32), 64)]
T = 5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W,box,rect,pad", CASES)
def test_the_box_conversion_equals_its_definition(H, W, box, rect, pad, dtype):
    for B in (1, 2):
        frames = _bytes(f"in.{H}.{W}.{B}", (B, T, H, W, 3))
        frames[0, 0, box[0], box[1]] = torch.tensor([0, 255, 128], dtype=torch.uint8)
        src = Guarded(frames.shape, torch.uint8, pad, frames)
        for bx in (box, rect):
            want = reference_frames_box_to_video(frames, bx, dtype)
            out = Guarded(want.shape, dtype, pad)
            got = ops.frames_u8_box_to_video(src.view, bx, dtype, out=out.view)
            assert got.data_ptr() == out.view.data_ptr()
            assert torch.equal(bits(out.view.cpu()), bits(want)), (B, bx)
            assert out.intact() and src.intact()
        assert torch.equal(src.view.cpu(), frames)
        # the whole-frame box: the bits of the existing conversion, and of its definition
        whole = ops.frames_u8_box_to_video(src.view, (0, 0, H, W), dtype)
        assert torch.equal(bits(whole), bits(ops.frames_u8_to_video(src.view, dtype)))
        assert torch.equal(bits(whole.cpu()), bits(reference_frames_to_video(frames, dtype)))


def _decoder_samples(name, shape, dtype):
    """Decoder samples that exercise the clamp and the truncation: below -1, above 1, and exact multiples of 1 / 255 (as x = 2 k / 255 - 1
    rounds to them in float32), among values all over [-1.3, 1.3]."""
    v = det_uniform(name, shape, 1.3)
    flat = v.view(-1)
    k = torch.arange(flat.numel() // 3, dtype=torch.float32) % 256
    flat[::3][:k.numel()] = k * (2.0 / 255.0) - 1.0
    flat[1], flat[2], flat[4], flat[5] = -1.0, 1.0, -1.25, 1.25
    return v.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W,box,rect,pad", CASES)
def test_the_stitch_equals_its_definition(H, W, box, rect, pad, dtype):
    Tv, Ts, T_out, t0, nt, src_t0, t_dst = 4, 5, 6, 1, 2, 2, 3
    bh, bw = box[2], box[3]
    for B, Bs in ((1, 1), (2, 1), (2, 2)):
        source = _bytes(f"src.{H}.{W}.{Bs}", (Bs, Ts, H, W, 3))
        video = _decoder_samples(f"dec.{H}.{W}.{B}", (B, 3, Tv, bh, bw), dtype)
        edit = reference_video_to_frames(video[:, :, t0:t0 + nt])                      # the existing conversion's definition
        src, vid = Guarded(source.shape, torch.uint8, pad, source), Guarded(video.shape, dtype, pad, video)
        for feather in (0, 1, 3, max(rect[2], rect[3]) // 2 + 2):
            want = reference_video_box_stitch(source[:, src_t0:src_t0 + nt], edit, box, rect, feather)
            out = Guarded((B, T_out, H, W, 3), torch.uint8, pad)
            got = ops.video_box_stitch_u8(vid.view, src.view, box, rect, feather, out=out.view, frame_range=(t0, t0 + nt),
                                          dst_frame=t_dst, src_frame=src_t0)
            assert got.data_ptr() == out.view.data_ptr()
            res = out.view.cpu()
            assert torch.equal(res[:, t_dst:t_dst + nt], want), (B, Bs, feather)
            assert bool((res[:, :t_dst] == POISON).all()) and bool((res[:, t_dst + nt:] == POISON).all())      # the other frames: untouched
            assert out.intact() and src.intact() and vid.intact()
            # outside the rectangle: the source's bytes
            inside = torch.zeros(H, W, dtype=torch.bool)
            inside[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]] = True
            assert torch.equal(res[:, t_dst:t_dst + nt][:, :, ~inside], source[:, src_t0:src_t0 + nt].expand(B, -1, -1, -1, -1)[:, :, ~inside])
        assert torch.equal(src.view.cpu(), source) and torch.equal(bits(vid.view.cpu()), bits(video))
    # a rectangle that is the whole frame: the bytes of the existing conversion, whatever the feather
    video = _decoder_samples(f"dec.whole.{H}.{W}", (1, 3, 2, H, W), dtype).to(DEV)
    source = _bytes("src.whole", (1, 2, H, W, 3)).to(DEV)
    for feather in (0, 3):
        got = ops.video_box_stitch_u8(video, source, (0, 0, H, W), (0, 0, H, W), feather)
        assert torch.equal(got, ops.video_to_frames_u8(video))


def test_invalid_arguments_raise_and_launch_nothing():
    H, W, box, rect = 24, 32, (8, 16, 16, 16), (10, 18, 4, 4)
    frames = Guarded((1, 3, H, W, 3), torch.uint8)
    planes = Guarded((1, 3, 3, 16, 16), torch.float32)
    out = Guarded((1, 3, H, W, 3), torch.uint8)
    for bad in ((0, 0, 25, 32), (0, 0, 24, 33), (20, 0, 5, 8), (0, 30, 8, 4), (-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0)):
        with pytest.raises(ValueError, match="does not lie inside"):
            ops.frames_u8_box_to_video(frames.view, bad, torch.float32)
    with pytest.raises(ValueError, match="frames_u8_box_to_video.out"):
        ops.frames_u8_box_to_video(frames.view, box, torch.float32, out=planes.view[:, :, :2])
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        ops.frames_u8_box_to_video(frames.view, box, torch.float16)
    with pytest.raises(ValueError, match="uint8"):
        ops.frames_u8_box_to_video(planes.view, box, torch.float32)
    stitch = lambda **kw: ops.video_box_stitch_u8(planes.view, frames.view, **{**dict(box=box, rect=rect, feather=0, out=out.view), **kw})
    for bad in ((7, 18, 4, 4), (10, 15, 4, 4), (10, 18, 15, 4), (10, 18, 4, 15), (10, 18, 0, 4)):        # a rectangle not inside the box
        with pytest.raises(ValueError, match="does not lie inside the box"):
            stitch(rect=bad)
    for bad in ((9, 16, 16, 16), (8, 17, 16, 16), (-1, 16, 16, 16)):                                         # a box not inside the frame
        with pytest.raises(ValueError, match="does not lie inside a frame"):
            stitch(box=bad)
    with pytest.raises(ValueError, match="a box of"):
        stitch(box=(8, 16, 8, 16))
    with pytest.raises(ValueError, match="source frames"):                                                     # src_t0 + nt > Ts
        stitch(src_frame=1)
    with pytest.raises(ValueError, match="source frames"):
        stitch(src_frame=-1)
    with pytest.raises(ValueError, match="at offset"):                                                         # the destination range
        stitch(dst_frame=1)
    with pytest.raises(ValueError, match="at offset"):
        stitch(dst_frame=-1, frame_range=(0, 1))
    with pytest.raises(ValueError, match="frame_range"):
        stitch(frame_range=(2, 4))
    with pytest.raises(ValueError, match="feather"):
        stitch(feather=-1)
    with pytest.raises(ValueError, match="feather"):
        stitch(feather=1.5)
    with pytest.raises(ValueError, match="1 or B"):                                                            # Bs = 2 for B = 1
        ops.video_box_stitch_u8(planes.view, torch.zeros(2, 3, H, W, 3, device=DEV, dtype=torch.uint8), box, rect, out=out.view)
    lib, inv = _lib.load(), _lib.WAN_ERR_INVALID
    p = lambda g: g.view.data_ptr()
    assert lib.wan_frames_u8_box_to_video(None, p(planes), 0, 1, 3, H, W, 8, 16, 16, 16, None) == inv            # null pointers
    assert lib.wan_frames_u8_box_to_video(p(frames), None, 0, 1, 3, H, W, 8, 16, 16, 16, None) == inv
    assert lib.wan_frames_u8_box_to_video(p(frames), p(planes), 2, 1, 3, H, W, 8, 16, 16, 16, None) == inv       # no such dtype
    args = (1, 1, 3, 3, 3, H, W, 8, 16, 16, 16, 10, 18, 4, 4, 0, 0, 3, 0, 0)
    assert lib.wan_video_box_stitch_u8(None, 0, p(frames), p(out), *args, None) == inv
    assert lib.wan_video_box_stitch_u8(p(planes), 0, None, p(out), *args, None) == inv
    assert lib.wan_video_box_stitch_u8(p(planes), 0, p(frames), None, *args, None) == inv
    assert lib.wan_video_box_stitch_u8(p(planes), 2, p(frames), p(out), *args, None) == inv
    assert lib.wan_video_box_stitch_u8(p(planes), 0, p(frames), p(out), *(args[:17] + (4,) + args[18:]), None) == inv      # t0 + nt > T
    torch.cuda.synchronize()
    for g in (frames, planes, out):                                            # nothing was launched: every element is still the poison
        assert bool((g.buf == POISON).all())


# ------------------------------------------------------------------------------------------------ pipeline
TINY = dict(dim=256, ffn_dim=512, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)
STEPS, SHIFT, SEED = 3, 3.0, 7
G, FS, HL, WL = 1, 3, 12, 16           # source_frames=9 -> 3 latent frames; 96 x 128 pixels -> 12 x 16 cells
HP, WP = 96, 128
MASK = np.zeros((9, HP, WP), np.uint8)
MASK[:, 40:48, 56:64] = 255            # the cell (5, 7); grow 1 and feather 1 spread the weights over rows 3..7, columns 5..9
MARGIN = (16, 16)                      # 2 cells = edit_mask_grow + edit_mask_feather: call B's weights are call A's (asserted below)
HALO = 16                              # 2 cells
REGION = RegionPlan(0, 2, 10, 10)      # rows: [2, 8) and the margin = [0, 10); columns: [4, 10) and the margin = [2, 12)
BOX = RegionPlan(0, 0, 12, 14)         # the halo: rows clamped at the top, [0, 12); columns [0, 14), free on the right
TILES = dict(spatial_window=(32, 32), spatial_overlap=(16, 16))             # tiles of 4 x 4 cells: the region is larger
LATE = MASK.copy()
LATE[:5] = 0                           # pixel frames 5..8 = latent frame 2 only: with a time margin of 0 the loop runs on frames [1, 3)


@pytest.fixture(scope="module")
def sd():
    return deterministic_dit_state_dict(**TINY)


@pytest.fixture()
def model(sd):
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    m.load_state_dict(sd, device=DEV)
    return m


@pytest.fixture(scope="module")
def vae():
    v = AutoencoderKLWan()
    v.load_state_dict(deterministic_vae_state_dict(), device=DEV)
    return v


@pytest.fixture(scope="module")
def inputs():
    video = ((det_uniform("erv.video", (1, 9, HP, WP, 3), 0.5) + 0.5) * 255.0).clamp(0, 255).to(torch.uint8)
    return video, det_uniform("erv.ctx", (37, 64), 1.0).to(DEV), det_uniform("erv.neg", (9, 64), 1.0).to(DEV)


def _pipe(model, vae):
    return WanPipeline(vae=vae, transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))         # the deterministic sampler


def _call(pipe, inputs, mask=MASK, scale=1.0, **kw):
    video, ctx, neg = inputs
    kw = {**dict(video=video, height=HP, width=WP, generator=torch.Generator(device=DEV).manual_seed(SEED), cot=True), **kw}
    return pipe(prompt_embeds=[ctx], negative_prompt_embeds=[neg] if scale > 1 else None, source_frames=9, reasoning_frames=4,
                num_inference_steps=STEPS, guidance_scale=scale, shift=SHIFT, repeat_rope=True, output_type="uint8",
                weight_dtype=torch.float32, return_dict=True, edit_mask=mask, **kw)


def _call_a(pipe, inputs, feather=0, **kw):
    return _call(pipe, inputs, edit_region=True, edit_region_margin=MARGIN, edit_region_vae_halo=HALO, edit_region_stitch_feather=feather, **kw)


def _call_b(pipe, inputs, mask=MASK, noise_frames=FS + G, **kw):
    """Call B: the SAME pipeline without the new switch on the clip cropped in pixels to the box -- the mask cropped to the box, the box's
    height and width, latents = [vae.encode(box crop) | the box of call A's whole-frame noise], redrawn here from the same seed with the
    one _randn shape the pipeline draws."""
    y, x, h, w = BOX.pixels()
    dev = torch.device(DEV)
    crop = inputs[0][:, :, y:y + h, x:x + w].contiguous()
    source = pipe._encode_modes(crop, dev, torch.float32)
    noise = pipe._randn((1, 16, noise_frames, HL, WL), torch.Generator(device=DEV).manual_seed(SEED), dev, torch.float32)
    lat = torch.cat([source, noise[..., BOX.y0:BOX.y0 + BOX.h, BOX.x0:BOX.x0 + BOX.w]], dim=2)
    return _call(pipe, inputs, mask=np.ascontiguousarray(mask[:, y:y + h, x:x + w]), video=None, latents=lat, height=h, width=w,
                 generator=None, edit_region=True, edit_region_margin=MARGIN, **kw)


def _check_a_against_b(a, b, inputs, feather=0):
    video = inputs[0]
    rect, box = REGION.pixels(), BOX.pixels()
    assert a.edit_region == rect and a.edit_region_vae == box
    assert b.edit_region == (rect[0] - box[0], rect[1] - box[1], rect[2], rect[3]) and b.edit_region_vae is None     # A's, less the box's origin
    assert a.edit_region_time == b.edit_region_time
    assert a.latents.shape == b.latents.shape == (1, 16, 2 * FS + G, BOX.h, BOX.w)
    assert torch.equal(bits(a.latents), bits(b.latents))
    ng, ne = 1 + 4 * (G - 1), 9
    assert a.videos.shape == (1, ng + ne, HP, WP, 3) and a.videos.dtype == np.uint8 and b.videos.shape == (1, ng + ne, box[2], box[3], 3)
    want_edit = reference_video_box_stitch(video, torch.from_numpy(b.edit_videos), box, rect, feather)
    want_ground = reference_video_box_stitch(video[:, :ng], torch.from_numpy(b.ground_videos), box, rect, feather)
    assert torch.equal(torch.from_numpy(a.edit_videos), want_edit) and torch.equal(torch.from_numpy(a.ground_videos), want_ground)
    assert np.array_equal(a.videos, np.concatenate([a.ground_videos, a.edit_videos], axis=1))
    y, x, h, w = rect
    inside = np.zeros((HP, WP), bool)
    inside[y:y + h, x:x + w] = True
    assert np.array_equal(a.edit_videos[:, :, ~inside], video.numpy()[:, :, ~inside])          # outside the rectangle: the input's bytes
    assert np.array_equal(a.ground_videos[:, :, ~inside], video.numpy()[:, :ng][:, :, ~inside])
    assert not np.array_equal(a.edit_videos[:, :, inside], video.numpy()[:, :, inside])         # inside: the loop and the decode did run


def test_cropping_the_pixel_mask_to_the_box_and_cropping_the_weights_agree():
    """The margin is grow + feather cells, so the region's border is further from every marked cell than the dilation and the feather
    reach, and the feather clamps at borders: call B's weights, made of the mask cropped to the box, are call A's on the region."""
    y, x, h, w = BOX.pixels()
    inner = RegionPlan(REGION.y0 - BOX.y0, REGION.x0 - BOX.x0, REGION.h, REGION.w)
    assert region_vae_box(REGION, (HL, WL), (HALO // 8, HALO // 8)) == BOX
    for mask in (MASK, LATE):
        a = ops.region_crop(latent_edit_mask(mask)[None], REGION)
        assert torch.equal(a, ops.region_crop(latent_edit_mask(np.ascontiguousarray(mask[:, y:y + h, x:x + w]))[None], inner))


def _differ(x, y):
    return x.shape == y.shape and not np.array_equal(x, y)


def test_a_the_box_equals_the_cropped_call(model, vae, inputs):
    """The decisive case: without the feature the call does not exist.  Feather 0 and 4 against the one call B."""
    b = _call_b(_pipe(model, vae), inputs)
    a = {feather: _call_a(_pipe(model, vae), inputs, feather) for feather in (0, 4)}
    for feather in (0, 4):
        _check_a_against_b(a[feather], b, inputs, feather)
    assert _differ(a[0].edit_videos, a[4].edit_videos)


def test_b_the_time_axis_cropped_in_the_loop_and_whole_in_the_vae(model, vae, inputs):
    a = _call_a(_pipe(model, vae), inputs, mask=LATE, edit_region_time_margin=0)
    b = _call_b(_pipe(model, vae), inputs, mask=LATE, edit_region_time_margin=0)
    assert a.edit_region_time == (1, 8)                                        # latent frames [1, 3) = pixel frames 1..8
    _check_a_against_b(a, b, inputs)
    assert _differ(a.edit_videos, _call_a(_pipe(model, vae), inputs, mask=LATE).edit_videos)        # the time crop did happen


def test_c_with_guidance(model, vae, inputs):
    a = _call_a(_pipe(model, vae), inputs, scale=3.0)
    _check_a_against_b(a, _call_b(_pipe(model, vae), inputs, scale=3.0), inputs)
    assert _differ(a.edit_videos, _call_a(_pipe(model, vae), inputs).edit_videos)


def test_d_spatial_window_tiles_inside_the_region(model, vae, inputs):
    a = _call_a(_pipe(model, vae), inputs, **TILES)
    _check_a_against_b(a, _call_b(_pipe(model, vae), inputs, **TILES), inputs)
    assert _differ(a.edit_videos, _call_a(_pipe(model, vae), inputs).edit_videos)         # the tiles did run


def test_e_the_compare_clip_is_composed_from_the_stitched_frames(model, vae, inputs):
    from videocof_amd import reference_compare_frames
    a = _call_a(_pipe(model, vae), inputs, feather=4, compare=True)
    plain = _call(_pipe(model, vae), inputs, edit_region=True, edit_region_margin=MARGIN, compare=True)
    assert a.compare_videos.shape == plain.compare_videos.shape == (1, 9, HP, 2 * WP, 3)
    assert np.array_equal(a.compare_videos[:, :, :, :WP], plain.compare_videos[:, :, :, :WP])                # the left half: unchanged
    assert np.array_equal(a.compare_videos[:, :, :, WP:], a.edit_videos)                                     # the right half: the stitched edit
    assert torch.equal(torch.from_numpy(a.compare_videos), reference_compare_frames(inputs[0], torch.from_numpy(a.edit_videos)))
    assert np.array_equal(a.edit_videos, _call_a(_pipe(model, vae), inputs, feather=4).edit_videos)


def test_f_a_region_that_is_the_whole_frame_changes_nothing(model, vae, inputs):
    full = np.full((9, HP, WP), 255, np.uint8)
    plain = _call(_pipe(model, vae), inputs, mask=full, edit_region=True)
    a = _call(_pipe(model, vae), inputs, mask=full, edit_region=True, edit_region_vae_halo=HALO, edit_region_stitch_feather=3)
    assert a.edit_region == a.edit_region_vae == (0, 0, HP, WP) and plain.edit_region_vae is None
    assert torch.equal(bits(a.latents), bits(plain.latents))
    for name in ("videos", "ground_videos", "edit_videos"):
        assert np.array_equal(getattr(a, name), getattr(plain, name)), name


def test_g_the_switch_off_is_the_call_that_never_mentions_it(model, vae, inputs):
    never = _call(_pipe(model, vae), inputs, edit_region=True, edit_region_margin=MARGIN)
    off = _call(_pipe(model, vae), inputs, edit_region=True, edit_region_margin=MARGIN, edit_region_vae_halo=None, edit_region_stitch_feather=0)
    assert off.edit_region_vae is None and off.edit_region == never.edit_region == REGION.pixels()
    assert off.latents.shape == (1, 16, 2 * FS + G, HL, WL) and torch.equal(bits(off.latents), bits(never.latents))
    for name in ("videos", "ground_videos", "edit_videos"):
        assert np.array_equal(getattr(off, name), getattr(never, name)), name
    # and with the switch the frames differ from it inside the rectangle only: the VAE saw the box, not the frame
    a = _call_a(_pipe(model, vae), inputs)
    y, x, h, w = REGION.pixels()
    assert _differ(a.edit_videos[:, :, y:y + h, x:x + w], never.edit_videos[:, :, y:y + h, x:x + w])


def test_h_without_the_grounding_segment(model, vae, inputs):
    """cot=False: [source | target], no grounding frames -- the one segment is decoded and stitched into one clip of its own."""
    a = _call_a(_pipe(model, vae), inputs, feather=1, cot=False)
    b = _call_b(_pipe(model, vae), inputs, cot=False, noise_frames=FS)
    assert a.edit_region == REGION.pixels() and a.edit_region_vae == BOX.pixels() and a.ground_videos is None
    assert a.latents.shape == (1, 16, 2 * FS, BOX.h, BOX.w) and torch.equal(bits(a.latents), bits(b.latents))
    want = reference_video_box_stitch(inputs[0], torch.from_numpy(b.edit_videos), BOX.pixels(), REGION.pixels(), 1)
    assert a.videos.shape == (1, 9, HP, WP, 3) and torch.equal(torch.from_numpy(a.edit_videos), want) and a.videos is a.edit_videos
