"""Edit region, the VAE on the box only, on the CPU: the box rule swept over every bounding box of a small frame (inside the frame, around
the region, on the patch grid, and the shift identity that makes the feature testable bit for bit), the definitions of the two device
passes against the existing conversions' definitions, the ramp, the switches' checks (before any device work) and the entry points'
argument errors.  docs/TEST_BOUNDS.md, "Edit region: the VAE on the box"."""
import itertools
import os

import numpy as np
import pytest
import torch

from videocof_amd import (FlowUniPCMultistepScheduler, RegionPlan, WanPipeline, WanPipelineOutput, _lib, ops,
                          reference_frames_box_to_video, reference_video_box_stitch, region_plan, region_vae_box)
from videocof_amd.edit_region import region_stitch_feather, region_vae_halo_cells, stitch_weights
from videocof_amd.video_io import reference_frames_to_video, reference_video_to_frames

H, W, P = 12, 16, 2


# ------------------------------------------------------------------------------------------------ the rule
def test_the_box_of_every_bounding_box():
    """Every inclusive bounding box of a 12 x 16-cell frame, tile in {None, (6, 8)}, margin in {0, 2}, halo in {0, 2, 4} cells."""
    n = 0
    for tile, m in itertools.product((None, (6, 8)), (0, 2)):
        for y_lo, x_lo in itertools.product(range(H), range(W)):
            for y_hi, x_hi in itertools.product(range(y_lo, H), range(x_lo, W)):
                bounds = (y_lo, y_hi, x_lo, x_hi)
                r = region_plan(bounds, (H, W), (m, m), tile, P)
                for hc in (0, 2, 4):
                    b = region_vae_box(r, (H, W), (hc, hc))
                    n += 1
                    # inside the frame, around the region, on the patch grid
                    assert 0 <= b.y0 and b.y0 + b.h <= H and 0 <= b.x0 and b.x0 + b.w <= W, (bounds, r, b)
                    assert b.y0 <= r.y0 and r.y0 + r.h <= b.y0 + b.h and b.x0 <= r.x0 and r.x0 + r.w <= b.x0 + b.w, (bounds, r, b)
                    assert all(v % P == 0 for v in b), (bounds, r, b)
                    # the halo on every side, clamped at the borders
                    assert b.y0 == max(0, r.y0 - hc) and b.y0 + b.h == min(H, r.y0 + r.h + hc), (bounds, r, b)
                    assert b.x0 == max(0, r.x0 - hc) and b.x0 + b.w == min(W, r.x0 + r.w + hc), (bounds, r, b)
                    # the shift identity: the region planned inside the box is the region less the box's origin
                    inner = region_plan((y_lo - b.y0, y_hi - b.y0, x_lo - b.x0, x_hi - b.x0), (b.h, b.w), (m, m), tile, P)
                    assert inner == RegionPlan(r.y0 - b.y0, r.x0 - b.x0, r.h, r.w), (bounds, tile, m, hc, r, b, inner)
    assert n == 2 * 2 * 3 * (H * (H + 1) // 2) * (W * (W + 1) // 2)


def test_the_box_of_a_frame_off_the_patch_grid_and_of_unequal_halos():
    # 135 x 240 cells (1080 x 1920 pixels): the rule holds, the box need not lie on the patch grid
    assert region_vae_box(RegionPlan(75, 0, 60, 104), (135, 240), (4, 4)) == RegionPlan(71, 0, 64, 108)
    assert region_vae_box(RegionPlan(33, 64, 60, 104), (135, 240), (4, 4)).pixels() == (232, 480, 544, 896)
    assert region_vae_box(RegionPlan(2, 4, 4, 6), (H, W), (2, 6)) == RegionPlan(0, 0, 8, 16)
    assert region_vae_box(RegionPlan(0, 0, H, W), (H, W), (4, 4)) == RegionPlan(0, 0, H, W)
    assert region_vae_box(RegionPlan(2, 4, 4, 6), (H, W), (0, 0)) == RegionPlan(2, 4, 4, 6)
    for bad in ((2, 4, 4), (11, 4, 2, 2), (2, 15, 2, 2), (-1, 0, 2, 2), (0, 0, 0, 2)):
        with pytest.raises(ValueError, match="region"):
            region_vae_box(bad, (H, W), (2, 2))
    for frame, halo in (((H,), (2, 2)), ((H, W), (2,)), ((H, W), (-2, 2)), ((H, W), (True, 2)), ((0, W), (2, 2)), ((H, W), 2)):
        with pytest.raises(ValueError, match="cells"):
            region_vae_box((2, 4, 4, 6), frame, halo)


def test_the_switch_values():
    assert [region_vae_halo_cells(v) for v in (0, 16, 32, np.int64(48))] == [0, 2, 4, 6]
    for bad in (True, False, 16.0, "16", (16, 16), -16, 8, 24, 1):
        with pytest.raises(ValueError, match="edit_region_vae_halo"):
            region_vae_halo_cells(bad)
    assert [region_stitch_feather(v) for v in (0, 1, np.int32(7))] == [0, 1, 7]
    for bad in (True, False, 1.0, "1", (1,), -1, None):
        with pytest.raises(ValueError, match="edit_region_stitch_feather"):
            region_stitch_feather(bad)


# ------------------------------------------------------------------------------------------------ the definitions
def _bytes(seed, shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_box_conversion_extends_the_existing_definition(dtype):
    frames = _bytes(1, (2, 3, 10, 14, 3))
    whole = reference_frames_box_to_video(frames, (0, 0, 10, 14), dtype)
    assert whole.dtype == dtype and torch.equal(whole, reference_frames_to_video(frames, dtype))
    for box in ((0, 0, 4, 5), (3, 2, 7, 12), (9, 13, 1, 1), (1, 1, 8, 7)):
        y, x, h, w = box
        got = reference_frames_box_to_video(frames, box, dtype)
        assert got.shape == (2, 3, 3, h, w) and got.is_contiguous()
        assert torch.equal(got, whole[:, :, :, y:y + h, x:x + w])              # element-wise: the crop of the whole conversion
    for bad in ((0, 0, 11, 14), (0, 0, 10, 15), (-1, 0, 2, 2), (0, 13, 2, 2), (0, 0, 0, 2), (0, 0, 2)):
        with pytest.raises(ValueError, match="box"):
            reference_frames_box_to_video(frames, bad, dtype)
    with pytest.raises(ValueError, match="uint8"):
        reference_frames_box_to_video(frames.float(), (0, 0, 2, 2), dtype)


def test_the_ramp():
    Hf, Wf = 20, 30
    # a is monotone in d, 255 from d = f on, and never 0 inside the rectangle
    for f in (1, 2, 3, 7, 50):
        a = [255 if d >= f else (255 * (d + 1)) // (f + 1) for d in range(60)]
        assert all(a[i] <= a[i + 1] for i in range(59)) and a[0] >= 1 and all(v == 255 for v in a[f:]) and a[f - 1] < 255
        w = stitch_weights((Hf, Wf), (4, 6, 12, 18), f)                         # four interior edges
        for y, x in itertools.product(range(12), range(18)):
            d = min(y, 11 - y, x, 17 - x)
            assert w[y, x] == a[d], (f, y, x)
    assert (stitch_weights((Hf, Wf), (4, 6, 12, 18), 0) == 255).all()           # feather 0: the literal stitch
    # edges on the frame's border do not ramp
    assert (stitch_weights((Hf, Wf), (0, 0, Hf, Wf), 5) == 255).all()           # the whole frame: no edge ramps
    w = stitch_weights((Hf, Wf), (0, 0, 12, 18), 3)                             # the top-left corner: only bottom and right ramp
    assert (w[:9, :15] == 255).all() and w[11, 0] == 255 // 4 and w[0, 17] == 255 // 4 and w[10, 0] == 255 * 2 // 4 and w[0, 0] == 255
    w = stitch_weights((Hf, Wf), (8, 0, 12, Wf), 3)                             # a band at the bottom: only the top ramps
    assert (w[3:] == 255).all() and [int(v) for v in w[:3, 5]] == [63, 127, 191] and (w[:3] == w[:3, :1]).all()
    with pytest.raises(ValueError, match="feather"):
        stitch_weights((Hf, Wf), (0, 0, 2, 2), -1)
    with pytest.raises(ValueError, match="rectangle"):
        stitch_weights((Hf, Wf), (0, 0, 21, 2), 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_the_stitch_extends_the_existing_definitions(dtype):
    Hf, Wf = 10, 14
    source = _bytes(2, (1, 3, Hf, Wf, 3))
    video = (torch.rand((2, 3, 3, Hf, Wf), generator=torch.Generator().manual_seed(3)) * 2.6 - 1.3).to(dtype)
    edit = reference_video_to_frames(video)
    # feather 0 (and any feather) with a whole-frame rectangle: the existing byte conversion
    for f in (0, 4):
        assert torch.equal(reference_video_box_stitch(source, edit, (0, 0, Hf, Wf), (0, 0, Hf, Wf), f), edit)
    # feather 0: the edit's bytes inside the rectangle, the source's outside it -- whatever the box shows beyond the rectangle
    box, rect = (2, 2, 7, 10), (3, 4, 5, 6)
    got = reference_video_box_stitch(source, edit[:, :, 2:9, 2:12].contiguous(), box, rect, 0)
    want = source.expand(2, -1, -1, -1, -1).clone()
    want[:, :, 3:8, 4:10] = edit[:, :, 3:8, 4:10]
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    # with a feather: the composite's formula under the ramp's weights, the source outside
    got = reference_video_box_stitch(source, edit[:, :, 2:9, 2:12].contiguous(), box, rect, 2)
    a = torch.from_numpy(stitch_weights((Hf, Wf), rect, 2))[None, None, :, :, None]
    e, o = edit[:, :, 3:8, 4:10].long(), source[:, :, 3:8, 4:10].long()
    want = source.expand(2, -1, -1, -1, -1).clone()
    want[:, :, 3:8, 4:10] = ((a * e + (255 - a) * o + 127) // 255).to(torch.uint8)
    assert torch.equal(got, want) and not torch.equal(got[:, :, 3:8, 4:10], edit[:, :, 3:8, 4:10])
    assert torch.equal(got[:, :, 5, 6], edit[:, :, 5, 6])                      # d = 2 >= f: the edit's byte
    for bad_box, bad_rect in (((2, 2, 7, 10), (1, 4, 5, 6)), ((2, 2, 7, 10), (3, 4, 7, 6)), ((2, 2, 7, 10), (3, 4, 5, 9)),
                              ((2, 2, 9, 10), (3, 4, 5, 6)), ((2, 2, 7, 13), (3, 4, 5, 6)), ((2, 2, 6, 10), (3, 4, 5, 6))):
        with pytest.raises(ValueError, match="box|rectangle"):
            reference_video_box_stitch(source, edit[:, :, 2:9, 2:12].contiguous(), bad_box, bad_rect, 0)


# ------------------------------------------------------------------------------------------------ the switches
def test_the_pipeline_checks_the_switches_before_any_device_work():
    """A pipeline whose transformer and VAE are bare objects (any use of them is an AttributeError) gets to every refusal."""
    pipe = WanPipeline(vae=object(), transformer=object(), scheduler=FlowUniPCMultistepScheduler(shift=1))
    video = np.zeros((9, 32, 32, 3), np.uint8)
    ok = np.full((9, 32, 32), 255, np.uint8)
    kw = dict(video=video, source_frames=9, height=32, width=32, cot=True, output_type="uint8", edit_mask=ok)
    for bad in (True, False, 16.0, "16", (16, 16), -16, 8, 24):
        with pytest.raises(ValueError, match="edit_region_vae_halo"):
            pipe(edit_region=True, edit_region_vae_halo=bad, **kw)
    with pytest.raises(ValueError, match="edit_region_vae_halo"):
        pipe(edit_region_vae_halo=16, **kw)                                    # without edit_region=True
    for output_type in ("numpy", "latent"):
        with pytest.raises(ValueError, match="edit_region_vae_halo.*output_type"):
            pipe(edit_region=True, edit_region_vae_halo=16, **{**kw, "output_type": output_type})
    for bad_video in (torch.zeros(1, 3, 9, 32, 32), np.zeros((9, 32, 32, 3), np.float32), np.zeros((9, 32, 32), np.uint8)):
        with pytest.raises(ValueError, match="edit_region_vae_halo.*uint8"):
            pipe(edit_region=True, edit_region_vae_halo=16, **{**kw, "video": bad_video})
    with pytest.raises(ValueError, match="edit_region_vae_halo"):
        pipe(edit_region=True, edit_region_vae_halo=16, **{**kw, "video": None, "latents": torch.zeros(1, 16, 7, 4, 4)})
    for given in ("latents", "source_latents"):
        with pytest.raises(ValueError, match="edit_region_vae_halo.*latents"):
            pipe(edit_region=True, edit_region_vae_halo=16, **{**kw, given: torch.zeros(1, 16, 7 if given == "latents" else 3, 4, 4)})
    with pytest.raises(ValueError, match="edit_region_vae_halo.*source_frames, height, width"):
        pipe(edit_region=True, edit_region_vae_halo=16, **{**kw, "video": np.zeros((9, 32, 40, 3), np.uint8)})
    no_vae = WanPipeline(transformer=object(), scheduler=FlowUniPCMultistepScheduler(shift=1))
    with pytest.raises(ValueError, match="edit_region_vae_halo.*VAE"):
        no_vae(edit_region=True, edit_region_vae_halo=16, **kw)
    for bad in (True, False, 1.0, "1", (1,), -1, None):
        with pytest.raises(ValueError, match="edit_region_stitch_feather"):
            pipe(edit_region=True, edit_region_vae_halo=16, edit_region_stitch_feather=bad, **kw)
    with pytest.raises(ValueError, match="edit_region_stitch_feather"):
        pipe(edit_region=True, edit_region_stitch_feather=2, **kw)             # a feather without the halo
    with pytest.raises(NotImplementedError, match="capture_graph='loop'"):
        pipe(edit_region=True, edit_region_vae_halo=16, capture_graph="loop", **kw)
    with pytest.raises(TypeError, match="edit_region_vae_halos"):
        pipe(edit_region=True, edit_region_vae_halos=16, **kw)
    for halo, feather in ((0, 0), (16, 3), (np.int64(32), np.int32(1)), (None, 0)):
        with pytest.raises(ValueError, match="Provide either `prompt`"):       # good values get past the switches, to the next check
            pipe(edit_region=True, edit_region_vae_halo=halo, edit_region_stitch_feather=feather, **kw)
    assert WanPipelineOutput(videos=None).edit_region_vae is None


def test_cpu_tensors_raise_in_the_wrappers():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frames_u8_box_to_video(torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8), (0, 0, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.video_box_stitch_u8(torch.zeros(1, 3, 2, 4, 4), torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8), (0, 0, 4, 4), (0, 0, 2, 2))


# ------------------------------------------------------------------------------------------------ the entry points, without a GPU
def test_entry_points_refuse_bad_arguments_before_launching():
    lib, inv = _lib.load(), _lib.WAN_ERR_INVALID
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "wan_hip.h")).read()
    for sym in ("wan_frames_u8_box_to_video", "wan_video_box_stitch_u8"):
        assert sym in _lib.SIGNATURES and f"{sym}(" in header
    assert _lib.ABI_VERSION == 11                                     # additions only

    conv = lambda *a: lib.wan_frames_u8_box_to_video(*a, None)
    good = (8, 8, 0, 1, 3, 24, 32, 8, 16, 16, 16)                     # frames, out, out_dtype, B, T, H, W, by, bx, bh, bw
    for k in (0, 1):
        assert conv(*good[:k], None, *good[k + 1:]) == inv
    with pytest.raises(ValueError, match="wan_frames_u8_box_to_video: null tensor"):
        _lib.check(inv, "wan_frames_u8_box_to_video")
    assert conv(*good[:2], 2, *good[3:]) == inv
    for k in (3, 4, 5, 6):
        assert conv(*good[:k], 0, *good[k + 1:]) == inv
    for box in ((-1, 16, 16, 16), (8, -1, 16, 16), (9, 16, 16, 16), (8, 17, 16, 16), (8, 16, 0, 16), (8, 16, 16, 0),
                (1 << 30, 0, 1 << 30, 1), (0, (1 << 31) - 1, 1, (1 << 31) - 1)):
        assert conv(*good[:7], *box) == inv, box
    with pytest.raises(ValueError, match="does not lie inside a frame"):
        _lib.check(inv, "wan_frames_u8_box_to_video")
    assert conv(8, 8, 0, 1 << 16, 1 << 16, 24, 32, 8, 16, 16, 16) == inv            # 2^32 frames
    assert conv(8, 8, 0, 1, 1, 1 << 15, 1 << 15, 0, 0, 16, 16) == inv               # 3 * 2^30 bytes a frame

    st = lambda *a: lib.wan_video_box_stitch_u8(*a, None)
    # video, in_dtype, source, frames, B, Bs, T, Ts, T_out, H, W, by, bx, bh, bw, ry, rx, rh, rw, feather, t0, nt, src_t0, t_dst
    good = (8, 0, 8, 8, 2, 1, 4, 5, 6, 24, 32, 8, 16, 16, 16, 10, 18, 4, 4, 0, 1, 2, 2, 3)
    sub = lambda k, v: good[:k] + (v,) + good[k + 1:]
    for k in (0, 2, 3):
        assert st(*sub(k, None)) == inv
    with pytest.raises(ValueError, match="wan_video_box_stitch_u8: null tensor"):
        _lib.check(inv, "wan_video_box_stitch_u8")
    assert st(*sub(1, 2)) == inv and st(*sub(1, -1)) == inv
    for k in (4, 6, 7, 8, 9, 10):
        assert st(*sub(k, 0)) == inv, k
    for bs in (0, 3):
        assert st(*sub(5, bs)) == inv
    with pytest.raises(ValueError, match="1 or B"):
        _lib.check(inv, "wan_video_box_stitch_u8")
    for box in ((-1, 16, 16, 16), (9, 16, 16, 16), (8, 17, 16, 16), (8, 16, 0, 16)):
        assert st(*good[:11], *box, *good[15:]) == inv, box
    with pytest.raises(ValueError, match="does not lie inside a frame"):
        _lib.check(inv, "wan_video_box_stitch_u8")
    for rect in ((7, 18, 4, 4), (10, 15, 4, 4), (10, 18, 15, 4), (10, 18, 4, 15), (10, 18, 0, 4), (10, 18, 4, 0)):
        assert st(*good[:15], *rect, *good[19:]) == inv, rect
    with pytest.raises(ValueError, match="does not lie inside the box"):
        _lib.check(inv, "wan_video_box_stitch_u8")
    assert st(*sub(19, -1)) == inv
    with pytest.raises(ValueError, match="feather=-1"):
        _lib.check(inv, "wan_video_box_stitch_u8")
    assert st(*sub(20, -1)) == inv and st(*sub(20, 3)) == inv and st(*sub(21, -1)) == inv      # decoder frames [t0, t0 + nt) of T = 4
    assert st(*sub(22, -1)) == inv and st(*sub(22, 4)) == inv                                  # src_t0 + nt > Ts = 5
    with pytest.raises(ValueError, match="source frames"):
        _lib.check(inv, "wan_video_box_stitch_u8")
    assert st(*sub(23, -1)) == inv and st(*sub(23, 5)) == inv                                  # the destination range in T_out = 6
    with pytest.raises(ValueError, match="at offset"):
        _lib.check(inv, "wan_video_box_stitch_u8")
