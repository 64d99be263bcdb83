"""Edit region on the CPU: the region rule swept over every bounding box of a small frame, the torch definitions of the three device
passes, the switches' checks (before any device work) and the entry points' argument errors.  docs/TEST_BOUNDS.md, "Edit region"."""
import itertools
import os

import numpy as np
import pytest
import torch

from videocof_amd import (FlowUniPCMultistepScheduler, RegionPlan, WanPipeline, WanPipelineOutput, _lib, ops, reference_mask_bounds,
                          reference_region_crop, reference_region_restore, region_margin_cells, region_plan)

H, W, P = 12, 16, 2


# ------------------------------------------------------------------------------------------------ the rule
def _expected_axis(lo, hi, F, m, T, p):
    """The issue's statement of one axis, written out once more: (start, size, want, lo', hi')."""
    lo_a, hi_a = lo // p * p, (hi // p + 1) * p
    want = min(F, hi_a - lo_a + 2 * m)
    size = min(T, F) if T is not None and want <= T else want
    start = lo_a - m - ((size - want) // (2 * p)) * p
    return min(max(start, 0), F - size), size, want, lo_a, hi_a


@pytest.mark.parametrize("tile", [None, (6, 8)])
@pytest.mark.parametrize("margin", [0, 2])
def test_every_bounding_box_of_a_small_frame(tile, margin):
    boxes = 0
    for y_lo, y_hi in itertools.combinations_with_replacement(range(H), 2):
        for x_lo, x_hi in itertools.combinations_with_replacement(range(W), 2):
            r = region_plan((y_lo, y_hi, x_lo, x_hi), (H, W), (margin, margin), tile, P)
            assert isinstance(r, RegionPlan)
            for (start, size), (lo, hi), F, T in (((r.y0, r.h), (y_lo, y_hi), H, tile and tile[0]), ((r.x0, r.w), (x_lo, x_hi), W, tile and tile[1])):
                want_start, want_size, want, lo_a, hi_a = _expected_axis(lo, hi, F, margin, T, P)
                assert (start, size) == (want_start, want_size)                                        # the stated formula
                assert size % P == 0 and start % P == 0 and size >= P                                  # multiples of the patch, on its grid
                assert 0 <= start and start + size <= F                                                # inside the frame
                assert start <= max(lo_a - margin, 0) and start + size >= min(hi_a + margin, F)        # the clipped, margined box
                assert start <= lo and hi < start + size
                if T is not None and want <= T:
                    assert size == min(T, F)                                                           # one tile exactly when want <= T
                else:
                    assert size == want and (T is None or size > T)
            boxes += 1
    assert boxes == (H * (H + 1) // 2) * (W * (W + 1) // 2)


def test_borders_corners_and_the_whole_frame():
    plan = lambda b, m=(2, 2), t=(6, 8): region_plan(b, (H, W), m, t, P)
    assert plan((0, 0, 0, 0)) == (0, 0, 6, 8)                      # the corners: one tile, pushed inside
    assert plan((0, 0, 15, 15)) == (0, 8, 6, 8)
    assert plan((11, 11, 0, 0)) == (6, 0, 6, 8)
    assert plan((11, 11, 15, 15)) == (6, 8, 6, 8)
    assert plan((0, 0, 7, 8)) == (0, 4, 6, 8)                      # the top border: columns [6, 10) and the margin are the 8 of a tile
    assert plan((11, 11, 6, 7)) == (6, 4, 6, 8)                    # the bottom border: want = 6 columns from 4, (8 - 6) // 4 * 2 = 0 to the left
    assert plan((5, 6, 0, 0)) == (2, 0, 8, 8)                      # the left border: rows [4, 8) and the margin are 8 > 6: larger than a tile
    assert plan((5, 6, 15, 15)) == (2, 8, 8, 8)                    # the right border
    assert plan((0, 11, 0, 15)) == (0, 0, 12, 16)                  # the whole frame
    assert plan((0, 11, 0, 15), t=None) == (0, 0, 12, 16)
    assert plan((5, 5, 7, 7), m=(0, 0), t=None) == (4, 6, 2, 2)    # a single cell, no margin, no tile: its patch
    assert plan((5, 5, 7, 7), m=(0, 0)) == (2, 4, 6, 8)            # ... with a tile: centred on the grid, (6 - 2) // 4 * 2 = 2 rows above
    assert plan((5, 5, 7, 7), m=(2, 4), t=None) == (2, 2, 6, 10)
    # per-frame bounds as wan_mask_bounds returns them: the union, the empty frames' sentinels dropped
    per_frame = torch.tensor([[H, -1, W, -1], [4, 5, 6, 7], [2, 3, 10, 11], [H, -1, W, -1]], dtype=torch.int32)
    assert plan(per_frame, m=(0, 0), t=None) == plan((2, 5, 6, 11), m=(0, 0), t=None) == (2, 6, 4, 6)
    assert RegionPlan(2, 6, 4, 6).pixels() == (16, 48, 32, 48)


def test_a_frame_that_is_no_multiple_of_the_patch_runs_as_tiles():
    """135 x 240 cells (1080 x 1920 pixels) with a 60 x 104 tile: a small box gets one tile, inside the frame."""
    r = region_plan((100, 110, 20, 40), (135, 240), (8, 8), (60, 104), P)
    assert (r.h, r.w) == (60, 104) and 0 <= r.y0 <= 135 - 60 and r.y0 <= 100 - 8 and r.y0 + 60 >= 112 + 8 and r.x0 <= 12 and r.x0 + 104 >= 50
    r = region_plan((130, 134, 0, 3), (135, 240), (8, 8), (60, 104), P)
    assert r == (75, 0, 60, 104)


def test_bad_plans_raise():
    with pytest.raises(ValueError, match="edit_mask is empty"):
        region_plan((H, -1, W, -1), (H, W), (2, 2), None, P)
    with pytest.raises(ValueError, match="edit_mask is empty"):
        region_plan(np.array([[H, -1, W, -1]] * 3), (H, W), (2, 2), (6, 8), P)
    with pytest.raises(ValueError, match="margin_cells"):
        region_plan((0, 1, 0, 1), (H, W), (1, 2), None, P)
    with pytest.raises(ValueError, match="margin_cells"):
        region_plan((0, 1, 0, 1), (H, W), (-2, 2), None, P)
    with pytest.raises(ValueError, match="tile_cells"):
        region_plan((0, 1, 0, 1), (H, W), (2, 2), (5, 8), P)
    with pytest.raises(ValueError, match="frame_cells"):
        region_plan((0, 1, 0, 1), (H,), (2, 2), None, P)
    with pytest.raises(ValueError, match="leave a frame"):
        region_plan((0, H, 0, 1), (H, W), (2, 2), None, P)
    assert region_margin_cells((64, 0)) == (8, 0) and region_margin_cells((16, 160)) == (2, 20)
    for bad in ((8, 16), (16, -16), (16.0, 16), (True, 16), 16, (16, 16, 16)):
        with pytest.raises(ValueError, match="edit_region_margin"):
            region_margin_cells(bad)


# ------------------------------------------------------------------------------------------------ the definitions
def test_bounds_of_a_known_mask():
    w = torch.zeros(2, 4, 5, 7, dtype=torch.uint8)
    w[0, 0, 1, 2], w[1, 0, 3, 6] = 1, 255              # frame 0: two samples, two corners of its box
    w[1, 2, 4, 0] = 7                                  # frame 2: one cell, the second sample only; frames 1 and 3: empty
    assert reference_mask_bounds(w).tolist() == [[1, 3, 2, 6], [5, -1, 7, -1], [4, 4, 0, 0], [5, -1, 7, -1]]
    assert reference_mask_bounds(w).dtype == torch.int32
    assert reference_mask_bounds(torch.full((1, 1, 3, 4), 9, dtype=torch.uint8)).tolist() == [[0, 2, 0, 3]]
    with pytest.raises(ValueError, match="uint8"):
        reference_mask_bounds(w.float())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("G", [0, 1, 2])
def test_restore_of_a_crop_pins_the_outside_to_the_source(dtype, G):
    B, C, cc, h, w = 2, 3, 2, 6, 8
    gen = torch.Generator().manual_seed(G)
    state = torch.randn(B, C, 2 * cc + G, h, w, generator=gen).to(dtype)
    for region in ((0, 0, 2, 2), (4, 6, 2, 2), (2, 2, 4, 4), (0, 0, h, w), (3, 5, 1, 1)):
        y0, x0, hr, wr = region
        crop = reference_region_crop(state, region)
        assert crop.shape == (B, C, 2 * cc + G, hr, wr) and crop.is_contiguous()
        assert torch.equal(crop, state[..., y0:y0 + hr, x0:x0 + wr])
        out = reference_region_restore(state[:, :, :cc], crop, (y0, x0))
        assert out.shape == state.shape and out.dtype == dtype
        inside = torch.zeros(h, w, dtype=torch.bool)
        inside[y0:y0 + hr, x0:x0 + wr] = True
        assert torch.equal(out[:, :, :cc], state[:, :, :cc])                                              # source frames: the source
        assert torch.equal(out[:, :, cc:][..., inside], state[:, :, cc:][..., inside])                    # inside: the region's
        assert torch.equal(out[:, :, cc + G:][..., ~inside], state[:, :, :cc][..., ~inside])              # outside: the target IS the source
        assert torch.equal(out[:, :, cc:cc + G][..., ~inside], state[:, :, :G][..., ~inside])             # ... and grounding frame g source frame g
    with pytest.raises(ValueError, match="does not lie inside"):
        reference_region_crop(state, (0, 0, h + 1, w))
    with pytest.raises(ValueError, match="does not lie inside"):
        reference_region_restore(state[:, :, :cc], state[..., :2, :2], (h - 1, 0))
    with pytest.raises(ValueError, match="grounding frames"):
        reference_region_restore(state[:, :, :1], torch.zeros(B, C, 4, 2, 2, dtype=dtype), (0, 0))          # G = 2 > cc = 1


# ------------------------------------------------------------------------------------------------ the switches
def test_the_pipeline_checks_the_switches_before_any_device_work():
    """A pipeline whose transformer is a bare object (any use of it is an AttributeError) gets to every refusal."""
    pipe = WanPipeline(transformer=object(), scheduler=FlowUniPCMultistepScheduler(shift=1))
    kw = dict(latents=torch.zeros(1, 16, 15, 4, 4), source_frames=25, height=32, width=32, cot=True, output_type="latent")
    ok = np.full((25, 32, 32), 255, np.uint8)
    with pytest.raises(ValueError, match="no edit_mask"):
        pipe(edit_region=True, **kw)
    for bad in ((24, 16), (16, 8), (-16, 16), (16, -16), 16, (16.0, 16)):
        with pytest.raises(ValueError, match="edit_region_margin"):
            pipe(edit_mask=ok, edit_region=True, edit_region_margin=bad, **kw)
    with pytest.raises(NotImplementedError, match="capture_graph='loop'"):
        pipe(edit_mask=ok, edit_region=True, capture_graph="loop", **kw)
    with pytest.raises(TypeError, match="edit_regions"):
        pipe(edit_mask=ok, edit_regions=True, **kw)
    with pytest.raises(TypeError, match="edit_region_margins"):
        pipe(edit_mask=ok, edit_region=True, edit_region_margins=(16, 16), **kw)
    assert WanPipelineOutput(videos=None).edit_region is None


def test_cpu_tensors_raise_in_the_wrappers():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mask_bounds(torch.zeros(1, 2, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.region_crop(torch.zeros(1, 2, 5, 4, 4), (0, 0, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.region_restore(torch.zeros(1, 2, 2, 4, 4), torch.zeros(1, 2, 5, 2, 2), (0, 0))


# ------------------------------------------------------------------------------------------------ the entry points, without a GPU
def test_entry_points_refuse_bad_arguments_before_launching():
    lib = _lib.load()
    inv = _lib.WAN_ERR_INVALID
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "wan_hip.h")).read()
    for sym in ("wan_mask_bounds", "wan_region_crop", "wan_region_restore"):
        assert sym in _lib.SIGNATURES and f"{sym}(" in header
    assert _lib.ABI_VERSION == 11                                     # additions only

    bounds = lambda *a: lib.wan_mask_bounds(*a, None)
    assert bounds(None, 8, 1, 3, 4, 4) == inv and bounds(8, None, 1, 3, 4, 4) == inv
    with pytest.raises(ValueError, match="null tensor"):
        _lib.check(inv, "wan_mask_bounds")
    assert bounds(8, 8, 0, 3, 4, 4) == inv and bounds(8, 8, 1, 0, 4, 4) == inv and bounds(8, 8, 1, 3, 0, 4) == inv
    assert bounds(8, 6, 1, 3, 4, 4) == inv                            # the words' address
    assert bounds(8, 8, 16, 1 << 12, 1 << 8, 1 << 8) == inv           # 2^32 weights
    with pytest.raises(ValueError, match="weights"):
        _lib.check(inv, "wan_mask_bounds")

    crop = lambda *a: lib.wan_region_crop(*a, None)
    good = (8, 8, 2, 10, 6, 8, 2, 2, 4, 4)                            # out, in, elem_bytes, R, H, W, y0, x0, hr, wr
    for k in (0, 1):
        assert crop(*good[:k], None, *good[k + 1:]) == inv
    with pytest.raises(ValueError, match="null tensor"):
        _lib.check(inv, "wan_region_crop")
    assert crop(*good[:2], 3, *good[3:]) == inv and crop(*good[:2], 8, *good[3:]) == inv
    with pytest.raises(ValueError, match="1, 2 or 4"):
        _lib.check(inv, "wan_region_crop")
    for box in ((-2, 2, 4, 4), (2, -2, 4, 4), (2, 2, 5, 4), (2, 2, 4, 7), (2, 2, 0, 4), (2, 2, 4, 0), (6, 0, 1, 1), (0, 8, 1, 1),
                (1 << 30, 0, 1 << 30, 1), (0, (1 << 31) - 1, 1, (1 << 31) - 1)):
        assert crop(*good[:6], *box) == inv, box
    with pytest.raises(ValueError, match="does not lie inside"):
        _lib.check(inv, "wan_region_crop")
    assert crop(*good[:3], 0, *good[4:]) == inv and crop(*good[:3], 1 << 31, *good[4:]) == inv
    assert crop(8, 8, 1, 1, 1 << 16, 1 << 16, 0, 0, 1, 1) == inv      # 2^32 elements a frame

    restore = lambda *a: lib.wan_region_restore(*a, None)
    good = (8, 8, 8, 2, 1, 2, 2, 1, 6, 8, 2, 2, 4, 4)                 # out, source, region, elem_bytes, B, C, cc, G, H, W, y0, x0, hr, wr
    for k in (0, 1, 2):
        assert restore(*good[:k], None, *good[k + 1:]) == inv
    with pytest.raises(ValueError, match="null tensor"):
        _lib.check(inv, "wan_region_restore")
    assert restore(*good[:3], 3, *good[4:]) == inv
    assert restore(*good[:7], 3, *good[8:]) == inv and restore(*good[:7], -1, *good[8:]) == inv           # G > cc, G < 0
    with pytest.raises(ValueError, match="G=-1"):
        _lib.check(inv, "wan_region_restore")
    assert restore(*good[:4], 0, *good[5:]) == inv and restore(*good[:6], 0, *good[7:]) == inv
    for box in ((3, 2, 4, 4), (2, 5, 4, 4), (-1, 0, 2, 2), (0, 0, 7, 8), (0, 0, 6, 9), (0, 0, 0, 0)):
        assert restore(*good[:10], *box) == inv, box
    with pytest.raises(ValueError, match="does not lie inside"):
        _lib.check(inv, "wan_region_restore")
    assert restore(*good[:4], 1 << 15, 1 << 15, *good[6:]) == inv     # 2^30 rows of 5 frames
