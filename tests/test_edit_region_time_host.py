"""Edit region, the time axis, on the CPU: the frame-range rule swept over every (lo, hi) of short clips, the torch definitions of the
two device passes, the switch's checks (before any device work) and the entry points' argument errors.  docs/TEST_BOUNDS.md, "Edit
region: the time axis"."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from videocof_amd import (FlowUniPCMultistepScheduler, TimeRegion, WanPipeline, WanPipelineOutput, _lib, ops, reference_region_crop,
                          reference_region_crop_frames, reference_region_restore, reference_region_restore_frames, region_time_margin_frames,
                          region_time_plan)

H, W = 6, 8
EMPTY, FULL = (H, -1, W, -1), (1, 4, 2, 5)


def _bounds(Fs, lo, hi, holes=()):
    """Per-frame bounds as wan_mask_bounds returns them: a box on the frames lo..hi (but `holes`), the empty sentinel elsewhere."""
    return np.array([FULL if lo <= f <= hi and f not in holes else EMPTY for f in range(Fs)], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the rule
def test_every_frame_range_of_short_clips():
    cases = 0
    for Fs in range(1, 10):
        for m, G in itertools.product(range(4), range(min(3, Fs) + 1)):
            for lo, hi in itertools.combinations_with_replacement(range(Fs), 2):
                r = region_time_plan(_bounds(Fs, lo, hi), Fs, m, G)
                assert isinstance(r, TimeRegion)
                core = hi - lo + 1 + 2 * m                                                 # the issue's statement, written out once more
                n = min(Fs, max(core, 2, G))
                t0 = min(max(lo - m - max(n - core, 0) // 2, 0), Fs - n)
                assert r == (t0, n)
                assert 0 <= r.t0 and r.n >= 1 and r.t0 + r.n <= Fs                         # inside the clip
                assert r.t0 <= max(lo - m, 0) and r.t0 + r.n - 1 >= min(hi + m, Fs - 1)    # contains [lo - m, hi + m], clipped
                assert r.n >= min(Fs, max(2, G))                                           # the floor
                cases += 1
    assert cases == sum(4 * (min(3, Fs) + 1) * Fs * (Fs + 1) // 2 for Fs in range(1, 10))


def test_empty_frames_drop_out_and_an_empty_mask_raises():
    assert region_time_plan(_bounds(9, 3, 6, holes=(4, 5)), 9, 0) == region_time_plan(_bounds(9, 3, 6), 9, 0) == (3, 4)
    assert region_time_plan(torch.from_numpy(_bounds(9, 5, 5)), 9, 0) == (5, 2)            # one frame: the floor of 2, the spare frame behind
    assert region_time_plan(_bounds(9, 5, 5), 9, 0, ground=3) == (4, 3)
    assert region_time_plan(_bounds(9, 0, 0), 9, 1) == (0, 3) and region_time_plan(_bounds(9, 8, 8), 9, 1) == (6, 3)
    assert region_time_plan(_bounds(9, 2, 3), 9, 3) == (0, 8) and region_time_plan(_bounds(9, 0, 8), 9, 0) == (0, 9)
    assert region_time_plan(_bounds(1, 0, 0), 1, 2, 1) == (0, 1)
    rows = _bounds(5, 2, 2)
    rows[3] = (2, 1, 0, 3)                                                                 # rows empty in y only, in x only: both empty
    rows[4] = (0, 3, 5, 4)
    assert region_time_plan(rows, 5, 0) == (2, 2)
    with pytest.raises(ValueError, match="edit_mask is empty"):
        region_time_plan(np.array([EMPTY] * 5), 5, 1)
    with pytest.raises(ValueError, match="5 latent frames"):
        region_time_plan(_bounds(4, 1, 2), 5, 1)
    for bad in (dict(frames=0), dict(margin_frames=-1), dict(margin_frames=1.0), dict(margin_frames=True), dict(ground=-1)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            region_time_plan(_bounds(5, 1, 2), **{"frames": 5, "margin_frames": 1, **bad})


def test_the_range_in_pixel_frames():
    assert TimeRegion(0, 5).pixels() == (0, 17) and TimeRegion(0, 1).pixels() == (0, 1)                # t0 = 0: the single first frame
    assert TimeRegion(2, 2).pixels() == (5, 8) and TimeRegion(1, 4).pixels() == (1, 16)                # t0 > 0: whole groups of 4
    assert TimeRegion(28, 20).pixels() == (109, 80)                                                    # pixel frames 109..188
    assert TimeRegion(1, 1).pixels(ratio=8) == (1, 8)
    assert region_time_margin_frames(0) == 0 and region_time_margin_frames(8) == 2 and region_time_margin_frames(np.int64(4)) == 1
    for bad in (True, False, 8.0, "8", (8,), -4, 6, 1):
        with pytest.raises(ValueError, match="edit_region_time_margin"):
            region_time_margin_frames(bad)


# ------------------------------------------------------------------------------------------------ the definitions
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
def test_the_definitions_extend_their_siblings(dtype):
    B, C, cc = 2, 3, 4
    gen = torch.Generator().manual_seed(3)
    make = lambda *shape: (torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8) if dtype == torch.uint8
                           else torch.randn(*shape, generator=gen).to(dtype))
    for G in (0, 1, 2, 4):
        Ft = 2 * cc + G
        state = make(B, C, Ft, H, W)
        source = state[:, :, :cc]
        for region in ((0, 0, H, W), (1, 2, 4, 4), (5, 7, 1, 1)):
            y0, x0, hr, wr = region
            # one run (0, F) is the spatial crop; (0, cc) is the spatial restore
            assert torch.equal(reference_region_crop_frames(state, [(0, Ft)], region), reference_region_crop(state, region))
            final = make(B, C, Ft, hr, wr)
            assert torch.equal(reference_region_restore_frames(source, final, (y0, x0), (0, cc)), reference_region_restore(source, final, (y0, x0)))
            inside = torch.zeros(H, W, dtype=torch.bool)
            inside[y0:y0 + hr, x0:x0 + wr] = True
            for t0, n in ((0, 2), (1, 2), (3, 1), (1, 3), (0, 4), (2, 2)):
                runs = [(t0, n)] + ([(cc, G)] if G else []) + [(cc + G + t0, n)]
                crop = reference_region_crop_frames(state, runs, region)
                assert crop.shape == (B, C, 2 * n + G, hr, wr) and crop.is_contiguous()
                assert torch.equal(crop[:, :, :n], state[:, :, t0:t0 + n, y0:y0 + hr, x0:x0 + wr])
                assert torch.equal(crop[:, :, n:n + G], state[:, :, cc:cc + G, y0:y0 + hr, x0:x0 + wr])
                assert torch.equal(crop[:, :, n + G:], state[:, :, cc + G + t0:cc + G + t0 + n, y0:y0 + hr, x0:x0 + wr])
                final = make(B, C, 2 * n + G, hr, wr)
                out = reference_region_restore_frames(source, final, (y0, x0), (t0, n))
                assert out.shape == state.shape and out.dtype == dtype
                assert torch.equal(reference_region_crop_frames(out, runs, region)[:, :, n:], final[:, :, n:])     # cropping it gives the region back
                assert torch.equal(out[:, :, :cc], source)
                in_range = torch.zeros(cc, dtype=torch.bool)
                in_range[t0:t0 + n] = True
                target = out[:, :, cc + G:]
                assert torch.equal(target[:, :, ~in_range], source[:, :, ~in_range])                                # outside the range: the source
                assert torch.equal(target[..., ~inside], source[..., ~inside])                                      # outside the box: the source
                assert torch.equal(out[:, :, cc:cc + G][..., ~inside], source[:, :, :G][..., ~inside])
    w = make(2, 5, H, W)                                                                                            # the weights: one run
    assert torch.equal(reference_region_crop_frames(w, [(1, 3)], (1, 2, 4, 4)), w[:, 1:4, 1:5, 2:6])


def test_the_definitions_refuse_what_the_entry_points_refuse():
    x = torch.zeros(1, 2, 5, H, W)
    for runs in ([], [(0, 1)] * 4, [(0, 2), (1, 2)], [(2, 1), (0, 1)], [(4, 2)], [(0, 0)], [(-1, 2)]):
        with pytest.raises(ValueError, match="runs"):
            reference_region_crop_frames(x, runs, (0, 0, 2, 2))
    with pytest.raises(ValueError, match="does not lie inside"):
        reference_region_crop_frames(x, [(0, 1)], (0, 0, H + 1, W))
    src = torch.zeros(1, 2, 2, H, W)
    with pytest.raises(ValueError, match="do not lie inside"):
        reference_region_restore_frames(src, torch.zeros(1, 2, 5, 2, 2), (0, 0), (1, 2))
    with pytest.raises(ValueError, match="do not lie inside"):
        reference_region_restore_frames(src, torch.zeros(1, 2, 5, 2, 2), (0, 0), (-1, 2))
    with pytest.raises(ValueError, match="grounding frames"):
        reference_region_restore_frames(src, torch.zeros(1, 2, 5, 2, 2), (0, 0), (0, 1))                 # G = 3 > cc = 2
    with pytest.raises(ValueError, match="does not lie inside"):
        reference_region_restore_frames(src, torch.zeros(1, 2, 5, 2, 2), (H - 1, 0), (0, 2))


# ------------------------------------------------------------------------------------------------ the switch
def test_the_pipeline_checks_the_switch_before_any_device_work():
    """A pipeline whose transformer is a bare object (any use of it is an AttributeError) gets to every refusal."""
    pipe = WanPipeline(transformer=object(), scheduler=FlowUniPCMultistepScheduler(shift=1))
    kw = dict(latents=torch.zeros(1, 16, 15, 4, 4), source_frames=25, height=32, width=32, cot=True, output_type="latent")
    ok = np.full((25, 32, 32), 255, np.uint8)
    for bad in (True, False, 8.0, "8", (8, 8), -4, 6, 2):
        with pytest.raises(ValueError, match="edit_region_time_margin"):
            pipe(edit_mask=ok, edit_region=True, edit_region_time_margin=bad, **kw)
    with pytest.raises(ValueError, match="edit_region_time_margin"):
        pipe(edit_mask=ok, edit_region_time_margin=8, **kw)                    # without edit_region=True
    with pytest.raises(ValueError, match="edit_region_time_margin"):
        pipe(edit_region_time_margin=8, **kw)
    with pytest.raises(NotImplementedError, match="capture_graph='loop'"):
        pipe(edit_mask=ok, edit_region=True, edit_region_time_margin=8, capture_graph="loop", **kw)
    with pytest.raises(TypeError, match="edit_region_time_margins"):
        pipe(edit_mask=ok, edit_region=True, edit_region_time_margins=8, **kw)
    for good in (0, 8, np.int64(4)):
        with pytest.raises(ValueError, match="Provide either `prompt`"):       # a good value gets past the switches, to the next check
            pipe(edit_mask=ok, edit_region=True, edit_region_time_margin=good, **kw)
    assert WanPipelineOutput(videos=None).edit_region_time is None and WanPipelineOutput(videos=None).edit_region is None


def test_cpu_tensors_raise_in_the_wrappers():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.region_crop_frames(torch.zeros(1, 2, 5, 4, 4), [(0, 2)], (0, 0, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.region_restore_frames(torch.zeros(1, 2, 2, 4, 4), torch.zeros(1, 2, 3, 2, 2), (0, 0), (0, 1))


# ------------------------------------------------------------------------------------------------ the entry points, without a GPU
def test_entry_points_refuse_bad_arguments_before_launching():
    lib = _lib.load()
    inv = _lib.WAN_ERR_INVALID
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "wan_hip.h")).read()
    for sym in ("wan_region_crop_frames", "wan_region_restore_frames"):
        assert sym in _lib.SIGNATURES and f"{sym}(" in header
    assert _lib.ABI_VERSION == 11                                     # additions only

    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    crop = lambda *a: lib.wan_region_crop_frames(*a, None)
    good = (8, 8, 2, 10, 9, 6, 8, ints(1, 2, 4, 1, 6, 2), 3, 2, 2, 4, 4)      # out, in, elem_bytes, R, F, H, W, runs, n_runs, y0, x0, hr, wr
    assert crop(*good[:7], None, *good[8:]) == inv                            # null runs
    with pytest.raises(ValueError, match="not null"):
        _lib.check(inv, "wan_region_crop_frames")
    for k in (0, 1):
        assert crop(*good[:k], None, *good[k + 1:]) == inv
    with pytest.raises(ValueError, match="wan_region_crop_frames: null tensor"):
        _lib.check(inv, "wan_region_crop_frames")
    assert crop(*good[:2], 3, *good[3:]) == inv and crop(*good[:2], 8, *good[3:]) == inv
    with pytest.raises(ValueError, match="1, 2 or 4"):
        _lib.check(inv, "wan_region_crop_frames")
    assert crop(*good[:8], 0, *good[9:]) == inv and crop(*good[:7], ints(0, 1, 1, 1, 2, 1, 3, 1), 4, *good[9:]) == inv      # 0 and 4 runs
    with pytest.raises(ValueError, match="1 to 3"):
        _lib.check(inv, "wan_region_crop_frames")
    for runs in ((1, 3, 3, 1), (0, 2, 1, 2),          # overlap
                 (4, 1, 1, 2), (4, 1, 4, 1),          # descend, repeat
                 (0, 2, 8, 2), (9, 1), (-1, 2),       # leave [0, F)
                 (0, 0), (1, 2, 4, -1),               # empty
                 (0, (1 << 31) - 1, 3, 2)):
        assert crop(*good[:7], ints(*runs), len(runs) // 2, *good[9:]) == inv, runs
    with pytest.raises(ValueError, match="run 0"):
        _lib.check(inv, "wan_region_crop_frames")
    for box in ((-2, 2, 4, 4), (2, -2, 4, 4), (2, 2, 5, 4), (2, 2, 4, 7), (2, 2, 0, 4), (2, 2, 4, 0), (6, 0, 1, 1), (0, 8, 1, 1),
                (1 << 30, 0, 1 << 30, 1), (0, (1 << 31) - 1, 1, (1 << 31) - 1)):
        assert crop(*good[:9], *box) == inv, box
    with pytest.raises(ValueError, match="does not lie inside"):
        _lib.check(inv, "wan_region_crop_frames")
    assert crop(*good[:3], 0, *good[4:]) == inv and crop(*good[:4], 0, *good[5:]) == inv                 # no clips, no frames
    assert crop(*good[:3], 1 << 31, *good[4:]) == inv and crop(*good[:3], 1 << 62, *good[4:]) == inv      # 2^31 clips and more
    assert crop(*good[:3], 1 << 28, *good[4:]) == inv                                                     # 9 * 2^28 frames in all
    assert crop(8, 8, 1, 1, 1, 1 << 16, 1 << 16, ints(0, 1), 1, 0, 0, 1, 1) == inv                        # 2^32 elements a frame
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        _lib.check(inv, "wan_region_crop_frames")

    restore = lambda *a: lib.wan_region_restore_frames(*a, None)
    good = (8, 8, 8, 2, 1, 2, 4, 1, 6, 8, 1, 2, 2, 2, 4, 4)           # out, source, region, elem_bytes, B, C, cc, G, H, W, t0, n, y0, x0, hr, wr
    for k in (0, 1, 2):
        assert restore(*good[:k], None, *good[k + 1:]) == inv
    with pytest.raises(ValueError, match="wan_region_restore_frames: null tensor"):
        _lib.check(inv, "wan_region_restore_frames")
    assert restore(*good[:3], 3, *good[4:]) == inv
    assert restore(*good[:7], 5, *good[8:]) == inv and restore(*good[:7], -1, *good[8:]) == inv          # G > cc, G < 0
    with pytest.raises(ValueError, match="G=-1"):
        _lib.check(inv, "wan_region_restore_frames")
    assert restore(*good[:4], 0, *good[5:]) == inv and restore(*good[:6], 0, *good[7:]) == inv
    for t0, n in ((3, 2), (0, 5), (4, 1), (-1, 2), (1, 0), (0, -1), (1, (1 << 31) - 1)):                  # t0 + n > cc, t0 < 0, n < 1
        assert restore(*good[:10], t0, n, *good[12:]) == inv, (t0, n)
    with pytest.raises(ValueError, match="do not lie inside the 4 source frames"):
        _lib.check(inv, "wan_region_restore_frames")
    for box in ((3, 2, 4, 4), (2, 5, 4, 4), (-1, 0, 2, 2), (0, 0, 7, 8), (0, 0, 6, 9), (0, 0, 0, 0)):
        assert restore(*good[:12], *box) == inv, box
    with pytest.raises(ValueError, match="does not lie inside"):
        _lib.check(inv, "wan_region_restore_frames")
    assert restore(*good[:4], 1 << 15, 1 << 15, *good[6:]) == inv     # 2^30 rows of 9 frames
