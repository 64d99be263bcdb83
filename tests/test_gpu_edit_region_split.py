"""-m gpu: edit region, a mask of separate objects split into boxes -- wan_mask_spans / wan_region_crop_split / wan_region_restore_split
against their torch definitions (word for word and bit for bit, with guard bands) and against the frames forms, and
WanPipeline(edit_region=True, edit_region_split=K) against call B built by hand: the starting latents and the weights cropped with the
torch definition, the plain edit_mask call of K' samples on them, and the torch definition's restore.  DESIGN.md 13.6."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from videocof_amd import (FlowUniPCMultistepScheduler, RegionPlan, SplitPlan, WanPipeline, _lib, latent_edit_mask, ops,
                          reference_mask_spans, reference_region_crop_split, reference_region_restore_split, region_split_plan,
                          region_time_plan)
from videocof_amd.edit_region import spans_bounds
from videocof_amd.weights import det_uniform

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pipeline_trace import POS_ROWS, RecordingTransformer, prompts, record  # noqa: E402
from test_gpu_edit_region_follow import DEV, POISON, RANGES, Guarded, _call, _pipe, _runs, _values, bits, model, sd  # noqa: E402,F401

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the spans
def _sparse(shape, seed, density=0.06):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) < density) * torch.randint(1, 256, shape, generator=g)).to(torch.uint8)


@pytest.mark.parametrize("shape", [(2, 3, 10, 37), (1, 2, 16, 48), (1, 2, 135, 240), (1, 1, 3, 300)], ids=lambda s: "x".join(map(str, s)))
def test_spans_equal_the_definition(shape):
    """[2, 3, 10, 37]: an odd width, so a 1-byte unit; 48 and 240 columns: 16-byte units (3 and 15 to a row, rows sharing a workgroup);
    300 columns behind an odd band: more than 256 units to a row.  Frame 1 is empty, and rows and columns of the others are."""
    a = _sparse(shape, sum(shape))
    if shape[1] > 1:
        a[:, 1] = 0
    a[:, 0, 1] = 0
    a[:, 0, :, 5] = 0
    for pad in (64, 3) if shape[-1] != 300 else (3,):                          # a band of 3 bytes: the unit falls to one byte through the base
        wts = Guarded(a.shape, torch.uint8, pad, a)
        want = reference_mask_spans(a)
        out = Guarded(want.shape, torch.int16, 64)
        got = ops.mask_spans(wts.view, out=out.view)
        assert got.data_ptr() == out.view.data_ptr()
        assert torch.equal(out.view.cpu(), want)
        assert out.intact() and wts.intact() and torch.equal(wts.view.cpu(), a)
        assert spans_bounds(out.view, shape[2:]).tolist() == ops.mask_bounds(wts.view).tolist()
    full = torch.full(shape, 3, dtype=torch.uint8)
    assert torch.equal(ops.mask_spans(full.to(DEV)).cpu(), reference_mask_spans(full))


def test_spans_reject_what_they_cannot_hold():
    lib, inv = _lib.load(), _lib.WAN_ERR_INVALID
    for shape in ((1, 1, 1, 32768), (1, 1, 32768, 1)):
        out = Guarded((1, 32769, 2), torch.int16)
        with pytest.raises(ValueError, match="32768"):
            ops.mask_spans(torch.ones(shape, dtype=torch.uint8, device=DEV), out=out.view)
        torch.cuda.synchronize()
        assert bool((out.buf == POISON).all())
    w, out = torch.ones(1, 2, 4, 6, dtype=torch.uint8, device=DEV), Guarded((2, 10, 2), torch.int16)
    p = out.view.data_ptr()
    assert lib.wan_mask_spans(None, p, 1, 2, 4, 6, None) == inv and lib.wan_mask_spans(w.data_ptr(), None, 1, 2, 4, 6, None) == inv
    assert lib.wan_mask_spans(w.data_ptr(), p, 0, 2, 4, 6, None) == inv and lib.wan_mask_spans(w.data_ptr(), p, 1, 2, 0, 6, None) == inv
    assert lib.wan_mask_spans(w.data_ptr(), p + 2, 1, 2, 4, 6, None) == inv    # a pair is one word
    assert lib.wan_mask_spans(w.data_ptr(), p, 1 << 16, 1 << 14, 4, 6, None) == inv            # 2^31 weights or more
    torch.cuda.synchronize()
    assert bool((out.buf == POISON).all())
    with pytest.raises(ValueError, match="mask_spans.out"):
        ops.mask_spans(w, out=torch.zeros(2, 10, 2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="contiguous uint8"):
        ops.mask_spans(w[0])


# ------------------------------------------------------------------------------------------------ the crop and the restore
# (H, W, hr, wr, origins, cuts, axis, guard elements).  The access unit divides W, wr, EVERY x0 and, for a column cut, every cut:
#   0  two boxes side by side, the cut at 8: 16 bytes in fp32 and bf16, 8 in uint8
#   1  the cut at 6, an odd multiple of the patch 2: 8 / 4 / 2 bytes; box 0 reaches past what it owns, box 1 starts before its own
#   2  three overlapping boxes at odd x0, cuts at 2 and 3: one element
#   3  a cut along the rows, three boxes that overlap and reach past what they own; x0 = 2: 8 / 4 / 2 bytes
#   4  one box that owns the frame (the frames forms)
#   5  case 0 behind a 3-element band: one element through the bases alone
#   6  rows longer than 256 units, cut along the rows
#   7  eight boxes, the most
SPLITS = [(6, 16, 4, 8, [[0, 0], [2, 8]], [0, 8, 16], 1, 64), (6, 16, 4, 8, [[1, 0], [2, 4]], [0, 6, 16], 1, 64),
          (5, 7, 3, 5, [[0, 0], [1, 1], [2, 2]], [0, 2, 3, 7], 1, 64), (9, 8, 4, 4, [[0, 0], [2, 4], [5, 2]], [0, 3, 6, 9], 0, 64),
          (6, 12, 6, 8, [[0, 4]], [0, 12], 1, 64), (6, 16, 4, 8, [[0, 0], [2, 8]], [0, 8, 16], 1, 3),
          (3, 300, 2, 290, [[0, 0], [1, 5]], [0, 2, 3], 0, 64),
          (4, 16, 2, 2, [[k % 3, 2 * k] for k in range(8)], list(range(0, 16, 2)) + [16], 1, 64)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8], ids=["fp32", "bf16", "u8"])
@pytest.mark.parametrize("H,W,hr,wr,origins,cuts,axis,pad", SPLITS)
def test_crop_and_restore_equal_the_torch_definitions(H, W, hr, wr, origins, cuts, axis, pad, dtype):
    C, K = 2, len(origins)
    for B in (1, 2):
        for cc, G, t0, n in RANGES:                                            # runs with and without G, one, two and three of them
            Ft = 2 * cc + G
            full = _values(f"ers.{H}.{W}.{B}.{cc}.{G}", (B, C, Ft, H, W), dtype)
            state = Guarded(full.shape, dtype, pad, full)
            source = Guarded((B, C, cc, H, W), dtype, pad, full[:, :, :cc])
            runs = _runs(cc, G, t0, n)
            for clip in (False, True):
                want = reference_region_crop_split(full, runs, origins, cuts, axis, (hr, wr), clip=clip)
                crop = Guarded(want.shape, dtype, pad)
                got = ops.region_crop_split(state.view, runs, origins, cuts, axis, (hr, wr), clip=clip, out=crop.view)
                assert got.data_ptr() == crop.view.data_ptr()
                assert torch.equal(bits(crop.view.cpu()), bits(want)), (B, runs, clip)
                assert crop.intact() and state.intact()
            final = _values(f"ers.final.{H}.{W}.{B}.{t0}.{n}", (K * B, C, 2 * n + G, hr, wr), dtype)
            fin = Guarded(final.shape, dtype, pad, final)
            want_full = reference_region_restore_split(full[:, :, :cc], final, origins, cuts, axis, (t0, n))
            out = Guarded(full.shape, dtype, pad)
            got = ops.region_restore_split(source.view, fin.view, origins, cuts, axis, (t0, n), out=out.view)
            assert got.data_ptr() == out.view.data_ptr()
            res = out.view.cpu()
            assert torch.equal(bits(res), bits(want_full)), (B, runs)
            assert out.intact() and fin.intact() and source.intact()
            src = full[:, :, :cc]
            covered = torch.zeros(H, W, dtype=torch.bool)                      # inside a box AND inside what its band owns
            for k, (y0, x0) in enumerate(origins):
                own = torch.zeros(H, W, dtype=torch.bool)
                own[(slice(None), slice(cuts[k], cuts[k + 1])) if axis else slice(cuts[k], cuts[k + 1])] = True
                own[:y0] = own[y0 + hr:] = False
                own[:, :x0] = own[:, x0 + wr:] = False
                assert not (covered & own).any()                               # one of K + 1 places for every cell
                covered |= own
            for f in range(cc):                                                # everywhere else, and outside the range: the source
                keep = torch.ones(H, W, dtype=torch.bool) if not t0 <= f < t0 + n else ~covered
                assert torch.equal(bits(res[:, :, cc + G + f][..., keep]), bits(src[:, :, f][..., keep]))
            assert torch.equal(bits(res[:, :, :cc]), bits(src))
            assert torch.equal(bits(state.view.cpu()), bits(full)) and torch.equal(bits(source.view.cpu()), bits(src))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8], ids=["fp32", "bf16", "u8"])
@pytest.mark.parametrize("H,W,hr,wr,x0,pad", [(6, 16, 4, 8, 8, 64), (6, 12, 4, 8, 4, 64), (5, 7, 3, 5, 1, 64), (6, 16, 4, 8, 3, 64),
                                              (6, 16, 4, 8, 0, 3)])
def test_one_box_gives_the_bytes_of_the_frames_forms(H, W, hr, wr, x0, pad, dtype):
    B, C = 2, 2
    for cc, G, t0, n in RANGES[:6]:
        full = _values(f"ers.one.{H}.{W}.{cc}.{G}", (B, C, 2 * cc + G, H, W), dtype)
        state = Guarded(full.shape, dtype, pad, full)
        source = Guarded((B, C, cc, H, W), dtype, pad, full[:, :, :cc])
        runs = _runs(cc, G, t0, n)
        for axis in (0, 1):
            y0, cuts = H - hr, [0, (H, W)[axis]]
            same = ops.region_crop_frames(state.view, runs, (y0, x0, hr, wr))
            for clip in (False, True):
                got = ops.region_crop_split(state.view, runs, [[y0, x0]], cuts, axis, (hr, wr), clip=clip)
                assert got.shape == (1,) + same.shape and torch.equal(bits(got[0]), bits(same))
            final = _values(f"ers.onef.{H}.{W}.{t0}.{n}", same.shape, dtype).to(DEV)
            assert torch.equal(bits(ops.region_restore_split(source.view, final, [[y0, x0]], cuts, axis, (t0, n))),
                               bits(ops.region_restore_frames(source.view, final, (y0, x0), (t0, n))))
        assert state.intact() and source.intact()


def test_invalid_boxes_raise_and_launch_nothing():
    src = Guarded((1, 2, 3, 6, 8), torch.float32)
    out = Guarded((1, 2, 7, 6, 8), torch.float32)
    small = Guarded((2, 2, 5, 2, 4), torch.float32)                             # two boxes of one sample, n = 2, G = 1
    two, cut2 = [[0, 0], [2, 4]], [0, 4, 8]
    crop_out = Guarded((2, 1, 2, 5, 2, 4), torch.float32)
    runs = [(0, 2), (3, 1), (4, 2)]
    bad = [dict(origins=[[0, 0]] * 9, cuts=list(range(9)) + [9]),              # more than 8 boxes
           dict(origins=[[5, 0], [2, 4]]), dict(origins=[[0, 5], [2, 4]]), dict(origins=[[-1, 0], [2, 4]]), dict(origins=[[0, 0], [2, -1]]),
           dict(cuts=[0, 4, 4]), dict(cuts=[0, 5, 4]), dict(cuts=[0, 8, 8]), dict(cuts=[1, 4, 8]), dict(cuts=[0, 4, 6]),     # cuts that do not ascend
           dict(axis=2), dict(axis=-1), dict(axis=0)]                          # (along the rows the cuts would end at 6)
    for change in bad:
        a = {**dict(origins=two, cuts=cut2, axis=1), **change}
        with pytest.raises(ValueError):
            ops.region_restore_split(src.view, small.view if len(a["origins"]) == 2 else torch.zeros(9, 2, 5, 2, 4, device=DEV),
                                     a["origins"], a["cuts"], a["axis"], (0, 2), out=out.view)
        with pytest.raises(ValueError):
            ops.region_crop_split(out.view, runs, a["origins"], a["cuts"], a["axis"], (2, 4),
                                  out=crop_out.view if len(a["origins"]) == 2 else None)
    with pytest.raises(ValueError, match="9 boxes"):
        ops.region_crop_split(out.view, runs, [[0, 0]] * 9, list(range(9)) + [9], 1, (2, 4))
    with pytest.raises(ValueError, match="box 1: .*does not lie inside"):
        ops.region_crop_split(out.view, runs, [[0, 0], [5, 4]], cut2, 1, (2, 4), out=crop_out.view)
    with pytest.raises(ValueError, match="the cuts ascend"):
        ops.region_restore_split(src.view, small.view, two, [0, 8, 8], 1, (0, 2), out=out.view)
    with pytest.raises(ValueError, match="cuts = 3 integers"):
        ops.region_crop_split(out.view, runs, two, [0, 8], 1, (2, 4))
    with pytest.raises(ValueError, match="state samples"):
        ops.region_restore_split(src.view, small.view[:1], two, cut2, 1, (0, 2), out=out.view)
    with pytest.raises(ValueError, match="do not lie inside the 3 source frames"):
        ops.region_restore_split(src.view, small.view, two, cut2, 1, (2, 2), out=out.view)
    with pytest.raises(ValueError, match="region_restore_split.out"):
        ops.region_restore_split(src.view, small.view, two, cut2, 1, (0, 2), out=out.view[:, :, :6])
    with pytest.raises(ValueError, match="region_crop_split.out"):
        ops.region_crop_split(out.view, runs, two, cut2, 1, (2, 4), out=crop_out.view[:1])
    for r in ([], [(0, 1)] * 4, [(0, 2), (1, 2)], [(6, 2)], [(0, 0)]):
        with pytest.raises(ValueError, match="run"):
            ops.region_crop_split(out.view, r, two, cut2, 1, (2, 4))
    with pytest.raises(ValueError, match="1, 2 or 4"):
        ops.region_crop_split(torch.zeros(2, 6, 8, device=DEV, dtype=torch.float64), [(0, 1)], two, cut2, 1, (2, 4))
    p = lambda g: g.view.data_ptr()
    lib, inv = _lib.load(), _lib.WAN_ERR_INVALID
    c_runs = (ctypes.c_int * 6)(0, 2, 3, 1, 4, 2)
    o2, c2 = (ctypes.c_int * 4)(0, 0, 2, 4), (ctypes.c_int * 3)(0, 4, 8)
    o9, c9 = (ctypes.c_int * 18)(*([0] * 18)), (ctypes.c_int * 10)(*range(10))
    off, flat = (ctypes.c_int * 4)(0, 0, 5, 4), (ctypes.c_int * 3)(0, 8, 8)
    restore, crop = lib.wan_region_restore_split, lib.wan_region_crop_split
    assert restore(None, p(src), p(small), 4, 1, 2, 3, 1, 6, 8, 0, 2, o2, c2, 2, 1, 2, 4, None) == inv   # null pointers
    assert restore(p(out), p(src), None, 4, 1, 2, 3, 1, 6, 8, 0, 2, o2, c2, 2, 1, 2, 4, None) == inv
    assert restore(p(out), p(src), p(small), 4, 1, 2, 3, 1, 6, 8, 0, 2, None, c2, 2, 1, 2, 4, None) == inv
    assert restore(p(out), p(src), p(small), 4, 1, 2, 3, 1, 6, 8, 0, 2, o2, None, 2, 1, 2, 4, None) == inv
    assert restore(p(out), p(src), p(small), 4, 1, 2, 3, 1, 6, 8, 0, 2, o9, c9, 9, 1, 2, 4, None) == inv     # more than 8 boxes
    assert restore(p(out), p(src), p(small), 4, 1, 2, 3, 1, 6, 8, 0, 2, o2, c2, 0, 1, 2, 4, None) == inv
    assert restore(p(out), p(src), p(small), 4, 1, 2, 3, 1, 6, 8, 0, 2, off, c2, 2, 1, 2, 4, None) == inv    # a corner outside the frame
    assert restore(p(out), p(src), p(small), 4, 1, 2, 3, 1, 6, 8, 0, 2, o2, flat, 2, 1, 2, 4, None) == inv   # cuts that do not ascend
    assert restore(p(out), p(src), p(small), 4, 1, 2, 3, 1, 6, 8, 0, 2, o2, c2, 2, 0, 2, 4, None) == inv     # the cuts end at 8, the rows at 6
    assert restore(p(out), p(src), p(small), 4, 1, 2, 3, 4, 6, 8, 0, 2, o2, c2, 2, 1, 2, 4, None) == inv     # G > cc
    assert restore(p(out), p(src), p(small), 3, 1, 2, 3, 1, 6, 8, 0, 2, o2, c2, 2, 1, 2, 4, None) == inv     # elements of 3 bytes
    assert crop(None, p(out), 4, 2, 7, 6, 8, c_runs, 3, o2, c2, 2, 1, 0, 2, 4, None) == inv
    assert crop(p(crop_out), None, 4, 2, 7, 6, 8, c_runs, 3, o2, c2, 2, 1, 0, 2, 4, None) == inv
    assert crop(p(crop_out), p(out), 4, 2, 7, 6, 8, None, 3, o2, c2, 2, 1, 0, 2, 4, None) == inv
    assert crop(p(crop_out), p(out), 4, 2, 7, 6, 8, c_runs, 3, None, c2, 2, 1, 0, 2, 4, None) == inv
    assert crop(p(crop_out), p(out), 4, 2, 7, 6, 8, c_runs, 3, o2, None, 2, 1, 1, 2, 4, None) == inv
    assert crop(p(crop_out), p(out), 4, 2, 7, 6, 8, c_runs, 3, o9, c9, 9, 1, 0, 2, 4, None) == inv
    assert crop(p(crop_out), p(out), 4, 2, 7, 6, 8, c_runs, 3, off, c2, 2, 1, 0, 2, 4, None) == inv
    assert crop(p(crop_out), p(out), 4, 2, 7, 6, 8, c_runs, 3, o2, flat, 2, 1, 1, 2, 4, None) == inv
    assert crop(p(crop_out), p(out), 4, 2, 5, 6, 8, c_runs, 3, o2, c2, 2, 1, 0, 2, 4, None) == inv           # a run leaves F = 5
    torch.cuda.synchronize()
    for g in (src, out, small, crop_out):                                      # nothing was launched: every element is still the poison
        assert bool((g.buf == POISON).all())


# ------------------------------------------------------------------------------------------------ pipeline
STEPS, SHIFT = 3, 3.0
G, FS, HL, WL = 1, 5, 16, 24           # source_frames=17 -> 5 latent frames; 128 x 192 pixels -> 16 x 24 cells
SIZE = dict(source_frames=17, height=128, width=192)
MARGIN = (16, 16)
PIXEL_FRAMES = [slice(0, 1)] + [slice(4 * f - 3, 4 * f + 1) for f in range(1, FS)]       # the pixel frames of latent frame f
A_CELL, B_CELL = (3, 3), (11, 11)      # the two objects, one latent cell each


def _mask(cells, frames=range(FS), shape=(128, 192), count=17):
    m = np.zeros((count,) + shape, np.uint8)
    for y, x in cells:
        for f in frames:
            m[PIXEL_FRAMES[f], 8 * y:8 * y + 8, 8 * x:8 * x + 8] = 255
    return m


# grow 1 and feather 1 spread a cell's weights 2 cells to every side: object A covers rows and columns 1 .. 5, B 9 .. 13.  With a
# margin of 2 cells each wants 6 + 4 = 10 cells on both axes: A's box starts at -2 clamped to 0, B's at 8 - 2 = 6.  The patches 0 .. 2
# and 4 .. 6 are occupied on either axis, so both cost 2 x 10 x 10 = 200 cells (the union: 16 x 18 = 288) and the columns win the tie;
# the cut is 2 * ((2 + 1 + 4) // 2) = 6: box A (columns 0 .. 9) reaches past what its band owns, and B's weights at column 9 lie in it.
TWO = _mask([A_CELL, B_CELL])
ONE = _mask([B_CELL])
SPLIT = SplitPlan(1, 10, 10, np.array([[0, 0], [6, 6]], np.int32), np.array([0, 6, 24], np.int32))
UNION = RegionPlan(0, 0, 16, 18)


@pytest.fixture(scope="module")
def inputs():
    lat = torch.cat([det_uniform("ers.src", (1, 16, FS, HL, WL), 1.0), det_uniform("ers.noise", (1, 16, FS + G, HL, WL), 1.0)], dim=2)
    return lat.to(DEV), det_uniform("ers.ctx", (37, 64), 1.0).to(DEV), det_uniform("ers.neg", (9, 64), 1.0).to(DEV)


def _call_a(pipe, inputs, **kw):
    return _call(pipe, inputs, **{**SIZE, **kw})


def _state_runs(time):
    t0, n = time
    return [(t0, n), (FS, G), (FS + G + t0, n)]


def _box_masks(cells, split, time, frames):
    """The pixel masks of call B, one per box: box k holds the objects of band k only, at their place in the box, on the pixel frames
    of the range (B's first latent frame is one pixel frame)."""
    t0, n = time
    out = []
    for k, (y0, x0) in enumerate(split.origins):
        mine = [(y - y0, x - x0) for y, x in cells if split.cuts[k] <= (y, x)[split.axis] < split.cuts[k + 1]]
        out.append(_mask(mine, [f - t0 for f in frames if t0 <= f < t0 + n], (8 * split.h, 8 * split.w), 1 + 4 * (n - 1)))
    return np.stack(out)


def _call_b(pipe, inputs, split, time, cells=(A_CELL, B_CELL), frames=range(FS), mask=TWO, scale=1.0, steps_out=None, **kw):
    """Call B, by hand: the starting latents cropped with the TORCH definition into K' samples, the plain edit_mask call on them with
    one pixel mask per sample (its weights are call A's, cropped and clipped with the torch definition: checked), no region option."""
    full, ctx, neg = inputs
    t0, n = time
    K = len(split.origins)
    boxes = split.origins, split.cuts, split.axis, (split.h, split.w)
    lat = reference_region_crop_split(full.cpu(), _state_runs(time), *boxes).flatten(0, 1).to(DEV)
    small = _box_masks(cells, split, time, frames)
    weights = latent_edit_mask(mask)[None]
    assert torch.equal(reference_region_crop_split(weights.cpu(), [(t0, n)], *boxes, clip=True).flatten(0, 1), latent_edit_mask(small).cpu())
    cb = None if steps_out is None else (lambda p, i, t, d: steps_out.append(d["latents"].clone()) or {})
    return pipe(latents=lat, prompt_embeds=[ctx] * K, negative_prompt_embeds=[neg] * K if scale > 1 else None, reasoning_frames=4,
                num_inference_steps=STEPS, guidance_scale=scale, shift=SHIFT, repeat_rope=True, cot=True, output_type="latent",
                weight_dtype=torch.float32, callback_on_step_end=cb, return_dict=True, edit_mask=small,
                source_frames=1 + 4 * (n - 1), height=8 * split.h, width=8 * split.w, **kw)


def _check_a_against_b(a, b, inputs, split, time):
    t0, n = time
    full, K = inputs[0], len(split.origins)
    assert a.edit_regions == split.pixels() and a.edit_region == split.enclosing().pixels() and a.edit_region_track is None
    assert b.edit_region is None and b.edit_regions is None
    assert a.latents.shape == full.shape and b.latents.shape == (K,) + full.shape[1:2] + (2 * n + G, split.h, split.w)
    src = full[:, :, :FS].cpu()
    want = reference_region_restore_split(src, b.latents.cpu(), split.origins, split.cuts, split.axis, time)
    got = a.latents.cpu()
    assert torch.equal(bits(got), bits(want))
    outside = torch.ones(HL, WL, dtype=torch.bool)                              # outside both boxes: the source's bits
    for y0, x0 in split.origins:
        outside[y0:y0 + split.h, x0:x0 + split.w] = False
    assert outside.any()
    for f in range(FS):
        keep = outside if t0 <= f < t0 + n else torch.ones_like(outside)
        assert torch.equal(bits(got[:, :, FS + G + f][..., keep]), bits(src[:, :, f][..., keep]))
        if f < G:
            assert torch.equal(bits(got[:, :, FS + f][..., outside]), bits(src[:, :, f][..., outside]))
    start = reference_region_crop_split(full.cpu(), [(FS + G + t0, n)], split.origins, split.cuts, split.axis, (split.h, split.w))
    assert not torch.equal(b.latents[:, :, n + G:].cpu(), start.flatten(0, 1))  # the loop did run


def test_the_plan_of_the_two_objects():
    spans = ops.mask_spans(latent_edit_mask(TWO)[None]).cpu()
    assert spans_bounds(spans, (HL, WL)).tolist() == [[1, 13, 1, 13]] * FS
    plan = region_split_plan(spans, (HL, WL), (2, 2), None, 2, max_regions=2)
    assert isinstance(plan, SplitPlan) and (plan.axis, plan.h, plan.w) == (SPLIT.axis, SPLIT.h, SPLIT.w)
    assert plan.origins.tolist() == SPLIT.origins.tolist() and plan.cuts.tolist() == SPLIT.cuts.tolist()
    assert plan.enclosing() == RegionPlan(0, 0, 16, 16) and 2 * plan.h * plan.w < UNION.h * UNION.w


def test_a_the_boxes_equal_the_cropped_call_of_two_samples(model, inputs):
    """The decisive case: without the feature the keyword is a TypeError.  The callback sees the box-major state."""
    seen = []
    a = _call_a(_pipe(model), inputs, steps_out=seen, edit_mask=TWO, edit_region=True, edit_region_margin=MARGIN, edit_region_split=2)
    b = _call_b(_pipe(model), inputs, SPLIT, (0, FS))
    _check_a_against_b(a, b, inputs, SPLIT, (0, FS))
    assert a.edit_regions == ((0, 0, 80, 80), (48, 48, 80, 80)) and a.edit_region == (0, 0, 128, 128)
    assert a.edit_region_time is None and a.edit_region_vae is None
    assert len(seen) == STEPS and all(s.shape == b.latents.shape for s in seen) and torch.equal(bits(seen[-1]), bits(b.latents))
    union = _call_a(_pipe(model), inputs, edit_mask=TWO, edit_region=True, edit_region_margin=MARGIN)       # one rectangle: other context
    assert union.edit_region == UNION.pixels() and union.edit_regions is None
    assert not torch.equal(union.latents[:, :, FS + G:], a.latents[:, :, FS + G:])
    more = _call_a(_pipe(model), inputs, edit_mask=TWO, edit_region=True, edit_region_margin=MARGIN, edit_region_split=8)
    assert torch.equal(bits(more.latents), bits(a.latents)) and more.edit_regions == a.edit_regions         # two objects: two boxes at most


def _trace(split, scale=1.0, ratio=None, mask=TWO, **kw):
    stub = RecordingTransformer(DEV)
    stub.cfg_skip_ratio = ratio
    pipe = WanPipeline(transformer=stub, scheduler=FlowUniPCMultistepScheduler(shift=1))
    lat = torch.randn(1, 16, 2 * FS + G, HL, WL, generator=torch.Generator().manual_seed(7))
    pos, neg = prompts(DEV)
    out = pipe(latents=lat, prompt_embeds=pos, negative_prompt_embeds=neg if scale > 1 else None, guidance_scale=scale, reasoning_frames=4,
               num_inference_steps=STEPS, shift=SHIFT, cot=True, output_type="latent", return_dict=True, edit_mask=mask, edit_region=True,
               **({} if split is None else dict(edit_region_split=split)), **SIZE, **{**dict(edit_region_margin=MARGIN), **kw})
    return pipe, stub, out


def test_b_one_object_is_edit_region_alone(model, inputs):
    plain = _call_a(_pipe(model), inputs, edit_mask=ONE, edit_region=True, edit_region_margin=MARGIN)
    a = _call_a(_pipe(model), inputs, edit_mask=ONE, edit_region=True, edit_region_margin=MARGIN, edit_region_split=4)
    assert a.edit_region == plain.edit_region == (48, 48, 80, 80) and a.edit_regions is None
    assert torch.equal(bits(a.latents), bits(plain.latents))
    (_, alone, out_alone), (_, split, out_split) = _trace(None, mask=ONE), _trace(4, mask=ONE)
    assert split.calls == alone.calls and len(split.calls) == STEPS and split.calls[0]["x"] == (1, 16, 2 * FS + G, 10, 10)
    assert not any(c["suspended"] for c in split.calls) and torch.equal(out_alone.latents, out_split.latents)


def test_c_with_a_time_margin(model, inputs):
    frames = (1, 2, 3)
    mask = _mask([A_CELL, B_CELL], frames)
    spans = ops.mask_spans(latent_edit_mask(mask)[None]).cpu()
    assert region_time_plan(spans_bounds(spans, (HL, WL)), FS, 0, G) == (1, 3)
    a = _call_a(_pipe(model), inputs, edit_mask=mask, edit_region=True, edit_region_margin=MARGIN, edit_region_split=2,
                edit_region_time_margin=0)
    b = _call_b(_pipe(model), inputs, SPLIT, (1, 3), frames=frames, mask=mask)
    _check_a_against_b(a, b, inputs, SPLIT, (1, 3))
    assert a.edit_region_time == (1, 12)


def test_d_with_a_spatial_window_every_box_is_one_tile(model, inputs):
    """spatial_window = 64 x 64 pixels = 8 x 8 cells, no margin: the common want (6 cells) fits the tile, so the boxes are tile-sized
    (2 x 64 cells against the union's 14 x 14) and the model sees ONE forward of K' samples per step."""
    tiles = dict(spatial_window=(64, 64), spatial_overlap=(16, 16), edit_region_margin=(0, 0))
    seen = []
    a = _call_a(_pipe(model), inputs, steps_out=seen, edit_mask=TWO, edit_region=True, edit_region_split=2, **tiles)
    spans = ops.mask_spans(latent_edit_mask(TWO)[None]).cpu()
    split = region_split_plan(spans, (HL, WL), (0, 0), (8, 8), 2, max_regions=2)
    assert (split.h, split.w) == (8, 8) and split.origins.tolist() == [[0, 0], [8, 8]] and split.cuts.tolist() == [0, 6, 24]
    b = _call_b(_pipe(model), inputs, split, (0, FS))
    _check_a_against_b(a, b, inputs, split, (0, FS))
    assert all(s.shape == b.latents.shape for s in seen)                       # one tile each: the state is never the windowed one
    pipe, stub, out = _trace(2, **tiles)
    x, seq = (2, 16, 2 * FS + G, 8, 8), math.ceil(8 * 8 / 4 * (2 * FS + G))
    assert stub.calls == [record(i, x, [POS_ROWS] * 2, t, seq, FS, G, suspended=True, cache=True)
                          for i, t in enumerate(pipe.scheduler.timesteps.tolist())]
    assert out.edit_regions == split.pixels()


def test_e_with_guidance_and_with_cfg_skip(model, inputs):
    a = _call_a(_pipe(model), inputs, scale=3.0, edit_mask=TWO, edit_region=True, edit_region_margin=MARGIN, edit_region_split=2)
    b = _call_b(_pipe(model), inputs, SPLIT, (0, FS), scale=3.0)
    _check_a_against_b(a, b, inputs, SPLIT, (0, FS))
    assert not torch.equal(b.latents, _call_b(_pipe(model), inputs, SPLIT, (0, FS)).latents)
    # a model with enable_cfg_skip on halves ANY batch of two or more on its late steps: an unguided batch of boxes is none of its
    # business -- the boxes go through as windows do, the rule suspended
    pipe, stub, _ = _trace(2, ratio=0.5)
    assert len(stub.calls) == STEPS and all(c["x"][0] == 2 and c["suspended"] and not c["halved"] for c in stub.calls)
    _, lone, _ = _trace(None, ratio=0.5)                                       # (one rectangle: one sample, nothing to suspend)
    assert all(c["x"][0] == 1 and not c["suspended"] for c in lone.calls)


def test_f_with_a_step_graph(model, inputs):
    pipe = _pipe(model)
    a = _call_a(pipe, inputs, edit_mask=TWO, edit_region=True, edit_region_margin=MARGIN, edit_region_split=2, capture_graph="step")
    assert pipe._graphed.replays >= 1
    _check_a_against_b(a, _call_b(_pipe(model), inputs, SPLIT, (0, FS)), inputs, SPLIT, (0, FS))


def test_g_malformed_calls_raise(model, inputs):
    pipe = _pipe(model)
    with pytest.raises(ValueError, match="edit_region_split extends edit_region=True"):
        _call_a(pipe, inputs, edit_mask=TWO, edit_region_split=2)
    with pytest.raises(ValueError, match="edit_region=True: the region is where `edit_mask` is"):
        _call_a(pipe, inputs, edit_region=True, edit_region_split=2)
    for bad in (1, 9, 0, -2, 2.0, True, "2", (2,)):
        with pytest.raises(ValueError, match="edit_region_split"):
            _call_a(pipe, inputs, edit_mask=TWO, edit_region=True, edit_region_split=bad)
    with pytest.raises(ValueError, match="edit_region_split with edit_region_follow"):
        _call_a(pipe, inputs, edit_mask=TWO, edit_region=True, edit_region_split=2, edit_region_follow=0)
    with pytest.raises(ValueError, match="edit_region_split with edit_region_vae_halo"):
        _call_a(pipe, inputs, edit_mask=TWO, edit_region=True, edit_region_split=2, edit_region_vae_halo=16)
    with pytest.raises(ValueError, match="edit_mask is empty"):
        _call_a(pipe, inputs, edit_mask=np.zeros((17, 128, 192), np.uint8), edit_region=True, edit_region_split=2)
