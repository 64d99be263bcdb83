"""Edit region, a mask of separate objects split into boxes (CPU): the definition ``reference_mask_spans`` on hand-written masks, the
rule ``region_split_plan`` -- its properties over a seeded sweep against a brute-force restatement that works on the mask's cells, not
on spans -- and the torch definitions ``reference_region_crop_split`` / ``reference_region_restore_split`` against K' calls of the
frames forms and an ownership mask written out in plain torch.  DESIGN.md 13.6."""
import itertools

import numpy as np
import pytest
import torch

from videocof_amd import (RegionPlan, SplitPlan, reference_mask_bounds, reference_mask_spans, reference_region_crop_frames,
                          reference_region_crop_split, reference_region_restore_frames, reference_region_restore_split, region_plan,
                          region_split_plan)
from videocof_amd.edit_region import region_split_count, spans_bounds

EMPTY_TEXT = "edit_mask is empty"


def _weights(h, w, rects, frames=1, samples=1):
    """uint8 [samples, frames, h, w]: 200 on every rectangle (sample, frame, y0, y1, x0, x1), inclusive."""
    a = torch.zeros(samples, frames, h, w, dtype=torch.uint8)
    for b, f, y0, y1, x0, x1 in rects:
        a[b, f, y0:y1 + 1, x0:x1 + 1] = 200
    return a


# ------------------------------------------------------------------------------------------------ the spans
def test_spans_of_hand_written_masks():
    h, w = 4, 6
    s = reference_mask_spans(torch.zeros(1, 2, h, w, dtype=torch.uint8))                   # empty frames
    assert s.dtype == torch.int16 and s.shape == (2, h + w, 2)
    assert s[:, :h].tolist() == [[[w, -1]] * h] * 2 and s[:, h:].tolist() == [[[h, -1]] * w] * 2
    s = reference_mask_spans(_weights(h, w, [(0, 0, 2, 2, 5, 5)]))                          # one cell, the last column
    assert s[0, :h].tolist() == [[w, -1], [w, -1], [5, 5], [w, -1]]
    assert s[0, h:].tolist() == [[h, -1]] * 5 + [[2, 2]]
    s = reference_mask_spans(torch.full((1, 1, h, w), 1, dtype=torch.uint8))                # a full frame (any non-zero weight counts)
    assert s[0, :h].tolist() == [[0, w - 1]] * h and s[0, h:].tolist() == [[0, h - 1]] * w
    # a row that crosses two objects (of two samples): its span covers the gap; frame 1 is empty
    s = reference_mask_spans(_weights(h, w, [(0, 0, 0, 1, 0, 1), (1, 0, 1, 3, 4, 5)], frames=2, samples=2))
    assert s[0, :h].tolist() == [[0, 1], [0, 5], [4, 5], [4, 5]]
    assert s[0, h:].tolist() == [[0, 1], [0, 1], [h, -1], [h, -1], [1, 3], [1, 3]]
    assert s[1, :h].tolist() == [[w, -1]] * h


def test_a_frames_bounds_are_the_min_and_max_of_its_spans():
    rng = np.random.default_rng(3)
    for _ in range(20):
        h, w = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        a = torch.from_numpy((rng.random((2, 3, h, w)) < 0.15).astype(np.uint8) * 9)
        a[:, 1] = 0
        assert spans_bounds(reference_mask_spans(a), (h, w)).tolist() == reference_mask_bounds(a).tolist()
    with pytest.raises(ValueError, match="uint8"):
        reference_mask_spans(torch.zeros(1, 1, 2, 2))
    with pytest.raises(ValueError, match="32768"):
        reference_mask_spans(torch.zeros(1, 1, 1, 32768, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ the rule, restated on cells
def _axis_naive(lo, hi, F, m, T, p, size=None):
    lo_a, hi_a = lo // p * p, (hi // p + 1) * p
    want = min(F, hi_a - lo_a + 2 * m)
    if size is None:
        return want
    start = lo_a - m - ((size - want) // (2 * p)) * p
    return min(max(start, 0), F - size)


def _brute_force(cells, frame, margin, tile, p, K):
    """The rule on the set of non-zero cells (y, x): every (axis, k) with the gaps the rule keeps -- found by enumerating ALL subsets
    of k - 1 gaps and taking the one whose widths, widest first, are lexicographically largest, the earliest positions among equals --
    and for every such candidate the boxes from the cells of each band.  Returns the list of (cost, k, axis, h, w, boxes, cuts) in
    the order of the tie rules (smaller k, then columns)."""
    out = []
    for k in range(1, K + 1):
        for axis in (1, 0):
            F, m, T = frame[axis], margin[axis], None if tile is None else tile[axis]
            Fo, mo, To = frame[1 - axis], margin[1 - axis], None if tile is None else tile[1 - axis]
            occupied = sorted({c[axis] // p for c in cells})
            bands = []                                                         # runs of occupied patches
            for i in occupied:
                if bands and bands[-1][1] == i - 1:
                    bands[-1][1] = i
                else:
                    bands.append([i, i])
            gaps = [bands[g + 1][0] - bands[g][1] - 1 for g in range(len(bands) - 1)]
            if k - 1 > len(gaps):
                continue
            keep = max(itertools.combinations(range(len(gaps)), k - 1),
                       key=lambda c: (sorted((gaps[g] for g in c), reverse=True), [-g for g in sorted(c, key=lambda g: (-gaps[g], g))]))
            groups, first = [], 0
            for g in sorted(keep):
                groups.append((first, g))
                first = g + 1
            groups.append((first, len(bands) - 1))
            cuts = [0] + [p * ((bands[b][1] + 1 + bands[b + 1][0]) // 2) for _, b in groups[:-1]] + [F]
            members = [[c for c in cells if bands[a][0] <= c[axis] // p <= bands[b][1]] for a, b in groups]
            ext = [(min(c[axis] for c in ms), max(c[axis] for c in ms), min(c[1 - axis] for c in ms), max(c[1 - axis] for c in ms))
                   for ms in members]
            want = max(_axis_naive(e[0], e[1], F, m, T, p) for e in ext)
            wanto = max(_axis_naive(e[2], e[3], Fo, mo, To, p) for e in ext)
            size = min(T, F) if T is not None and want <= T else want
            sizeo = min(To, Fo) if To is not None and wanto <= To else wanto
            starts = [(_axis_naive(e[0], e[1], F, m, T, p, size), _axis_naive(e[2], e[3], Fo, mo, To, p, sizeo)) for e in ext]
            h, w = (sizeo, size) if axis == 1 else (size, sizeo)
            boxes = [(so, s) if axis == 1 else (s, so) for s, so in starts]
            out.append((k * h * w, k, axis, h, w, boxes, cuts))
            if k == 1:
                break                                                          # k = 1 is the same for both axes
    return out


def _random_mask(rng):
    H, W = int(rng.integers(4, 25)), int(rng.integers(4, 41))
    on = np.zeros((H, W), bool)
    for _ in range(int(rng.integers(1, 6))):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        on[y:y + int(rng.integers(1, 5)), x:x + int(rng.integers(1, 7))] = True
    return H, W, on


def _spans_of(on, frames=1):
    """The spans of a mask whose union over frames is ``on``: its cells dealt out over ``frames`` latent frames."""
    H, W = on.shape
    a = torch.zeros(1, frames, H, W, dtype=torch.uint8)
    for i, (y, x) in enumerate(np.argwhere(on)):
        a[0, i % frames, y, x] = 255
    return reference_mask_spans(a)


def test_the_plan_over_a_seeded_sweep():
    """About 200 masks of at most 24 x 40 cells.  `kept gaps` of the brute force are the ones the rule's own order fixes (the widest,
    of equal gaps the earlier one), found among all subsets; the cost must be the least over (axis, k) and the tie rules must hold."""
    rng = np.random.default_rng(20)
    split = 0
    for case in range(200):
        H, W, on = _random_mask(rng)
        p = int(rng.choice([1, 2, 2, 2]))
        margin = (p * int(rng.integers(0, 3)), p * int(rng.integers(0, 3)))
        tile = None if rng.random() < 0.5 else (p * int(rng.integers(2, 8)), p * int(rng.integers(2, 8)))
        K = int(rng.integers(2, 9))
        cells = [tuple(c) for c in np.argwhere(on).tolist()]
        plan = region_split_plan(_spans_of(on, frames=int(rng.integers(1, 4))), (H, W), margin, tile, p, max_regions=K)
        cands = _brute_force(cells, (H, W), margin, tile, p, K)
        cost, k, axis, h, w, boxes, cuts = min(cands, key=lambda c: c[0])       # min takes the first of equals: the tie rules' order
        if k == 1:
            bounds = [min(c[0] for c in cells), max(c[0] for c in cells), min(c[1] for c in cells), max(c[1] for c in cells)]
            assert plan == region_plan(bounds, (H, W), margin, tile, p) and isinstance(plan, RegionPlan), case
            assert plan.h * plan.w == cost and (plan.y0, plan.x0) == boxes[0]
            continue
        split += 1
        assert isinstance(plan, SplitPlan) and plan.origins.dtype == np.int32 and plan.cuts.dtype == np.int32, case
        assert (len(plan.origins) * plan.h * plan.w, len(plan.origins), plan.axis, plan.h, plan.w) == (cost, k, axis, h, w), case
        assert plan.origins.tolist() == [list(b) for b in boxes] and plan.cuts.tolist() == cuts, case
        F = (H, W)[axis]
        assert plan.cuts[0] == 0 and plan.cuts[-1] == F and (np.diff(plan.cuts) > 0).all() and (plan.cuts[1:-1] % p == 0).all()
        for y0, x0 in plan.origins:                                            # inside the frame, one size, on the patch grid
            assert 0 <= y0 and y0 + plan.h <= H and 0 <= x0 and x0 + plan.w <= W
            assert y0 % p == 0 or y0 == H - plan.h
            assert x0 % p == 0 or x0 == W - plan.w
        for y, x in cells:                                                     # every cell inside its band's box and what the band owns
            band = int(np.searchsorted(plan.cuts, (y, x)[axis], side="right")) - 1
            y0, x0 = plan.origins[band]
            assert y0 <= y < y0 + plan.h and x0 <= x < x0 + plan.w, (case, y, x)
    assert split >= 30                                                         # the sweep does reach the split path


def test_one_object_or_a_split_that_does_not_pay_is_region_plan():
    frame, margin = (24, 40), (2, 2)
    one = np.zeros(frame, bool)
    one[5:9, 10:16] = True
    for K in (2, 4, 8):
        assert region_split_plan(_spans_of(one), frame, margin, None, 2, max_regions=K) == region_plan([5, 8, 10, 15], frame, margin, None, 2)
    near = np.zeros(frame, bool)                                               # two objects a patch apart: with the margins two boxes
    near[4:8, 10:14] = near[4:8, 16:20] = True                                 # cost 2 * 8 * 8 = 128 cells, their union 8 * 14 = 112
    plan = region_split_plan(_spans_of(near), frame, margin, None, 2, max_regions=2)
    assert plan == RegionPlan(2, 8, 8, 14)


def test_the_axis_of_the_cut():
    frame, margin = (24, 40), (2, 2)
    stacked = np.zeros(frame, bool)
    stacked[1:4, 10:14] = stacked[18:22, 11:15] = True                         # one above the other: rows
    plan = region_split_plan(_spans_of(stacked), frame, margin, None, 2, max_regions=2)
    assert plan.axis == 0 and (plan.h, plan.w) == (8, 10) and plan.origins.tolist() == [[0, 8], [16, 8]]
    assert plan.cuts.tolist() == [0, 10, 24] and plan.enclosing() == RegionPlan(0, 8, 24, 10)
    assert plan.pixels() == ((0, 64, 64, 80), (128, 64, 64, 80))
    diagonal = np.zeros(frame, bool)
    diagonal[2:6, 2:6] = diagonal[16:20, 30:34] = True                         # either axis costs the same: columns win the tie
    plan = region_split_plan(_spans_of(diagonal), frame, margin, None, 2, max_regions=2)
    assert plan.axis == 1 and (plan.h, plan.w) == (8, 8) and plan.origins.tolist() == [[0, 0], [14, 28]]
    assert plan.cuts.tolist() == [0, 18, 40]
    three = diagonal.copy()
    three[8:12, 14:18] = True                                                  # K caps the boxes: the widest gap is kept, and the
                                                                               # lone band's box is centred on it: 16 - 2, 30 - 6
    assert len(region_split_plan(_spans_of(three), frame, (0, 0), None, 2, max_regions=3).origins) == 3
    two = region_split_plan(_spans_of(three), frame, (0, 0), None, 2, max_regions=2)
    assert two.axis == 1 and two.cuts.tolist() == [0, 24, 40] and two.origins.tolist() == [[2, 2], [14, 24]] and (two.h, two.w) == (10, 16)


def test_a_one_patch_gap_at_an_odd_cell():
    """Cells 0..4 and 7..9 of a row: patches 0..2 and 3..4 are occupied with patch 2 -- no gap; cells 0..3 and 7..9: patch 2 (cells
    4, 5) is the gap although the cells 4..6 are empty, and the cut is a patch boundary inside it."""
    frame = (4, 10)
    touching = np.zeros(frame, bool)
    touching[0, 0:5] = touching[0, 7:10] = True
    assert isinstance(region_split_plan(_spans_of(touching), frame, (0, 0), None, 2, max_regions=2), RegionPlan)
    gap = np.zeros(frame, bool)
    gap[0:2, 0:4] = gap[0:2, 7:10] = True
    plan = region_split_plan(_spans_of(gap), frame, (0, 0), None, 2, max_regions=2)
    assert plan.axis == 1 and plan.cuts.tolist() == [0, 4, 10] and (plan.h, plan.w) == (2, 4) and plan.origins.tolist() == [[0, 0], [0, 6]]
    wide = np.zeros((4, 14), bool)
    wide[0:2, 0:2] = wide[0:2, 9:14] = True                                    # patches 0 and 4..6: the gap is patches 1..3, the cut 2 * ((1 + 4) // 2)
    plan = region_split_plan(_spans_of(wide), (4, 14), (0, 0), None, 2, max_regions=2)
    assert plan.cuts.tolist() == [0, 4, 14] and plan.w == 6 and plan.origins.tolist() == [[0, 0], [0, 8]]


def test_with_a_tile_the_boxes_take_its_size():
    frame = (24, 40)
    diagonal = np.zeros(frame, bool)
    diagonal[2:6, 2:6] = diagonal[16:20, 30:34] = True
    plan = region_split_plan(_spans_of(diagonal), frame, (2, 2), (12, 16), 2, max_regions=2)
    assert (plan.h, plan.w) == (12, 16) and plan.origins.tolist() == [[0, 0], [12, 24]]       # the spare context half on either side, clamped
    # the union does not fit the tile, so `region_plan` keeps its own size: 22 x 36 cells against 2 x 12 x 16
    assert region_plan([2, 19, 2, 33], frame, (2, 2), (12, 16), 2) == RegionPlan(0, 0, 22, 36)
    single = region_split_plan(_spans_of(diagonal[:8, :8]), (8, 8), (2, 2), (12, 16), 2, max_regions=2)
    assert single == RegionPlan(0, 0, 8, 8)


def test_argument_errors_raise():
    frame = (6, 8)
    on = np.zeros(frame, bool)
    on[1, 1] = True
    good = _spans_of(on)
    with pytest.raises(ValueError, match=EMPTY_TEXT):
        region_split_plan(_spans_of(np.zeros(frame, bool)), frame, (0, 0), None, 2, max_regions=2)
    for K in (1, 9, 0, True, 2.0, "2", None):
        with pytest.raises(ValueError, match="max_regions"):
            region_split_plan(good, frame, (0, 0), None, 2, max_regions=K)
        with pytest.raises(ValueError, match="edit_region_split"):
            region_split_count(K)
    assert [region_split_count(K) for K in (2, 8, np.int64(3))] == [2, 8, 3]
    for spans in (good[:, :-1], good[0], good.float(), torch.zeros(0, 14, 2, dtype=torch.int16)):
        with pytest.raises(ValueError, match="spans"):
            region_split_plan(spans, frame, (0, 0), None, 2, max_regions=2)
    with pytest.raises(ValueError, match="margin_cells"):
        region_split_plan(good, frame, (1, 0), None, 2, max_regions=2)
    with pytest.raises(ValueError, match="tile_cells"):
        region_split_plan(good, frame, (0, 0), (3, 4), 2, max_regions=2)
    with pytest.raises(ValueError, match="patch"):
        region_split_plan(good, frame, (0, 0), None, 0, max_regions=2)
    bad = good.clone()
    bad[0, 1] = torch.tensor([1, 8])                                           # a span that leaves the frame's 8 columns
    with pytest.raises(ValueError, match="leave a frame"):
        region_split_plan(bad, frame, (0, 0), None, 2, max_regions=2)


# ------------------------------------------------------------------------------------------------ the crop and the restore
def _owned(k, cuts, axis, H, W):
    own = torch.zeros(H, W, dtype=torch.bool)
    for y in range(H):
        for x in range(W):
            own[y, x] = cuts[k] <= (y, x)[axis] < cuts[k + 1]
    return own


SPLITS = [  # (H, W, hr, wr, origins, cuts, axis): overlapping boxes, boxes that reach past what they own, K = 1, 2, 3, both axes
    (6, 16, 4, 8, [[0, 0], [2, 8]], [0, 6, 16], 1),
    (6, 16, 4, 8, [[1, 3], [2, 5]], [0, 7, 16], 1),
    (9, 7, 4, 5, [[0, 0], [2, 2], [5, 1]], [0, 3, 6, 9], 0),
    (6, 12, 6, 8, [[0, 4]], [0, 12], 1),
    (5, 7, 3, 5, [[0, 0], [1, 1], [2, 2]], [0, 2, 3, 7], 1),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8], ids=["fp32", "bf16", "u8"])
@pytest.mark.parametrize("H,W,hr,wr,origins,cuts,axis", SPLITS)
def test_the_definitions_agree_with_the_frames_forms_and_an_ownership_mask(H, W, hr, wr, origins, cuts, axis, dtype):
    g = torch.Generator().manual_seed(H * W)
    K, B, C = len(origins), 2, 2
    for cc, G, t0, n in ((3, 1, 0, 3), (3, 1, 1, 2), (4, 0, 3, 1), (2, 2, 0, 2)):
        full = torch.randint(1, 200, (B, C, 2 * cc + G, H, W), generator=g).to(dtype)
        runs = [(0, 2 * cc + G)] if (t0, n) == (0, cc) else [(t0, n)] + ([(cc, G)] if G else []) + [(cc + G + t0, n)]
        for clip in (False, True):
            got = reference_region_crop_split(full, runs, origins, cuts, axis, (hr, wr), clip=clip)
            assert got.shape == (K, B, C, 2 * n + G, hr, wr) and got.is_contiguous()
            for k, (y0, x0) in enumerate(origins):
                want = reference_region_crop_frames(full, runs, (y0, x0, hr, wr))
                if clip:
                    want = want * _owned(k, cuts, axis, H, W)[y0:y0 + hr, x0:x0 + wr].to(dtype)
                assert torch.equal(got[k], want), (k, clip)
        final = torch.randint(200, 250, (K * B, C, 2 * n + G, hr, wr), generator=g).to(dtype)
        src = full[:, :, :cc]
        got = reference_region_restore_split(src, final, origins, cuts, axis, (t0, n))
        want = torch.cat([src, src[:, :, :G], src], dim=2)
        for k, (y0, x0) in enumerate(origins):                                 # K calls of the frames form, each kept where band k owns
            one = reference_region_restore_frames(src, final[k * B:(k + 1) * B], (y0, x0), (t0, n))
            inside = torch.zeros(H, W, dtype=torch.bool)
            inside[y0:y0 + hr, x0:x0 + wr] = True
            take = inside & _owned(k, cuts, axis, H, W)
            want = torch.where(take, one, want)
        assert torch.equal(got, want)
        if K == 1:
            assert torch.equal(got, reference_region_restore_frames(src, final, origins[0], (t0, n)))
            assert torch.equal(reference_region_crop_split(full, runs, origins, cuts, axis, (hr, wr), clip=True)[0],
                               reference_region_crop_frames(full, runs, (*origins[0], hr, wr)))


def test_the_definitions_reject_malformed_boxes():
    x = torch.zeros(2, 3, 6, 8)
    ok = dict(origins=[[0, 0], [2, 4]], cuts=[0, 4, 8], axis=1, size=(4, 4))
    assert reference_region_crop_split(x, [(0, 3)], **ok).shape == (2, 2, 3, 4, 4)
    for change in (dict(origins=[[0, 0]] * 9, cuts=list(range(9)) + [8]), dict(origins=[[3, 0], [2, 4]]), dict(origins=[[0, 5], [2, 4]]),
                   dict(cuts=[0, 4, 4]), dict(cuts=[0, 5, 4]), dict(cuts=[1, 4, 8]), dict(cuts=[0, 4, 6]), dict(cuts=[0, 8]),
                   dict(axis=2), dict(axis=0), dict(size=(4,)), dict(origins=np.zeros((2, 2), np.float32))):
        with pytest.raises(ValueError):
            reference_region_crop_split(x, [(0, 3)], **{**ok, **change})
    src, state = torch.zeros(1, 2, 3, 6, 8), torch.zeros(2, 2, 7, 4, 4)
    assert reference_region_restore_split(src, state, ok["origins"], ok["cuts"], 1, (0, 3)).shape == (1, 2, 7, 6, 8)
    with pytest.raises(ValueError, match="state samples"):
        reference_region_restore_split(src, state[:1], ok["origins"], ok["cuts"], 1, (0, 3))
    with pytest.raises(ValueError, match="do not lie inside"):
        reference_region_restore_split(src, state, ok["origins"], ok["cuts"], 1, (2, 3))
    with pytest.raises(ValueError, match="cuts"):
        reference_region_restore_split(src, state, ok["origins"], [0, 8, 8], 1, (0, 3))
