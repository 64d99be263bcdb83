"""Edit region: run the denoise loop only where the edit mask is.  The rule (host arithmetic, no GPU needed) and torch
restatements of the three device passes.

With ``edit_mask`` the loop already pins everything outside the mask to the source, so a call with ``edit_region=True`` crops the loop
state once to a rectangle around the mask's non-zero latent weights, runs the ordinary loop on that smaller clip and puts the result
back into the source latents once.  ``region_plan`` fixes the rectangle; ``reference_mask_bounds`` / ``reference_region_crop`` /
``reference_region_restore`` state what ``wan_mask_bounds`` / ``wan_region_crop`` / ``wan_region_restore`` compute (ops.mask_bounds,
ops.region_crop, ops.region_restore), bit for bit.

The time axis is cropped only where the call gives ``edit_region_time_margin``: ``region_time_plan`` then fixes ONE contiguous range of
latent frames around the frames the mask touches, and ``reference_region_crop_frames`` / ``reference_region_restore_frames`` state what
``wan_region_crop_frames`` / ``wan_region_restore_frames`` compute.  The model then sees a clip whose first latent frame is not the
clip's first (the causal VAE's special frame) -- as every temporal context window but the first does already: the same
class of approximation, opt-in, lossy, no quality claim.

With ``edit_region_vae_halo`` the VAE, too, sees only a part of the frame: ``region_vae_box`` fixes the BOX it encodes and decodes (the
region's rectangle and a halo), ``reference_frames_box_to_video`` / ``reference_video_box_stitch`` state what
``wan_frames_u8_box_to_video`` / ``wan_video_box_stitch_u8`` compute on either side of it (ops.frames_u8_box_to_video,
ops.video_box_stitch_u8), bit for bit and byte for byte: the frames that come back are the source's own bytes outside the rectangle.

With ``edit_region_follow`` the rectangle keeps ONE size and takes a corner per latent frame: ``region_track_plan`` fixes the corners
from the same per-frame bounds (a sliding union over ``span`` latent frames is the only smoothing), and ``reference_region_crop_track``
/ ``reference_region_restore_track`` state what ``wan_region_crop_track`` / ``wan_region_restore_track`` compute.  Source frame f,
target frame f and the weights of frame f are cropped at the same corner, so the loop's pin to the source stays exact; the model sees
a stabilised crop whose background slides: opt-in, lossy, no quality claim.

With ``edit_region_split`` a mask of separate objects is split into at most K bands along ONE axis, every band gets a box of ONE common
size, and the boxes run as samples of the ordinary loop: ``reference_mask_spans`` states what ``wan_mask_spans`` brings to the host (per
row and per column the extent of the non-zero weights), ``region_split_plan`` fixes the boxes and the part of the frame each band owns,
and ``reference_region_crop_split`` / ``reference_region_restore_split`` state what ``wan_region_crop_split`` /
``wan_region_restore_split`` compute.  A box sees only itself; opt-in, lossy, no quality claim.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

__all__ = ["RegionPlan", "region_plan", "region_margin_cells", "reference_mask_bounds", "reference_region_crop",
           "reference_region_restore", "TimeRegion", "region_time_plan", "region_time_margin_frames", "reference_region_crop_frames",
           "reference_region_restore_frames", "region_vae_box", "region_vae_halo_cells", "region_stitch_feather",
           "reference_frames_box_to_video", "reference_video_box_stitch", "stitch_weights", "TrackPlan", "region_track_plan",
           "region_follow_frames", "reference_region_crop_track", "reference_region_restore_track", "REGION_TRACK_MAX_FRAMES",
           "SplitPlan", "region_split_plan", "region_split_count", "spans_bounds", "reference_mask_spans",
           "reference_region_crop_split", "reference_region_restore_split", "REGION_SPLIT_MAX"]

REGION_MARGIN_UNIT = 16         # pixels: the VAE's spatial ratio 8 times the patch 2 -- a margin keeps the region on the patch grid
REGION_TRACK_MAX_FRAMES = 512   # WAN_REGION_TRACK_MAX_FRAMES: the frames a table of corners may have (it travels in the kernel's arguments)
REGION_SPLIT_MAX = 8            # WAN_REGION_SPLIT_MAX: the boxes a split may have (their table travels in the kernel's arguments)


class RegionPlan(NamedTuple):
    """The rectangle the loop runs on, in LATENT cells: rows [y0, y0 + h), columns [x0, x0 + w) of every frame."""
    y0: int
    x0: int
    h: int
    w: int

    def pixels(self, ratio: int = 8) -> Tuple[int, int, int, int]:
        """(y, x, h, w) in pixels."""
        return self.y0 * ratio, self.x0 * ratio, self.h * ratio, self.w * ratio


def _axis(lo: int, hi: int, F: int, m: int, T: Optional[int], p: int) -> Tuple[int, int, int]:
    """One axis of the rule: (start, size, want)."""
    lo_a, hi_a = lo // p * p, (hi // p + 1) * p                     # the bounds on the patch grid, [lo', hi')
    want = min(F, hi_a - lo_a + 2 * m)
    size = min(T, F) if T is not None and want <= T else want       # one tile, the trained size, with as much context as fits
    start = lo_a - m - ((size - want) // (2 * p)) * p               # the spare context, half on either side, on the grid
    return min(max(start, 0), F - size), size, want


def _plan_args(who: str, bounds, frame_cells, margin_cells, tile_cells, patch):
    """The argument checks of ``region_plan`` and ``region_track_plan``: (bounds int64 [rows, 4], p, [(H, W), (my, mx), (Ty, Tx)])."""
    b = np.asarray(bounds.cpu() if torch.is_tensor(bounds) else bounds, dtype=np.int64).reshape(-1, 4)
    p = int(patch)
    if p < 1:
        raise ValueError(f"{who}: patch={patch!r} (>= 1)")
    pairs = []
    for name, v in (("frame_cells", frame_cells), ("margin_cells", margin_cells), ("tile_cells", tile_cells)):
        if v is None and name == "tile_cells":
            pairs.append((None, None))
            continue
        if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) != 2 or any(
                isinstance(e, bool) or not isinstance(e, (int, np.integer)) for e in v):
            raise ValueError(f"{who}: {name}={v!r} is not a pair (rows, columns) of latent cell counts")
        if name == "frame_cells":
            if any(int(e) < 1 for e in v):
                raise ValueError(f"{who}: frame_cells={tuple(v)!r}: each at least 1")
        elif any(int(e) < (0 if name == "margin_cells" else p) or int(e) % p for e in v):
            raise ValueError(f"{who}: {name}={tuple(v)!r}: each a {'non-negative' if name == 'margin_cells' else 'positive'} "
                             f"multiple of the patch {p}")
        pairs.append((int(v[0]), int(v[1])))
    return b, p, pairs


def region_plan(bounds, frame_cells, margin_cells, tile_cells=None, patch: int = 2) -> RegionPlan:
    """The region of a mask whose non-zero latent weights have the inclusive ``bounds`` = (y_lo, y_hi, x_lo, x_hi) -- one such row, or one
    per latent frame as ``mask_bounds`` returns them ([Fs, 4]; the union is taken, rows of an empty frame, (h, -1, w, -1), drop out).
    Everything in LATENT cells: ``frame_cells`` = (H, W), ``margin_cells`` = (rows, columns) of context kept around the bounds,
    ``tile_cells`` = the (rows, columns) of ``spatial_window`` or None, ``patch`` = the DiT's spatial patch.  Per axis, with lo, hi the
    bounds, F the frame's extent, p the patch, m the margin and T the tile's extent or None:

        lo' = lo // p * p,  hi' = (hi // p + 1) * p,  want = min(F, hi' - lo' + 2 m)
        size  = min(T, F)  if T is given and want <= T  (one tile: the trained size, with as much context as fits)  else  want
        start = clamp(lo' - m - ((size - want) // (2 p)) * p, 0, F - size)

    Every region lies inside the frame and contains [lo' - m, hi' + m) clipped to the frame; m and T must be multiples of p, and where
    F is one too (every frame the model takes whole) the region's sides are multiples of p and it lies on the frame's own patch grid.
    (A frame of 135 rows, 1080 pixels, is none: it only runs as ``spatial_window`` tiles, which start anywhere, and so does a region
    of it.)  An empty mask raises ``ValueError``."""
    b, p, ((H, W), (my, mx), (Ty, Tx)) = _plan_args("region_plan", bounds, frame_cells, margin_cells, tile_cells, patch)
    b = b[(b[:, 1] >= b[:, 0]) & (b[:, 3] >= b[:, 2])]
    if b.shape[0] == 0:
        raise ValueError("edit_mask is empty (every latent weight is zero): there is no region to run the loop on")
    y_lo, y_hi, x_lo, x_hi = int(b[:, 0].min()), int(b[:, 1].max()), int(b[:, 2].min()), int(b[:, 3].max())
    if y_lo < 0 or y_hi >= H or x_lo < 0 or x_hi >= W:
        raise ValueError(f"region_plan: bounds rows [{y_lo}, {y_hi}] x columns [{x_lo}, {x_hi}] leave a frame of {H} x {W} cells")
    y0, h, _ = _axis(y_lo, y_hi, H, my, Ty, p)
    x0, w, _ = _axis(x_lo, x_hi, W, mx, Tx, p)
    return RegionPlan(y0, x0, h, w)


def region_margin_cells(margin, ratio: int = 8) -> Tuple[int, int]:
    """The pipeline's ``edit_region_margin`` = (rows, columns) in PIXELS as latent cells; each a non-negative multiple of 16 pixels (the
    VAE's spatial ratio 8 times the patch 2), which keeps the region on the patch grid."""
    if isinstance(margin, (str, bytes)) or not hasattr(margin, "__len__") or len(margin) != 2:
        raise ValueError(f"edit_region_margin={margin!r} is not a pair (rows, columns) of pixel counts")
    for e in margin:
        if isinstance(e, bool) or not isinstance(e, (int, np.integer)):
            raise ValueError(f"edit_region_margin={tuple(margin)!r}: {e!r} is not an integer pixel count")
        if e < 0 or e % REGION_MARGIN_UNIT:
            raise ValueError(f"edit_region_margin={tuple(margin)!r}: {e} must be a non-negative multiple of {REGION_MARGIN_UNIT} pixels "
                             "(the VAE's spatial ratio 8 times the patch 2)")
    return int(margin[0]) // ratio, int(margin[1]) // ratio


class TrackPlan(NamedTuple):
    """The box that follows the mask, in LATENT cells: one size (h, w) for the clip and ``origins`` int32 [Fs, 2] = (y0_f, x0_f), the
    corner of source frame f's box."""
    h: int
    w: int
    origins: np.ndarray

    def pixels(self, ratio: int = 8):
        """((h, w), ((y_f, x_f), ...)) in pixels."""
        return (self.h * ratio, self.w * ratio), tuple((int(y) * ratio, int(x) * ratio) for y, x in self.origins)

    def enclosing(self) -> RegionPlan:
        """The rectangle that encloses every frame's box."""
        y0, x0 = (int(v) for v in self.origins.min(axis=0))
        y1, x1 = (int(v) for v in self.origins.max(axis=0))
        return RegionPlan(y0, x0, y1 - y0 + self.h, x1 - x0 + self.w)


def _track_axis(lo, hi, F: int, m: int, T: Optional[int], p: int) -> Tuple[np.ndarray, int]:
    """One axis of the rule for every frame at once: (starts int64 [Fs], size).  ``lo``, ``hi``: int64 [Fs], never empty."""
    lo_a, hi_a = lo // p * p, (hi // p + 1) * p
    want_f = np.minimum(F, hi_a - lo_a + 2 * m)
    want = int(want_f.max())
    size = min(T, F) if T is not None and want <= T else want
    start = lo_a - m - ((size - want_f) // (2 * p)) * p
    return np.clip(start, 0, F - size), size


def region_track_plan(bounds, frame_cells, margin_cells, tile_cells=None, patch: int = 2, span: int = 0) -> TrackPlan:
    """The box that FOLLOWS a mask whose non-zero latent weights have the per-frame ``bounds`` [Fs, 4] of ``mask_bounds``: one size for
    the whole clip, one corner per latent frame.  The arguments are ``region_plan``'s, and ``span`` >= 0, in latent frames:

        U_f = the union of the non-empty rows bounds[g] with |g - f| <= span                                   (the sliding union)
        a frame whose U_f is empty takes the U of the nearest frame whose U is not (the earlier one on a tie)

    and per axis and frame, with lo_f, hi_f taken from U_f and F, p, m, T as in ``region_plan``:

        lo'_f = lo_f // p * p,  hi'_f = (hi_f // p + 1) * p,  want_f = min(F, hi'_f - lo'_f + 2 m),  want = max over f of want_f
        size    = min(T, F)  if T is given and want <= T  else  want
        start_f = clamp(lo'_f - m - ((size - want_f) // (2 p)) * p, 0, F - size)

    Every box lies inside the frame; box f contains [lo'_f - m, hi'_f + m) clipped to the frame; corners are on the patch grid except
    where the clamp to F - size moves them off it on a frame that is no multiple of p, as in ``region_plan``.  The span is the only
    smoothing: a larger one gives a larger, calmer box, and span >= Fs - 1 is ``region_plan`` exactly, on every frame.  An empty mask
    raises ``ValueError``."""
    who = "region_track_plan"
    b, p, ((H, W), (my, mx), (Ty, Tx)) = _plan_args(who, bounds, frame_cells, margin_cells, tile_cells, patch)
    if isinstance(span, bool) or not isinstance(span, (int, np.integer)) or span < 0:
        raise ValueError(f"{who}: span={span!r}: an integer >= 0, in latent frames")
    Fs, s = b.shape[0], int(span)
    on = (b[:, 1] >= b[:, 0]) & (b[:, 3] >= b[:, 2])
    if not on.any():
        raise ValueError("edit_mask is empty (every latent weight is zero): there is no region to run the loop on")
    y_lo, y_hi, x_lo, x_hi = int(b[on, 0].min()), int(b[on, 1].max()), int(b[on, 2].min()), int(b[on, 3].max())
    if y_lo < 0 or y_hi >= H or x_lo < 0 or x_hi >= W:
        raise ValueError(f"{who}: bounds rows [{y_lo}, {y_hi}] x columns [{x_lo}, {x_hi}] leave a frame of {H} x {W} cells")
    u = np.zeros((Fs, 4), np.int64)
    full = np.zeros(Fs, bool)
    for f in range(Fs):
        near = b[max(0, f - s):f + s + 1][on[max(0, f - s):f + s + 1]]
        if near.shape[0]:
            u[f], full[f] = (near[:, 0].min(), near[:, 1].max(), near[:, 2].min(), near[:, 3].max()), True
    have = np.flatnonzero(full)
    for f in np.flatnonzero(~full):
        u[f] = u[have[np.argmin(np.abs(have - f))]]          # argmin takes the first of equals: the earlier frame on a tie
    ys, h = _track_axis(u[:, 0], u[:, 1], H, my, Ty, p)
    xs, w = _track_axis(u[:, 2], u[:, 3], W, mx, Tx, p)
    return TrackPlan(h, w, np.stack([ys, xs], axis=1).astype(np.int32))


def region_follow_frames(follow, ratio: int = 4) -> int:
    """The pipeline's ``edit_region_follow`` in PIXEL frames as the ``span`` of ``region_track_plan`` in latent frames: a non-negative
    multiple of the VAE's temporal ratio."""
    if isinstance(follow, bool) or not isinstance(follow, (int, np.integer)):
        raise ValueError(f"edit_region_follow={follow!r} is not an integer count of pixel frames")
    if follow < 0 or follow % ratio:
        raise ValueError(f"edit_region_follow={follow} must be a non-negative multiple of {ratio} pixel frames (the VAE's temporal ratio)")
    return int(follow) // ratio


class SplitPlan(NamedTuple):
    """The boxes of a mask of separate objects, in LATENT cells: ``axis`` = the axis the frame is cut along (1: columns, the cuts are
    column indices; 0: rows), one size (h, w) for all boxes, ``origins`` int32 [K', 2] = (y0_k, x0_k), and ``cuts`` int32 [K' + 1]:
    band k OWNS [cuts[k], cuts[k + 1]) on the cut axis and everything on the other one."""
    axis: int
    h: int
    w: int
    origins: np.ndarray
    cuts: np.ndarray

    def pixels(self, ratio: int = 8):
        """((y, x, h, w), ...) in pixels, one per box."""
        return tuple((int(y) * ratio, int(x) * ratio, self.h * ratio, self.w * ratio) for y, x in self.origins)

    def enclosing(self) -> RegionPlan:
        """The rectangle that encloses every box."""
        y0, x0 = (int(v) for v in self.origins.min(axis=0))
        y1, x1 = (int(v) for v in self.origins.max(axis=0))
        return RegionPlan(y0, x0, y1 - y0 + self.h, x1 - x0 + self.w)


def _spans_array(spans, H: int, W: int, who: str) -> np.ndarray:
    s = np.asarray(spans.cpu() if torch.is_tensor(spans) else spans)
    if s.ndim != 3 or s.shape[1:] != (H + W, 2) or s.dtype.kind not in "iu" or s.shape[0] < 1:
        raise ValueError(f"{who}: spans = integer [Fs, {H} + {W}, 2] for a frame of {H} x {W} cells (mask_spans), got {s.dtype} {s.shape}")
    return s.astype(np.int64)


def spans_bounds(spans, frame_cells) -> np.ndarray:
    """The per-frame bounds int32 [Fs, 4] = (y_lo, y_hi, x_lo, x_hi) of ``mask_bounds`` out of the spans of ``mask_spans``: a frame's
    bounds are the min and max of its spans; (h, -1, w, -1) for a frame without a non-zero weight."""
    H, W = int(frame_cells[0]), int(frame_cells[1])
    s = _spans_array(spans, H, W, "spans_bounds")
    rows, cols = s[:, :H], s[:, H:]
    return np.stack([cols[:, :, 0].min(axis=1), cols[:, :, 1].max(axis=1), rows[:, :, 0].min(axis=1), rows[:, :, 1].max(axis=1)],
                    axis=1).astype(np.int32)


def _split_axis(lo, hi, F: int, m: int, T: Optional[int], p: int) -> Tuple[np.ndarray, int]:
    """One axis of the rule for every band at once: (starts int64 [bands], size).  ``_axis`` with want = the largest band's."""
    lo_a, hi_a = lo // p * p, (hi // p + 1) * p
    want_b = np.minimum(F, hi_a - lo_a + 2 * m)
    want = int(want_b.max())
    size = min(T, F) if T is not None and want <= T else want
    start = lo_a - m - ((size - want_b) // (2 * p)) * p
    return np.clip(start, 0, F - size), size


def _split_candidate(lo, hi, F: int, keep, p: int):
    """The bands of one axis with the gaps ``keep`` kept and every other one merged across.  ``lo``, ``hi``: int64 [F], per cell of the
    cut axis the union span on the OTHER axis (hi < lo: the cell is empty).  Returns (cut-axis bounds int64 [k, 2], other-axis bounds
    int64 [k, 2], cuts int64 [k + 1]) -- or the runs of occupied patches and the gaps between them where ``keep`` is None."""
    on = hi >= lo
    patches = -(-F // p)
    occupied = np.array([on[i * p:(i + 1) * p].any() for i in range(patches)])
    edges = np.flatnonzero(np.diff(np.concatenate([[False], occupied, [False]]).astype(np.int8)))
    first, last = edges[0::2], edges[1::2] - 1               # the bands: runs [first_i, last_i] of occupied patches
    if keep is None:
        return first, last
    keep = sorted(keep)                                      # gap g lies between band g and band g + 1
    a = np.array([0] + [g + 1 for g in keep])                # the first band of every merged band
    b = np.array(keep + [len(first) - 1])                    # and its last
    cut_b, other_b = [], []
    for i, j in zip(a, b):
        cells = np.arange(first[i] * p, min((last[j] + 1) * p, F))
        cells = cells[on[cells]]
        cut_b.append((cells[0], cells[-1]))
        other_b.append((lo[cells].min(), hi[cells].max()))
    cuts = [0] + [p * ((last[j] + 1 + first[j + 1]) // 2) for j in b[:-1]] + [F]
    return np.array(cut_b, np.int64), np.array(other_b, np.int64), np.array(cuts, np.int64)


def region_split_plan(spans, frame_cells, margin_cells, tile_cells=None, patch: int = 2, max_regions: int = 2):
    """The boxes of a mask of SEPARATE objects, from the ``spans`` int16 [Fs, h + w, 2] of ``mask_spans``: at most ``max_regions`` (2 to 8)
    bands along ONE axis, columns or rows, and a box of ONE common size for every band.  The other arguments are ``region_plan``'s.

        1. The union over frames is taken: per row the span of its non-zero columns, per column the span of its non-zero rows.
        2. Per axis, patch i is occupied if any cell i p .. i p + p - 1 is; runs of occupied patches are the bands, runs of empty ones
           between them the gaps.
        3. For k = 1 .. min(max_regions, bands) the k - 1 widest gaps are kept (of equal gaps the earlier one) and the others merged
           across.
        4. A band's bounds on the cut axis are its first and last occupied cell; on the other axis the min and max of the spans of its
           rows or columns -- exact for a cut along one axis.
        5. Per axis, with lo_b, hi_b a band's bounds and F, p, m, T as in ``region_plan``:
               lo'_b = lo_b // p * p,  hi'_b = (hi_b // p + 1) * p,  want_b = min(F, hi'_b - lo'_b + 2 m),  want = max over b of want_b
               size    = min(T, F)  if T is given and want <= T  else  want
               start_b = clamp(lo'_b - m - ((size - want_b) // (2 p)) * p, 0, F - size)
        6. A candidate costs k * h * w cells; the cheapest over (axis, k) is taken, ties go to the smaller k, then to columns.
        7. Between band i - 1 and band i the cut is p * ((last patch of i - 1 + 1 + first patch of i) // 2): a patch boundary inside
           the gap.  cuts[0] = 0, cuts[K'] = F.  Band i owns [cuts[i], cuts[i + 1]) on the cut axis, everything on the other.

    k = 1 is the same for both axes and IS ``region_plan`` of the bounds: a mask of one object, or one whose split does not pay, returns
    that ``RegionPlan``; otherwise a ``SplitPlan``.  Boxes may overlap and may reach past what their band owns (context); all of a
    band's mask lies inside both its box and what it owns.  Keeping the widest gaps is a rule, not a search: another choice of gaps
    can be cheaper.  An empty mask raises ``ValueError``."""
    who = "region_split_plan"
    _, p, ((H, W), (my, mx), (Ty, Tx)) = _plan_args(who, np.zeros((0, 4)), frame_cells, margin_cells, tile_cells, patch)
    K = region_split_count(max_regions, who + ": max_regions")
    s = _spans_array(spans, H, W, who)
    lo, hi = s[:, :, 0].min(axis=0), s[:, :, 1].max(axis=0)                    # the union over frames
    if not (hi >= lo).any():
        raise ValueError("edit_mask is empty (every latent weight is zero): there is no region to run the loop on")
    if lo[:H][hi[:H] >= lo[:H]].min() < 0 or hi[:H].max() >= W or lo[H:][hi[H:] >= lo[H:]].min() < 0 or hi[H:].max() >= H:
        raise ValueError(f"{who}: the spans leave a frame of {H} x {W} cells")
    single = region_plan(spans_bounds(s, (H, W)), (H, W), (my, mx), tile_cells, p)
    best, best_cost = single, single.h * single.w
    # (axis 1: the cut runs along the columns, whose spans are rows; axis 0: along the rows, whose spans are columns)
    axes = {1: (lo[H:], hi[H:], W, mx, Tx, H, my, Ty), 0: (lo[:H], hi[:H], H, my, Ty, W, mx, Tx)}
    gaps = {}
    for axis, (alo, ahi, F, _, _, _, _, _) in axes.items():
        first, last = _split_candidate(alo, ahi, F, None, p)
        width = first[1:] - last[:-1] - 1
        gaps[axis] = sorted(range(len(width)), key=lambda g: (-width[g], g))       # widest first, of equal gaps the earlier one
    for k in range(2, K + 1):
        for axis in (1, 0):
            alo, ahi, F, m, T, Fo, mo, To = axes[axis]
            if k - 1 > len(gaps[axis]):
                continue
            cut_b, other_b, cuts = _split_candidate(alo, ahi, F, gaps[axis][:k - 1], p)
            starts, size = _split_axis(cut_b[:, 0], cut_b[:, 1], F, m, T, p)
            ostarts, osize = _split_axis(other_b[:, 0], other_b[:, 1], Fo, mo, To, p)
            if k * size * osize < best_cost:
                (ys, h), (xs, w) = ((ostarts, osize), (starts, size)) if axis == 1 else ((starts, size), (ostarts, osize))
                best, best_cost = SplitPlan(axis, h, w, np.stack([ys, xs], axis=1).astype(np.int32), cuts.astype(np.int32)), k * size * osize
    return best


def region_split_count(split, name: str = "edit_region_split") -> int:
    """The pipeline's ``edit_region_split``: an integer count of boxes from 2 to 8."""
    if isinstance(split, bool) or not isinstance(split, (int, np.integer)) or not 2 <= split <= REGION_SPLIT_MAX:
        raise ValueError(f"{name}={split!r}: an integer from 2 to {REGION_SPLIT_MAX}, the most boxes the mask is split into")
    return int(split)


class TimeRegion(NamedTuple):
    """The frames the loop runs on, in LATENT frames of the source segment: [t0, t0 + n)."""
    t0: int
    n: int

    def pixels(self, ratio: int = 4) -> Tuple[int, int]:
        """(first pixel frame, pixel frame count): the causal VAE's first latent frame is one pixel frame, every other ``ratio``."""
        first = 0 if self.t0 == 0 else ratio * self.t0 - (ratio - 1)
        return first, ratio * (self.t0 + self.n - 1) - first + 1


def region_time_plan(bounds, frames: int, margin_frames: int, ground: int = 0) -> TimeRegion:
    """The frame range of a mask whose non-zero latent weights have the per-frame ``bounds`` [Fs, 4] of ``mask_bounds``.  With lo, hi
    the first and last non-empty row (y_hi >= y_lo and x_hi >= x_lo), Fs = ``frames`` the source segment's latent frames, m =
    ``margin_frames`` latent frames of context on either side and G = ``ground`` grounding frames:

        core = hi - lo + 1 + 2 m
        n    = min(Fs, max(core, 2, G))
        t0   = clamp(lo - m - max(n - core, 0) // 2, 0, Fs - n)

    The floor max(2, G) keeps the cropped clip a layout the model, ``window_plan`` (windows of at least 2 frames) and the restore
    (G <= n) accept.  The range lies inside the clip and contains [lo - m, hi + m] clipped to it.  It is NOT widened to the temporal
    window's length (unlike the one-tile rule in space): every length up to the window is a trained one, and attention grows with
    n squared.  An empty mask raises ``ValueError``."""
    b = np.asarray(bounds.cpu() if torch.is_tensor(bounds) else bounds, dtype=np.int64).reshape(-1, 4)
    for name, v, least in (("frames", frames, 1), ("margin_frames", margin_frames, 0), ("ground", ground, 0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
            raise ValueError(f"region_time_plan: {name}={v!r}: an integer >= {least}")
    Fs, m, G = int(frames), int(margin_frames), int(ground)
    if b.shape[0] != Fs:
        raise ValueError(f"region_time_plan: {b.shape[0]} rows of bounds for {Fs} latent frames")
    on = np.flatnonzero((b[:, 1] >= b[:, 0]) & (b[:, 3] >= b[:, 2]))
    if on.size == 0:
        raise ValueError("edit_mask is empty (every latent weight is zero): there is no region to run the loop on")
    lo, hi = int(on[0]), int(on[-1])
    core = hi - lo + 1 + 2 * m
    n = min(Fs, max(core, 2, G))
    t0 = lo - m - max(n - core, 0) // 2
    return TimeRegion(min(max(t0, 0), Fs - n), n)


def region_time_margin_frames(margin, ratio: int = 4) -> int:
    """The pipeline's ``edit_region_time_margin`` in PIXEL frames as latent frames: a non-negative multiple of the VAE's temporal
    ratio."""
    if isinstance(margin, bool) or not isinstance(margin, (int, np.integer)):
        raise ValueError(f"edit_region_time_margin={margin!r} is not an integer count of pixel frames")
    if margin < 0 or margin % ratio:
        raise ValueError(f"edit_region_time_margin={margin} must be a non-negative multiple of {ratio} pixel frames (the VAE's temporal ratio)")
    return int(margin) // ratio


def region_vae_box(region, frame_cells, halo_cells) -> RegionPlan:
    """The box the VAE encodes and decodes with ``edit_region_vae_halo``, in LATENT cells: the region's rectangle widened by
    ``halo_cells`` = (rows, columns) on every side and clamped to the frame ``frame_cells`` = (H, W).  Per axis

        b0 = max(0, start - hc),  b1 = min(F, start + size + hc)

    The box lies inside the frame and contains the region.  The pipeline's halo is a multiple of 16 pixels, so hc is a multiple of the
    patch 2 and the box lies on the frame's patch grid wherever the region does; planning the region inside the box
    (``region_plan`` on the bounds less the box's origin, with ``frame_cells`` = the box) then gives the same region less the box's
    origin.  (Not claimed where the frame is no multiple of the patch, 135 rows for 1080 pixels: the option works there too, the VAE
    needs multiples of 8 pixels only.)  No finite halo is exact: the VAE's receptive field is many 3 x 3 convolutions deep and its
    mid-block attention is global over the frame it sees, so every value is a guess."""
    if len(region) != 4:
        raise ValueError(f"region_vae_box: region = (y0, x0, h, w) in cells, got {region!r}")
    for name, v in (("frame_cells", frame_cells), ("halo_cells", halo_cells)):
        if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) != 2 or any(
                isinstance(e, bool) or not isinstance(e, (int, np.integer)) or e < (1 if name == "frame_cells" else 0) for e in v):
            raise ValueError(f"region_vae_box: {name}={v!r} is not a pair (rows, columns) of latent cell counts")
    y0, x0, h, w = _box(region, int(frame_cells[0]), int(frame_cells[1]), "region_vae_box")
    (H, W), (hy, hx) = (int(v) for v in frame_cells), (int(v) for v in halo_cells)
    by0, by1 = max(0, y0 - hy), min(H, y0 + h + hy)
    bx0, bx1 = max(0, x0 - hx), min(W, x0 + w + hx)
    return RegionPlan(by0, bx0, by1 - by0, bx1 - bx0)


def region_vae_halo_cells(halo, ratio: int = 8) -> int:
    """The pipeline's ``edit_region_vae_halo`` in PIXELS as latent cells: a non-negative multiple of 16 pixels (the VAE's spatial ratio
    8 times the patch 2), which keeps the box on the patch grid."""
    if isinstance(halo, bool) or not isinstance(halo, (int, np.integer)):
        raise ValueError(f"edit_region_vae_halo={halo!r} is not an integer pixel count")
    if halo < 0 or halo % REGION_MARGIN_UNIT:
        raise ValueError(f"edit_region_vae_halo={halo} must be a non-negative multiple of {REGION_MARGIN_UNIT} pixels (the VAE's spatial "
                         "ratio 8 times the patch 2)")
    return int(halo) // ratio


def region_stitch_feather(feather) -> int:
    """The pipeline's ``edit_region_stitch_feather``: a non-negative integer count of pixels."""
    if isinstance(feather, bool) or not isinstance(feather, (int, np.integer)) or feather < 0:
        raise ValueError(f"edit_region_stitch_feather={feather!r} is not a non-negative integer pixel count")
    return int(feather)


# ------------------------------------------------------------------------------------------------ the device passes, in torch
def reference_mask_bounds(weights: torch.Tensor) -> torch.Tensor:
    """``wan_mask_bounds`` in torch: weights uint8 [Bm, Fs, h, w] -> int32 [Fs, 4] = (y_lo, y_hi, x_lo, x_hi) per latent frame, the
    inclusive bounds of the non-zero weights over all samples; (h, -1, w, -1) for a frame without one."""
    if weights.dim() != 4 or weights.dtype != torch.uint8:
        raise ValueError(f"reference_mask_bounds: expected uint8 [Bm, Fs, h, w], got {weights.dtype} {tuple(weights.shape)}")
    _, Fs, h, w = weights.shape
    on = (weights != 0).any(dim=0)
    out = torch.empty((Fs, 4), dtype=torch.int32)
    for f in range(Fs):
        ys, xs = on[f].any(dim=1).nonzero().flatten(), on[f].any(dim=0).nonzero().flatten()
        out[f] = torch.tensor([int(ys[0]), int(ys[-1]), int(xs[0]), int(xs[-1])] if ys.numel() else [h, -1, w, -1], dtype=torch.int32)
    return out


def _box(region, H: int, W: int, who: str) -> Tuple[int, int, int, int]:
    if len(region) != 4:
        raise ValueError(f"{who}: region = (y0, x0, h, w) in cells, got {region!r}")
    y0, x0, hr, wr = (int(v) for v in region)
    if y0 < 0 or x0 < 0 or hr < 1 or wr < 1 or y0 + hr > H or x0 + wr > W:
        raise ValueError(f"{who}: the region [{y0}, {y0} + {hr}) x [{x0}, {x0} + {wr}) does not lie inside a frame of {H} x {W}")
    return y0, x0, hr, wr


def reference_region_crop(x: torch.Tensor, region) -> torch.Tensor:
    """``wan_region_crop`` in torch: the sub-box ``region`` = (y0, x0, h, w) of every frame of ``x`` [..., H, W], contiguous."""
    if x.dim() < 2:
        raise ValueError(f"reference_region_crop: expected [..., H, W], got {tuple(x.shape)}")
    y0, x0, hr, wr = _box(region, x.shape[-2], x.shape[-1], "reference_region_crop")
    return x[..., y0:y0 + hr, x0:x0 + wr].contiguous()


def reference_region_restore(source: torch.Tensor, state: torch.Tensor, origin) -> torch.Tensor:
    """``wan_region_restore`` in torch: ``source`` [B, C, cc, H, W] (the full-frame source block) and ``state`` [B, C, cc + G + cc, hr,
    wr] (the loop's final state on the region whose corner is ``origin`` = (y0, x0)) -> the full-frame state [B, C, cc + G + cc, H, W]:
    the source frames are the source; grounding frame g is source frame g outside the region and the region's grounding inside;
    target frame f is source frame f outside the region and the region's target inside."""
    if source.dim() != 5 or state.dim() != 5 or source.shape[:2] != state.shape[:2] or source.dtype != state.dtype:
        raise ValueError(f"reference_region_restore: source {source.dtype} {tuple(source.shape)} and state {state.dtype} "
                         f"{tuple(state.shape)}: expected [B, C, cc, H, W] and [B, C, cc + G + cc, hr, wr] of one dtype")
    cc, G = source.shape[2], state.shape[2] - 2 * source.shape[2]
    if not 0 <= G <= cc:
        raise ValueError(f"reference_region_restore: {state.shape[2]} state frames for {cc} source frames: G={G} grounding frames "
                         f"(0 <= G <= cc)")
    y0, x0, hr, wr = _box((origin[0], origin[1], state.shape[3], state.shape[4]), source.shape[3], source.shape[4],
                          "reference_region_restore")
    out = torch.cat([source, source[:, :, :G], source], dim=2)
    out[:, :, cc:, y0:y0 + hr, x0:x0 + wr] = state[:, :, cc:]
    return out


def _runs(runs, F: int, who: str):
    runs = [(int(a), int(c)) for a, c in runs]
    end = 0
    if not 1 <= len(runs) <= 3:
        raise ValueError(f"{who}: {len(runs)} runs of frames (1 to 3 pairs (start, count))")
    for a, c in runs:
        if a < end or c < 1 or a + c > F:
            raise ValueError(f"{who}: the run [{a}, {a} + {c}) of runs {runs} is empty, descends, overlaps or leaves the {F} frames")
        end = a + c
    return runs


def reference_region_crop_frames(x: torch.Tensor, runs, region) -> torch.Tensor:
    """``wan_region_crop_frames`` in torch: ``x`` [..., F, H, W]; ``runs`` = 1 to 3 pairs (start, count) of frames, ascending and not
    overlapping; the sub-box ``region`` = (y0, x0, h, w) of the listed frames, one run after the other, contiguous."""
    if x.dim() < 3:
        raise ValueError(f"reference_region_crop_frames: expected [..., F, H, W], got {tuple(x.shape)}")
    runs = _runs(runs, x.shape[-3], "reference_region_crop_frames")
    y0, x0, hr, wr = _box(region, x.shape[-2], x.shape[-1], "reference_region_crop_frames")
    return torch.cat([x[..., a:a + c, y0:y0 + hr, x0:x0 + wr] for a, c in runs], dim=-3).contiguous()


def reference_region_restore_frames(source: torch.Tensor, state: torch.Tensor, origin, frames) -> torch.Tensor:
    """``wan_region_restore_frames`` in torch: ``source`` [B, C, cc, H, W] and ``state`` [B, C, n + G + n, hr, wr], the loop's final state
    on the source frames ``frames`` = (t0, n) and the box whose corner is ``origin`` = (y0, x0) -> the whole state [B, C, cc + G + cc,
    H, W]: the source frames are the source; grounding frame g is the region's inside the box and source frame g outside; target frame f
    is the region's where t0 <= f < t0 + n and inside the box, and source frame f everywhere else."""
    if source.dim() != 5 or state.dim() != 5 or source.shape[:2] != state.shape[:2] or source.dtype != state.dtype:
        raise ValueError(f"reference_region_restore_frames: source {source.dtype} {tuple(source.shape)} and state {state.dtype} "
                         f"{tuple(state.shape)}: expected [B, C, cc, H, W] and [B, C, n + G + n, hr, wr] of one dtype")
    if len(frames) != 2:
        raise ValueError(f"reference_region_restore_frames: frames = (t0, n) in latent frames, got {frames!r}")
    t0, n = int(frames[0]), int(frames[1])
    cc, G = source.shape[2], state.shape[2] - 2 * n
    if t0 < 0 or n < 1 or t0 + n > cc:
        raise ValueError(f"reference_region_restore_frames: the frames [{t0}, {t0} + {n}) do not lie inside the {cc} source frames")
    if not 0 <= G <= cc:
        raise ValueError(f"reference_region_restore_frames: {state.shape[2]} state frames for a range of {n}: G={G} grounding frames "
                         f"(0 <= G <= cc = {cc})")
    y0, x0, hr, wr = _box((origin[0], origin[1], state.shape[3], state.shape[4]), source.shape[3], source.shape[4],
                          "reference_region_restore_frames")
    out = torch.cat([source, source[:, :, :G], source], dim=2)
    out[:, :, cc:cc + G, y0:y0 + hr, x0:x0 + wr] = state[:, :, n:n + G]
    out[:, :, cc + G + t0:cc + G + t0 + n, y0:y0 + hr, x0:x0 + wr] = state[:, :, n + G:]
    return out


def _origins(origins, frames: int, size, H: int, W: int, who: str) -> np.ndarray:
    """A table of corners, checked: int64 [frames, 2], every box of ``size`` = (h, w) inside a frame of H x W."""
    o = np.asarray(origins.cpu() if torch.is_tensor(origins) else origins)
    if o.ndim != 2 or o.shape[1] != 2 or o.dtype.kind not in "iu":
        raise ValueError(f"{who}: origins = integer [frames, 2] pairs (y0, x0) in cells, got {o.dtype} {o.shape}")
    if not 1 <= o.shape[0] <= REGION_TRACK_MAX_FRAMES or o.shape[0] != frames:
        raise ValueError(f"{who}: {o.shape[0]} rows of origins for {frames} frames (one each, at most {REGION_TRACK_MAX_FRAMES})")
    if len(size) != 2:
        raise ValueError(f"{who}: size = (h, w) in cells, got {size!r}")
    o = o.astype(np.int64)
    for f, (y0, x0) in enumerate(o):
        _box((y0, x0, size[0], size[1]), H, W, f"{who}: frame {f}")
    return o


def reference_region_crop_track(x: torch.Tensor, runs, origins, size) -> torch.Tensor:
    """``wan_region_crop_track`` in torch: ``x`` [..., F, H, W]; ``runs`` as in ``reference_region_crop_frames``; ``origins`` integer
    [F, 2] = the corner (y0, x0) of every INPUT frame's box; ``size`` = (h, w), one for all.  The box of the listed frames, each at its
    own corner, one run after the other, contiguous.  (The loop state [source | grounding | target] takes a table over its 2 cc + G
    frames: grounding g has source frame g's corner, target f source frame f's.)"""
    if x.dim() < 3:
        raise ValueError(f"reference_region_crop_track: expected [..., F, H, W], got {tuple(x.shape)}")
    runs = _runs(runs, x.shape[-3], "reference_region_crop_track")
    o = _origins(origins, x.shape[-3], size, x.shape[-2], x.shape[-1], "reference_region_crop_track")
    hr, wr = int(size[0]), int(size[1])
    return torch.stack([x[..., f, o[f, 0]:o[f, 0] + hr, o[f, 1]:o[f, 1] + wr] for a, c in runs for f in range(a, a + c)],
                       dim=-3).contiguous()


def reference_region_restore_track(source: torch.Tensor, state: torch.Tensor, origins, frames) -> torch.Tensor:
    """``wan_region_restore_track`` in torch: ``reference_region_restore_frames`` with the box of source frame f at ``origins[f]``
    (integer [cc, 2]): grounding frame g is the region's inside box g and source frame g outside it; target frame f is the region's
    where t0 <= f < t0 + n and inside box f, and source frame f everywhere else."""
    who = "reference_region_restore_track"
    if source.dim() != 5 or state.dim() != 5 or source.shape[:2] != state.shape[:2] or source.dtype != state.dtype:
        raise ValueError(f"{who}: source {source.dtype} {tuple(source.shape)} and state {state.dtype} "
                         f"{tuple(state.shape)}: expected [B, C, cc, H, W] and [B, C, n + G + n, hr, wr] of one dtype")
    if len(frames) != 2:
        raise ValueError(f"{who}: frames = (t0, n) in latent frames, got {frames!r}")
    t0, n = int(frames[0]), int(frames[1])
    cc, G = source.shape[2], state.shape[2] - 2 * n
    if t0 < 0 or n < 1 or t0 + n > cc:
        raise ValueError(f"{who}: the frames [{t0}, {t0} + {n}) do not lie inside the {cc} source frames")
    if not 0 <= G <= cc:
        raise ValueError(f"{who}: {state.shape[2]} state frames for a range of {n}: G={G} grounding frames (0 <= G <= cc = {cc})")
    hr, wr = int(state.shape[3]), int(state.shape[4])
    o = _origins(origins, cc, (hr, wr), source.shape[3], source.shape[4], who)
    out = torch.cat([source, source[:, :, :G], source], dim=2)
    for g in range(G):
        out[:, :, cc + g, o[g, 0]:o[g, 0] + hr, o[g, 1]:o[g, 1] + wr] = state[:, :, n + g]
    for k in range(n):
        y0, x0 = o[t0 + k]
        out[:, :, cc + G + t0 + k, y0:y0 + hr, x0:x0 + wr] = state[:, :, n + G + k]
    return out


def reference_mask_spans(weights: torch.Tensor) -> torch.Tensor:
    """``wan_mask_spans`` in torch: weights uint8 [Bm, Fs, h, w] -> int16 [Fs, h + w, 2].  Per latent frame the first h pairs are, per
    row, the inclusive (x_lo, x_hi) of the non-zero weights over all samples, (w, -1) for a row without one; the next w pairs are, per
    column, (y_lo, y_hi), (h, -1) for a column without one."""
    if weights.dim() != 4 or weights.dtype != torch.uint8:
        raise ValueError(f"reference_mask_spans: expected uint8 [Bm, Fs, h, w], got {weights.dtype} {tuple(weights.shape)}")
    _, Fs, h, w = weights.shape
    if h >= 32768 or w >= 32768:
        raise ValueError(f"reference_mask_spans: a frame of {h} x {w} cells (each below 32768: the spans are int16)")
    on = (weights != 0).any(dim=0).cpu()
    out = torch.empty((Fs, h + w, 2), dtype=torch.int16)
    for f in range(Fs):
        for lines, start, empty in ((on[f], 0, w), (on[f].t(), h, h)):
            for i, line in enumerate(lines):
                at = line.nonzero().flatten()
                out[f, start + i] = torch.tensor([int(at[0]), int(at[-1])] if at.numel() else [empty, -1], dtype=torch.int16)
    return out


def _split_table(origins, cuts, axis, size, H: int, W: int, who: str):
    """The boxes of a split, checked: (origins int64 [K, 2], cuts int64 [K + 1], axis)."""
    o = np.asarray(origins.cpu() if torch.is_tensor(origins) else origins)
    c = np.asarray(cuts.cpu() if torch.is_tensor(cuts) else cuts)
    if o.ndim != 2 or o.shape[1] != 2 or o.dtype.kind not in "iu" or not 1 <= o.shape[0] <= REGION_SPLIT_MAX:
        raise ValueError(f"{who}: origins = integer [K, 2] pairs (y0, x0) in cells, 1 to {REGION_SPLIT_MAX} boxes, got {o.dtype} {o.shape}")
    if isinstance(axis, bool) or axis not in (0, 1):
        raise ValueError(f"{who}: axis={axis!r} (1: the cuts are columns, 0: rows)")
    F = (H, W)[axis]
    if c.ndim != 1 or c.dtype.kind not in "iu" or c.shape[0] != o.shape[0] + 1 or c[0] != 0 or c[-1] != F or (np.diff(c) < 1).any():
        raise ValueError(f"{who}: cuts = {o.shape[0] + 1} ascending integers from 0 to {F}, got {c.tolist() if c.ndim == 1 else c.shape}")
    if len(size) != 2:
        raise ValueError(f"{who}: size = (h, w) in cells, got {size!r}")
    o = o.astype(np.int64)
    for k, (y0, x0) in enumerate(o):
        _box((y0, x0, size[0], size[1]), H, W, f"{who}: box {k}")
    return o, c.astype(np.int64), int(axis)


def _owned(k: int, cuts, axis: int, H: int, W: int) -> torch.Tensor:
    """bool [H, W]: the cells band k owns."""
    own = torch.zeros(H, W, dtype=torch.bool)
    if axis == 1:
        own[:, int(cuts[k]):int(cuts[k + 1])] = True
    else:
        own[int(cuts[k]):int(cuts[k + 1])] = True
    return own


def reference_region_crop_split(x: torch.Tensor, runs, origins, cuts, axis: int, size, clip: bool = False) -> torch.Tensor:
    """``wan_region_crop_split`` in torch: ``x`` [R..., F, H, W]; ``runs`` as in ``reference_region_crop_frames``; ``origins`` integer
    [K, 2], ``cuts`` integer [K + 1] and ``axis`` as in ``SplitPlan``; ``size`` = (h, w), one for all -> [K, R..., Fo, h, w], box-major:
    box k of the listed frames.  With ``clip`` everything outside what band k owns is ZERO in box k (the weights: there the loop pins
    the cells of another band's object to the source)."""
    who = "reference_region_crop_split"
    if x.dim() < 3:
        raise ValueError(f"{who}: expected [..., F, H, W], got {tuple(x.shape)}")
    runs = _runs(runs, x.shape[-3], who)
    H, W = int(x.shape[-2]), int(x.shape[-1])
    o, c, axis = _split_table(origins, cuts, axis, size, H, W, who)
    hr, wr = int(size[0]), int(size[1])
    out = []
    for k, (y0, x0) in enumerate(o):
        src = torch.where(_owned(k, c, axis, H, W), x, torch.zeros((), dtype=x.dtype)) if clip else x
        out.append(torch.cat([src[..., a:a + n, y0:y0 + hr, x0:x0 + wr] for a, n in runs], dim=-3))
    return torch.stack(out).contiguous()


def reference_region_restore_split(source: torch.Tensor, state: torch.Tensor, origins, cuts, axis: int, frames) -> torch.Tensor:
    """``wan_region_restore_split`` in torch: ``source`` [B, C, cc, H, W] and ``state`` [K B, C, n + G + n, hr, wr], box-major, the loop's
    final state on the source frames ``frames`` = (t0, n) and the K boxes of ``origins`` / ``cuts`` / ``axis`` -> [B, C, cc + G + cc, H,
    W]: source frames are the source; a grounding or target cell takes box k's value where it lies inside box k AND inside what band k
    owns (the target only in frames t0 <= f < t0 + n); everywhere else it is the source, bit for bit."""
    who = "reference_region_restore_split"
    if source.dim() != 5 or state.dim() != 5 or source.shape[1] != state.shape[1] or source.dtype != state.dtype:
        raise ValueError(f"{who}: source {source.dtype} {tuple(source.shape)} and state {state.dtype} "
                         f"{tuple(state.shape)}: expected [B, C, cc, H, W] and [K B, C, n + G + n, hr, wr] of one dtype")
    if len(frames) != 2:
        raise ValueError(f"{who}: frames = (t0, n) in latent frames, got {frames!r}")
    t0, n = int(frames[0]), int(frames[1])
    B, _, cc, H, W = (int(v) for v in source.shape)
    G = state.shape[2] - 2 * n
    if t0 < 0 or n < 1 or t0 + n > cc:
        raise ValueError(f"{who}: the frames [{t0}, {t0} + {n}) do not lie inside the {cc} source frames")
    if not 0 <= G <= cc:
        raise ValueError(f"{who}: {state.shape[2]} state frames for a range of {n}: G={G} grounding frames (0 <= G <= cc = {cc})")
    hr, wr = int(state.shape[3]), int(state.shape[4])
    o, c, axis = _split_table(origins, cuts, axis, (hr, wr), H, W, who)
    if state.shape[0] != len(o) * B:
        raise ValueError(f"{who}: {state.shape[0]} state samples for {len(o)} boxes of {B} samples")
    out = torch.cat([source, source[:, :, :G], source], dim=2)
    for k, (y0, x0) in enumerate(o):
        take = _owned(k, c, axis, H, W)[y0:y0 + hr, x0:x0 + wr]
        box = state[k * B:(k + 1) * B]
        for dst, src in ((slice(cc, cc + G), slice(n, n + G)), (slice(cc + G + t0, cc + G + t0 + n), slice(n + G, 2 * n + G))):
            view = out[:, :, dst, y0:y0 + hr, x0:x0 + wr]
            view[..., take] = box[:, :, src][..., take]
    return out


def _pixel_rect(rect, H: int, W: int, who: str, what: str, of: str) -> Tuple[int, int, int, int]:
    if len(rect) != 4:
        raise ValueError(f"{who}: {what} = (y, x, h, w) in pixels, got {rect!r}")
    y, x, h, w = (int(v) for v in rect)
    if y < 0 or x < 0 or h < 1 or w < 1 or y + h > H or x + w > W:
        raise ValueError(f"{who}: the {what} [{y}, {y} + {h}) x [{x}, {x} + {w}) does not lie inside {of} of {H} x {W}")
    return y, x, h, w


def reference_frames_box_to_video(frames_u8: torch.Tensor, box, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``wan_frames_u8_box_to_video`` in torch: the box ``box`` = (y, x, h, w) in pixels of uint8 ``frames_u8`` [B, T, H, W, 3] ->
    [B, 3, T, h, w] in ``dtype``: ``video_io.reference_frames_to_video``'s arithmetic (float32 ``x * (2.0 / 255.0) - 1.0``, two
    operations rounded one after the other, then the cast) on the cropped frames."""
    if frames_u8.dim() != 5 or frames_u8.shape[-1] != 3 or frames_u8.dtype != torch.uint8:
        raise ValueError(f"reference_frames_box_to_video: expected uint8 [B, T, H, W, 3], got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    y, x, h, w = _pixel_rect(box, frames_u8.shape[2], frames_u8.shape[3], "reference_frames_box_to_video", "box", "a frame")
    v = frames_u8[:, :, y:y + h, x:x + w].permute(0, 4, 1, 2, 3).float()
    v = v * (2.0 / 255.0) - 1.0
    return v.to(dtype).contiguous()


def stitch_weights(frame, rect, feather: int) -> np.ndarray:
    """The ramp of ``reference_video_box_stitch``: int64 [h, w] weights a over the rectangle ``rect`` = (y, x, h, w) of a frame
    ``frame`` = (H, W).  d = the least distance of the pixel to an edge of the rectangle that does not lie on the frame's border (none:
    infinity); a = 255 if feather == 0 or d >= feather else (255 * (d + 1)) // (feather + 1)."""
    (H, W), f = (int(v) for v in frame), int(feather)
    ry, rx, rh, rw = _pixel_rect(rect, H, W, "stitch_weights", "rectangle", "a frame")
    if f < 0:
        raise ValueError(f"stitch_weights: feather={feather} pixels (not negative)")
    far = np.iinfo(np.int64).max
    ys, xs = np.arange(rh, dtype=np.int64), np.arange(rw, dtype=np.int64)
    dy, dx = np.full(rh, far), np.full(rw, far)
    if ry > 0:
        dy = np.minimum(dy, ys)
    if ry + rh < H:
        dy = np.minimum(dy, rh - 1 - ys)
    if rx > 0:
        dx = np.minimum(dx, xs)
    if rx + rw < W:
        dx = np.minimum(dx, rw - 1 - xs)
    d = np.minimum(dy[:, None], dx[None, :])
    if f == 0:
        return np.full((rh, rw), 255, np.int64)
    return np.where(d >= f, 255, (255 * (np.minimum(d, f) + 1)) // (f + 1))


def reference_video_box_stitch(source_u8: torch.Tensor, edit_u8: torch.Tensor, box, rect, feather: int = 0) -> torch.Tensor:
    """``wan_video_box_stitch_u8`` in numpy int64 on the host: ``source_u8`` uint8 [Bs, T, H, W, 3] (Bs = 1 or B), ``edit_u8`` uint8
    [B, T, bh, bw, 3] = the decoder's frames on the box ``box`` = (y, x, bh, bw) as bytes (``video_io.reference_video_to_frames`` of
    the decoder's output; frame t stitches against source frame t) -> uint8 [B, T, H, W, 3].  With ``rect`` = (y, x, h, w) the region's
    rectangle in frame pixels, inside the box, o the source's byte, e the edit's and a = ``stitch_weights``:

        outside the rectangle   out = o
        inside it               out = (a * e + (255 - a) * o + 127) // 255

    ``feather`` 0 is the literal stitch; edges of the rectangle on the frame's border do not ramp."""
    if source_u8.dim() != 5 or edit_u8.dim() != 5 or source_u8.dtype != torch.uint8 or edit_u8.dtype != torch.uint8 \
            or source_u8.shape[-1] != 3 or edit_u8.shape[-1] != 3 or source_u8.shape[0] not in (1, edit_u8.shape[0]) \
            or source_u8.shape[1] != edit_u8.shape[1]:
        raise ValueError(f"reference_video_box_stitch: source {source_u8.dtype} {tuple(source_u8.shape)} and edit {edit_u8.dtype} "
                         f"{tuple(edit_u8.shape)}: expected uint8 [1 or B, T, H, W, 3] and [B, T, bh, bw, 3]")
    H, W = int(source_u8.shape[2]), int(source_u8.shape[3])
    by, bx, bh, bw = _pixel_rect(box, H, W, "reference_video_box_stitch", "box", "a frame")
    if tuple(edit_u8.shape[2:4]) != (bh, bw):
        raise ValueError(f"reference_video_box_stitch: a box of {bh} x {bw} pixels for edit frames of {tuple(edit_u8.shape[2:4])}")
    ry, rx, rh, rw = _pixel_rect(rect, H, W, "reference_video_box_stitch", "rectangle", "a frame")
    if ry < by or rx < bx or ry + rh > by + bh or rx + rw > bx + bw:
        raise ValueError(f"reference_video_box_stitch: the rectangle {tuple(rect)} does not lie inside the box {tuple(box)}")
    a = stitch_weights((H, W), (ry, rx, rh, rw), feather)[None, None, :, :, None]
    out = source_u8.cpu().numpy().astype(np.int64)
    out = np.broadcast_to(out, (edit_u8.shape[0],) + out.shape[1:]).copy()
    e = edit_u8.cpu().numpy().astype(np.int64)[:, :, ry - by:ry - by + rh, rx - bx:rx - bx + rw]
    o = out[:, :, ry:ry + rh, rx:rx + rw]
    out[:, :, ry:ry + rh, rx:rx + rw] = (a * e + (255 - a) * o + 127) // 255
    return torch.from_numpy(out.astype(np.uint8))
