"""Temporal context windows: the plan (host arithmetic, no GPU needed) and torch restatements of the two device passes.

A clip of ``Fs`` latent frames is denoised as ``K`` overlapping windows of ``n`` latent frames, all of the same length; each step
runs the model on the windows, blends their predictions into one prediction for the clip and steps the sampler once
("Temporal context windows").  ``window_plan`` fixes where the windows start and with which weight each of them
enters a frame; ``reference_window_gather`` / ``reference_window_blend`` state what ``wan_window_gather`` / ``wan_window_blend``
compute, in plain torch (the blend in float32 with separately rounded products and sums: the kernel's bits).

Spatial context windows are the same in three axes: a ``TilePlan`` holds one ``WindowPlan`` per axis (t, y, x, all
in latent cells), the windows are its K = Kt * Ky * Kx tiles of one shape, and ``reference_tile_gather`` / ``reference_tile_blend``
state what ``wan_tile_gather`` / ``wan_tile_blend`` compute.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

__all__ = ["WindowPlan", "window_plan", "window_latent_frames", "reference_window_gather", "reference_window_blend",
           "TilePlan", "spatial_window_cells", "reference_tile_gather", "reference_tile_blend"]


@dataclass(frozen=True)
class WindowPlan:
    frames: int                     # Fs, latent frames of the clip
    window: int                     # n, latent frames of every window (Fs itself when the clip fits one window)
    overlap: int                    # o, the overlap asked for (the pulled-back last window may overlap its neighbour by more)
    starts: Tuple[int, ...]         # a_k, ascending; the last one is Fs - n
    alpha: np.ndarray               # float32 [K, Fs]: normalised weight of window k at global frame f, 0 where k does not cover f

    @property
    def K(self) -> int:
        return len(self.starts)

    @property
    def n(self) -> int:
        return self.window

    def covering(self, f: int) -> Tuple[int, ...]:
        """The windows that cover global frame f, ascending."""
        return tuple(k for k, a in enumerate(self.starts) if a <= f < a + self.window)


def window_plan(frames: int, window: int, overlap: int) -> WindowPlan:
    """Where the windows of a clip start and how their predictions are weighted; all three arguments in LATENT frames.

    ``frames <= window``: one window at 0 of length ``frames`` (the caller takes the unwindowed path).  Otherwise the stride is
    s = window - overlap, K = ceil((frames - window) / s) + 1, a_k = k * s for k < K - 1 and a_{K-1} = frames - window: the last
    window is pulled back so that all windows have the same length.  Raw weight of a window at its local frame j:
    w(j) = min(j + 1, n - j, overlap + 1), a ramp over the overlap; ``alpha[k][f]`` = w_k(f - a_k) / (sum over the windows covering
    f), computed in float64 and rounded once to float32 -- exactly 1 where one window covers f."""
    for name, v in (("frames", frames), ("window", window), ("overlap", overlap)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"window_plan: {name}={v!r} is not an integer")
    frames, window, overlap = int(frames), int(window), int(overlap)
    if frames < 1:
        raise ValueError(f"window_plan: frames={frames} (>= 1)")
    if window < 2:
        raise ValueError(f"window_plan: window={window} (>= 2)")
    if not 0 <= overlap <= window - 1:
        raise ValueError(f"window_plan: overlap={overlap} (0 .. window - 1 = {window - 1})")
    if frames <= window:
        return WindowPlan(frames, frames, overlap, (0,), np.ones((1, frames), dtype=np.float32))
    s = window - overlap
    K = -(-(frames - window) // s) + 1
    starts = tuple(k * s for k in range(K - 1)) + (frames - window,)
    raw = np.zeros((K, frames), dtype=np.float64)
    j = np.arange(window)
    w = np.minimum(np.minimum(j + 1, window - j), overlap + 1).astype(np.float64)
    for k, a in enumerate(starts):
        raw[k, a:a + window] = w
    alpha = (raw / raw.sum(axis=0, keepdims=True)).astype(np.float32)
    return WindowPlan(frames, window, overlap, starts, alpha)


def window_latent_frames(temporal_window, temporal_overlap, ratio: int = 4) -> Tuple[int, int]:
    """The pipeline's ``temporal_window`` / ``temporal_overlap`` (PIXEL frames) as latent frame counts, by the rule
    ``(x - 1) // ratio + 1`` it uses for ``source_frames``.  ``temporal_window`` must be ratio * m + 1 with at least two latent
    frames, ``temporal_overlap`` a multiple of ``ratio`` that leaves the windows a stride."""
    for name, v in (("temporal_window", temporal_window), ("temporal_overlap", temporal_overlap)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name}={v!r} is not an integer frame count")
    tw, to, ratio = int(temporal_window), int(temporal_overlap), int(ratio)
    if tw < ratio + 1 or (tw - 1) % ratio != 0:
        raise ValueError(f"temporal_window={tw} must be {ratio} * m + 1 frames with m >= 1 (the VAE's temporal ratio is {ratio})")
    if to < 0 or to % ratio != 0:
        raise ValueError(f"temporal_overlap={to} must be a non-negative multiple of the VAE's temporal ratio {ratio}")
    n = (tw - 1) // ratio + 1
    o = (to - 1) // ratio + 1           # (0 -> 0: floor division)
    if o > n - 1:
        raise ValueError(f"temporal_overlap={to} ({o} latent frames) leaves windows of temporal_window={tw} ({n} latent frames) "
                         f"no stride: at most {ratio * (n - 1)}")
    return n, o


def _starts_of(plan) -> Tuple[int, ...]:
    return tuple(int(a) for a in (plan.starts if isinstance(plan, WindowPlan) else plan))


def reference_window_gather(state: torch.Tensor, plan, window: int, ground: int, k0: int = 0, k1: Optional[int] = None,
                            rep: int = 1) -> torch.Tensor:
    """``wan_window_gather`` in torch: windows [k0, k1) of ``state`` [B, C, Fs + K*G + Fs, h, w] as the batch
    [rep][k1 - k0][B] x [C, n + G + n, h, w].  ``plan``: a WindowPlan or its starts."""
    starts, n, G = _starts_of(plan), int(window), int(ground)
    K = len(starts)
    k1 = K if k1 is None else k1
    Fs = (state.shape[2] - K * G) // 2
    wins = [torch.cat([state[:, :, a:a + n], state[:, :, Fs + k * G:Fs + (k + 1) * G],
                       state[:, :, Fs + K * G + a:Fs + K * G + a + n]], dim=2) for k, a in list(enumerate(starts))[k0:k1]]
    return torch.cat(wins * int(rep))


def reference_window_blend(pred: torch.Tensor, plan: WindowPlan, ground: int) -> torch.Tensor:
    """``wan_window_blend`` in torch: ``pred`` [K*B, C, n + G + n, h, w] (window-major) -> the prediction for the state
    [B, C, Fs + K*G + Fs, h, w].  float32 products and sums, each rounded on its own, in ascending window order; the result is
    rounded once to ``pred.dtype``."""
    K, n, Fs, G = plan.K, plan.window, plan.frames, int(ground)
    B = pred.shape[0] // K
    p = pred.reshape(K, B, *pred.shape[1:])
    out = torch.zeros(B, pred.shape[1], 2 * Fs + K * G, *pred.shape[3:], dtype=pred.dtype, device=pred.device)
    for k in range(K):
        out[:, :, Fs + k * G:Fs + (k + 1) * G] = p[k][:, :, n:n + G]
    alpha = torch.from_numpy(plan.alpha)
    for f in range(Fs):
        acc = None
        for k in plan.covering(f):
            term = alpha[k, f].to(pred.device) * p[k][:, :, n + G + f - plan.starts[k]].float()
            acc = term if acc is None else acc + term
        out[:, :, Fs + K * G + f] = acc.to(pred.dtype)
    return out


# ------------------------------------------------------------------------------------------------ spatial context windows
@dataclass(frozen=True)
class TilePlan:
    """Windows in three axes: ``t``, ``y``, ``x`` are the axes' ``window_plan(extent, window, overlap)`` in LATENT cells (an axis
    whose extent fits its window has one window of the whole extent).  The K = Kt * Ky * Kx tiles all have the shape
    ``(n, th, tw)``; tile ``k = (kt * Ky + ky) * Kx + kx``.  Its weight at latent position (f, y, x) is
    ``round(round(at[kt][f] * ay[ky][y]) * ax[kx][x])`` in float32 (``at := 1`` for grounding frames): ``at[kt][f]`` exactly when
    Ky = Kx = 1, exactly 1 where one tile covers the position."""
    t: WindowPlan
    y: WindowPlan
    x: WindowPlan

    @property
    def Kt(self) -> int:
        return self.t.K

    @property
    def Ky(self) -> int:
        return self.y.K

    @property
    def Kx(self) -> int:
        return self.x.K

    @property
    def K(self) -> int:
        return self.t.K * self.y.K * self.x.K

    @property
    def shape(self) -> Tuple[int, int, int]:
        """(n, th, tw): latent frames, rows and columns of every tile."""
        return self.t.window, self.y.window, self.x.window

    @property
    def extent(self) -> Tuple[int, int, int]:
        """(Fs, H, W): latent frames, rows and columns of the clip."""
        return self.t.frames, self.y.frames, self.x.frames

    def index(self, kt: int, ky: int, kx: int) -> int:
        return (kt * self.Ky + ky) * self.Kx + kx

    def split(self, k: int) -> Tuple[int, int, int]:
        """(kt, ky, kx) of tile k."""
        if not 0 <= k < self.K:
            raise IndexError(f"tile {k} of {self.K}")
        return k // (self.Ky * self.Kx), (k // self.Kx) % self.Ky, k % self.Kx

    def origin(self, k: int) -> Tuple[int, int, int]:
        """(a_t, y0, x0): where tile k starts."""
        kt, ky, kx = self.split(k)
        return self.t.starts[kt], self.y.starts[ky], self.x.starts[kx]

    def weights(self, k: int, ground: bool = False) -> np.ndarray:
        """float32 [Fs, H, W] ([H, W] for grounding frames): tile k's weight at every position of the clip, 0 outside the tile."""
        kt, ky, kx = self.split(k)
        ay, ax = self.y.alpha[ky], self.x.alpha[kx]
        if ground:
            return (np.float32(1.0) * ay)[:, None] * ax[None, :]
        return (self.t.alpha[kt][:, None] * ay[None, :])[:, :, None] * ax[None, None, :]      # float32: each product rounded on its own

    def covering(self, f: int, y: int, x: int) -> Tuple[int, ...]:
        """The tiles that cover latent position (f, y, x), ascending."""
        return tuple(self.index(kt, ky, kx) for kt in self.t.covering(f) for ky in self.y.covering(y) for kx in self.x.covering(x))


def spatial_window_cells(spatial_window, spatial_overlap, ratio: int = 8, patch: int = 2) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """The pipeline's ``spatial_window`` = (h, w) / ``spatial_overlap`` = (oy, ox), both in PIXELS, as latent cells:
    ``((th, tw), (oy, ox))``.  Each side of ``spatial_window`` must be a multiple of ratio * patch (a tile is patchified on its
    own) and at least that; each side of ``spatial_overlap`` a non-negative multiple of ``ratio`` that leaves the tiles a stride."""
    ratio, patch = int(ratio), int(patch)
    pairs = []
    for name, v in (("spatial_window", spatial_window), ("spatial_overlap", spatial_overlap)):
        if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) != 2:
            raise ValueError(f"{name}={v!r} is not a pair (rows, columns) of pixel counts")
        for e in v:
            if isinstance(e, bool) or not isinstance(e, (int, np.integer)):
                raise ValueError(f"{name}={tuple(v)!r}: {e!r} is not an integer pixel count")
        pairs.append((int(v[0]), int(v[1])))
    (wh, ww), (oh, ow) = pairs
    unit = ratio * patch
    for side in (wh, ww):
        if side < unit or side % unit != 0:
            raise ValueError(f"spatial_window={(wh, ww)}: {side} must be a positive multiple of {unit} pixels (the VAE's spatial ratio "
                             f"{ratio} times the patch {patch})")
    for side in (oh, ow):
        if side < 0 or side % ratio != 0:
            raise ValueError(f"spatial_overlap={(oh, ow)}: {side} must be a non-negative multiple of the VAE's spatial ratio {ratio}")
    cells, over = (wh // ratio, ww // ratio), (oh // ratio, ow // ratio)
    for n, o, side in zip(cells, over, (oh, ow)):
        if o > n - 1:
            raise ValueError(f"spatial_overlap={(oh, ow)}: {side} pixels ({o} cells) leave tiles of spatial_window={(wh, ww)} "
                             f"({cells[0]} x {cells[1]} cells) no stride: at most {ratio * (n - 1)}")
    return cells, over


def reference_tile_gather(state: torch.Tensor, plan: TilePlan, ground: int, k0: int = 0, k1: Optional[int] = None,
                          rep: int = 1) -> torch.Tensor:
    """``wan_tile_gather`` in torch: tiles [k0, k1) of ``state`` [B, C, Fs + Kt*G + Fs, H, W] as the batch
    [rep][k1 - k0][B] x [C, n + G + n, th, tw]; the spatial tiles of one temporal window share its grounding block."""
    (n, th, tw), (Fs, _, _), G, Kt = plan.shape, plan.extent, int(ground), plan.Kt
    k1 = plan.K if k1 is None else k1
    tiles = []
    for k in range(k0, k1):
        kt = plan.split(k)[0]
        a, y0, x0 = plan.origin(k)
        s = state[:, :, :, y0:y0 + th, x0:x0 + tw]
        tiles.append(torch.cat([s[:, :, a:a + n], s[:, :, Fs + kt * G:Fs + (kt + 1) * G],
                                s[:, :, Fs + Kt * G + a:Fs + Kt * G + a + n]], dim=2))
    return torch.cat(tiles * int(rep))


def reference_tile_blend(pred: torch.Tensor, plan: TilePlan, ground: int) -> torch.Tensor:
    """``wan_tile_blend`` in torch: ``pred`` [K*B, C, n + G + n, th, tw] (tile-major) -> the prediction for the state
    [B, C, Fs + Kt*G + Fs, H, W].  Source frames 0; grounding frame g of block kt and target frame f at (y, x): the sum over the
    covering tiles in ascending k of w * p, in float32 with the first term round(w * p) and every later one
    acc = round(acc + round(w * p)); one rounding to ``pred.dtype``."""
    (n, th, tw), (Fs, H, W), G, Kt, K = plan.shape, plan.extent, int(ground), plan.Kt, plan.K
    B = pred.shape[0] // K
    p = pred.reshape(K, B, *pred.shape[1:])
    acc = torch.zeros(B, pred.shape[1], Kt * G + Fs, H, W, dtype=torch.float32, device=pred.device)
    seen = torch.zeros(Kt * G + Fs, H, W, dtype=torch.bool, device=pred.device)

    def add(frames, ys, xs, w, x):
        term = w.to(pred.device) * x.float()
        region, s = acc[:, :, frames, ys, xs], seen[frames, ys, xs]
        region.copy_(torch.where(s, region + term, term))
        s.fill_(True)

    for k in range(K):
        kt = plan.split(k)[0]
        a, y0, x0 = plan.origin(k)
        ys, xs = slice(y0, y0 + th), slice(x0, x0 + tw)
        if G:
            add(slice(kt * G, (kt + 1) * G), ys, xs, torch.from_numpy(plan.weights(k, ground=True)[ys, xs]), p[k][:, :, n:n + G])
        add(slice(Kt * G + a, Kt * G + a + n), ys, xs, torch.from_numpy(plan.weights(k)[a:a + n, ys, xs]), p[k][:, :, n + G:])
    out = torch.zeros(B, pred.shape[1], 2 * Fs + Kt * G, H, W, dtype=pred.dtype, device=pred.device)
    out[:, :, Fs:] = acc.to(pred.dtype)
    return out
