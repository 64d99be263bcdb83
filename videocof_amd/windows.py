"""Temporal context windows: the plan (host arithmetic, no GPU needed) and torch restatements of the two device passes.

A clip of ``Fs`` latent frames is denoised as ``K`` overlapping windows of ``n`` latent frames, all of the same length; each step
runs the model on the windows, blends their predictions into one prediction for the clip and steps the sampler once
("Temporal context windows").  ``window_plan`` fixes where the windows start and with which weight each of them
enters a frame; ``reference_window_gather`` / ``reference_window_blend`` state what ``wan_window_gather`` / ``wan_window_blend``
compute, in plain torch (the blend in float32 with separately rounded products and sums: the kernel's bits).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

__all__ = ["WindowPlan", "window_plan", "window_latent_frames", "reference_window_gather", "reference_window_blend"]


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
