"""Local self-attention plans: which 64-key tiles every 256-row query block attends.

Opt-in and LOSSY -- the reference attends densely; no quality claim is made (``clip_stats`` is the tool to judge a checkpoint with).

Token rule.  Tokens are ordered (frame, row y, column x).  A token belongs to the source segment, the grounding frames or the target
segment ([source | grounding | target] along the frame axis, as ``frame_split_indices`` / ``ground_frame_indices`` describe them);
without a source segment there is one segment.  ``f`` is the token's frame index INSIDE its segment, so source frame f and target
frame f correspond.  Query a may attend key b iff at least one of

* a or b is a grounding token (grounding tokens are global both ways);
* b lies in a non-grounding frame with ``f_b < sink_frames``;
* ``|f_a - f_b| <= window_frames`` and ``|y_a - y_b| <= window_rows`` -- across and within the segments alike; columns are never
  restricted.

Block rule.  The pair (query block of 256 rows, key tile of 64 keys) is listed iff ANY token pair inside it is allowed; inside a listed
tile all keys are attended.  The kernel (``wan_attention_fwd_sparse``) therefore computes exactly dense attention over the keys of the
listed tiles, which is what ``reference_sparse_attention`` restates in torch.

Everything here but ``reference_sparse_attention`` is numpy on the host.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

Q_BLOCK, K_TILE = 256, 64       # the kernel's workgroup and key-tile sizes (kWanAttnQPerWG, kWanAttnKV)


@dataclass(frozen=True)
class LocalAttentionPlan:
    """CSR lists: query block i attends the physical key tiles ``tiles[row_ptr[i]:row_ptr[i + 1]]`` (strictly ascending, non-empty)."""
    row_ptr: np.ndarray         # int32 [n_qblocks + 1]
    tiles: np.ndarray           # int32 [listed]
    n_qblocks: int
    n_ktiles: int
    q_len: int                  # query rows the plan was made for (>= the token count: the padded sequence length)
    k_len: int                  # keys = tokens of the grid

    @property
    def listed(self) -> int:
        return int(self.tiles.size)

    @property
    def density(self) -> float:
        """Listed (block, tile) pairs over all pairs: the share of the dense kernel's tile visits that remains."""
        return self.listed / float(self.n_qblocks * self.n_ktiles)

    def row(self, i: int) -> np.ndarray:
        return self.tiles[self.row_ptr[i]:self.row_ptr[i + 1]]


def _segments(frames: int, frame_split_indices, ground_frame_indices) -> Tuple[np.ndarray, np.ndarray]:
    """Per frame of the grid: (is grounding frame, frame index inside its segment)."""
    split = _one(frame_split_indices, "frame_split_indices")
    ground = _one(ground_frame_indices, "ground_frame_indices")
    is_ground = np.zeros(frames, dtype=bool)
    f = np.arange(frames, dtype=np.int64)
    if split is None:
        if ground is not None:
            raise ValueError("ground_frame_indices without frame_split_indices: grounding frames follow a source segment")
        return is_ground, f
    n = int(split)
    g0, g1 = (n, n) if ground is None else (int(ground[0]), int(ground[1]))
    if not (0 < n <= frames) or g0 != n or not (g0 <= g1 <= frames):
        raise ValueError(f"frame_split_indices={n}, ground_frame_indices=({g0}, {g1}) do not describe [source | grounding | target] "
                         f"in {frames} frames")
    is_ground[g0:g1] = True
    f[g1:] -= g1
    return is_ground, f


def _one(per_sample, name):
    """The model's arguments are per-sample lists whose entries must agree (wan_transformer3d._rope_map); one bare entry is accepted."""
    if per_sample is None:
        return None
    pair = name == "ground_frame_indices"
    entries = list(per_sample) if isinstance(per_sample, (list, tuple)) else [per_sample]
    if pair and entries and not isinstance(entries[0], (list, tuple)):
        entries = [entries]                                  # one bare (start, end)
    vals = {tuple(int(v) for v in e) if pair else int(e) for e in entries}
    if len(vals) > 1:
        raise NotImplementedError(f"all samples of a call must share {name}")
    return next(iter(vals)) if vals else None


def _check_windows(window_frames, window_rows, sink_frames):
    for name, v in (("window_frames", window_frames), ("window_rows", window_rows), ("sink_frames", sink_frames)):
        if isinstance(v, bool) or int(v) != v or v < 0:
            raise ValueError(f"{name}={v!r}: a whole number >= 0")


def _row_rule(grid, frame_split_indices, ground_frame_indices, window_frames, window_rows, sink_frames) -> np.ndarray:
    """The token rule between token ROWS (frame, y) -- columns are never restricted, so all tokens of a row share it: bool [F*R, F*R]."""
    F, R, _ = (int(v) for v in grid)
    is_ground, f = _segments(F, frame_split_indices, ground_frame_indices)
    g = np.repeat(is_ground, R)
    fr = np.repeat(f, R)
    y = np.tile(np.arange(R, dtype=np.int64), F)
    near = (np.abs(fr[:, None] - fr[None, :]) <= window_frames) & (np.abs(y[:, None] - y[None, :]) <= window_rows)
    sink = ~g & (fr < sink_frames)
    return g[:, None] | g[None, :] | sink[None, :] | near


def reference_local_mask(grid: Sequence[int], frame_split_indices, ground_frame_indices, window_frames: int, window_rows: int,
                         sink_frames: int = 1) -> np.ndarray:
    """The token rule by brute force: bool [L, L], entry [a, b] = query a may attend key b.  For tests (L^2 bytes)."""
    _check_windows(window_frames, window_rows, sink_frames)
    F, R, W = (int(v) for v in grid)
    is_ground, seg_f = _segments(F, frame_split_indices, ground_frame_indices)
    L = F * R * W
    mask = np.zeros((L, L), dtype=bool)
    frame = np.arange(L) // (R * W)
    y = np.arange(L) % (R * W) // W
    g, f = is_ground[frame], seg_f[frame]
    for a in range(L):
        mask[a] = g[a] | g | (~g & (f < sink_frames)) | ((np.abs(f[a] - f) <= window_frames) & (np.abs(y[a] - y) <= window_rows))
    return mask


def block_lift(mask: np.ndarray, q_len: Optional[int] = None) -> np.ndarray:
    """The block rule applied to a token mask: bool [ceil(q_len / 256), ceil(L / 64)], True where ANY token pair of the block is."""
    Lq_tok, Lk = mask.shape
    q_len = Lq_tok if q_len is None else int(q_len)
    nqb, nkt = -(-q_len // Q_BLOCK), -(-Lk // K_TILE)
    out = np.zeros((nqb, nkt), dtype=bool)
    for i in range(nqb):
        rows = mask[i * Q_BLOCK:min((i + 1) * Q_BLOCK, Lq_tok)]
        if rows.shape[0] == 0:
            continue
        hit = rows.any(axis=0)
        for j in range(nkt):
            out[i, j] = hit[j * K_TILE:(j + 1) * K_TILE].any()
    return out


def plan_from_blocks(blocks: np.ndarray, q_len: int, k_len: int) -> LocalAttentionPlan:
    """CSR lists from a bool [n_qblocks, n_ktiles] matrix.  A block without any listed tile -- only a block of padding rows behind the
    last token can be one -- lists tile 0: every list must be non-empty, and what those rows compute is never read."""
    blocks = np.asarray(blocks, dtype=bool)
    nqb, nkt = blocks.shape
    if nqb != -(-int(q_len) // Q_BLOCK) or nkt != -(-int(k_len) // K_TILE):
        raise ValueError(f"a [{nqb}, {nkt}] block matrix does not describe q_len={q_len}, k_len={k_len}")
    blocks = blocks.copy()
    blocks[~blocks.any(axis=1), 0] = True
    counts = blocks.sum(axis=1)
    row_ptr = np.zeros(nqb + 1, dtype=np.int32)
    np.cumsum(counts, out=row_ptr[1:])
    tiles = np.nonzero(blocks)[1].astype(np.int32)          # row-major: ascending inside every row
    return LocalAttentionPlan(row_ptr, tiles, nqb, nkt, int(q_len), int(k_len))


def local_attention_plan(grid: Sequence[int], frame_split_indices, ground_frame_indices, window_frames: int, window_rows: int,
                         sink_frames: int = 1, q_len: Optional[int] = None) -> LocalAttentionPlan:
    """The block rule for a token grid (frames, rows, columns).  ``frame_split_indices`` / ``ground_frame_indices`` as the model's
    forward takes them (per-sample lists whose entries agree, or one value / one (start, end) pair; None = no source segment).
    ``q_len``: query rows of the call when the sequence is padded beyond the grid's tokens (default: the token count); query blocks
    that hold no token list tile 0.

    Works on token ROWS (all tokens of a (frame, y) row share the rule): a block or tile covers a contiguous range of rows, and
    "any pair allowed" is a 2-D range query on the row rule -- answered with prefix sums, O((F R)^2) instead of O(L^2)."""
    _check_windows(window_frames, window_rows, sink_frames)
    F, R, W = (int(v) for v in grid)
    if min(F, R, W) < 1:
        raise ValueError(f"grid={tuple(grid)}")
    L = F * R * W
    q_len = L if q_len is None else int(q_len)
    if q_len < L:
        raise ValueError(f"q_len={q_len} is less than the grid's {L} tokens")
    rule = _row_rule((F, R, W), frame_split_indices, ground_frame_indices, int(window_frames), int(window_rows), int(sink_frames))
    U = F * R
    pre = np.zeros((U + 1, U + 1), dtype=np.int32)
    np.cumsum(np.cumsum(rule, axis=0, dtype=np.int32), axis=1, out=pre[1:, 1:])
    nqb, nkt = -(-q_len // Q_BLOCK), -(-L // K_TILE)
    q0 = np.arange(nqb, dtype=np.int64) * Q_BLOCK
    q1 = np.minimum(q0 + Q_BLOCK, L) - 1                    # last TOKEN of the block (a block of padding rows: q1 < q0)
    k0 = np.arange(nkt, dtype=np.int64) * K_TILE
    k1 = np.minimum(k0 + K_TILE, L) - 1
    has_tokens = q1 >= q0
    qa, qb = np.minimum(q0, L - 1) // W, np.maximum(q1, 0) // W + 1          # row ranges [qa, qb)
    ka, kb = k0 // W, k1 // W + 1
    hits = pre[qb[:, None], kb[None, :]] - pre[qa[:, None], kb[None, :]] - pre[qb[:, None], ka[None, :]] + pre[qa[:, None], ka[None, :]]
    return plan_from_blocks((hits > 0) & has_tokens[:, None], q_len, L)


def reference_sparse_attention(q, k, v, plan: LocalAttentionPlan, scale: float):
    """What ``wan_attention_fwd_sparse`` computes, in torch: fp32 math on the (bf16) inputs, per query block a dense softmax attention
    over the keys of its listed tiles.  q [B, Lq, H*128], k / v [B, Lk, H*128] (v NOT transposed) -> fp32 [B, Lq, H*128]."""
    import torch
    B, Lq, C = q.shape
    Lk, H = k.shape[1], C // 128
    if -(-Lq // Q_BLOCK) != plan.n_qblocks or -(-Lk // K_TILE) != plan.n_ktiles:
        raise ValueError(f"the plan ({plan.n_qblocks} blocks, {plan.n_ktiles} tiles) does not fit Lq={Lq}, Lk={Lk}")
    qf = q.float().view(B, Lq, H, 128).permute(0, 2, 1, 3)
    kf = k.float().view(B, Lk, H, 128).permute(0, 2, 1, 3)
    vf = v.float().view(B, Lk, H, 128).permute(0, 2, 1, 3)
    out = torch.empty(B, H, Lq, 128, dtype=torch.float32, device=q.device)
    offs = torch.arange(K_TILE, device=q.device)
    for i in range(plan.n_qblocks):
        tiles = torch.as_tensor(plan.row(i).astype(np.int64), device=q.device)
        keys = (tiles[:, None] * K_TILE + offs[None, :]).reshape(-1)
        keys = keys[keys < Lk]
        r0, r1 = i * Q_BLOCK, min((i + 1) * Q_BLOCK, Lq)
        s = torch.matmul(qf[:, :, r0:r1], kf[:, :, keys].transpose(-1, -2)) * float(scale)
        out[:, :, r0:r1] = torch.matmul(torch.softmax(s, dim=-1), vf[:, :, keys])
    return out.permute(0, 2, 1, 3).reshape(B, Lq, C)
