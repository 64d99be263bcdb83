"""Frames in, frames out: the uint8 frames of a video reader / writer around ``WanPipeline.__call__``.

What the reference's command line does on the host on both sides of its pipeline runs here as two HIP kernels:

    in   fast_infer.py:43-92   load_video_frames: pick ``source_frames`` frames (stride, start frame, repeat-last padding),
                               ``uint8 [T, H, W, 3]`` -> ``float32 [1, 3, T, H, W]`` by ``x * (2.0 / 255.0) - 1.0``
         -> ``load_video_frames`` (the frame selection, bytes stay bytes) + ``frames_to_video`` (``wan_frames_u8_to_video``)
    out  pipeline_wan.py:423-428 + videox_fun/utils/utils.py:59-68   ``(x / 2 + 0.5).clamp(0, 1)``, ``.cpu().float().numpy()``,
                               ``b c t h w -> t h w c``, ``(x * 255).astype(np.uint8)``
         -> ``video_to_frames`` (``wan_video_to_frames_u8``)

``frames_to_video`` / ``video_to_frames`` take device tensors only (a CPU tensor raises, like every op).  The two
``reference_*`` functions restate the reference's host arithmetic in torch, op for op; they are what the kernels are tested
against (tests/test_video_io_host.py pins them to the reference itself) and are never called by the product path.

Any clip in, same-size clip out: the reference's command line passes the clip's own size straight through (fast_infer.py:409-423),
so a clip that is no multiple of 16 in the latent's terms, or far larger than what the checkpoints were trained at, has to be
resized on the host first.  ``fit_size`` / ``fit_plan`` choose the size and the geometry (the training loader's resize and
centre crop, videox_fun/data/dataset_image_video.py:464-477), ``fit_frames`` runs it on the device in bytes before
``WanPipeline.__call__`` and ``restore_frames`` brings the edit back to the clip's size after it (``wan_frames_u8_resample``, one
launch each).  The filter is the 8-bit antialiased triangle in integers; ``reference_fit_frames`` restates it
in numpy and is what the kernel equals bit for bit.

Keep what the edit left alone: an edit is local, but the whole clip comes back through the VAE and the DiT (and, after the fit,
upscaled).  ``change_mask`` finds where the edit differs from the frames the pipeline saw, ``composite_frames`` puts the edit back
into the ORIGINAL frames under that mask, ``keep_unedited`` does both (``wan_change_mask``, ``wan_plane_u8_resample``,
``wan_frames_u8_composite``).  Nothing in the reference does this; the definition is ours, in integers:
``reference_change_mask`` / ``reference_composite_frames`` state it in numpy and are what the kernels equal byte for byte.

Edit inside a mask: the other half of ``keep_unedited``, before the fact.  A caller who knows where the edit may happen passes that
mask to ``WanPipeline.__call__(edit_mask=...)`` and the denoising loop itself pins the rest of the clip to its source every step
(DESIGN.md 13.4).  ``fit_mask`` brings the mask of the original clip to the fitted size (``wan_plane_u8_resample``),
``latent_edit_mask`` turns it into per-cell weights (``wan_latent_mask_u8``); ``reference_latent_edit_mask``,
``reference_masked_prediction`` and ``reference_fit_mask`` state the definitions on the host and are what the kernels equal bit for bit.

How far is clip A from clip B: ``clip_stats`` is one pass of integer kernels over two uint8 clips (``wan_clip_stats``) that yields, per
frame and split by a mask, the histogram of byte differences, the histogram of ``change_mask``'s smoothed difference and the sums of
x264's 8-bit SSIM; ``ClipStats`` turns those into PSNR, MAE, quantiles, SSIM and the ``threshold`` for ``change_mask`` on the host.
``vae_roundtrip_frames`` gives the clip a checkpoint's VAE alone makes of a clip, the floor under every such number.
``reference_clip_stats`` states the definition in numpy and is what the kernels equal word for word.

Bring the edit's colours back to the source's: ``color_match`` estimates one gain and offset per frame and RGB channel from the pixels
the edit left alone (``wan_color_stats``, ``wan_color_coef``) and applies it to the whole frame (``wan_frames_u8_affine``), in exact
integers; ``reference_color_match`` and its three steps state the definition in Python ints.  It stands where
the reference's writer has ``color_transfer_post_process``, and is not that function: no LAB, no OpenCV tables.

What the writer makes of more than one sample, and the compare clip: ``grid_frames`` is ``save_videos_grid`` up to the encoder
(videox_fun/utils/utils.py:59-68: the ``make_grid(nrow=6)`` mosaic with its 2-pixel zero border, ``rescale``, the byte conversion)
and ``compare_frames`` is ``save_side_by_side`` (fast_infer.py:183-206: ``_normalize_to_01`` of source and edit, the crop to the
common T/H/W, ``torch.cat(dim=4)``) followed by that writer -- both one launch of ``wan_frames_u8_compose`` per clip, the range
rule of ``_normalize_to_01`` decided on the device (``wan_video_range_flag``).  The left half of the compare clip is NOT the
source's bytes: the reference shows ``trunc(((u * (2 / 255) - 1) + 1) / 2 * 255)`` in float32, which moves some byte values.
``reference_grid_frames`` / ``reference_compare_frames`` restate the host code in torch.
"""
from __future__ import annotations

import functools
import math
import os
from dataclasses import dataclass
from fractions import Fraction
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import ops

__all__ = ["frames_to_video", "video_to_frames", "load_video_frames", "reference_frames_to_video", "reference_video_to_frames",
           "fit_size", "fit_plan", "FitPlan", "fit_frames", "restore_frames", "reference_fit_frames",
           "change_mask", "composite_frames", "keep_unedited", "reference_change_mask", "reference_composite_frames",
           "latent_edit_mask", "fit_mask", "reference_latent_edit_mask", "reference_masked_prediction", "reference_fit_mask",
           "ClipStats", "clip_stats", "reference_clip_stats", "vae_roundtrip_frames",
           "color_match", "color_match_coefficients", "reference_color_match", "reference_color_stats", "reference_color_coefficients",
           "reference_frames_affine",
           "grid_layout", "grid_frames", "compare_frames", "reference_grid_frames", "reference_compare_frames",
           "select_frame_indices", "yuv_matrix", "chroma_shape", "yuv_to_frames", "frames_to_yuv", "reference_yuv_to_frames",
           "reference_frames_to_yuv", "YuvClip", "read_y4m", "load_y4m_frames", "write_y4m"]

COEF_BITS = 22                  # fixed-point bits of a filter coefficient: 8 + 22 bits of product and a sum of weights of 1 fit 32 bits
MAX_TAPS = 24                   # WAN_RESAMPLE_MAX_TAPS of include/wan_hip.h: an 11x downscale


def frames_to_video(frames_u8: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """uint8 ``[B, T, H, W, 3]`` or ``[T, H, W, 3]`` on the device -> ``[B, 3, T, H, W]`` in ``dtype`` (bfloat16 | float32):
    bit for bit ``load_video_frames``' float32 video (fast_infer.py:88-90) cast once to ``dtype``."""
    if frames_u8.dim() == 4:
        frames_u8 = frames_u8.unsqueeze(0)
    return ops.frames_u8_to_video(frames_u8, dtype)


def video_to_frames(video: torch.Tensor, out: Optional[torch.Tensor] = None, frame_range: Optional[Tuple[int, int]] = None,
                    dst_frame: int = 0) -> torch.Tensor:
    """The decoder's ``[B, 3, T, H, W]`` (the VAE's dtype) on the device -> uint8 ``[B, T, H, W, 3]`` on the device, the bytes
    ``save_videos_grid`` writes.  ``frame_range`` / ``out`` / ``dst_frame``: see ``ops.video_to_frames_u8``."""
    return ops.video_to_frames_u8(video, out, frame_range, dst_frame)


def reference_frames_to_video(frames_u8: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """fast_infer.py:88-90 in torch on whatever device holds ``frames_u8`` ([B, T, H, W, 3]), then the cast the pipeline applies
    (``video.to(dtype)``, pipeline_wan.py:397)."""
    x = frames_u8.permute(0, 4, 1, 2, 3).float()
    x = x * (2.0 / 255.0) - 1.0
    return x.to(dtype).contiguous()


def reference_video_to_frames(video: torch.Tensor) -> torch.Tensor:
    """pipeline_wan.py:426-427 in the video's dtype, then utils.py:60-67 for one video per call: uint8 [B, T, H, W, 3].
    (``astype(np.uint8)`` of a float32 in [0, 255] truncates; ``.to(torch.uint8)`` does the same.)"""
    x = (video / 2 + 0.5).clamp(0, 1).float()
    x = x.permute(0, 2, 3, 4, 1)
    return (x * 255).to(torch.uint8).contiguous()


def select_frame_indices(total: int, source_frames: int, generator: Optional[torch.Generator] = None) -> list:
    """The frames fast_infer.py:60-80 picks of a clip of ``total`` frames: ``stride = max(1, total // source_frames)``, the start
    frame one draw of ``torch.randint`` (the global generator unless ``generator`` is given), ``start + i * stride`` while they
    exist, the last one repeated up to ``source_frames``; ``[]`` for an empty clip.  The one rule ``load_video_frames`` and
    ``load_y4m_frames`` share: the same seed picks the same frames."""
    total, source_frames = int(total), int(source_frames)
    stride = max(1, total // source_frames)
    start = int(torch.randint(0, max(1, total - stride * source_frames), (1,), generator=generator)[0].item())
    idx = [start + i * stride for i in range(source_frames) if start + i * stride < total]
    if idx:
        idx += [idx[-1]] * (source_frames - len(idx))
    return idx


def load_video_frames(video: Union[str, np.ndarray, torch.Tensor], source_frames: int,
                      generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, int, int]:
    """fast_infer.py:43-92 without the float conversion: ``source_frames`` frames of a clip as uint8 ``[T, H, W, 3]``.

    ``video``: a uint8 ``[N, H, W, 3]`` array / tensor of all decoded frames, or a path (read through ``imageio`` if it is
    installed -- it is optional).  As the reference: ``stride = max(1, N // source_frames)``, start frame drawn by
    ``torch.randint(0, max(1, N - stride * source_frames), (1,))`` (the global generator unless ``generator`` is given), frames
    ``start + i * stride`` while they exist, the last one repeated up to ``source_frames`` (an empty clip gives black 480 x 832
    frames).  Returns ``(frames, height, width)`` with the clip's own size: nothing is resized or cropped.  Hand ``frames`` to
    ``WanPipeline.__call__(video=...)``."""
    if source_frames is None or int(source_frames) < 1:
        raise ValueError("load_video_frames: pass source_frames >= 1")
    source_frames = int(source_frames)
    if isinstance(video, (str, bytes)) or hasattr(video, "__fspath__"):
        try:
            import imageio
        except ImportError as e:
            raise RuntimeError("load_video_frames: reading a file needs `imageio` (optional); pass the decoded frames as a "
                               "uint8 [N, H, W, 3] array instead") from e
        reader = imageio.get_reader(video)
        try:
            video = np.stack([np.asarray(f) for f in reader])
        finally:
            reader.close()
    frames = torch.as_tensor(video)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"load_video_frames: expected uint8 [N, H, W, 3] frames, got {frames.dtype} {tuple(frames.shape)}")
    idx = select_frame_indices(int(frames.shape[0]), source_frames, generator)
    if not idx:
        return torch.zeros(source_frames, 480, 832, 3, dtype=torch.uint8), 480, 832
    out = frames[torch.as_tensor(idx, device=frames.device)].contiguous()
    return out, int(out.shape[1]), int(out.shape[2])


# ---------------------------------------------------------------------------------------------- fit any clip to the model's grid
def fit_size(height: int, width: int, max_area: int = 480 * 832, multiple: int = 16) -> Tuple[int, int]:
    """The size a ``height`` x ``width`` clip is run at: its aspect ratio (up to the rounding), both sides multiples of
    ``multiple`` (16 = the VAE's 8 x the spatial patch 2) and ``H * W <= max_area`` (the checkpoints were trained around
    480 x 832).  A clip that already is on that grid and within the area keeps its size.

    Each side is ``sqrt(max_area * ratio)`` rounded down to the grid (at least ``multiple``).  A side whose exact value lies nearer
    to the next multiple then takes that one where the area still allows it, the longer side first: 1080 x 1920 has the exact
    sides 473.96 x 842.60, the floors 464 x 832, and 842.60 is nearer to 848, which fits (464 x 848 <= 480 x 832) -- 480 for the
    height then no longer does.  So no side is more than one grid step from the clip's ratio."""
    height, width, max_area, multiple = int(height), int(width), int(max_area), int(multiple)
    if height < 1 or width < 1 or multiple < 1 or max_area < multiple * multiple:
        raise ValueError(f"fit_size: height={height} width={width} max_area={max_area} multiple={multiple}")
    if height % multiple == 0 and width % multiple == 0 and height * width <= max_area:
        return height, width
    exact = [math.sqrt(max_area * height / width), math.sqrt(max_area * width / height)]
    size = [max(multiple, int(math.floor(e / multiple)) * multiple) for e in exact]
    for i in (0, 1):                        # a side held up at `multiple` (an extreme ratio) is paid for by the other one
        size[i] = max(multiple, min(size[i], max_area // size[1 - i] // multiple * multiple))
    for i in ((0, 1) if height > width else (1, 0)):
        if exact[i] - size[i] > multiple / 2 and (size[i] + multiple) * size[1 - i] <= max_area:
            size[i] += multiple
    return size[0], size[1]


@dataclass(frozen=True)
class FitPlan:
    """Resize by ``scale`` to ``new_height`` x ``new_width``, then keep ``out_height`` x ``out_width`` from ``(y0, x0)`` on.
    ``source_window`` = ``(y, x, h, w)``: the rectangle of the original clip the fitted frame covers."""
    height: int
    width: int
    out_height: int
    out_width: int
    scale: float
    new_height: int
    new_width: int
    y0: int
    x0: int
    source_window: Tuple[int, int, int, int]


def fit_plan(height: int, width: int, out_height: int, out_width: int) -> FitPlan:
    """The training loader's resize and centre crop (videox_fun/data/dataset_image_video.py:464-477): scale so that the frame
    covers the target in both axes, crop the centre."""
    h, w, oh, ow = int(height), int(width), int(out_height), int(out_width)
    if min(h, w, oh, ow) < 1:
        raise ValueError(f"fit_plan: {h} x {w} -> {oh} x {ow}")
    scale = max(oh / h, ow / w)
    new_h, new_w = int(round(h * scale)), int(round(w * scale))
    y0, x0 = max((new_h - oh) // 2, 0), max((new_w - ow) // 2, 0)
    wy = min(max(int(round(y0 / scale)), 0), h - 1)
    wx = min(max(int(round(x0 / scale)), 0), w - 1)
    wh = min(max(int(round(oh / scale)), 1), h - wy)
    ww = min(max(int(round(ow / scale)), 1), w - wx)
    return FitPlan(h, w, oh, ow, scale, new_h, new_w, y0, x0, (wy, wx, wh, ww))


def resample_axis_table(in_size: int, new_size: int, start: int = 0, count: Optional[int] = None):
    """The integer filter of one axis resampled ``in_size -> new_size``, for the output indices ``[start, start + count)``:
    ``(xmin, n, k)`` = int32 ``[count]``, ``[count]``, ``[count, taps]``.  Output ``i`` is
    ``(2**21 + sum_j src[xmin[i] + j] * k[i, j]) >> 22`` clipped to a byte, ``j < n[i]``; ``k`` is zero from ``n[i]`` on and
    ``taps`` = the largest ``n``.  The antialiased triangle of Pillow's 8-bit BILINEAR resample, coefficients in float64."""
    in_size, new_size = int(in_size), int(new_size)
    count = new_size - start if count is None else int(count)
    if in_size < 1 or new_size < 1 or start < 0 or count < 1 or start + count > new_size:
        raise ValueError(f"resample_axis_table: {in_size} -> {new_size}, indices [{start}, {start} + {count})")
    scale = in_size / new_size
    fs = max(scale, 1.0)
    support = fs
    xmin, ns, rows = [], [], []
    for i in range(start, start + count):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - lo
        w = [max(0.0, 1.0 - abs((j + lo - center + 0.5) / fs)) for j in range(n)]
        total = 0.0
        for x in w:
            total += x
        if total != 0.0:
            w = [x / total for x in w]
        xmin.append(lo)
        ns.append(n)
        rows.append([int(0.5 + x * (1 << COEF_BITS)) for x in w])
    taps = max(ns)
    k = np.zeros((count, taps), dtype=np.int32)
    for i, r in enumerate(rows):
        k[i, :len(r)] = r
    return np.asarray(xmin, dtype=np.int32), np.asarray(ns, dtype=np.int32), k


def _resample_axis(x: np.ndarray, axis: int, table) -> np.ndarray:
    """One pass of the definition along ``axis`` of an integer array of bytes, in int64."""
    xmin, n, k = table
    x = np.moveaxis(x, axis, -1)
    idx = np.minimum(xmin[:, None].astype(np.int64) + np.arange(k.shape[1])[None, :], x.shape[-1] - 1)      # k is 0 where j >= n
    acc = (x[..., idx] * k.astype(np.int64)).sum(-1) + (1 << (COEF_BITS - 1))
    return np.moveaxis(np.clip(acc >> COEF_BITS, 0, 255), -1, axis)


def reference_fit_frames(frames_u8, out_height: int, out_width: int, plan: Optional[FitPlan] = None) -> torch.Tensor:
    """The definition of the fit in numpy on the host: uint8 ``[..., H, W, 3]`` -> ``[..., out_height, out_width, 3]``.  Two
    separable passes, horizontal first, the intermediate rounded to a byte; with ``plan`` unset the plan is ``fit_plan`` of the
    two sizes (a ``FitPlan`` without a crop, as ``restore_frames`` uses, resizes straight to the target)."""
    x = torch.as_tensor(frames_u8)
    if x.dtype != torch.uint8 or x.dim() < 3 or x.shape[-1] != 3:
        raise ValueError(f"reference_fit_frames: expected uint8 [..., H, W, 3], got {x.dtype} {tuple(x.shape)}")
    h, w = int(x.shape[-3]), int(x.shape[-2])
    plan = fit_plan(h, w, out_height, out_width) if plan is None else plan
    a = x.cpu().numpy().astype(np.int64)
    a = _resample_axis(a, -2, resample_axis_table(w, plan.new_width, plan.x0, plan.out_width))
    a = _resample_axis(a, -3, resample_axis_table(h, plan.new_height, plan.y0, plan.out_height))
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8)))


def _resize_plan(height: int, width: int, out_height: int, out_width: int) -> FitPlan:
    """A plain resize to the target, no crop (``restore_frames``)."""
    return FitPlan(height, width, out_height, out_width, max(out_height / height, out_width / width), out_height, out_width, 0, 0,
                   (0, 0, height, width))


@functools.lru_cache(maxsize=32)
def _device_table(in_size: int, new_size: int, start: int, count: int, device: str):
    """One axis' table as ``wan_frames_u8_resample`` reads it (include/wan_hip.h): int32 ``xmin[count]``, ``n[count]``,
    ``k[count][taps]``; built once per geometry and device."""
    xmin, n, k = resample_axis_table(in_size, new_size, start, count)
    if k.shape[1] > MAX_TAPS:
        raise RuntimeError(f"resample {in_size} -> {new_size}: {k.shape[1]} filter taps; the kernel is built for {MAX_TAPS} "
                           f"(a downscale of about {MAX_TAPS // 2 - 1}x)")
    packed = torch.from_numpy(np.concatenate([xmin, n, k.ravel()]))
    return packed.to(device), int(k.shape[1])


def _resample(frames: torch.Tensor, plan: FitPlan) -> torch.Tensor:
    dev = str(frames.device)
    xtab, kx = _device_table(plan.width, plan.new_width, plan.x0, plan.out_width, dev)
    ytab, ky = _device_table(plan.height, plan.new_height, plan.y0, plan.out_height, dev)
    return ops.frames_u8_resample(frames, plan.out_height, plan.out_width, xtab, kx, ytab, ky)


def _as_clip(frames_u8, what: str) -> torch.Tensor:
    x = torch.from_numpy(frames_u8) if isinstance(frames_u8, np.ndarray) else frames_u8
    if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() not in (4, 5) or x.shape[-1] != 3:
        raise ValueError(f"{what}: expected uint8 [T, H, W, 3] or [B, T, H, W, 3] frames, got "
                         f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    if not x.is_cuda:
        x = x.to(torch.device("cuda", torch.cuda.current_device()))          # bytes over the host link, as they are
    return x


def fit_frames(frames_u8, height: Optional[int] = None, width: Optional[int] = None,
               max_area: int = 480 * 832) -> Tuple[torch.Tensor, FitPlan]:
    """Fit a clip of any size to a size the model runs at, on the device, in bytes: resize (antialiased triangle) and centre
    crop in one launch.  ``frames_u8``: uint8 ``[T, H, W, 3]`` or ``[B, T, H, W, 3]``, host or device.  The target is
    ``(height, width)`` or, with both unset, ``fit_size`` of the clip's size under ``max_area``.  Returns the device frames,
    which ``WanPipeline.__call__(video=...)`` takes as they are, and the plan (``plan.out_height``, ``plan.out_width`` are the
    ``height`` / ``width`` of that call; ``plan.source_window`` is where the result belongs in the clip).  A clip already at the
    target is returned as it is: nothing is launched."""
    x = _as_clip(frames_u8, "fit_frames")
    h, w = int(x.shape[-3]), int(x.shape[-2])
    if (height is None) != (width is None):
        raise ValueError("fit_frames: pass both `height` and `width`, or neither")
    oh, ow = fit_size(h, w, max_area) if height is None else (int(height), int(width))
    plan = fit_plan(h, w, oh, ow)
    if (oh, ow) == (h, w):
        return x, plan
    out = _resample(x if x.dim() == 5 else x.unsqueeze(0), plan)
    return (out if x.dim() == 5 else out[0]), plan


def restore_frames(frames_u8, height: int, width: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The edit back at the clip's size: the same resample without a crop, from the model's size to ``(height, width)`` (usually
    the size of ``plan.source_window``), on the device.  ``frames_u8``: uint8 ``[T, H, W, 3]`` or ``[B, T, H, W, 3]``.  ``out``: a
    page-locked uint8 host tensor of the result's shape, filled by one copy and returned, as
    ``decode_latents(as_uint8=True)`` fills its ``out``; without it the device frames are returned."""
    x = _as_clip(frames_u8, "restore_frames")
    h, w = int(x.shape[-3]), int(x.shape[-2])
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError(f"restore_frames: height={height} width={width}")
    res = x if (height, width) == (h, w) else _resample(x if x.dim() == 5 else x.unsqueeze(0), _resize_plan(h, w, height, width))
    if x.dim() == 4 and res.dim() == 5:
        res = res[0]
    if out is None:
        return res
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(res.shape) or out.is_cuda or not out.is_contiguous():
        raise ValueError(f"restore_frames: out {out.dtype} {tuple(out.shape)} on {out.device} for uint8 host frames "
                         f"{tuple(res.shape)}")
    out.copy_(res.contiguous(), non_blocking=True)
    torch.cuda.current_stream(res.device).synchronize()
    return out


# ---------------------------------------------------------------------------------------------- keep what the edit left alone
MASK_MAX_SMOOTH, MASK_MAX_GROW, MASK_MAX_GROW_T = 7, 32, 4          # WAN_MASK_MAX_* of include/wan_hip.h


def _mask_args(what: str, threshold, smooth, grow, grow_t, feather) -> Tuple[int, int, int, int, int]:
    v = tuple(int(x) for x in (threshold, smooth, grow, grow_t, feather))
    threshold, smooth, grow, grow_t, feather = v
    if not (0 <= threshold <= 254 and 0 <= smooth <= MASK_MAX_SMOOTH and 0 <= grow <= MASK_MAX_GROW and
            0 <= grow_t <= MASK_MAX_GROW_T and 0 <= feather <= grow):
        raise ValueError(f"{what}: threshold={threshold} (0..254) smooth={smooth} (0..{MASK_MAX_SMOOTH}) grow={grow} "
                         f"(0..{MASK_MAX_GROW}) grow_t={grow_t} (0..{MASK_MAX_GROW_T}) feather={feather} (0..grow)")
    return v


def _box_sum(x: np.ndarray, radius: int, axes, clamp: bool) -> np.ndarray:
    """The exact sum of an int64 array over the ``2 * radius + 1`` window along each of ``axes``, one pass per axis.  Positions outside
    the array repeat its border (``clamp``: clamped indices) or count nothing."""
    for ax in axes:
        ax %= x.ndim
        pad = [(0, 0)] * x.ndim
        pad[ax] = (radius + 1, radius)
        c = np.cumsum(np.pad(x, pad, mode="edge" if clamp else "constant"), axis=ax)      # the extra leading element is subtracted out
        n = x.shape[ax]
        lead = (slice(None),) * ax
        x = c[lead + (slice(2 * radius + 1, 2 * radius + 1 + n),)] - c[lead + (slice(0, n),)]
    return x


def _mask_clips(source_u8, edit_u8, what: str):
    s, e = (torch.as_tensor(v).cpu() for v in (source_u8, edit_u8))
    for x in (s, e):
        if x.dtype != torch.uint8 or x.dim() not in (4, 5) or x.shape[-1] != 3:
            raise ValueError(f"{what}: expected uint8 [T, H, W, 3] or [B, T, H, W, 3] frames, got {x.dtype} {tuple(x.shape)}")
    if s.shape != e.shape:
        raise ValueError(f"{what}: source {tuple(s.shape)} and edit {tuple(e.shape)} differ in shape")
    return s.numpy().astype(np.int64), e.numpy().astype(np.int64)


def reference_change_mask(source_u8, edit_u8, *, threshold: int = 16, smooth: int = 2, grow: int = 12, grow_t: int = 1,
                          feather: int = 8) -> torch.Tensor:
    """The definition of ``change_mask`` in numpy int64 on the host: uint8 ``[T, H, W, 3]`` or
    ``[B, T, H, W, 3]`` source and edit -> uint8 ``[T, H, W]`` / ``[B, T, H, W]``.  What the kernels equal byte for byte; never called
    by the product path."""
    threshold, smooth, grow, grow_t, feather = _mask_args("reference_change_mask", threshold, smooth, grow, grow_t, feather)
    s, e = _mask_clips(source_u8, edit_u8, "reference_change_mask")
    d = np.abs(e - s).max(-1)                                                   # 1. the largest channel difference
    n = (2 * smooth + 1) ** 2
    sm = (2 * _box_sum(d, smooth, (-1, -2), True) + n) // (2 * n)               # 2. its rounded mean over the window, indices clamped
    b = (sm > threshold).astype(np.int64)                                       # 3.
    g = (_box_sum(b, grow, (-1, -2), False) > 0).astype(np.int64)               # 4. the maximum over the window: nothing outside the
    g = (_box_sum(g, grow_t, (-3,), False) > 0).astype(np.int64)                #    frame, nothing outside the sample's T frames
    m = (2 * feather + 1) ** 2
    alpha = (2 * 255 * _box_sum(g, feather, (-1, -2), True) + m) // (2 * m)     # 5. the rounded mean of 255 g, indices clamped
    return torch.from_numpy(np.ascontiguousarray(alpha.astype(np.uint8)))


def _check_composite(what: str, o_shape, e_shape, a_shape, plan: Optional[FitPlan]):
    """-> the window (y, x, h, w) of the original that the edit lands in."""
    o_shape, e_shape, a_shape = tuple(o_shape), tuple(e_shape), tuple(a_shape)
    if len(o_shape) != len(e_shape) or o_shape[:-3] != e_shape[:-3] or a_shape != e_shape[:-1]:
        raise ValueError(f"{what}: original {o_shape}, edit {e_shape}, alpha {a_shape}: expected the same leading sizes and an alpha of "
                         "the edit's [.., T, H, W]")
    if plan is None:
        if o_shape != e_shape:
            raise ValueError(f"{what}: original {o_shape} and edit {e_shape} differ in size; pass the FitPlan of fit_frames")
        return (0, 0, e_shape[-3], e_shape[-2])
    if o_shape[-3:-1] != (plan.height, plan.width) or e_shape[-3:-1] != (plan.out_height, plan.out_width):
        raise ValueError(f"{what}: the plan fits {plan.height} x {plan.width} to {plan.out_height} x {plan.out_width}; got an original "
                         f"of {o_shape[-3:-1]} and an edit of {e_shape[-3:-1]}")
    return tuple(int(v) for v in plan.source_window)


def reference_composite_frames(original_u8, edit_u8, alpha, plan: Optional[FitPlan] = None) -> torch.Tensor:
    """The definition of ``composite_frames`` in numpy int64 on the host: per byte ``(a * e + (255 - a) * o + 127) // 255``.  With
    ``plan`` (the ``FitPlan`` of ``fit_frames``) the edit and ``alpha`` first go to the size of ``plan.source_window`` -- the edit as
    ``restore_frames`` defines it, ``alpha`` through the same two passes and tables, horizontal first, the intermediate rounded to a
    byte -- and the bytes outside the window are the original's.  Never called by the product path."""
    o, e, a = (torch.as_tensor(v).cpu() for v in (original_u8, edit_u8, alpha))
    for x in (o, e, a):
        if x.dtype != torch.uint8:
            raise ValueError(f"reference_composite_frames: expected uint8 tensors, got {x.dtype}")
    if e.dim() not in (4, 5) or e.shape[-1] != 3 or o.shape[-1] != 3:
        raise ValueError(f"reference_composite_frames: expected [T, H, W, 3] or [B, T, H, W, 3] frames, got {tuple(o.shape)} and "
                         f"{tuple(e.shape)}")
    y, x, wh, ww = _check_composite("reference_composite_frames", o.shape, e.shape, a.shape, plan)
    H, W = int(e.shape[-3]), int(e.shape[-2])
    a = a.numpy().astype(np.int64)
    if (wh, ww) != (H, W):
        e = reference_fit_frames(e, wh, ww, _resize_plan(H, W, wh, ww))
        a = _resample_axis(a, -1, resample_axis_table(W, ww))
        a = _resample_axis(a, -2, resample_axis_table(H, wh))
    out = o.numpy().astype(np.int64)
    win = out[..., y:y + wh, x:x + ww, :]
    a = a[..., None]
    out[..., y:y + wh, x:x + ww, :] = (a * e.numpy().astype(np.int64) + (255 - a) * win + 127) // 255
    return torch.from_numpy(np.ascontiguousarray(out.astype(np.uint8)))


def change_mask(source_u8, edit_u8, *, threshold: int = 16, smooth: int = 2, grow: int = 12, grow_t: int = 1,
                feather: int = 8) -> torch.Tensor:
    """Where did the edit change the frames the pipeline saw: a feathered uint8 mask on the device, three launches of integer
    arithmetic (``wan_change_mask``; the definition is ``reference_change_mask``).

    ``source_u8``: the fitted frames handed to ``WanPipeline.__call__``; ``edit_u8``: ``out.edit_videos``; both uint8 ``[T, H, W, 3]``
    or ``[B, T, H, W, 3]`` of one shape, host or device.  Returns ``alpha`` uint8 ``[T, H, W]`` / ``[B, T, H, W]`` on the device: 255
    where the largest channel difference, averaged over ``(2 * smooth + 1)^2`` pixels, exceeds ``threshold``; that region grown by
    ``grow`` pixels and ``grow_t`` frames (within a sample) and its edge softened over ``2 * feather + 1`` pixels; 0 elsewhere.
    Limits: ``0 <= threshold <= 254``, ``smooth <= 7``, ``grow <= 32``, ``grow_t <= 4``, ``feather <= grow`` (so that a changed
    pixel always has alpha 255), else ``ValueError``.

    The defaults are guesses.  The right ``threshold`` sits just above what a VAE round trip alone does to an untouched pixel, which
    depends on the checkpoint and has not been measured: no real weights have been run yet.  Measure it on yours before relying on
    them: ``clip_stats(frames, vae_roundtrip_frames(vae, frames), smooth=smooth).threshold_for()`` is that ``threshold``, computed on
    the device."""
    args = _mask_args("change_mask", threshold, smooth, grow, grow_t, feather)
    s, e = _as_clip(source_u8, "change_mask.source"), _as_clip(edit_u8, "change_mask.edit")
    if s.shape != e.shape:
        raise ValueError(f"change_mask: source {tuple(s.shape)} and edit {tuple(e.shape)} differ in shape")
    alpha = ops.change_mask(s if s.dim() == 5 else s.unsqueeze(0), e if e.dim() == 5 else e.unsqueeze(0), *args)
    return alpha if s.dim() == 5 else alpha[0]


def composite_frames(original_u8, edit_u8, alpha, plan: Optional[FitPlan] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The edit over the original under ``alpha``, on the device in bytes: ``(a * e + (255 - a) * o + 127) // 255``
    (``wan_frames_u8_composite``; the definition is ``reference_composite_frames``).

    Without ``plan`` the three share ``T, H, W``.  With ``plan`` -- the ``FitPlan`` ``fit_frames`` returned -- ``original_u8`` is the
    clip BEFORE the fit (``[.., plan.height, plan.width, 3]``): inside ``plan.source_window`` the edit is ``restore_frames``' and
    ``alpha`` goes through the same resample as one-channel planes (``wan_plane_u8_resample``); outside it, where the fit cropped the
    frame away, the result is the original's bytes.  ``original_u8`` / ``edit_u8``: uint8 ``[T, H, W, 3]`` or ``[B, T, H, W, 3]``,
    ``alpha``: uint8 ``[T, H, W]`` / ``[B, T, H, W]`` at the edit's size; host or device.  ``out``: a page-locked uint8 host tensor of
    the original's shape, filled by one copy and returned, as in ``restore_frames``; without it the device frames are returned."""
    o, e = _as_clip(original_u8, "composite_frames.original"), _as_clip(edit_u8, "composite_frames.edit")
    a = torch.from_numpy(alpha) if isinstance(alpha, np.ndarray) else alpha
    if not torch.is_tensor(a) or a.dtype != torch.uint8:
        raise ValueError(f"composite_frames.alpha: expected a uint8 tensor, got {getattr(a, 'dtype', type(a))}")
    if not a.is_cuda:
        a = a.to(e.device)
    y, x, wh, ww = _check_composite("composite_frames", o.shape, e.shape, a.shape, plan)
    H, W = int(e.shape[-3]), int(e.shape[-2])
    e, a = e.reshape(-1, H, W, 3), a.reshape(-1, H, W)
    if (wh, ww) != (H, W):
        rp, dev = _resize_plan(H, W, wh, ww), str(e.device)
        xtab, kx = _device_table(rp.width, rp.new_width, 0, ww, dev)
        ytab, ky = _device_table(rp.height, rp.new_height, 0, wh, dev)
        e = ops.frames_u8_resample(e.unsqueeze(0), wh, ww, xtab, kx, ytab, ky)[0]
        a = ops.plane_u8_resample(a, wh, ww, xtab, kx, ytab, ky)
    res = ops.frames_u8_composite(o.reshape(-1, int(o.shape[-3]), int(o.shape[-2]), 3), e, a, (y, x, wh, ww)).view(o.shape)
    return _to_host(res, out, "composite_frames")


def keep_unedited(original_u8, source_u8, edit_u8, plan: Optional[FitPlan] = None, out: Optional[torch.Tensor] = None,
                  **mask_args) -> torch.Tensor:
    """``change_mask(source_u8, edit_u8, **mask_args)`` then ``composite_frames(original_u8, edit_u8, alpha, plan, out)``: the edit
    put back into the original clip, the original's bytes wherever the edit changed nothing.  ``original_u8``: the clip as loaded;
    ``source_u8``, ``plan``: what ``fit_frames`` made of it (``plan=None`` when the clip ran at its own size: then ``source_u8`` is
    ``original_u8``); ``edit_u8``: ``out.edit_videos``."""
    return composite_frames(original_u8, edit_u8, change_mask(source_u8, edit_u8, **mask_args), plan, out)


# ---------------------------------------------------------------------------------------------- edit inside a mask
LATENT_MASK_MAX_GROW, LATENT_MASK_MAX_GROW_T = 4, 2                 # WAN_LATENT_MASK_MAX_* of include/wan_hip.h
LATENT_CELL, LATENT_FRAMES = 8, 4                                   # pixels per latent cell, pixel frames per latent frame


def _latent_mask_args(what: str, grow, grow_t, feather) -> Tuple[int, int, int]:
    for name, v in (("grow", grow), ("grow_t", grow_t), ("feather", feather)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: {name}={v!r} is not an integer")
    grow, grow_t, feather = int(grow), int(grow_t), int(feather)
    if not (0 <= grow <= LATENT_MASK_MAX_GROW and 0 <= grow_t <= LATENT_MASK_MAX_GROW_T and 0 <= feather <= grow):
        raise ValueError(f"{what}: grow={grow} (0..{LATENT_MASK_MAX_GROW} latent cells) grow_t={grow_t} "
                         f"(0..{LATENT_MASK_MAX_GROW_T} latent frames) feather={feather} (0..grow)")
    return grow, grow_t, feather


def _as_mask(alpha_u8, what: str, cells: bool = True) -> torch.Tensor:
    """A uint8 [T, H, W] or [B, T, H, W] mask as a tensor where it is (host or device); ``cells``: H and W are multiples of 8."""
    a = torch.from_numpy(alpha_u8) if isinstance(alpha_u8, np.ndarray) else alpha_u8
    if not torch.is_tensor(a) or a.dtype != torch.uint8 or a.dim() not in (3, 4) or min(a.shape, default=0) < 1:
        raise ValueError(f"{what}: expected a uint8 [T, H, W] or [B, T, H, W] mask, got {getattr(a, 'dtype', type(a))} "
                         f"{tuple(getattr(a, 'shape', ()))}")
    if cells and (a.shape[-2] % LATENT_CELL or a.shape[-1] % LATENT_CELL):
        raise ValueError(f"{what}: a mask of {a.shape[-2]} x {a.shape[-1]} pixels is no whole number of {LATENT_CELL} x {LATENT_CELL} "
                         "latent cells")
    return a


def _dilate(x: np.ndarray, radius: int, axis: int) -> np.ndarray:
    """The maximum over the ``2 * radius + 1`` window along ``axis``; positions outside the array count nothing."""
    n = x.shape[axis]
    out = x.copy()
    for d in range(1, min(radius, n - 1) + 1):
        lo, hi = [slice(None)] * x.ndim, [slice(None)] * x.ndim
        lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
        lo, hi = tuple(lo), tuple(hi)
        out[lo] = np.maximum(out[lo], x[hi])
        out[hi] = np.maximum(out[hi], x[lo])
    return out


def reference_latent_edit_mask(alpha_u8, *, grow: int = 1, grow_t: int = 0, feather: int = 1) -> torch.Tensor:
    """The definition of ``latent_edit_mask`` in numpy int64 on the host: a pixel mask uint8 ``[T, H, W]`` or
    ``[B, T, H, W]`` -> latent-cell weights uint8 ``[Fl, H/8, W/8]`` / ``[B, Fl, H/8, W/8]``, ``Fl = 1 + ceil((T - 1) / 4)``.  What the
    kernels equal byte for byte; never called by the product path."""
    grow, grow_t, feather = _latent_mask_args("reference_latent_edit_mask", grow, grow_t, feather)
    t = _as_mask(alpha_u8, "reference_latent_edit_mask").cpu()
    a = (t if t.dim() == 4 else t.unsqueeze(0)).numpy().astype(np.int64)
    B, T, H, W = a.shape
    h, w = H // LATENT_CELL, W // LATENT_CELL
    Fl = 1 + (T - 1 + LATENT_FRAMES - 1) // LATENT_FRAMES
    cell = a.reshape(B, T, h, LATENT_CELL, w, LATENT_CELL).max(axis=(3, 5))
    p = np.empty((B, Fl, h, w), dtype=np.int64)                                 # 1. the maximum over a cell's pixels and pixel frames:
    p[:, 0] = cell[:, 0]                                                        #    latent frame 0 is pixel frame 0,
    for j in range(1, Fl):                                                      #    latent frame j >= 1 is frames 4j-3 .. min(4j, T-1)
        p[:, j] = cell[:, LATENT_FRAMES * j - (LATENT_FRAMES - 1):min(LATENT_FRAMES * j, T - 1) + 1].max(axis=1)
    g = _dilate(_dilate(p, grow, -1), grow, -2)                                 # 2. grey-scale dilation: nothing outside the frame,
    g = _dilate(g, grow_t, -3)                                                  #    nothing outside the sample's Fl frames
    m = (2 * feather + 1) ** 2
    out = (2 * _box_sum(g, feather, (-1, -2), True) + m) // (2 * m)             # 3. change_mask's step 5 at cell resolution
    out = torch.from_numpy(np.ascontiguousarray(out.astype(np.uint8)))
    return out if t.dim() == 4 else out[0]


def latent_edit_mask(alpha_u8, *, grow: int = 1, grow_t: int = 0, feather: int = 1) -> torch.Tensor:
    """Where may the edit happen, in the latents' terms: a pixel mask as the per-cell weights ``WanPipeline.__call__(edit_mask=...)``
    blends the prediction with, on the device (``wan_latent_mask_u8``; the definition is ``reference_latent_edit_mask``).

    ``alpha_u8``: uint8 ``[T, H, W]`` or ``[B, T, H, W]`` at the size the pipeline runs at (``fit_mask`` brings the mask of the original
    clip there), host or device; 255 = edit freely, 0 = keep the source.  Returns uint8 ``[Fl, H/8, W/8]`` / ``[B, Fl, H/8, W/8]`` on
    the device: per latent cell the largest mask value of its 8 x 8 pixels and its pixel frames, grown by ``grow`` cells and ``grow_t``
    latent frames (within a sample), the edge softened over ``2 * feather + 1`` cells.  Limits: ``grow <= 4``, ``grow_t <= 2``,
    ``feather <= grow`` (so that a cell holding a 255 pixel keeps weight 255), ``H`` and ``W`` multiples of 8, else ``ValueError``.

    The defaults are guesses: one cell (8 pixels) of margin and of feather around the mask.  No real checkpoint has been run with
    them and no quality is claimed; ``clip_stats`` of the result against the source, split by the mask, is the tool for judging
    them on yours."""
    args = _latent_mask_args("latent_edit_mask", grow, grow_t, feather)
    a = _as_mask(alpha_u8, "latent_edit_mask")
    if not a.is_cuda:
        a = a.to(torch.device("cuda", torch.cuda.current_device()))              # bytes over the host link, as they are
    out = ops.latent_mask(a if a.dim() == 4 else a.unsqueeze(0), *args)
    return out if a.dim() == 4 else out[0]


def reference_masked_prediction(pred, sample, weights, Fs: int, target_frame0: int, sigma: float) -> torch.Tensor:
    """The definition of ``ops.masked_prediction_`` in torch float32 on the host, one operation per line: returns the
    new prediction (nothing is changed in place).  ``pred``, ``sample``: ``[B, C, F, h, w]`` of one dtype (fp32 or bf16), ``weights``:
    uint8 ``[Bm, Fs, h, w]`` with ``Bm`` in {1, B}.  What the kernel equals bit for bit; never called by the product path."""
    p, x, a = (torch.as_tensor(t).cpu() for t in (pred, sample, weights))
    Fs, t0 = int(Fs), int(target_frame0)
    if p.dtype not in (torch.float32, torch.bfloat16) or x.dtype != p.dtype or p.dim() != 5 or x.shape != p.shape:
        raise ValueError(f"reference_masked_prediction: expected two [B, C, F, h, w] tensors of one dtype (fp32 or bf16), got {p.dtype} "
                         f"{tuple(p.shape)} and {x.dtype} {tuple(x.shape)}")
    B, _, F, h, w = p.shape
    if a.dtype != torch.uint8 or a.dim() != 4 or tuple(a.shape[1:]) != (Fs, h, w) or a.shape[0] not in (1, B):
        raise ValueError(f"reference_masked_prediction: expected uint8 weights [1 or {B}, {Fs}, {h}, {w}], got {a.dtype} {tuple(a.shape)}")
    if Fs < 1 or t0 < Fs or t0 + Fs > F:
        raise ValueError(f"reference_masked_prediction: Fs={Fs} source frames and the target at [{t0}, {t0} + {Fs}) do not fit {F} frames")
    sig = torch.tensor(float(sigma), dtype=torch.float32)
    if not bool(sig > 0) or not bool(torch.isfinite(sig)):
        raise ValueError(f"reference_masked_prediction: sigma={sigma} (a finite value above 0)")
    a = a[:, None]                                                               # shared by the channels
    v = p[:, :, t0:t0 + Fs].float()
    xt = x[:, :, t0:t0 + Fs].float()
    s = x[:, :, :Fs].float()
    wgt = a.float() / torch.tensor(255.0, dtype=torch.float32)
    d = xt - s
    r = d / sig                                                                  # the prediction whose x0 = xt - sigma * r is the source
    inside = wgt * v
    rest = 1.0 - wgt
    outside = rest * r
    new = (inside + outside).to(p.dtype)                                         # one rounding to the tensors' dtype (nearest even)
    out = p.clone()
    out[:, :, t0:t0 + Fs] = torch.where(a == 255, p[:, :, t0:t0 + Fs], new)      # weight 255: not written
    return out


def _check_fit_mask(what: str, a: torch.Tensor, plan: FitPlan) -> None:
    if not isinstance(plan, FitPlan):
        raise ValueError(f"{what}: `plan` is the FitPlan fit_frames returned, got {type(plan).__name__}")
    if tuple(a.shape[-2:]) != (plan.height, plan.width):
        raise ValueError(f"{what}: the plan fits {plan.height} x {plan.width} to {plan.out_height} x {plan.out_width}; got a mask of "
                         f"{tuple(a.shape[-2:])} (expected [.., T, {plan.height}, {plan.width}])")


def reference_fit_mask(alpha_u8, plan: FitPlan) -> torch.Tensor:
    """The definition of ``fit_mask`` in numpy int64 on the host: ``reference_fit_frames``' two passes and tables (horizontal first, the
    intermediate rounded to a byte, the plan's crop window) on a one-channel plane.  Never called by the product path."""
    t = _as_mask(alpha_u8, "reference_fit_mask", cells=False).cpu()
    _check_fit_mask("reference_fit_mask", t, plan)
    a = t.numpy().astype(np.int64)
    a = _resample_axis(a, -1, resample_axis_table(plan.width, plan.new_width, plan.x0, plan.out_width))
    a = _resample_axis(a, -2, resample_axis_table(plan.height, plan.new_height, plan.y0, plan.out_height))
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8)))


def fit_mask(alpha_u8, plan: FitPlan) -> torch.Tensor:
    """The mask of the ORIGINAL clip at the size ``fit_frames`` brought the clip to, on the device: the same crop window, tables and two
    passes as the frames, as a one-channel plane (``wan_plane_u8_resample``; the definition is ``reference_fit_mask``).  ``alpha_u8``:
    uint8 ``[T, plan.height, plan.width]`` or ``[B, T, ..]``, host or device; ``plan``: what ``fit_frames`` returned.  The result
    (``[.., T, plan.out_height, plan.out_width]``) is the mask both ``WanPipeline.__call__(edit_mask=...)`` and the final
    ``composite_frames(original, edit, alpha, plan)`` take.  A mask already at the target is returned as it is: nothing is launched."""
    a = _as_mask(alpha_u8, "fit_mask", cells=False)
    _check_fit_mask("fit_mask", a, plan)
    if not a.is_cuda:
        a = a.to(torch.device("cuda", torch.cuda.current_device()))
    if (plan.out_height, plan.out_width) == (plan.height, plan.width):
        return a
    dev = str(a.device)
    xtab, kx = _device_table(plan.width, plan.new_width, plan.x0, plan.out_width, dev)
    ytab, ky = _device_table(plan.height, plan.new_height, plan.y0, plan.out_height, dev)
    out = ops.plane_u8_resample(a.reshape(-1, plan.height, plan.width), plan.out_height, plan.out_width, xtab, kx, ytab, ky)
    return out.view(tuple(a.shape[:-2]) + (plan.out_height, plan.out_width))


# ---------------------------------------------------------------------------------------------- how far is clip A from clip B
SSIM_C1, SSIM_C2, SSIM_ONE = 416, 235963, 1 << 20       # x264 / ffmpeg's 8-bit constants for 64 pixels; the fixed point of a window's q


@dataclass(frozen=True)
class ClipStats:
    """Exact integer statistics of two uint8 clips per frame, split into region 0 (alpha == 0, or no alpha) and region 1 (alpha != 0):
    what ``wan_clip_stats`` computes (include/wan_hip.h).  ``..`` is nothing for ``[T, H, W, 3]`` clips and ``B``
    for a batch.  The methods are host arithmetic on these arrays and nothing else, so ``clip_stats`` and ``reference_clip_stats``
    share them.  ``region``: 0, 1 or None (both pooled); ``per_frame=False`` pools the frame axis (a batch keeps its samples)."""
    diff_hist: np.ndarray            # int64 [.., T, 2, 256]: bytes (all channels) with |a - b| == v
    smooth_hist: np.ndarray          # int64 [.., T, 2, 256]: pixels whose smoothed difference (change_mask's steps 1-2) == v
    ssim_sum: np.ndarray             # int64 [.., T, 2]: the sum of the windows' q, 2^20 = identical
    ssim_windows: np.ndarray         # int64 [.., T, 2]: the number of windows, all three colour planes
    smooth: int

    @staticmethod
    def _pool(x: np.ndarray, region, per_frame: bool, axis: int) -> np.ndarray:
        """``x``: [.., T, 2, (256)] with the region at ``axis`` -> [.., T, (256)] or, pooled over the frames, [.., (256)]."""
        if region is not None and int(region) not in (0, 1):
            raise ValueError(f"ClipStats: region={region!r} (0, 1 or None)")
        x = x.sum(axis) if region is None else np.take(x, int(region), axis=axis)
        return x if per_frame else x.sum(axis)               # the frame axis has moved to where the region was

    def _diff(self, region, per_frame):
        h = self._pool(self.diff_hist, region, per_frame, -2)
        return h, h.sum(-1), np.arange(256, dtype=np.int64)

    def psnr(self, region=None, per_frame: bool = True) -> np.ndarray:
        """``10 log10(255^2 count / SSE)`` in float64 over the bytes; ``inf`` where the SSE is 0, ``nan`` where there are no bytes."""
        h, count, v = self._diff(region, per_frame)
        sse = (h * v * v).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = 10.0 * np.log10(65025.0 * count / sse)
        return np.where(count == 0, np.nan, np.where(sse == 0, np.inf, out))

    def mae(self, region=None, per_frame: bool = True) -> np.ndarray:
        """The mean absolute byte difference in float64; ``nan`` where there are no bytes."""
        h, count, v = self._diff(region, per_frame)
        with np.errstate(invalid="ignore"):
            return np.where(count == 0, np.nan, (h * v).sum(-1) / count)

    def max_diff(self, region=None, per_frame: bool = True) -> np.ndarray:
        """The largest absolute byte difference (int64; 0 where there are no bytes)."""
        h, _, v = self._diff(region, per_frame)
        return np.where(h > 0, v, 0).max(-1)

    def quantile(self, q: float, region=None, per_frame: bool = True) -> np.ndarray:
        """The smallest ``v`` such that ``ceil(q count)`` bytes differ by at most ``v`` (int64; 0 where there are no bytes)."""
        if not 0.0 <= float(q) <= 1.0:
            raise ValueError(f"ClipStats.quantile: q={q!r} (0..1)")
        h, count, _ = self._diff(region, per_frame)
        need = np.ceil(float(q) * count).astype(np.int64)
        return (np.cumsum(h, -1) >= need[..., None]).argmax(-1).astype(np.int64)

    def ssim(self, region=None, per_frame: bool = True) -> np.ndarray:
        """The mean SSIM of the region's 8 x 8 windows over the three colour planes, ``ssim_sum / (2^20 ssim_windows)`` in float64;
        ``nan`` without windows."""
        s, n = (self._pool(x, region, per_frame, -1) for x in (self.ssim_sum, self.ssim_windows))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n == 0, np.nan, s / (float(SSIM_ONE) * n))

    def threshold_for(self, max_changed: float = 1e-3, region=None) -> int:
        """The ``threshold`` for ``change_mask(..., smooth=self.smooth)`` under which these two clips count as unchanged: the smallest
        ``t`` in 0..254 such that the pixels with a smoothed difference above ``t``, over all frames (and samples), number at most
        ``floor(max_changed * pixels)``; 254 if none does.  Run it on a clip and its ``vae_roundtrip_frames``."""
        h = self._pool(self.smooth_hist, region, True, -2).reshape(-1, 256).sum(0)
        above = int(h.sum()) - np.cumsum(h)                                      # above[t]: pixels with s > t
        ok = np.nonzero(above[:255] <= math.floor(float(max_changed) * int(h.sum())))[0]
        return int(ok[0]) if ok.size else 254


def _stats_smooth(what: str, smooth) -> int:
    smooth = int(smooth)
    if not 0 <= smooth <= MASK_MAX_SMOOTH:
        raise ValueError(f"{what}: smooth={smooth} (0..{MASK_MAX_SMOOTH})")
    return smooth


def _stats_alpha(what: str, alpha, shape):
    """-> alpha as a uint8 tensor of the clips' [.., T, H, W], or None."""
    if alpha is None:
        return None
    a = torch.from_numpy(alpha) if isinstance(alpha, np.ndarray) else alpha
    if not torch.is_tensor(a) or a.dtype != torch.uint8 or tuple(a.shape) != tuple(shape[:-1]):
        raise ValueError(f"{what}: alpha {getattr(a, 'dtype', type(a))} {tuple(getattr(a, 'shape', ()))} for clips {tuple(shape)}: "
                         f"expected uint8 {tuple(shape[:-1])}")
    return a


def _clip_stats_of(words: np.ndarray, lead, smooth: int) -> ClipStats:
    """int64 [N, 2, 514] as the kernel lays it out -> ClipStats with the clips' leading sizes."""
    w = np.ascontiguousarray(words).reshape(*lead, 2, ops.CLIP_STATS_WORDS)
    return ClipStats(w[..., :256].copy(), w[..., 256:512].copy(), w[..., 512].copy(), w[..., 513].copy(), smooth)


def reference_clip_stats(a_u8, b_u8, alpha=None, *, smooth: int = 2) -> ClipStats:
    """The definition of ``clip_stats`` in numpy int64 (float64 for the one division of an SSIM window) on the host, DESIGN.md section
    4.3.4.  What the kernels equal word for word; never called by the product path."""
    smooth = _stats_smooth("reference_clip_stats", smooth)
    a, b = _mask_clips(a_u8, b_u8, "reference_clip_stats")
    al = _stats_alpha("reference_clip_stats", alpha, a.shape)
    lead, (H, W) = a.shape[:-3], a.shape[-3:-1]
    a, b = a.reshape(-1, H, W, 3), b.reshape(-1, H, W, 3)
    N = a.shape[0]
    region = np.zeros((N, H, W), np.int64) if al is None else (al.cpu().numpy().reshape(N, H, W) != 0).astype(np.int64)
    frame = np.arange(N, dtype=np.int64)[:, None, None]
    words = np.zeros((N, 2, ops.CLIP_STATS_WORDS), np.int64)

    diff = np.abs(a - b)                                                        # the byte histogram
    key = ((frame * 2 + region)[..., None] * 256 + diff).ravel()
    words[:, :, :256] = np.bincount(key, minlength=N * 512).reshape(N, 2, 256)

    n = (2 * smooth + 1) ** 2                                                   # the smoothed histogram: reference_change_mask's steps 1-2
    sm = (2 * _box_sum(diff.max(-1), smooth, (-1, -2), True) + n) // (2 * n)
    key = ((frame * 2 + region) * 256 + sm).ravel()
    words[:, :, 256:512] = np.bincount(key, minlength=N * 512).reshape(N, 2, 256)

    h4, w4 = H >> 2, W >> 2                                                     # SSIM
    if h4 >= 2 and w4 >= 2:
        def blocks(x):                                                          # [N, 4 h4, 4 w4, ..] -> the 4 x 4 blocks' sums
            x = x[:, :4 * h4, :4 * w4]
            return x.reshape(N, h4, 4, w4, 4, *x.shape[3:]).sum((2, 4))

        def windows(x):                                                         # 2 x 2 neighbouring blocks
            return x[:, :-1, :-1] + x[:, 1:, :-1] + x[:, :-1, 1:] + x[:, 1:, 1:]

        s1, s2, ss, s12 = (windows(blocks(x)) for x in (a, b, a * a + b * b, a * b))
        vars_, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
        f = [x.astype(np.float64) for x in (2 * s1 * s2 + SSIM_C1, 2 * covar + SSIM_C2, s1 * s1 + s2 * s2 + SSIM_C1, vars_ + SSIM_C2)]
        q = np.rint((f[0] * f[1]) / (f[2] * f[3]) * float(SSIM_ONE)).astype(np.int64).sum(-1)      # [N, h4 - 1, w4 - 1]: three planes
        wr = (windows(blocks(region)) != 0).astype(np.int64)
        for r in (0, 1):
            words[:, r, 512] = np.where(wr == r, q, 0).sum((1, 2))
            words[:, r, 513] = 3 * (wr == r).sum((1, 2))
    return _clip_stats_of(words, lead, smooth)


def clip_stats(a_u8, b_u8, alpha=None, *, smooth: int = 2) -> ClipStats:
    """How far is clip ``b_u8`` from clip ``a_u8``: one pass of integer kernels over the two clips on the device
    (``wan_clip_stats``, four launches; the definition is ``reference_clip_stats``), then one copy of ``T * 2 * 514`` words to the
    host.  PSNR, MAE, the maximum, quantiles, SSIM and the ``threshold`` for ``change_mask`` follow from those on the host
    (``ClipStats``), each for the pixels where ``alpha`` is 0 and where it is not.

    ``a_u8``, ``b_u8``: uint8 ``[T, H, W, 3]`` or ``[B, T, H, W, 3]`` of one shape, host or device; ``alpha``: uint8 ``[T, H, W]`` /
    ``[B, T, H, W]`` as ``change_mask`` returns it, or None (everything is region 0); ``0 <= smooth <= 7``, else ``ValueError``."""
    smooth = _stats_smooth("clip_stats", smooth)
    a, b = _as_clip(a_u8, "clip_stats.a"), _as_clip(b_u8, "clip_stats.b")
    if a.shape != b.shape:
        raise ValueError(f"clip_stats: a {tuple(a.shape)} and b {tuple(b.shape)} differ in shape")
    al = _stats_alpha("clip_stats", alpha, a.shape)
    if al is not None:
        al = al.to(a.device)
    a5, b5, al5 = (x if x is None or a.dim() == 5 else x.unsqueeze(0) for x in (a, b, al))
    return _clip_stats_of(ops.clip_stats(a5, b5, al5, smooth).cpu().numpy(), a.shape[:-3], smooth)


def vae_roundtrip_frames(vae, frames_u8) -> torch.Tensor:
    """The bytes ``WanPipeline`` would return for a clip if the DiT changed nothing: frames -> video -> the mode of the VAE's
    posterior -> decoded -> frames, in the VAE's dtype, on the device.  ``frames_u8``: uint8 ``[T, H, W, 3]`` or ``[B, T, H, W, 3]``,
    host or device; returns device frames of the same shape.  ``clip_stats(frames, vae_roundtrip_frames(vae, frames))`` is the error
    floor of a checkpoint in pixels, and its ``threshold_for()`` the ``threshold`` that ``change_mask`` needs to ignore it."""
    x = _as_clip(frames_u8, "vae_roundtrip_frames")
    video = ops.frames_u8_to_video(x if x.dim() == 5 else x.unsqueeze(0), vae.dtype)
    latents = torch.cat([vae.encode(video[i:i + 1])[0].mode() for i in range(video.shape[0])])
    frames = ops.video_to_frames_u8(vae.decode(latents.to(vae.dtype)).sample)
    return frames if x.dim() == 5 else frames[0]


# ---------------------------------------------------------------------------------------------- colour match
COLOR_ONE, COLOR_MAX_POOL_T = ops.COLOR_ONE, ops.COLOR_MAX_POOL_T


def _color_args(what: str, pool_t, gain, min_pixels) -> Tuple[int, bool, int]:
    if isinstance(pool_t, bool) or not isinstance(pool_t, (int, np.integer)) or not 0 <= int(pool_t) <= COLOR_MAX_POOL_T:
        raise ValueError(f"{what}: pool_t={pool_t!r} (an int, 0..{COLOR_MAX_POOL_T})")
    if isinstance(min_pixels, bool) or not isinstance(min_pixels, (int, np.integer)) or not 0 <= int(min_pixels) < 2 ** 31:
        raise ValueError(f"{what}: min_pixels={min_pixels!r} (an int, 0..2^31 - 1)")
    if not isinstance(gain, (bool, np.bool_)):
        raise ValueError(f"{what}: gain={gain!r} (True or False)")
    return int(pool_t), bool(gain), int(min_pixels)


def _color_clips(what: str, edit, ref, alpha):
    """The three as tensors ``[B, T, H, W, 3]``, ``[B, T or 1, H, W, 3]`` and ``[B, T or 1, H, W]`` / None (views, wherever they
    live), and the edit's leading sizes."""
    e, r = (torch.from_numpy(v) if isinstance(v, np.ndarray) else v for v in (edit, ref))
    if not torch.is_tensor(e) or e.dtype != torch.uint8 or e.dim() not in (4, 5) or e.shape[-1] != 3:
        raise ValueError(f"{what}: edit_u8: expected uint8 [T, H, W, 3] or [B, T, H, W, 3] frames, got "
                         f"{getattr(e, 'dtype', type(e))} {tuple(getattr(e, 'shape', ()))}")
    lead = tuple(e.shape[:-3])
    e5 = e if e.dim() == 5 else e.unsqueeze(0)
    B, T, H, W, _ = (int(v) for v in e5.shape)
    if not torch.is_tensor(r) or r.dtype != torch.uint8:
        raise ValueError(f"{what}: ref_u8: expected a uint8 tensor, got {getattr(r, 'dtype', type(r))}")
    one_frame = r.dim() == 3 and e.dim() == 4                                   # [H, W, 3] for the clip, its alpha [H, W]
    if one_frame:
        r = r[None]
    if tuple(r.shape) not in (tuple(e.shape), lead[:-1] + (1, H, W, 3)):
        raise ValueError(f"{what}: ref_u8 {tuple(r.shape)} for an edit {tuple(e.shape)}: expected the edit's shape, or one frame per "
                         f"sample ({'[H, W, 3] or [1, H, W, 3]' if e.dim() == 4 else '[B, 1, H, W, 3]'})")
    r5 = r if r.dim() == 5 else r.unsqueeze(0)
    a4 = None
    if alpha is not None:
        a = torch.from_numpy(alpha) if isinstance(alpha, np.ndarray) else alpha
        if torch.is_tensor(a) and a.dim() == 2 and one_frame:
            a = a[None]
        if not torch.is_tensor(a) or a.dtype != torch.uint8 or tuple(a.shape) != tuple(r.shape[:-1]):
            raise ValueError(f"{what}: alpha {getattr(a, 'dtype', type(a))} {tuple(getattr(a, 'shape', ()))} for a ref_u8 "
                             f"{tuple(r.shape)}: expected uint8 {tuple(r.shape[:-1])}")
        a4 = a if a.dim() == 4 else a.unsqueeze(0)
    return e5, r5, a4, lead


def reference_color_stats(ref_u8, edit_u8, alpha=None) -> np.ndarray:
    """The sums ``color_match`` estimates from, in numpy int64 on the host: int64 ``[.., T, 16]`` = per frame
    ``n``, then ``A, E, AA, EE`` per channel -- the sums of ``ref``, of ``edit`` and of their squares over the pixels whose ``alpha``
    is 0 -- and three zero words.  What ``wan_color_stats`` equals word for word; never called by the product path."""
    e, r, a, lead = _color_clips("reference_color_stats", *(None if v is None else torch.as_tensor(v).cpu() for v in (edit_u8, ref_u8, alpha)))
    e, r = e.numpy().astype(np.int64), r.numpy().astype(np.int64)
    B, T, H, W, _ = e.shape
    r = np.broadcast_to(r, e.shape)
    on = np.ones((B, T, H, W, 1), np.int64) if a is None else np.broadcast_to((a.numpy() == 0).astype(np.int64)[..., None], (B, T, H, W, 1))
    words = np.zeros((B, T, ops.COLOR_STATS_WORDS), np.int64)
    words[..., 0] = on.sum((2, 3, 4))
    for k, x in enumerate((r, e, r * r, e * e)):
        words[..., 1 + k:13:4] = (x * on).sum((2, 3))
    return words.reshape(*lead, ops.COLOR_STATS_WORDS)


def reference_color_coefficients(stats, *, pool_t: int = 2, gain: bool = True, min_pixels: int = 1024) -> np.ndarray:
    """``(g, b)`` per frame and channel from the sums of ``reference_color_stats``, in Python ints: int64 ``[.., T, 16]`` -> int32
    ``[.., T, 3, 2]``.  The sums of frame ``t`` are pooled over frames ``t - pool_t .. t + pool_t`` of its sample; then, with
    ``ONE = 4096``: below ``max(1, min_pixels)`` counted pixels ``(ONE, 0)``; else ``g = isqrt(((Vs >> k) << 24) // (Ve >> k))``
    clamped to ``[ONE / 2, 2 * ONE]`` with ``Vs = n * AA - A * A``, ``Ve = n * EE - E * E`` and ``k`` what brings the larger to 38
    bits (``ONE`` where ``gain`` is off or ``Ve == 0``, ``2 * ONE`` where the shift leaves nothing of ``Ve``), and
    ``b = (ONE * A - g * E + n // 2) // n``.  What ``wan_color_coef`` equals word for word."""
    pool_t, gain, min_pixels = _color_args("reference_color_coefficients", pool_t, gain, min_pixels)
    s = np.asarray(stats.cpu() if torch.is_tensor(stats) else stats)
    if s.dtype != np.int64 or s.ndim not in (2, 3) or s.shape[-1] != ops.COLOR_STATS_WORDS:
        raise ValueError(f"reference_color_coefficients: stats: expected int64 [T, 16] or [B, T, 16], got {s.dtype} {s.shape}")
    lead = s.shape[:-1]
    s3 = s.reshape(-1, lead[-1], ops.COLOR_STATS_WORDS)
    T, ONE = s3.shape[1], COLOR_ONE
    coef = np.zeros((s3.shape[0], T, 3, 2), np.int32)
    for bi in range(s3.shape[0]):
        for t in range(T):
            pooled = [sum(int(s3[bi, u, w]) for u in range(max(t - pool_t, 0), min(t + pool_t, T - 1) + 1)) for w in range(13)]
            n = pooled[0]
            for c in range(3):
                A, E, AA, EE = pooled[1 + 4 * c:5 + 4 * c]
                g, b = ONE, 0
                if n >= max(1, min_pixels):
                    Vs, Ve = n * AA - A * A, n * EE - E * E
                    if gain and Ve != 0:
                        k = max(0, max(Vs, Ve).bit_length() - 38)
                        vs, ve = Vs >> k, Ve >> k
                        g = 2 * ONE if ve == 0 else math.isqrt((vs << 24) // ve)
                        g = min(max(g, ONE // 2), 2 * ONE)
                    b = (ONE * A - g * E + (n >> 1)) // n
                coef[bi, t, c] = (g, b)
    return coef.reshape(*lead, 3, 2)


def reference_frames_affine(frames_u8, coef) -> torch.Tensor:
    """``clamp((g * x + b + 2048) >> 12, 0, 255)`` per byte in numpy int64: uint8 ``[.., H, W, 3]`` frames and int ``[.., 3, 2]``
    coefficients with the same leading sizes.  What ``wan_frames_u8_affine`` equals byte for byte."""
    x = torch.as_tensor(frames_u8).cpu()
    k = np.asarray(coef.cpu() if torch.is_tensor(coef) else coef).astype(np.int64)
    if x.dtype != torch.uint8 or x.dim() < 3 or x.shape[-1] != 3 or k.shape != tuple(x.shape[:-3]) + (3, 2):
        raise ValueError(f"reference_frames_affine: uint8 [.., H, W, 3] frames and [.., 3, 2] coefficients, got {x.dtype} "
                         f"{tuple(x.shape)} and {k.shape}")
    g, b = k[..., None, None, :, 0], k[..., None, None, :, 1]
    y = (g * x.numpy().astype(np.int64) + b + COLOR_ONE // 2) >> 12
    return torch.from_numpy(np.ascontiguousarray(np.clip(y, 0, 255).astype(np.uint8)))


def reference_color_match(edit_u8, ref_u8, alpha=None, *, pool_t: int = 2, gain: bool = True, min_pixels: int = 1024) -> torch.Tensor:
    """The definition of ``color_match`` on the host: ``reference_color_stats``, ``reference_color_coefficients``,
    ``reference_frames_affine``.  Never called by the product path."""
    coef = reference_color_coefficients(reference_color_stats(ref_u8, edit_u8, alpha), pool_t=pool_t, gain=gain, min_pixels=min_pixels)
    return reference_frames_affine(edit_u8, coef)


def _color_coefficients(what: str, edit_u8, ref_u8, alpha, pool_t, gain, min_pixels):
    pool_t, gain, min_pixels = _color_args(what, pool_t, gain, min_pixels)
    e, r, a, lead = _color_clips(what, edit_u8, ref_u8, alpha)
    if not e.is_cuda:
        e = e.to(torch.device("cuda", torch.cuda.current_device()))          # bytes over the host link, as they are
    r, a = r.to(e.device), None if a is None else a.to(e.device)
    return e, ops.color_coef(ops.color_stats(r, e, a), pool_t, gain, min_pixels), lead


def _color_match_segment(seg: torch.Tensor, source_u8: torch.Tensor, mask: Optional[torch.Tensor], args):
    """``WanPipeline(color_match=...)``: the edit segment's device frames ``[B, T, H, W, 3]`` matched IN PLACE to the source frames
    where ``mask`` (``edit_mask``: ``[T, H, W]`` / ``[B, T, H, W]``) is 0 -> the coefficients ``[B, T, 3, 2]``.  ``seg`` may be a frame
    range of a longer clip: a sample's frames are contiguous then, the batch is not, and the samples go one by one (pooling never
    crosses a sample, so that is the same result); one source or mask for several samples is paired with each the same way, without
    a copy.  With ``source_u8`` and ``mask`` on the device this is launches only; tensors on the host are uploaded here first, which
    waits for the stream as every such copy does."""
    B, T, H, W, _ = (int(v) for v in seg.shape)
    src = (source_u8 if source_u8.dim() == 5 else source_u8.unsqueeze(0)).to(seg.device)
    if tuple(src.shape[1:]) != (T, H, W, 3) or src.shape[0] not in (1, B):
        raise ValueError(f"color_match: the edit segment is {tuple(seg.shape)} and the source frames are {tuple(src.shape)}: one "
                         "transform per frame needs a source frame for every edit frame")
    if mask is not None:
        mask = (mask if mask.dim() == 4 else mask.unsqueeze(0)).to(seg.device)
    whole = seg.is_contiguous() and src.shape[0] == B and (mask is None or mask.shape[0] == B)
    coef = torch.empty(B, T, 3, 2, device=seg.device, dtype=torch.int32)
    for b in (slice(0, B),) if whole else (slice(k, k + 1) for k in range(B)):
        one = (lambda t: t[b] if t.shape[0] == B else t)                                # a sample's own source / mask, or the shared one
        n = b.stop - b.start
        ops.color_coef(ops.color_stats(one(src), seg[b], None if mask is None else one(mask)), *args, out=coef[b])
        flat = seg[b].view(n * T, H, W, 3)
        ops.frames_u8_affine(flat, coef[b].view(n * T, 3, 2), out=flat)
    return coef


def color_match_coefficients(edit_u8, ref_u8, alpha=None, *, pool_t: int = 2, gain: bool = True, min_pixels: int = 1024) -> torch.Tensor:
    """The table ``color_match`` applies: int32 ``[T, 3, 2]`` / ``[B, T, 3, 2]`` = ``(g, b)`` per frame and channel on the device, in
    units of 1/4096 (``out = (g * x + b + 2048) >> 12``), for callers who want to look at it or apply it elsewhere
    (``ops.frames_u8_affine``).  The arguments are ``color_match``'s."""
    _, coef, lead = _color_coefficients("color_match_coefficients", edit_u8, ref_u8, alpha, pool_t, gain, min_pixels)
    return coef.view(*lead, 3, 2)


def color_match(edit_u8, ref_u8, alpha=None, *, pool_t: int = 2, gain: bool = True, min_pixels: int = 1024,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Bring the edit's colours back to the reference clip's: per frame and RGB channel one gain and offset, estimated from the pixels
    the edit left alone and applied to the WHOLE frame, on the device in exact integers (``wan_color_stats``, ``wan_color_coef``,
    ``wan_frames_u8_affine``: four launches; the definition is ``reference_color_match``).  The gain is the
    ratio of the standard deviations and the offset what then makes the means equal -- Reinhard's transfer, per RGB channel.

    ``edit_u8``: uint8 ``[T, H, W, 3]`` or ``[B, T, H, W, 3]``, host or device.  ``ref_u8``: the clip to match, of the same shape --
    or ONE frame, ``[H, W, 3]`` / ``[1, H, W, 3]`` / ``[B, 1, H, W, 3]``, which every frame of the sample is then matched to
    (``ref_u8 = edit_u8[:1]`` is the rule of the reference's ``color_transfer_post_process``: every frame towards frame 0).
    ``alpha``: uint8 of ``ref_u8``'s ``[.., H, W]`` as ``change_mask`` returns it, or None: only pixels with ``alpha == 0`` are
    estimated from; None counts all.  ``pool_t``: the sums of a frame are pooled with those of ``pool_t`` frames either side (within
    a sample), ``0 <= pool_t <= 8``; a value of ``T - 1`` or more gives one transform for the clip.  ``gain=False``: offsets only.
    A frame (pooled) with fewer than ``min_pixels`` counted pixels is left as it is.  Else ``ValueError``.  ``out``: a page-locked
    uint8 host tensor of the edit's shape, filled by one copy and returned, as in ``composite_frames``; without it the device
    frames are returned (a new tensor; ``edit_u8`` is not written).

    The defaults ``pool_t=2`` and ``min_pixels=1024`` are guesses: no real checkpoint has been run, so how much the round trip's
    shift wobbles from frame to frame, and how few pixels still give a stable estimate, has not been measured.  Limits: this is RGB
    per channel, so a hue rotation is not corrected; it is one transform per frame, so a shift that varies over the frame is not;
    it is NOT OpenCV's 8-bit LAB transfer, which the reference's writer uses.  No quality is claimed:
    ``clip_stats(source, matched, alpha=mask)`` is the tool to judge the result with."""
    e, coef, lead = _color_coefficients("color_match", edit_u8, ref_u8, alpha, pool_t, gain, min_pixels)
    B, T, H, W, _ = e.shape
    res = ops.frames_u8_affine(e.contiguous().view(B * T, H, W, 3), coef.view(B * T, 3, 2)).view(*lead, H, W, 3)
    return _to_host(res, out, "color_match")


# ---------------------------------------------------------------------------------------------- the writer's grid, the compare clip
GRID_PADDING = 2                # torchvision.utils.make_grid's default, which save_videos_grid leaves as it is (pad_value 0)


def grid_layout(batch: int, height: int, width: int, n_rows: int = 6):
    """torchvision's ``make_grid(nrow=n_rows, padding=2)`` of ``batch`` images of ``height`` x ``width``:
    ``(canvas_height, canvas_width, [(y, x) of sample k])``.  One image is returned as it is, without a border."""
    batch, height, width, n_rows = int(batch), int(height), int(width), int(n_rows)
    if batch < 1 or height < 1 or width < 1 or n_rows < 1:
        raise ValueError(f"grid_layout: batch={batch} height={height} width={width} n_rows={n_rows}")
    if batch == 1:
        return height, width, [(0, 0)]
    xmaps = min(n_rows, batch)
    ymaps = -(-batch // xmaps)
    ch, cw = height + GRID_PADDING, width + GRID_PADDING
    return (ymaps * ch + GRID_PADDING, xmaps * cw + GRID_PADDING,
            [(GRID_PADDING + (k // xmaps) * ch, GRID_PADDING + (k % xmaps) * cw) for k in range(batch)])


def _videos_kind(videos, what: str):
    """-> (is_uint8, B, T, H, W) of float ``[B, 3, T, H, W]`` or uint8 ``[B, T, H, W, 3]``."""
    if not torch.is_tensor(videos) or videos.dim() != 5:
        raise ValueError(f"{what}: expected float32 / bfloat16 [B, 3, T, H, W] or uint8 [B, T, H, W, 3], got "
                         f"{getattr(videos, 'dtype', type(videos))} {tuple(getattr(videos, 'shape', ()))}")
    if videos.dtype == torch.uint8 and videos.shape[-1] == 3:
        return (True,) + tuple(int(v) for v in videos.shape[:4])
    if videos.dtype in (torch.float32, torch.bfloat16) and videos.shape[1] == 3:
        return (False, int(videos.shape[0])) + tuple(int(v) for v in videos.shape[2:])
    raise ValueError(f"{what}: expected float32 / bfloat16 [B, 3, T, H, W] or uint8 [B, T, H, W, 3], got {videos.dtype} "
                     f"{tuple(videos.shape)}")


def _need_device(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor is on {t.device}; the HIP path has no CPU fallback")


def _to_host(res: torch.Tensor, out: Optional[torch.Tensor], what: str) -> torch.Tensor:
    """``out`` = a page-locked uint8 host tensor of the result's shape, filled by one copy (as ``restore_frames`` fills its own)."""
    if out is None:
        return res
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(res.shape) or out.is_cuda or not out.is_contiguous():
        raise ValueError(f"{what}: out {out.dtype} {tuple(out.shape)} on {out.device} for uint8 host frames {tuple(res.shape)}")
    out.copy_(res, non_blocking=True)
    torch.cuda.current_stream(res.device).synchronize()
    return out


def grid_frames(videos: torch.Tensor, rescale: bool = False, n_rows: int = 6, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The frames ``save_videos_grid(videos, rescale=rescale, n_rows=n_rows)`` hands to its encoder (utils.py:59-68), made on the
    device: float32 / bfloat16 ``[B, 3, T, H, W]`` -> uint8 ``[T, Hg, Wg, 3]``, ``trunc(x * 255)`` (of ``(x + 1) / 2`` with
    ``rescale``) of every sample at its place in ``grid_layout``; the border and the unused cells of a last row are the writer's
    byte of ``make_grid``'s 0: 0, or 127 = ``trunc((0 + 1) / 2 * 255)`` with ``rescale``, which the reference applies to the whole grid.  uint8
    ``[B, T, H, W, 3]`` frames (``output_type="uint8"``) are laid out as they are (``rescale`` does not apply to bytes).  One sample
    gives its own frames, no border.  ``out``: a page-locked uint8 host tensor of the result's shape, filled by one copy."""
    u8, B, T, H, W = _videos_kind(videos, "grid_frames")
    _need_device(videos, "grid_frames")
    if u8 and rescale:
        raise ValueError("grid_frames: rescale applies to float videos, not to uint8 frames")
    hg, wg, cells = grid_layout(B, H, W, n_rows)
    canvas = torch.empty(T, hg, wg, 3, device=videos.device, dtype=torch.uint8)
    mode = ops.COMPOSE_COPY if u8 else ops.COMPOSE_WRITER
    ops.frames_u8_compose(canvas, [dict(tensor=videos[k], mode=mode, rescale=rescale, dst=cells[k]) for k in range(B)],
                          pad=127 if rescale else 0)
    return _to_host(canvas, out, "grid_frames")


def compare_frames(source: torch.Tensor, edit: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The frames of the reference's compare clip (``save_side_by_side``, fast_infer.py:183-206, then the writer), made on the
    device: uint8 ``[B, T', H', 2 W', 3]`` with ``T'``, ``H'``, ``W'`` the smaller of the two clips' along each axis (both are cropped
    from the start of the axis), the source on the left, the edit on the right.

    ``source``: the uint8 ``[B, T, H, W, 3]`` frames the clip was loaded from -- shown as the reference shows the float video its
    loader makes of them (``LOADER_ROUNDTRIP``, include/wan_hip.h) -- or that float video ``[B, 3, T, H, W]`` itself.  ``edit``: the
    uint8 frames of ``output_type="uint8"`` (the writer's bytes of a video in [0, 1], which ``_normalize_to_01`` leaves alone: copied)
    or the float video.  A float clip goes through ``_normalize_to_01``; whether it rescales is decided on the device over the whole
    tensor, as there.  ``out``: a page-locked uint8 host tensor of the result's shape, filled by one copy."""
    su8, B, Ts, Hs, Ws = _videos_kind(source, "compare_frames.source")
    eu8, Be, Te, He, We = _videos_kind(edit, "compare_frames.edit")
    _need_device(source, "compare_frames.source")
    _need_device(edit, "compare_frames.edit")
    if B != Be or source.device != edit.device:
        raise ValueError(f"compare_frames: {B} source clips on {source.device}, {Be} edits on {edit.device}")
    T, H, W = min(Ts, Te), min(Hs, He), min(Ws, We)
    sflag = ops.video_range_flag(source)
    eflag = None if eu8 else ops.video_range_flag(edit)
    canvas = torch.empty(B, T, H, 2 * W, 3, device=source.device, dtype=torch.uint8)
    for b in range(B):
        left = dict(tensor=source[b], mode=ops.COMPOSE_LOADER_ROUNDTRIP if su8 else ops.COMPOSE_NORMALIZE, flag=sflag,
                    window=(0, 0, 0, T, H, W), dst=(0, 0))
        right = dict(tensor=edit[b], mode=ops.COMPOSE_COPY if eu8 else ops.COMPOSE_NORMALIZE, flag=eflag,
                     window=(0, 0, 0, T, H, W), dst=(0, W))
        ops.frames_u8_compose(canvas[b], [left, right])
    return _to_host(canvas, out, "compare_frames")


def _reference_normalize_to_01(video: torch.Tensor) -> torch.Tensor:
    """fast_infer.py:183-189."""
    vmin = float(video.min())
    vmax = float(video.max())
    if vmin < 0.0 or vmax > 1.0:
        video = (video + 1.0) / 2.0
    return video.clamp(0.0, 1.0)


def _reference_writer_bytes(x: torch.Tensor) -> torch.Tensor:
    """utils.py:67 ``(x * 255).numpy().astype(np.uint8)`` (truncation), on float32 (a bfloat16 tensor has no numpy form: ``.float()``
    first, as the pipeline's ``decode_latents`` does before its frames reach the writer)."""
    return torch.from_numpy((x.float() * 255).numpy().astype(np.uint8))


def reference_grid_frames(videos: torch.Tensor, rescale: bool = False, n_rows: int = 6) -> torch.Tensor:
    """utils.py:60-67 on the host: ``[B, 3, T, H, W]`` -> uint8 ``[T, Hg, Wg, 3]`` (``make_grid`` restated by ``grid_layout``: a
    zero canvas, sample k copied to its cell).  uint8 ``[B, T, H, W, 3]`` frames are laid out as bytes."""
    u8, B, T, H, W = _videos_kind(videos, "reference_grid_frames")
    x = videos.detach().cpu()
    x = x.permute(1, 0, 4, 2, 3) if u8 else x.permute(2, 0, 1, 3, 4)          # "b c t h w -> t b c h w"
    hg, wg, cells = grid_layout(B, H, W, n_rows)
    grid = torch.zeros(T, 3, hg, wg, dtype=x.dtype)
    for k, (y0, x0) in enumerate(cells):
        grid[:, :, y0:y0 + H, x0:x0 + W] = x[:, k]
    grid = grid.permute(0, 2, 3, 1)                                            # .transpose(0, 1).transpose(1, 2) per frame
    if u8:
        return grid.contiguous()
    if rescale:
        grid = (grid + 1.0) / 2.0
    return _reference_writer_bytes(grid).contiguous()


def reference_compare_frames(source: torch.Tensor, edit: torch.Tensor) -> torch.Tensor:
    """fast_infer.py:192-205 and the writer on the host -> uint8 ``[B, T', H', 2 W', 3]`` (one grid-less clip per sample).  uint8
    source frames first become the loader's float32 video (fast_infer.py:88-90); uint8 edit frames are the writer's bytes of a
    video in [0, 1] already -- ``_normalize_to_01`` and the writer give those bytes back -- and are placed as they are."""
    su8, B, _, _, _ = _videos_kind(source, "reference_compare_frames.source")
    eu8, Be, _, _, _ = _videos_kind(edit, "reference_compare_frames.edit")
    if B != Be:
        raise ValueError(f"reference_compare_frames: {B} source clips, {Be} edits")
    a = source.detach().cpu()
    a = _reference_normalize_to_01(reference_frames_to_video(a) if su8 else a)
    b = edit.detach().cpu()
    b = b.permute(0, 4, 1, 2, 3) if eu8 else _reference_normalize_to_01(b)
    T, H, W = min(a.shape[2], b.shape[2]), min(a.shape[3], b.shape[3]), min(a.shape[4], b.shape[4])
    a = _reference_writer_bytes(a[:, :, :T, :H, :W])                           # the writer is element-wise: bytes before the cat
    b = b[:, :, :T, :H, :W] if eu8 else _reference_writer_bytes(b[:, :, :T, :H, :W])
    return torch.cat([a, b], dim=4).permute(0, 2, 3, 4, 1).contiguous()


# ---------------------------------------------------------------------------------------------- YCbCr planes in and out, .y4m files
YUV_BITS = 16                   # fixed-point bits of a matrix coefficient
YUV_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}           # (Kr, Kb)
# chroma layout -> (subsampled horizontally, subsampled vertically, horizontally left co-sited); None: no chroma planes
CHROMA_LAYOUTS = {"420jpeg": (True, True, False), "420mpeg2": (True, True, True), "422": (True, False, True),
                  "444": (False, False, False), "mono": None}
_Y4M_CHROMA_TAGS = {"420jpeg": "420jpeg", "420mpeg2": "420mpeg2", "420": "420jpeg", "422": "422", "444": "444", "mono": "mono"}
_Y4M_MAGIC = b"YUV4MPEG2"
_Y4M_FRAME = b"FRAME\n"


def _yuv_range(full_range: bool) -> Tuple[int, int, int]:
    """(luma span, chroma span, luma offset)."""
    return (255, 255, 0) if full_range else (219, 224, 16)


@functools.lru_cache(maxsize=None)
def _yuv_tables(matrix: str, full_range: bool):
    if matrix not in YUV_MATRICES:
        raise ValueError(f"yuv_matrix: matrix {matrix!r}; expected one of {sorted(YUV_MATRICES)}")
    kr, kb = YUV_MATRICES[matrix]
    kg = 1.0 - kr - kb
    ys, cs, _ = _yuv_range(bool(full_range))
    one = float(1 << YUV_BITS)
    m = np.array([[kr, kg, kb],
                  [-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), (1 - kb) / (2 * (1 - kb))],
                  [(1 - kr) / (2 * (1 - kr)), -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr))]], dtype=np.float64)
    m *= np.array([[ys / 255.0], [cs / 255.0], [cs / 255.0]])
    fwd = np.rint(m * one).astype(np.int64)
    for row, target in enumerate((int(np.rint(ys / 255.0 * one)), 0, 0)):
        fwd[row, int(np.argmax(np.abs(fwd[row])))] += target - int(fwd[row].sum())
    ky, kc = 255.0 / ys, 255.0 / cs
    inv = np.array([[ky, 0.0, 2 * (1 - kr) * kc],
                    [ky, -2 * (1 - kb) * kb / kg * kc, -2 * (1 - kr) * kr / kg * kc],
                    [ky, 2 * (1 - kb) * kc, 0.0]], dtype=np.float64)
    inv = np.rint(inv * one).astype(np.int64)
    fwd.setflags(write=False)
    inv.setflags(write=False)
    return fwd, inv


def yuv_matrix(matrix: str = "bt601", full_range: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The two integer tables of the YCbCr definition (include/wan_hip.h) as int64 ``[3, 3]``:
    ``forward`` (rows Y, Cb, Cr over R, G, B) and ``inverse`` (rows R, G, B over Y - yo, Cb - 128, Cr - 128), in 16-bit fixed point,
    rounded from float64.  Each forward row is adjusted in its largest entry to sum to exactly ``rint(ys / 255 * 2**16)``, 0, 0, so a
    grey pixel has Cb = Cr = 128 exactly.  ``matrix``: ``"bt601"`` | ``"bt709"``; limited range is Y in [16, 235], chroma in [16, 240]."""
    return _yuv_tables(str(matrix), bool(full_range))


def _chroma_layout(chroma: str, what: str):
    if chroma not in _Y4M_CHROMA_TAGS:
        raise ValueError(f"{what}: chroma layout {chroma!r}; expected one of {sorted(_Y4M_CHROMA_TAGS)}")
    name = _Y4M_CHROMA_TAGS[chroma]
    return name, CHROMA_LAYOUTS[name]


def chroma_shape(height: int, width: int, chroma: str) -> Tuple[int, int]:
    """Rows and columns of a chroma plane of a ``height`` x ``width`` frame: halves are rounded up; ``(0, 0)`` for mono."""
    _, lay = _chroma_layout(chroma, "chroma_shape")
    if lay is None:
        return 0, 0
    return ((height + 1) // 2 if lay[1] else height), ((width + 1) // 2 if lay[0] else width)


def _up_taps(n_out: int, n_in: int, sub: bool, cosited: bool):
    """Per output index the two source indices (clamped to the plane) and their weights in quarters."""
    i = np.arange(n_out, dtype=np.int64)
    if not sub:
        return i, np.full(n_out, 4, np.int64), i, np.zeros(n_out, np.int64)
    h, odd = i // 2, (i & 1).astype(bool)
    if cosited:
        i0, w0, i1, w1 = h, np.where(odd, 2, 4), np.where(odd, h + 1, h), np.where(odd, 2, 0)
    else:
        i0, w0, i1, w1 = np.where(odd, h, h - 1), np.where(odd, 3, 1), np.where(odd, h + 1, h), np.where(odd, 1, 3)
    return np.clip(i0, 0, n_in - 1), w0.astype(np.int64), np.clip(i1, 0, n_in - 1), w1.astype(np.int64)


def _as_plane(x, what: str) -> np.ndarray:
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError(f"{what}: expected uint8 [T, rows, columns], got {a.dtype} {a.shape}")
    return a


def reference_yuv_to_frames(y, cb=None, cr=None, *, chroma: str = "420jpeg", matrix: str = "bt601",
                            full_range: bool = False) -> torch.Tensor:
    """The definition of the way in, in numpy int64 on the host: planes ``[T, H, W]`` / ``[T, Ch, Cw]`` -> uint8 ``[T, H, W, 3]``.
    What ``yuv_to_frames`` equals byte for byte; never called by the product path."""
    name, lay = _chroma_layout(chroma, "reference_yuv_to_frames")
    yy = _as_plane(y, "reference_yuv_to_frames.y").astype(np.int64)
    T, H, W = yy.shape
    _, inv = yuv_matrix(matrix, full_range)
    yo = _yuv_range(full_range)[2]
    if lay is None:
        u = v = np.full_like(yy, 128)
    else:
        ch, cw = chroma_shape(H, W, name)
        iy0, wy0, iy1, wy1 = _up_taps(H, ch, lay[1], False)                   # the vertical axis is always centred
        ix0, wx0, ix1, wx1 = _up_taps(W, cw, lay[0], lay[2])
        planes = []
        for nm, c in (("cb", cb), ("cr", cr)):
            c = _as_plane(c, f"reference_yuv_to_frames.{nm}").astype(np.int64)
            if c.shape != (T, ch, cw):
                raise ValueError(f"reference_yuv_to_frames.{nm}: expected [{T}, {ch}, {cw}] for {name}, got {c.shape}")
            r0, r1 = c[:, iy0] * wy0[None, :, None], c[:, iy1] * wy1[None, :, None]
            s = (r0[:, :, ix0] + r1[:, :, ix0]) * wx0 + (r0[:, :, ix1] + r1[:, :, ix1]) * wx1
            planes.append((s + 8) >> 4)
        u, v = planes
    src = np.stack([yy - yo, u - 128, v - 128], axis=-1)                       # [T, H, W, 3]
    rgb = (src @ inv.T + (1 << (YUV_BITS - 1))) >> YUV_BITS
    return torch.from_numpy(np.clip(rgb, 0, 255).astype(np.uint8))


def reference_frames_to_yuv(frames_u8, *, chroma: str = "420jpeg", matrix: str = "bt601", full_range: bool = False):
    """The definition of the way out, in numpy int64 on the host: uint8 ``[T, H, W, 3]`` -> ``(y, cb, cr)`` uint8 tensors
    ``[T, H, W]`` / ``[T, Ch, Cw]``, ``chroma`` = ``"420jpeg"`` (centre siting) or ``"444"``.  Never called by the product path."""
    name, lay = _chroma_layout(chroma, "reference_frames_to_yuv")
    if name not in ("420jpeg", "444"):
        raise ValueError(f"reference_frames_to_yuv: writes 420jpeg or 444, not {chroma!r}")
    x = torch.as_tensor(frames_u8)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f"reference_frames_to_yuv: expected uint8 [T, H, W, 3], got {x.dtype} {tuple(x.shape)}")
    rgb = x.cpu().numpy().astype(np.int64)
    fwd, _ = yuv_matrix(matrix, full_range)
    off = np.array([_yuv_range(full_range)[2], 128, 128], dtype=np.int64)
    ycc = np.clip((rgb @ fwd.T + (off << YUV_BITS) + (1 << (YUV_BITS - 1))) >> YUV_BITS, 0, 255)
    out = [ycc[..., 0]]
    for c in (ycc[..., 1], ycc[..., 2]):
        if lay[0]:
            c = np.pad(c, ((0, 0), (0, c.shape[1] & 1), (0, c.shape[2] & 1)), mode="edge")
            c = (c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + 2) >> 2
        out.append(c)
    return tuple(torch.from_numpy(np.ascontiguousarray(p.astype(np.uint8))) for p in out)


def _default_matrix(height: int) -> str:
    """The format carries no matrix tag: HD material is BT.709, everything smaller BT.601 (what players assume)."""
    return "bt709" if int(height) >= 720 else "bt601"


def yuv_to_frames(y: torch.Tensor, cb: Optional[torch.Tensor] = None, cr: Optional[torch.Tensor] = None, *, chroma: str = "420jpeg",
                  matrix: str = "bt601", full_range: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """8-bit YCbCr planes on the device -> uint8 ``[T, H, W, 3]`` RGB frames on the device, one launch of ``wan_yuv_to_frames_u8``.
    ``y``: uint8 ``[T, H, W]``; ``cb`` / ``cr``: uint8 ``[T, Ch, Cw]`` (``chroma_shape``), strided views of any alignment -- the planes
    inside an uploaded ``.y4m`` file, padded decoder surfaces, or the two halves of an NV12 ``CbCr`` plane (``uv[..., 0]``,
    ``uv[..., 1]``).  ``chroma``: a key of ``CHROMA_LAYOUTS`` (``"420"`` = ``"420jpeg"``); ``"mono"`` takes no chroma planes.  CPU
    tensors raise, like every op.  ``out``: a contiguous uint8 ``[T, H, W, 3]`` device tensor to fill."""
    name, lay = _chroma_layout(chroma, "yuv_to_frames")
    if (lay is None) != (cb is None and cr is None):
        raise ValueError(f"yuv_to_frames: chroma={chroma!r} with{'out' if cb is None else ''} chroma planes")
    _, inv = yuv_matrix(matrix, full_range)
    sub_x, sub_y, cosited = lay if lay is not None else (False, False, False)
    return ops.yuv_to_frames_u8(y, cb, cr, sub_x, sub_y, cosited, inv.ravel().tolist(), _yuv_range(full_range)[2], out)


def _plane_views(buf: torch.Tensor, height: int, width: int, chroma: str, prefix: int = 0):
    """The ``[T, H, W]`` / ``[T, Ch, Cw]`` views of a uint8 ``[T, prefix + frame_bytes]`` buffer in the ``.y4m`` frame layout (Y, Cb, Cr
    one after the other, rows packed); ``(y, None, None)`` for mono."""
    T, pitch = int(buf.shape[0]), int(buf.stride(0)) if buf.shape[0] > 1 else int(buf.shape[1])
    ch, cw = chroma_shape(height, width, chroma)
    base = buf.storage_offset() + prefix

    def view(off, rows, cols):
        return torch.as_strided(buf, (T, rows, cols), (pitch, cols, 1), base + off)
    y = view(0, height, width)
    if ch == 0:
        return y, None, None
    return y, view(height * width, ch, cw), view(height * width + ch * cw, ch, cw)


def y4m_frame_bytes(height: int, width: int, chroma: str) -> int:
    ch, cw = chroma_shape(height, width, chroma)
    return int(height) * int(width) + 2 * ch * cw


def frames_to_yuv(frames_u8: torch.Tensor, *, chroma: str = "420", matrix: str = "bt601", full_range: bool = False,
                  frame_prefix: bytes = b""):
    """uint8 ``[T, H, W, 3]`` RGB frames on the device -> 8-bit YCbCr on the device, one launch of ``wan_frames_u8_to_yuv``.  Returns
    ``(buffer, (y, cb, cr))``: one uint8 ``[T, frame_bytes]`` buffer in the ``.y4m`` frame layout and the three plane views into it.
    ``chroma``: ``"420"`` / ``"420jpeg"`` (centre siting) or ``"444"``.  ``frame_prefix``: bytes put in front of every frame (the file's
    ``FRAME`` line; the buffer is then ``[T, len(frame_prefix) + frame_bytes]``).  CPU tensors raise, like every op."""
    name, lay = _chroma_layout(chroma, "frames_to_yuv")
    if name not in ("420jpeg", "444"):
        raise ValueError(f"frames_to_yuv: writes 420jpeg or 444, not {chroma!r}")
    if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise ValueError(f"frames_to_yuv: expected uint8 [T, H, W, 3] frames, got {getattr(frames_u8, 'dtype', type(frames_u8))} "
                         f"{tuple(getattr(frames_u8, 'shape', ()))}")
    T, H, W, _ = (int(v) for v in frames_u8.shape)
    fwd, _ = yuv_matrix(matrix, full_range)
    npre = len(frame_prefix)
    buf = torch.empty(T, npre + y4m_frame_bytes(H, W, name), device=frames_u8.device, dtype=torch.uint8)
    if npre:
        buf[:, :npre] = torch.frombuffer(bytearray(frame_prefix), dtype=torch.uint8).to(buf.device)
    y, cb, cr = _plane_views(buf, H, W, name, npre)
    ops.frames_u8_to_yuv(frames_u8, y, cb, cr, lay[0], fwd.ravel().tolist(), _yuv_range(full_range)[2])
    return buf, (y, cb, cr)


@dataclass(frozen=True)
class YuvClip:
    """A ``.y4m`` file as ``read_y4m`` maps it: nothing is copied, ``data`` is a read-only ``numpy.memmap`` of the whole file and
    ``offsets[i]`` the byte at which frame ``i``'s planes start (``frame_bytes`` each: Y, Cb, Cr)."""
    path: str
    width: int
    height: int
    fps: Optional[Fraction]
    chroma: str                     # a key of CHROMA_LAYOUTS
    full_range: Optional[bool]      # XCOLORRANGE of the header; None when the file has no such tag
    frames: int
    frame_bytes: int
    offsets: np.ndarray
    data: np.ndarray
    aspect: Optional[str] = None

    def planes(self, index: int):
        """``(y, cb, cr)`` of frame ``index`` as numpy views of the map (``cb`` = ``cr`` = None for mono)."""
        if not 0 <= index < self.frames:
            raise IndexError(f"frame {index} of {self.frames}")
        o, n = int(self.offsets[index]), self.height * self.width
        ch, cw = chroma_shape(self.height, self.width, self.chroma)
        y = self.data[o:o + n].reshape(self.height, self.width)
        if ch == 0:
            return y, None, None
        return y, self.data[o + n:o + n + ch * cw].reshape(ch, cw), self.data[o + n + ch * cw:o + n + 2 * ch * cw].reshape(ch, cw)


def read_y4m(path) -> YuvClip:
    """Map a YUV4MPEG2 file: the header's ``W H F I A C X`` tags and the place of every frame.  8-bit progressive ``C420jpeg``,
    ``C420mpeg2``, ``C420`` (the format's default, read as 420jpeg), ``C422``, ``C444`` and ``Cmono`` are accepted, ``XCOLORRANGE=FULL``
    is honoured; interlaced clips, more than 8 bits, ``C411`` and ``C420paldv`` raise ``ValueError`` with the tag in the message.
    ``FRAME`` lines may carry parameters, so frames are found by parsing (at once when every marker is the bare ``FRAME``)."""
    path = os.fspath(path)
    size = os.path.getsize(path)
    if size < len(_Y4M_MAGIC) + 1:
        raise ValueError(f"read_y4m: {path}: not a YUV4MPEG2 file ({size} bytes)")
    data = np.memmap(path, dtype=np.uint8, mode="r")
    head = bytes(data[:min(size, 65536)])
    if not head.startswith(_Y4M_MAGIC) or head[len(_Y4M_MAGIC):len(_Y4M_MAGIC) + 1] not in (b" ", b"\n"):
        raise ValueError(f"read_y4m: {path}: bad magic {head[:10]!r}; expected {_Y4M_MAGIC!r}")
    end = head.find(b"\n")
    if end < 0:
        raise ValueError(f"read_y4m: {path}: no end of the header line in the first {len(head)} bytes")
    width = height = None
    fps = aspect = full_range = None
    chroma = "420jpeg"
    for tag in head[len(_Y4M_MAGIC):end].decode("ascii", errors="replace").split():
        key, val = tag[0], tag[1:]
        if key in "WH":
            if not val.isdigit() or int(val) < 1:
                raise ValueError(f"read_y4m: {path}: bad size tag {tag!r}")
            width, height = (int(val), height) if key == "W" else (width, int(val))
        elif key == "F":
            num, _, den = val.partition(":")
            if not (num.isdigit() and den.isdigit()):
                raise ValueError(f"read_y4m: {path}: bad frame rate tag {tag!r}")
            fps = Fraction(int(num), int(den)) if int(den) else None
        elif key == "I":
            if val not in ("p", "?"):
                raise ValueError(f"read_y4m: {path}: interlaced clip ({tag!r}); only progressive frames are read")
        elif key == "A":
            aspect = val
        elif key == "C":
            if val not in _Y4M_CHROMA_TAGS:
                why = "more than 8 bits per sample" if "p1" in val or val.startswith("mono1") else "not supported"
                raise ValueError(f"read_y4m: {path}: chroma tag {tag!r}: {why}; accepted: "
                                 + ", ".join("C" + k for k in _Y4M_CHROMA_TAGS))
            chroma = _Y4M_CHROMA_TAGS[val]
        elif key == "X":
            if val.upper().startswith("COLORRANGE="):
                full_range = val.upper().split("=", 1)[1] == "FULL"
    if width is None or height is None:
        raise ValueError(f"read_y4m: {path}: the header has no W / H tag")
    fb = y4m_frame_bytes(height, width, chroma)
    start, body = end + 1, size - (end + 1)
    step = len(_Y4M_FRAME) + fb
    offsets = None
    if body % step == 0:                                                       # fast path: every marker the bare FRAME line
        n = body // step
        marks = np.lib.stride_tricks.as_strided(data[start:], (n, len(_Y4M_FRAME)), (step, 1)) if n else np.zeros((0, 6), np.uint8)
        if bool((marks == np.frombuffer(_Y4M_FRAME, np.uint8)).all()):
            offsets = start + np.arange(n, dtype=np.int64) * step + len(_Y4M_FRAME)
    if offsets is None:
        found, pos = [], start
        while pos < size:
            line = bytes(data[pos:min(size, pos + 4096)])
            nl = line.find(b"\n")
            if not line.startswith(b"FRAME") or nl < 0 or line[5:6] not in (b" ", b"\n"):
                raise ValueError(f"read_y4m: {path}: no FRAME line at byte {pos} (frame {len(found)})")
            pos += nl + 1
            if pos + fb > size:
                raise ValueError(f"read_y4m: {path}: frame {len(found)} is truncated: {size - pos} of {fb} bytes")
            found.append(pos)
            pos += fb
        offsets = np.asarray(found, dtype=np.int64)
    return YuvClip(path, width, height, fps, chroma, full_range, int(len(offsets)), fb, offsets, data, aspect)


def _default_device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def load_y4m_frames(path, source_frames: int, generator: Optional[torch.Generator] = None, matrix: Optional[str] = None,
                    full_range: Optional[bool] = None) -> Tuple[torch.Tensor, int, int]:
    """``load_video_frames`` for a ``.y4m`` file, with nothing but this package: the same frame selection
    (``select_frame_indices``: the same seed picks the same frames), then ONLY the selected frames go through one page-locked staging
    buffer and one copy to the device -- 1.5 bytes per pixel for 4:2:0 -- where ``yuv_to_frames`` makes the RGB frames.  Returns
    ``(uint8 [source_frames, H, W, 3] on the device, H, W)``; hand the frames to ``fit_frames`` / ``WanPipeline.__call__``.
    ``matrix=None``: ``"bt709"`` when ``H >= 720``, else ``"bt601"`` (the format has no matrix tag).  ``full_range=None``: the header's
    ``XCOLORRANGE``, else limited.  An empty clip gives black 480 x 832 frames, as ``load_video_frames`` does."""
    if source_frames is None or int(source_frames) < 1:
        raise ValueError("load_y4m_frames: pass source_frames >= 1")
    source_frames = int(source_frames)
    clip = read_y4m(path)
    idx = select_frame_indices(clip.frames, source_frames, generator)
    dev = _default_device()
    if not idx:
        return torch.zeros(source_frames, 480, 832, 3, dtype=torch.uint8, device=dev), 480, 832
    distinct = [i for k, i in enumerate(idx) if k == 0 or i != idx[k - 1]]      # the padding repeats the last frame: staged once
    stage = torch.empty(len(distinct), clip.frame_bytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    host = stage.numpy()
    for k, i in enumerate(distinct):
        o = int(clip.offsets[i])
        host[k] = clip.data[o:o + clip.frame_bytes]
    buf = stage.to(dev, non_blocking=True)
    y, cb, cr = _plane_views(buf, clip.height, clip.width, clip.chroma)
    full = bool(clip.full_range) if full_range is None else bool(full_range)
    frames = yuv_to_frames(y, cb, cr, chroma=clip.chroma, matrix=matrix or _default_matrix(clip.height), full_range=full)
    if len(distinct) < len(idx):
        frames = torch.cat([frames, frames[-1:].expand(len(idx) - len(distinct), -1, -1, -1)]).contiguous()
    return frames, clip.height, clip.width


def write_y4m(path, frames_u8, fps=16, *, chroma: str = "420", matrix: Optional[str] = None, full_range: bool = False) -> None:
    """Write uint8 ``[T, H, W, 3]`` RGB frames (device or host) as a YUV4MPEG2 file any ``ffmpeg`` reads: converted on the device
    (``frames_to_yuv``), one copy into page-locked memory, then the header and the frames in one write each.  ``fps``: an int, a
    ``Fraction`` or ``(num, den)``.  ``chroma``: ``"420"`` (tagged ``C420jpeg``) or ``"444"``.  ``matrix=None``: ``"bt709"`` when
    ``H >= 720``, else ``"bt601"``.  Full range is tagged ``XCOLORRANGE=FULL``."""
    x = torch.from_numpy(frames_u8) if isinstance(frames_u8, np.ndarray) else frames_u8
    if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3 or x.shape[0] < 1:
        raise ValueError(f"write_y4m: expected uint8 [T, H, W, 3] frames, got {getattr(x, 'dtype', type(x))} "
                         f"{tuple(getattr(x, 'shape', ()))}")
    name, _ = _chroma_layout(chroma, "write_y4m")
    rate = Fraction(*fps) if isinstance(fps, (tuple, list)) else Fraction(fps)
    if rate <= 0:
        raise ValueError(f"write_y4m: fps={fps}")
    if not x.is_cuda:
        x = x.to(_default_device())                                            # bytes over the host link, as they are
    T, H, W, _ = (int(v) for v in x.shape)
    buf, _ = frames_to_yuv(x, chroma=name, matrix=matrix or _default_matrix(H), full_range=full_range, frame_prefix=_Y4M_FRAME)
    host = torch.empty(buf.shape, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    host.copy_(buf, non_blocking=True)
    if buf.is_cuda:
        torch.cuda.current_stream(buf.device).synchronize()
    header = f"YUV4MPEG2 W{W} H{H} F{rate.numerator}:{rate.denominator} Ip A1:1 C{name}"
    if full_range:
        header += " XCOLORRANGE=FULL"
    with open(os.fspath(path), "wb") as f:
        f.write(header.encode("ascii") + b"\n")
        f.write(memoryview(host.numpy()).cast("B"))
