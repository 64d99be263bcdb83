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
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import ops

__all__ = ["frames_to_video", "video_to_frames", "load_video_frames", "reference_frames_to_video", "reference_video_to_frames",
           "fit_size", "fit_plan", "FitPlan", "fit_frames", "restore_frames", "reference_fit_frames",
           "grid_layout", "grid_frames", "compare_frames", "reference_grid_frames", "reference_compare_frames"]

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
    total = int(frames.shape[0])
    stride = max(1, total // source_frames)
    start = int(torch.randint(0, max(1, total - stride * source_frames), (1,), generator=generator)[0].item())
    idx = [start + i * stride for i in range(source_frames) if start + i * stride < total]
    if not idx:
        return torch.zeros(source_frames, 480, 832, 3, dtype=torch.uint8), 480, 832
    idx += [idx[-1]] * (source_frames - len(idx))
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
