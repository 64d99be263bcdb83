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
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import ops

__all__ = ["frames_to_video", "video_to_frames", "load_video_frames", "reference_frames_to_video", "reference_video_to_frames"]


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
