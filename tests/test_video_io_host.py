"""Host side of the uint8 video I/O (videocof_amd/video_io.py), no GPU.

The GPU tests (tests/test_gpu_video_io.py) compare the two HIP kernels with ``reference_frames_to_video`` /
``reference_video_to_frames``, torch restatements of the reference's host code.  Here those restatements are pinned to the
reference itself: where its tree is present, the statements of fast_infer.py:88-90 and videox_fun/utils/utils.py:60-67 are read
from it and executed as they stand (only ``torchvision.utils.make_grid`` is stood in for when torchvision is absent: one video
per call makes it the identity); everywhere, they are compared with tests/golden/video_io_ref.npz, recorded from those
statements by ``record_video_io_golden.py`` beside this file.  Equality throughout: the arithmetic is deterministic."""
import os
import textwrap
import types

import numpy as np
import pytest
import torch

from oracle.ref_import import REFERENCE_ROOT
from videocof_amd import load_video_frames, ops, video_io
from videocof_amd.video_io import reference_frames_to_video, reference_video_to_frames

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "video_io_ref.npz")


def reference_lines(relpath, first, last):
    """Lines first..last (1-based, inclusive) of a reference source file, dedented."""
    with open(os.path.join(REFERENCE_ROOT, relpath)) as f:
        lines = f.read().splitlines()
    return textwrap.dedent("\n".join(lines[first - 1:last]))


def reference_present():
    return os.path.isfile(os.path.join(REFERENCE_ROOT, "fast_infer.py")) and \
        os.path.isfile(os.path.join(REFERENCE_ROOT, "videox_fun", "utils", "utils.py"))


def run_reference_loader(frames_thwc: np.ndarray) -> torch.Tensor:
    """fast_infer.py:88-90 on `frames` (what ``np.array(frames)`` of its PIL list is: uint8 [T, H, W, 3]) -> float32 [1, 3, T, H, W]."""
    ns = {"torch": torch, "np": np, "frames": frames_thwc}
    exec(reference_lines("fast_infer.py", 88, 90), ns)
    return ns["input_video"]


def run_reference_writer(videos_bcthw: torch.Tensor) -> np.ndarray:
    """utils.py:60-67 on float32 [1, 3, T, H, W] frames in [0, 1] -> uint8 [T, H, W, 3]: line 60, then the loop body 63-67 per frame."""
    from einops import rearrange
    try:
        import torchvision
    except ImportError:                       # one video per call: the grid of a single image is that image
        def make_grid(x, nrow=8):
            assert x.dim() == 4 and x.shape[0] == 1 and x.shape[1] == 3
            return x[0]
        torchvision = types.SimpleNamespace(utils=types.SimpleNamespace(make_grid=make_grid))
    ns = {"torch": torch, "np": np, "rearrange": rearrange, "torchvision": torchvision, "videos": videos_bcthw, "n_rows": 6,
          "rescale": False}
    exec(reference_lines("videox_fun/utils/utils.py", 60, 60), ns)
    body = reference_lines("videox_fun/utils/utils.py", 63, 67)
    outputs = []
    for x in ns["videos"]:
        ns["x"] = x
        exec(body, ns)
        outputs.append(ns["x"])
    return np.stack(outputs)


def boundary_video():
    """bf16 [1, 3, T, 16, 16]: every bf16 value in [-1.5, 1.5] (the decoder clamps to [-1, 1]; the margin covers the clamp)."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    vals = bits[torch.isfinite(bits.float()) & (bits.float().abs() <= 1.5)]
    assert 30000 < vals.numel() < (1 << 16)
    n = 3 * 16 * 16
    t = -(-vals.numel() // n)
    vals = torch.cat([vals, vals[:t * n - vals.numel()]])
    return vals.view(1, 3, t, 16, 16)


def test_restatements_equal_the_reference_statements():
    if not reference_present():
        pytest.skip("reference tree not present: see test_restatements_equal_the_recorded_fixture")
    g = torch.Generator().manual_seed(11)
    frames = torch.randint(0, 256, (5, 30, 52, 3), generator=g, dtype=torch.uint8)
    allb = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    for fr in (frames, allb):
        want = run_reference_loader(fr.numpy())
        got = reference_frames_to_video(fr[None])
        assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape and torch.equal(got, want)
    # the writer on what decode_latents hands it: (x / 2 + 0.5).clamp(0, 1) in the VAE's dtype, as float32 on the host
    for video in (boundary_video(), torch.randn(1, 3, 5, 30, 52, generator=g).mul(0.6).bfloat16(),
                  torch.randn(1, 3, 5, 30, 52, generator=g).mul(0.6)):
        unit = (video / 2 + 0.5).clamp(0, 1).cpu().float()                # pipeline_wan.py:426-427
        want = run_reference_writer(unit)
        got = reference_video_to_frames(video)[0].numpy()
        assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


def test_restatements_equal_the_recorded_fixture(golden):
    """The same pin for a checkout without the reference: inputs and the reference statements' outputs as recorded."""
    g = golden("video_io_ref")
    fr = torch.from_numpy(g["frames_u8"])
    assert torch.equal(reference_frames_to_video(fr[None]), torch.from_numpy(g["loader_out"]))
    assert torch.equal(reference_frames_to_video(fr[None], torch.bfloat16).view(torch.int16),
                       torch.from_numpy(g["loader_out"]).bfloat16().view(torch.int16))
    assert np.array_equal(reference_video_to_frames(boundary_video())[0].numpy(), g["writer_out_boundary"])
    v = torch.from_numpy(g["video_bf16_bits"]).view(torch.bfloat16)
    assert np.array_equal(reference_video_to_frames(v)[0].numpy(), g["writer_out_bf16"])
    v = torch.from_numpy(g["video_f32"])
    assert np.array_equal(reference_video_to_frames(v)[0].numpy(), g["writer_out_f32"])


def test_truncation_not_rounding_at_the_byte_boundaries():
    """float32 frames just below and at k / 255: the byte is floor(x * 255) of the float32 product, never the nearest."""
    k = torch.arange(0, 256, dtype=torch.float32)
    at = k / 255.0
    below = torch.nextafter(at, torch.tensor(-1.0))
    for unit in (at, below):
        video = (unit * 2 - 1).view(1, 1, 1, 16, 16).expand(1, 3, 1, 16, 16).contiguous()
        got = reference_video_to_frames(video)
        want = ((video / 2 + 0.5).clamp(0, 1) * 255).numpy().astype(np.uint8)
        assert np.array_equal(got.numpy()[0, 0, :, :, 0], want[0, 0, 0])
    assert int(reference_video_to_frames(torch.full((1, 3, 1, 1, 1), 0.999))[0, 0, 0, 0, 0]) == 254     # 254.87 -> 254
    assert int(reference_video_to_frames(torch.ones(1, 3, 1, 1, 1))[0, 0, 0, 0, 0]) == 255
    assert int(reference_video_to_frames(torch.full((1, 3, 1, 1, 1), 7.0))[0, 0, 0, 0, 0]) == 255
    assert int(reference_video_to_frames(torch.full((1, 3, 1, 1, 1), -7.0))[0, 0, 0, 0, 0]) == 0


def clip(n, h=4, w=6):
    """n frames, frame i filled with i."""
    return np.broadcast_to(np.arange(n, dtype=np.uint8)[:, None, None, None], (n, h, w, 3)).copy()


@pytest.mark.parametrize("total,source_frames", [(5, 9), (9, 9), (33, 33), (40, 33), (100, 33), (200, 33), (1, 1), (7, 1)])
def test_load_video_frames_picks_the_references_frames(total, source_frames):
    """fast_infer.py:56-85: stride, start frame (the same torch.randint draw), frames while they exist, last frame repeated."""
    stride = max(1, total // source_frames)
    torch.manual_seed(3)
    start = torch.randint(0, max(1, total - stride * source_frames), (1,))[0].item()
    want = [start + i * stride for i in range(source_frames) if start + i * stride < total]
    want += [want[-1]] * (source_frames - len(want))
    torch.manual_seed(3)
    frames, h, w = load_video_frames(clip(total), source_frames)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (source_frames, 4, 6, 3) and (h, w) == (4, 6)
    assert frames[:, 0, 0, 0].tolist() == want
    assert torch.equal(frames, torch.from_numpy(clip(total))[want])
    # a tensor in, and a private generator leaves the global one alone
    g = torch.Generator().manual_seed(3)
    state = torch.get_rng_state()
    frames2, _, _ = load_video_frames(torch.from_numpy(clip(total)), source_frames, generator=g)
    assert torch.equal(frames2, frames) and torch.equal(torch.get_rng_state(), state)


def test_load_video_frames_edges():
    assert load_video_frames(clip(200), 33)[0][:, 0, 0, 0].diff().unique().tolist() == [6]          # stride 200 // 33
    short, _, _ = load_video_frames(clip(5), 9)
    assert short[:, 0, 0, 0].tolist() == [0, 1, 2, 3, 4, 4, 4, 4, 4]
    empty, h, w = load_video_frames(np.zeros((0, 8, 8, 3), np.uint8), 3)
    assert tuple(empty.shape) == (3, 480, 832, 3) and (h, w) == (480, 832) and int(empty.max()) == 0
    with pytest.raises(ValueError, match="uint8"):
        load_video_frames(np.zeros((4, 8, 8, 3), np.float32), 3)
    with pytest.raises(ValueError, match="source_frames"):
        load_video_frames(clip(4), None)
    try:
        import imageio  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="imageio"):
            load_video_frames("clip.mp4", 3)


def test_ops_raise_on_cpu_tensors_and_bad_arguments():
    fr = torch.zeros(1, 2, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frames_u8_to_video(fr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video_io.frames_to_video(fr[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.video_to_frames_u8(torch.zeros(1, 3, 2, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video_io.video_to_frames(torch.zeros(1, 3, 2, 16, 16, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.video_to_frames_u8(torch.zeros(1, 3, 2, 16, 16, dtype=torch.float16))


def test_the_library_validates_before_it_launches():
    """The C entry points reject null tensors, bad dtypes, frame ranges and offsets outside their clips (no kernel is launched)."""
    from videocof_amd import _lib
    lib = _lib.load()
    assert lib.wan_frames_u8_to_video(None, None, 1, 1, 1, 16, 16, None) == _lib.WAN_ERR_INVALID
    assert lib.wan_frames_u8_to_video(16, 16, 2, 1, 1, 16, 16, None) == _lib.WAN_ERR_INVALID            # out_dtype
    assert lib.wan_frames_u8_to_video(16, 16, 1, 1, 0, 16, 16, None) == _lib.WAN_ERR_INVALID            # T = 0
    assert lib.wan_video_to_frames_u8(None, 1, None, 1, 4, 16, 16, 0, 4, 4, 0, None) == _lib.WAN_ERR_INVALID
    assert lib.wan_video_to_frames_u8(16, 1, 16, 1, 4, 16, 16, 2, 3, 8, 0, None) == _lib.WAN_ERR_INVALID     # frames [2, 5) of 4
    assert lib.wan_video_to_frames_u8(16, 1, 16, 1, 4, 16, 16, 0, 4, 5, 2, None) == _lib.WAN_ERR_INVALID     # 4 frames at 2 of 5
    assert lib.wan_video_to_frames_u8(16, 1, 16, 1, 4, 16, 16, -1, 2, 5, 0, None) == _lib.WAN_ERR_INVALID
    with pytest.raises(ValueError, match="5-frame clip"):
        _lib.check(lib.wan_video_to_frames_u8(16, 1, 16, 1, 4, 16, 16, 0, 4, 5, 2, None), "wan_video_to_frames_u8")
    assert lib.wan_video_to_frames_u8(16, 1, 16, 1, 4, 16, 16, 1, 0, 5, 5, None) == _lib.WAN_OK              # nt = 0: nothing to do
    assert {"wan_frames_u8_to_video", "wan_video_to_frames_u8"} <= set(_lib.SIGNATURES) and _lib.ABI_VERSION == 11
