"""-m gpu: the uint8 video I/O kernels (wan_frames_u8_to_video, wan_video_to_frames_u8) and their pipeline surface against
the torch restatements of the reference's host code (videocof_amd/video_io.py ``reference_*``, pinned to the reference by
tests/test_video_io_host.py).  EQUALITY everywhere: kernel 1 is two float32 operations and one cast, kernel 2 two roundings in
the VAE's dtype, a float32 product and a truncation; the reference is deterministic.  The restatement runs on the CPU for the
small inputs and, for the full-size clips, with the same torch ops on the device (checked against the CPU run on a frame)."""
import numpy as np
import pytest
import torch

from videocof_amd import (AutoencoderKLWan, FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel, frames_to_video,
                          ops, video_to_frames)
from videocof_amd.video_io import reference_frames_to_video, reference_video_to_frames
from videocof_amd.weights import deterministic_dit_state_dict, deterministic_vae_state_dict, det_uniform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 16, 16), (5, 30, 52), (33, 480, 832), (81, 480, 832)]        # (5, 30, 52): odd byte rows, the element-wise kernels
DTYPES = [torch.bfloat16, torch.float32]
TINY = dict(dim=256, ffn_dim=512, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def mismatches(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((bits(a) != bits(b)).sum()) if a.dtype != torch.uint8 else int((a != b).sum())


def all_bf16(limit=1.5):
    v = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    return v[torch.isfinite(v.float()) & (v.float().abs() <= limit)]


# ------------------------------------------------------------------ kernel 1
@pytest.mark.parametrize("dtype", DTYPES)
def test_frames_to_video_all_byte_values_in_every_channel(dtype):
    fr = torch.zeros(3, 1, 16, 16, 3, dtype=torch.uint8)
    for c in range(3):
        fr[c, 0, :, :, c] = torch.arange(256, dtype=torch.uint8).view(16, 16)          # the other two channels stay 0
        fr[c, 0, :, :, (c + 1) % 3] = torch.arange(255, -1, -1, dtype=torch.uint8).view(16, 16)
    want = reference_frames_to_video(fr, dtype)
    got = ops.frames_u8_to_video(fr.to(DEV), dtype)
    n = mismatches(got.cpu(), want)
    print(f"frames->video all bytes {dtype}: {n} mismatches of {want.numel()}")
    assert got.dtype == dtype and tuple(got.shape) == (3, 3, 1, 16, 16) and n == 0
    # [T, H, W, 3] form of the public function
    assert mismatches(frames_to_video(fr[0].to(DEV), dtype).cpu(), want[:1]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_frames_to_video_random_frames(shape, B, dtype):
    T, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(T * 7 + B)
    fr = torch.randint(0, 256, (B, T, H, W, 3), device=DEV, dtype=torch.uint8, generator=g)
    got = ops.frames_u8_to_video(fr, dtype)
    small = T * H * W <= 1 << 16
    want = reference_frames_to_video(fr.cpu(), dtype).to(DEV) if small else reference_frames_to_video(fr, dtype)
    n = mismatches(got, want)
    print(f"frames->video {B}x{shape} {dtype}: {n} mismatches of {want.numel()}")
    assert n == 0
    if not small:                               # the device restatement is the CPU one: last frame of the last sample
        assert mismatches(want[-1:, :, -1:].cpu(), reference_frames_to_video(fr[-1:, -1:].cpu(), dtype)) == 0


# ------------------------------------------------------------------ kernel 2
def test_video_to_frames_every_bf16_value():
    vals = all_bf16()
    assert vals.numel() < 1 << 16
    n = 3 * 16 * 16
    t = -(-vals.numel() // n)
    for shift in (0, 1, 2):                    # every value in every channel position
        v = torch.cat([vals, vals[:t * n - vals.numel()]]).roll(shift * 256 * t).view(1, 3, t, 16, 16)
        want = reference_video_to_frames(v)
        got = ops.video_to_frames_u8(v.to(DEV)).cpu()
        m = mismatches(got, want)
        print(f"video->frames every bf16 value (shift {shift}): {m} mismatches of {want.numel()}")
        assert m == 0
    # the same values as float32 input (the VAE's dtype when the pipeline runs in float32)
    v32 = v.float()
    assert mismatches(ops.video_to_frames_u8(v32.to(DEV)).cpu(), reference_video_to_frames(v32)) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_video_to_frames_truncates_at_the_byte_boundaries(dtype):
    """Values whose (x / 2 + 0.5) lands at, just below and just above each k / 255: the reference's side (truncation)."""
    k = torch.arange(0, 256, dtype=torch.float64) / 255.0
    unit = torch.cat([k, k - 2.0 ** -9, k + 2.0 ** -9, k - 2.0 ** -20, k + 2.0 ** -20, k - 2.0 ** -24, k + 2.0 ** -24])
    x = ((unit * 2 - 1).float()).to(dtype)
    pad = (-x.numel()) % 768
    x = torch.cat([x, x[:pad]]).view(1, 3, -1, 16, 16)
    want = reference_video_to_frames(x)
    got = ops.video_to_frames_u8(x.to(DEV)).cpu()
    m = mismatches(got, want)
    rounded = ((x.float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 4, 1)
    print(f"video->frames boundaries {dtype}: {m} mismatches; {int((rounded != want).sum())} of {want.numel()} differ from rounding")
    assert m == 0 and int((rounded != want).sum()) > 0          # the inputs do tell truncation from rounding


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_video_to_frames_random_frames_ranges_and_offsets(shape, B, dtype):
    T, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(T * 11 + B)
    x = (torch.randn(B, 3, T, H, W, device=DEV, generator=g) * 0.7).clamp(-1.5, 1.5).to(dtype)
    small = T * H * W <= 1 << 16
    want = reference_video_to_frames(x.cpu()).to(DEV) if small else reference_video_to_frames(x)
    got = ops.video_to_frames_u8(x)
    m = mismatches(got, want)
    print(f"video->frames {B}x{shape} {dtype}: {m} mismatches of {want.numel()}")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, T, H, W, 3) and m == 0
    if not small:
        assert mismatches(want[-1:, -1:].cpu(), reference_video_to_frames(x[-1:, :, -1:].cpu())) == 0
    # a frame range into an offset of a longer clip; the frames around it stay as they were
    t0, t1 = (0, 1) if T == 1 else (1, T - 1 if T > 2 else T)
    clip = torch.full((B, (t1 - t0) + 3, H, W, 3), 77, device=DEV, dtype=torch.uint8)
    back = video_to_frames(x, out=clip, frame_range=(t0, t1), dst_frame=2)
    assert back.data_ptr() == clip.data_ptr()
    assert mismatches(clip[:, 2:2 + t1 - t0], want[:, t0:t1]) == 0
    assert int((clip[:, :2] != 77).sum()) == 0 and int((clip[:, 2 + t1 - t0:] != 77).sum()) == 0
    # two segments side by side in one clip, as a CoF call writes grounding | edit
    if T > 1:
        clip2 = torch.zeros(B, T, H, W, 3, device=DEV, dtype=torch.uint8)
        video_to_frames(x, out=clip2, frame_range=(0, 1), dst_frame=0)
        video_to_frames(x, out=clip2, frame_range=(1, T), dst_frame=1)
        assert mismatches(clip2, want) == 0


def test_arguments_are_checked():
    x = torch.zeros(1, 3, 4, 16, 16, device=DEV, dtype=torch.bfloat16)
    clip = torch.zeros(1, 5, 16, 16, 3, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="frame_range"):
        ops.video_to_frames_u8(x, frame_range=(2, 5))
    with pytest.raises(ValueError, match="5-frame clip"):
        ops.video_to_frames_u8(x, out=clip, dst_frame=2)
    with pytest.raises(ValueError, match="expected a contiguous"):
        ops.video_to_frames_u8(x, out=clip[:, :, :8])
    with pytest.raises(ValueError, match=r"\[B, T, H, W, 3\]"):
        ops.frames_u8_to_video(torch.zeros(1, 4, 16, 16, 4, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError, match="expected torch.uint8"):
        ops.frames_u8_to_video(torch.zeros(1, 4, 16, 16, 3, device=DEV))
    assert tuple(ops.video_to_frames_u8(x, frame_range=(2, 2)).shape) == (1, 0, 16, 16, 3)


# ------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def pipe():
    vae = AutoencoderKLWan()
    vae.load_state_dict(deterministic_vae_state_dict(), device=DEV)
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    m.load_state_dict(deterministic_dit_state_dict(**TINY), device=DEV)
    return WanPipeline(vae=vae, transformer=m, scheduler=FlowUniPCMultistepScheduler(shift=1))


def run(pipe, video, output_type, cot, weight_dtype, **kw):
    ctx = [det_uniform("vio.ctx", (11, 64), 1.0).to(DEV)]
    gen = torch.Generator(device=DEV).manual_seed(7)
    return pipe(video=video, prompt_embeds=ctx, height=32, width=48, source_frames=9, reasoning_frames=4, num_inference_steps=2,
                guidance_scale=1.0, shift=3, repeat_rope=True, cot=cot, generator=gen, weight_dtype=weight_dtype,
                output_type=output_type, return_dict=True, **kw)


def to_bytes(x):
    """The reference writer on the pipeline's float32 [B, 3, T, H, W] numpy frames: `b c t h w -> t h w c`, (x * 255).astype(uint8)."""
    return (np.transpose(x, (0, 2, 3, 4, 1)) * 255).astype(np.uint8)


@pytest.mark.parametrize("weight_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("cot", [True, False])
def test_pipeline_uint8_output_is_the_writers_bytes(pipe, cot, weight_dtype):
    video = det_uniform("vio.video", (1, 3, 9, 32, 48), 0.8).to(DEV)
    a = run(pipe, video, "numpy", cot, weight_dtype)
    b = run(pipe, video, "uint8", cot, weight_dtype)
    assert torch.equal(a.latents, b.latents)
    nf = 10 if cot else 9
    assert a.videos.dtype == np.float32 and a.videos.shape == (1, 3, nf, 32, 48)
    assert isinstance(b.videos, np.ndarray) and b.videos.dtype == np.uint8 and b.videos.shape == (1, nf, 32, 48, 3)
    for name in ("videos", "edit_videos") + (("ground_videos",) if cot else ()):
        want, got = to_bytes(getattr(a, name)), getattr(b, name)
        print(f"pipeline uint8 {name} cot={cot} {weight_dtype}: {int((want != got).sum())} mismatches of {want.size}")
        assert got.dtype == np.uint8 and np.array_equal(want, got), name
    assert len(np.unique(b.videos)) > 16                      # a real picture, not a constant
    if cot:
        assert b.ground_videos.shape == (1, 1, 32, 48, 3) and b.edit_videos.shape == (1, 9, 32, 48, 3)
        assert np.shares_memory(b.videos, b.ground_videos) and np.shares_memory(b.videos, b.edit_videos)
        assert np.array_equal(b.videos[:, :1], b.ground_videos) and np.array_equal(b.videos[:, 1:], b.edit_videos)
    else:
        assert b.ground_videos is None and b.videos is b.edit_videos


def test_pipeline_numpy_output_is_unchanged(pipe):
    """output_type="numpy" still is decode_latents' float path on the same latents: (x / 2 + 0.5).clamp(0, 1).float()."""
    video = det_uniform("vio.video", (1, 3, 9, 32, 48), 0.8).to(DEV)
    a = run(pipe, video, "numpy", True, torch.bfloat16)
    lat = a.latents
    frames = pipe.vae.decode(lat[:, :, 4:].to(pipe.vae.dtype)).sample
    want = (frames / 2 + 0.5).clamp(0, 1).float().cpu().numpy()
    assert a.edit_videos.dtype == np.float32 and np.array_equal(a.edit_videos, want)
    assert np.array_equal(pipe.decode_latents(lat[:, :, 4:]), want)
    assert np.array_equal(pipe.decode_latents(lat[:, :, 4:], as_uint8=True), to_bytes(want))
    out = torch.empty(1, 9, 32, 48, 3, dtype=torch.uint8, pin_memory=True)
    got = pipe.decode_latents(lat[:, :, 4:], out=out, as_uint8=True)
    assert np.shares_memory(got, out.numpy()) and np.array_equal(got, to_bytes(want))
    with pytest.raises(TypeError, match="as_bytes"):
        pipe.decode_latents(lat[:, :, 4:], as_bytes=True)
    with pytest.raises(ValueError, match="not supported"):
        run(pipe, video, "pil", True, torch.bfloat16)


@pytest.mark.parametrize("weight_dtype", [torch.bfloat16, torch.float32])
def test_pipeline_uint8_video_gives_the_float_videos_latents(pipe, weight_dtype):
    """A uint8 `video` ([T, H, W, 3] or [B, T, H, W, 3], host or device) = the float video the reference's loader makes of it."""
    g = torch.Generator().manual_seed(5)
    fr = torch.randint(0, 256, (9, 32, 48, 3), generator=g, dtype=torch.uint8)
    loader_video = reference_frames_to_video(fr[None])                    # float32 [1, 3, 9, 32, 48] on the host, fast_infer.py:88-90
    want = run(pipe, loader_video, "latent", True, weight_dtype).latents
    for video in (fr, fr[None], fr.to(DEV), fr[None].to(DEV), fr.numpy()):
        got = run(pipe, video, "latent", True, weight_dtype).latents
        assert got.dtype == want.dtype and torch.equal(got, want)
    assert float(want[:, :, :3].abs().max()) > 0                            # the source latents are in there
