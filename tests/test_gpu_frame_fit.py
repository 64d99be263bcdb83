"""-m gpu: the clip fit on the device (wan_frames_u8_resample behind video_io.fit_frames / restore_frames) against
``reference_fit_frames``, the integer definition that tests/test_frame_fit_host.py pins to Pillow.  EQUALITY everywhere: both sides
are the same 32-bit integer arithmetic on the same host-built coefficient tables; there is no rounding to differ in.

The kernel's tile is 16 output rows x 64 output columns and it stages source rows in chunks of 16 KiB, so the shapes cover: outputs
smaller than a tile, several tiles with a remainder in both axes, more source rows than one chunk holds, byte rows that are no
multiple of 16 or even of 4 (every row then starts at another alignment), and a source view that starts at an odd address."""
import numpy as np
import pytest
import torch

from videocof_amd import (AutoencoderKLWan, FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel, fit_frames,
                          reference_fit_frames, restore_frames)
from videocof_amd.video_io import _resize_plan, fit_plan, fit_size
from videocof_amd.weights import deterministic_dit_state_dict, deterministic_vae_state_dict, det_uniform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(dim=256, ffn_dim=512, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)


def clip(t, h, w, seed=0, batch=None):
    shape = (t, h, w, 3) if batch is None else (batch, t, h, w, 3)
    fr = torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    fr.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)            # the first frame holds every byte value
    return fr


def check(fr, height, width):
    want = reference_fit_frames(fr, height, width)
    got, plan = fit_frames(fr.to(DEV), height, width)
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == tuple(want.shape)
    bad = int((got.cpu() != want).sum())
    print(f"fit {tuple(fr.shape)} -> {height} x {width}: {bad} mismatches of {want.numel()}")
    assert bad == 0
    assert plan == fit_plan(fr.shape[-3], fr.shape[-2], height, width)
    return got


@pytest.mark.parametrize("src,dst", [((37, 53), (32, 48)),         # odd source, a y crop of 1, 159-byte rows
                                     ((135, 240), (48, 80)),       # 2.8x downscale, x crop, two tiles, 51 source rows per tile in chunks of 21
                                     ((130, 70), (16, 16)),        # 4.4x downscale, many taps, y crop of 7
                                     ((24, 40), (48, 80)),         # 2x upscale
                                     ((50, 33), (32, 48)),         # upscale in one axis, a crop of 20 in the other
                                     ((17, 19), (16, 16)),         # windows clipped at both borders
                                     ((270, 480), (120, 208)),     # 8 x 4 tiles with a remainder in both axes
                                     ((211, 301), (40, 150))])     # 2x with a y crop of 32: 903-byte rows, remainders in both axes
def test_fit_equals_the_reference(src, dst):
    assert len(torch.unique(clip(2, *src)[0])) == 256
    check(clip(2, *src, seed=src[0]), *dst)


def test_eight_times_downscale_and_the_default_size():
    """128 -> 16 is 16 taps per axis, 130 -> 16 reaches the border arithmetic; with no size given the target is fit_size's."""
    fr = clip(1, 128, 130, seed=8)
    got = restore_frames(fr.to(DEV), 16, 16)                                # a plain resize, no crop: 8x and 8.125x
    assert torch.equal(got.cpu(), reference_fit_frames(fr, 16, 16, plan=_resize_plan(128, 130, 16, 16)))
    fr = clip(1, 100, 180, seed=9)
    got, plan = fit_frames(fr.to(DEV), max_area=48 * 80)
    assert (plan.out_height, plan.out_width) == fit_size(100, 180, 48 * 80) and tuple(got.shape) == (1, *fit_size(100, 180, 48 * 80), 3)
    assert torch.equal(got.cpu(), reference_fit_frames(fr, plan.out_height, plan.out_width))


def test_batch_and_time_indexing_and_host_input():
    fr = clip(3, 37, 53, seed=5, batch=2)
    got = check(fr, 32, 48)
    for b in range(2):
        for t in range(3):
            assert torch.equal(got[b, t].cpu(), reference_fit_frames(fr[b, t], 32, 48))
    host, _ = fit_frames(fr, 32, 48)                                        # a host tensor goes to the device as bytes
    assert host.is_cuda and torch.equal(host, got)
    host_np, _ = fit_frames(fr[0].numpy(), 32, 48)
    assert torch.equal(host_np, got[0])


def test_unaligned_and_non_contiguous_source_views():
    """A clip that starts one byte into its buffer (no row, and not the tensor, is 16-byte aligned: the pieces at the tensor's ends
    are read byte by byte, the rest with 16-byte loads from the boundary below) and a strided view (made contiguous first)."""
    fr = clip(2, 37, 53, seed=6)
    flat = torch.zeros(fr.numel() + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = fr.to(DEV).view(-1)
    view = flat[1:].view(fr.shape)
    assert view.data_ptr() % 2 == 1
    got, _ = fit_frames(view, 32, 48)
    want = reference_fit_frames(fr, 32, 48)
    assert torch.equal(got.cpu(), want)
    wide = clip(2, 37, 106, seed=7)
    strided = wide.to(DEV)[:, :, ::2]
    assert not strided.is_contiguous()
    got, _ = fit_frames(strided, 32, 48)
    assert torch.equal(got.cpu(), reference_fit_frames(wide[:, :, ::2].contiguous(), 32, 48))


def test_a_clip_at_the_target_size_is_returned_as_it_is():
    fr = clip(2, 32, 48).to(DEV)
    got, plan = fit_frames(fr, 32, 48)
    assert got is fr and plan.source_window == (0, 0, 32, 48)
    got, plan = fit_frames(fr)                                               # on the grid and within the area: its own size
    assert got is fr and (plan.out_height, plan.out_width) == (32, 48)
    with pytest.raises(ValueError, match="both"):
        fit_frames(fr, height=32)


def test_restore_round_trip_and_the_pinned_out_path():
    fr = clip(3, 32, 48, seed=11)
    plan = fit_plan(37, 53, 32, 48)
    _, _, wh, ww = plan.source_window
    assert (wh, ww) == (35, 53)
    want = reference_fit_frames(fr, 37, 53, plan=_resize_plan(32, 48, 37, 53))
    got = restore_frames(fr.to(DEV), 37, 53)
    assert got.is_cuda and tuple(got.shape) == (3, 37, 53, 3) and torch.equal(got.cpu(), want)
    out = torch.empty(3, 37, 53, 3, dtype=torch.uint8, pin_memory=True)
    back = restore_frames(fr.to(DEV), 37, 53, out=out)
    assert back is out and torch.equal(out, want)
    assert torch.equal(restore_frames(fr[None].to(DEV), wh, ww).cpu()[0],
                       reference_fit_frames(fr, wh, ww, plan=_resize_plan(32, 48, wh, ww)))
    with pytest.raises(ValueError, match="out"):
        restore_frames(fr.to(DEV), 37, 53, out=torch.empty(3, 37, 54, 3, dtype=torch.uint8))


# ------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def pipe():
    vae = AutoencoderKLWan()
    vae.load_state_dict(deterministic_vae_state_dict(), device=DEV)
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    m.load_state_dict(deterministic_dit_state_dict(**TINY), device=DEV)
    return WanPipeline(vae=vae, transformer=m, scheduler=FlowUniPCMultistepScheduler(shift=1))


def run(pipe, video):
    ctx = [det_uniform("vio.ctx", (11, 64), 1.0).to(DEV)]
    gen = torch.Generator(device=DEV).manual_seed(7)
    return pipe(video=video, prompt_embeds=ctx, height=32, width=48, source_frames=9, reasoning_frames=4, num_inference_steps=2,
                guidance_scale=1.0, shift=3, repeat_rope=True, cot=True, generator=gen, weight_dtype=torch.bfloat16,
                output_type="latent", return_dict=True)


def test_pipeline_takes_the_fitted_clip(pipe):
    fr = clip(9, 37, 53, seed=13)
    fitted, plan = fit_frames(fr, 32, 48)
    assert (plan.out_height, plan.out_width) == (32, 48) and fitted.is_cuda
    got = run(pipe, fitted).latents
    want = run(pipe, reference_fit_frames(fr, 32, 48)).latents
    assert got.dtype == want.dtype and torch.equal(got, want)
    assert float(want[:, :, :3].abs().max()) > 0
    with pytest.raises(ValueError, match="divisible by 8"):                 # the clip as it is: refused by the VAE, as before
        run(pipe, fr)
