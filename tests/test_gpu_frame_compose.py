"""-m gpu: wan_frames_u8_compose / wan_video_range_flag and their surface (``grid_frames``, ``compare_frames``,
``WanPipeline.__call__(compare=True)``) against the torch restatements of the reference's host code
(videocof_amd/video_io.py ``reference_grid_frames`` / ``reference_compare_frames``, pinned to the reference by
tests/test_frame_compose_host.py).  EQUALITY everywhere, zero differing bytes: the arithmetic is a handful of float32 operations,
each rounded on its own, and a truncation.  Results are written into canvases with poisoned guard bands (0xA5 inside, so a pad
pixel that is never written shows; 0x5A around, so a byte written outside shows)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_video_io_host import boundary_video  # noqa: E402
from videocof_amd import (AutoencoderKLWan, FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel, compare_frames,  # noqa: E402
                          grid_frames, ops, reference_compare_frames, reference_grid_frames)
from videocof_amd.video_io import grid_layout  # noqa: E402
from videocof_amd.weights import deterministic_dit_state_dict, deterministic_vae_state_dict, det_uniform  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64 + 5                    # bytes in front of the canvas: an odd count, so the canvas itself starts unaligned
TINY = dict(dim=256, ffn_dim=512, num_layers=1, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)


class Canvas:
    """A uint8 canvas of `shape` inside a poisoned buffer: [GUARD x 0x5A | canvas, pre-filled 0xA5 | 64 x 0x5A]."""

    def __init__(self, shape, front=GUARD):
        n = int(np.prod(shape))
        self.buf = torch.full((front + n + 64,), 0x5A, device=DEV, dtype=torch.uint8)
        self.view = self.buf[front:front + n].view(shape)
        self.view.fill_(0xA5)
        self.front, self.n = front, n

    def check(self, want, what):
        got = self.view.cpu()
        diff = int((got != want).sum())
        front, back = self.buf[:self.front].cpu(), self.buf[self.front + self.n:].cpu()
        print(f"{what}: {diff} differing bytes of {want.numel()}; guard bytes touched: {int((front != 0x5A).sum())} in front, "
              f"{int((back != 0x5A).sum())} behind")
        assert tuple(got.shape) == tuple(want.shape) and diff == 0, what
        assert bool((front == 0x5A).all()) and bool((back == 0x5A).all()), what


def compose_grid(videos, rescale, n_rows, front=GUARD):
    """grid_frames' launch into a guarded canvas."""
    u8 = videos.dtype == torch.uint8
    B, T, H, W = (videos.shape[0], videos.shape[1], videos.shape[2], videos.shape[3]) if u8 else \
        (videos.shape[0], videos.shape[2], videos.shape[3], videos.shape[4])
    hg, wg, cells = grid_layout(B, H, W, n_rows)
    c = Canvas((T, hg, wg, 3), front)
    ops.frames_u8_compose(c.view, [dict(tensor=videos[k], mode=ops.COMPOSE_COPY if u8 else ops.COMPOSE_WRITER, rescale=rescale,
                                        dst=cells[k]) for k in range(B)], pad=127 if rescale else 0)
    return c


def compose_compare(source, edit, front=GUARD):
    """compare_frames' launches (one sample) into a guarded canvas."""
    su8, eu8 = source.dtype == torch.uint8, edit.dtype == torch.uint8
    ss, es = (source.shape[1:4] if su8 else source.shape[2:5]), (edit.shape[1:4] if eu8 else edit.shape[2:5])
    T, H, W = (min(int(a), int(b)) for a, b in zip(ss, es))
    c = Canvas((T, H, 2 * W, 3), front)
    sflag = ops.video_range_flag(source)
    eflag = None if eu8 else ops.video_range_flag(edit)
    ops.frames_u8_compose(c.view, [
        dict(tensor=source[0], mode=ops.COMPOSE_LOADER_ROUNDTRIP if su8 else ops.COMPOSE_NORMALIZE, flag=sflag,
             window=(0, 0, 0, T, H, W), dst=(0, 0)),
        dict(tensor=edit[0], mode=ops.COMPOSE_COPY if eu8 else ops.COMPOSE_NORMALIZE, flag=eflag, window=(0, 0, 0, T, H, W),
             dst=(0, W))])
    return c


def byte_clip(B, T, H, W, seed):
    """uint8 [B, T, H, W, 3] with every byte value in every sample."""
    g = torch.Generator().manual_seed(seed)
    fr = torch.randint(0, 256, (B, T, H, W, 3), generator=g, dtype=torch.uint8)
    for b in range(B):
        fr[b].view(-1)[b:b + 256] = torch.arange(256, dtype=torch.uint8)
    return fr


def float_values(unit: bool):
    """float32 values at, just below and just above every k / 255, exact 0, 1 (and -1) and their neighbours; `unit`: of a video in
    [0, 1] (the writer as it is), else of one in [-1, 1] (``rescale``)."""
    k = torch.arange(0, 256, dtype=torch.float64) / 255.0
    u = torch.cat([k, k - 2.0 ** -20, k + 2.0 ** -20, k - 2.0 ** -24, k + 2.0 ** -24]).clamp(0, 1)
    v = (u if unit else u * 2 - 1).float()
    edge = torch.tensor([0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -126] if unit else [-1.0, 1.0, 0.0, -1.0 + 2.0 ** -24, 1.0 - 2.0 ** -24])
    return torch.cat([v, edge])


def float_clip(B, T, H, W, unit, seed, dtype=torch.float32):
    """[B, 3, T, H, W]: the boundary values first, uniform values after them; bfloat16 clips start with boundary_video()'s values."""
    g = torch.Generator().manual_seed(seed)
    n = B * 3 * T * H * W
    x = torch.rand(n, generator=g) if unit else torch.rand(n, generator=g) * 2 - 1
    vals = float_values(unit)
    if dtype == torch.bfloat16:
        bv = boundary_video().float().flatten()
        bv = bv[(bv >= (0 if unit else -1)) & (bv <= 1)]
        vals = bv[torch.randperm(bv.numel(), generator=g)]
    m = min(n, vals.numel())
    x[:m] = vals[:m]
    return x.view(B, 3, T, H, W).to(dtype)


# ------------------------------------------------------------------ grid
@pytest.mark.parametrize("W", [27, 28])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
def test_grid_two_rows_and_an_empty_cell(dtype, W):
    """B = 3 with n_rows = 2: two grid rows, one empty cell, the 2-pixel border; 3 * W unaligned (27) and aligned (28)."""
    B, T, H = 3, 3, 18
    for rescale in ((False,) if dtype == torch.uint8 else (False, True)):
        videos = byte_clip(B, T, H, W, 3) if dtype == torch.uint8 else float_clip(B, T, H, W, not rescale, 5 + W, dtype)
        want = reference_grid_frames(videos, rescale, 2)
        assert tuple(want.shape) == (T, 2 * (H + 2) + 2, 2 * (W + 2) + 2, 3) and \
            want[:, H + 4:, W + 4:].unique().tolist() == [127 if rescale else 0]         # the empty cell: make_grid's 0, rescaled or not
        for front in (GUARD, 64):                        # an unaligned and a 16-byte aligned canvas
            compose_grid(videos.to(DEV), rescale, 2, front).check(want, f"grid {dtype} W={W} rescale={rescale} front={front}")
        got = grid_frames(videos.to(DEV), rescale=rescale, n_rows=2)
        assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
        if dtype == torch.uint8:
            assert len(torch.unique(want)) == 256


def test_grid_of_one_sample_and_of_a_full_row():
    one = float_clip(1, 3, 18, 27, True, 11)
    want = reference_grid_frames(one)
    assert tuple(want.shape) == (3, 18, 27, 3)           # the frames themselves, no border
    compose_grid(one.to(DEV), False, 6).check(want, "grid B=1")
    seven = float_clip(7, 2, 6, 7, True, 12)             # n_rows = 6: a full row and one sample in the second
    out = torch.empty(reference_grid_frames(seven).shape, dtype=torch.uint8, pin_memory=True)
    got = grid_frames(seven.to(DEV), out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, reference_grid_frames(seven))


# ------------------------------------------------------------------ compare
@pytest.mark.parametrize("edit_dtype", [torch.uint8, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("src_dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("sizes", [((5, 20, 30), (3, 18, 27)), ((3, 18, 28), (3, 18, 28)), ((3, 18, 27), (4, 19, 31))])
def test_compare_crops_every_axis(sizes, src_dtype, edit_dtype):
    """Source 5/20/30 against edit 3/18/27: the crop is on every axis (and the other way round); one case of equal sizes."""
    (Ts, Hs, Ws), (Te, He, We) = sizes
    source = byte_clip(1, Ts, Hs, Ws, 21) if src_dtype == torch.uint8 else float_clip(1, Ts, Hs, Ws, False, 22, src_dtype)
    edit = byte_clip(1, Te, He, We, 23) if edit_dtype == torch.uint8 else float_clip(1, Te, He, We, True, 24, edit_dtype)
    want = reference_compare_frames(source, edit)
    W = min(Ws, We)
    assert tuple(want.shape) == (1, min(Ts, Te), min(Hs, He), 2 * W, 3)
    if src_dtype == torch.uint8:
        assert not torch.equal(want[0, :, :, :W], source[0, :want.shape[1], :want.shape[2], :W])      # the left half is not the bytes
    for front in (GUARD, 64):
        compose_compare(source.to(DEV), edit.to(DEV), front).check(want[0], f"compare {src_dtype} | {edit_dtype} {sizes} front={front}")
    got = compare_frames(source.to(DEV), edit.to(DEV))
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want)


def test_compare_all_byte_values_and_a_batch():
    allb = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16, 1).expand(2, 1, 16, 16, 3).contiguous()
    allb[1] = allb[1].flip(1)
    edit = byte_clip(2, 1, 16, 16, 31)
    want = reference_compare_frames(allb, edit)
    out = torch.empty(want.shape, dtype=torch.uint8, pin_memory=True)
    got = compare_frames(allb.to(DEV), edit.to(DEV), out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, want)
    assert int((want[:, :, :, :16] != allb).sum()) == 2 * 3 * 47          # the byte values the loader's round trip moves
    # a clip without a byte below 128: the loader's video is >= 0 and the reference does not rescale it
    high = torch.randint(128, 256, (1, 2, 6, 7, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(32))
    e = torch.randint(0, 256, (1, 2, 6, 7, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(33))
    assert torch.equal(compare_frames(high.to(DEV), e.to(DEV)).cpu(), reference_compare_frames(high, e))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", ["inside", "below", "above", "nan"])
def test_normalize_rule_is_decided_on_the_device(case, dtype):
    """Wholly inside [0, 1]: no rescale; ONE element at -1e-3, or at 1 + 1e-3: everything is rescaled; a NaN: no rescale.  The
    flag is written and read on the device: the launches are enqueued on a side stream and nothing is synchronised before the end."""
    x = float_clip(1, 3, 18, 27, True, 41)
    if case in ("below", "nan"):
        x[0, 1, 2, 7, 11] = -1e-3
    if case == "above":
        x[0, 2, 1, 17, 26] = 1 + 1e-3
    if case == "nan":
        x[0, 0, 0, 0, 0] = float("nan")
    x = x.to(dtype)
    edit = byte_clip(1, 3, 18, 27, 42)
    want = reference_compare_frames(x, edit)
    # what the rule must decide, from the values themselves (1 + 1e-3 is 1 in bfloat16: nothing to rescale there)
    outside, nan = bool(((x.float() < 0) | (x.float() > 1)).any()), bool(torch.isnan(x.float()).any())
    assert outside == (case != "inside" and not (case == "above" and dtype == torch.bfloat16)) and nan == (case == "nan")
    as_given = reference_compare_frames(x.nan_to_num(0.5).clamp(0, 1), edit)            # the clip without a rescale
    assert torch.equal(want[0, 1:], as_given[0, 1:]) == (nan or not outside)
    xd, ed = x.to(DEV), edit.to(DEV)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        flag = ops.video_range_flag(xd)
        got = compare_frames(xd, ed)
    stream.synchronize()
    assert int(flag.item()) == int(outside) + 2 * int(nan)
    got, want = got.cpu(), want.clone()
    if case == "nan":
        got[0, 0, 0, 0], want[0, 0, 0, 0] = 0, 0          # the byte a NaN becomes is the C cast's business
    print(f"normalize {case} {dtype}: {int((got != want).sum())} differing bytes of {want.numel()}")
    assert torch.equal(got, want)


def test_range_flag_over_unaligned_and_short_tensors():
    for dtype in (torch.float32, torch.bfloat16):
        for n in (1, 3, 1000, 4099):
            base = torch.rand(n + 1, device=DEV).to(dtype)
            for x in (base[:n], base[1:]):                # 16-byte aligned and not
                assert int(ops.video_range_flag(x).item()) == 0
                y = x.clone() if x.data_ptr() % 16 == 0 else torch.cat([x[:1], x])[1:]
                y[-1] = -0.5
                assert int(ops.video_range_flag(y).item()) == 1
                y[-1] = -0.0                              # -0.0 < 0.0 is false
                assert int(ops.video_range_flag(y).item()) == 0
    u = torch.full((4099,), 200, device=DEV, dtype=torch.uint8)
    assert int(ops.video_range_flag(u).item()) == 0
    u[-1] = 127
    assert int(ops.video_range_flag(u).item()) == 1


def test_arguments_are_checked():
    canvas = torch.zeros(3, 18, 54, 3, device=DEV, dtype=torch.uint8)
    fr = torch.zeros(3, 18, 27, 3, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="leave the"):
        ops.frames_u8_compose(canvas, [dict(tensor=fr, mode=ops.COMPOSE_COPY, dst=(0, 28))])
    with pytest.raises(ValueError, match="overlap"):
        ops.frames_u8_compose(canvas, [dict(tensor=fr, mode=ops.COMPOSE_COPY), dict(tensor=fr, mode=ops.COMPOSE_COPY, dst=(0, 26))])
    with pytest.raises(ValueError, match="window"):
        ops.frames_u8_compose(canvas, [dict(tensor=fr, mode=ops.COMPOSE_COPY, window=(0, 0, 1, 3, 18, 27))])
    with pytest.raises(ValueError, match="NORMALIZE needs the flag"):
        ops.frames_u8_compose(canvas, [dict(tensor=torch.zeros(3, 3, 18, 27, device=DEV), mode=ops.COMPOSE_NORMALIZE)])
    with pytest.raises(ValueError, match="contiguous"):
        ops.frames_u8_compose(canvas[:, :, :27], [])
    with pytest.raises(ValueError, match="rescale applies to float"):
        grid_frames(fr[None], rescale=True)
    with pytest.raises(ValueError, match="out "):
        grid_frames(fr[None], out=torch.empty(3, 18, 28, 3, dtype=torch.uint8))
    # a strided view as a source: every second column of a wider clip
    wide = torch.randint(0, 256, (3, 18, 54, 3), device=DEV, dtype=torch.uint8)
    ops.frames_u8_compose(canvas, [dict(tensor=wide[:, :, ::2], mode=ops.COMPOSE_COPY, dst=(0, 27))])
    assert torch.equal(canvas[:, :, 27:], wide[:, :, ::2]) and int(canvas[:, :, :27].max()) == 0


# ------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def pipe():
    vae = AutoencoderKLWan()
    vae.load_state_dict(deterministic_vae_state_dict(), device=DEV)
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64)
    m.load_state_dict(deterministic_dit_state_dict(**TINY), device=DEV)
    return WanPipeline(vae=vae, transformer=m, scheduler=FlowUniPCMultistepScheduler(shift=1))


def run(pipe, video, cot, **kw):
    ctx = [det_uniform("vio.ctx", (11, 64), 1.0).to(DEV)]
    gen = torch.Generator(device=DEV).manual_seed(7)
    return pipe(video=video, prompt_embeds=ctx, height=32, width=48, source_frames=9, reasoning_frames=4, num_inference_steps=2,
                guidance_scale=1.0, shift=3, repeat_rope=True, cot=cot, generator=gen, weight_dtype=torch.bfloat16,
                output_type="uint8", return_dict=True, **kw)


@pytest.mark.parametrize("cot", [True, False])
def test_pipeline_compare_clip(pipe, cot):
    fr = byte_clip(1, 9, 32, 48, 51)[0]
    plain = run(pipe, fr, cot)
    both = run(pipe, fr, cot, compare=True)
    assert plain.compare_videos is None
    assert torch.equal(plain.latents, both.latents)
    assert np.array_equal(plain.videos, both.videos) and np.array_equal(plain.edit_videos, both.edit_videos)
    if cot:
        assert np.array_equal(plain.ground_videos, both.ground_videos) and np.shares_memory(both.videos, both.edit_videos)
    want = reference_compare_frames(fr[None], torch.from_numpy(both.edit_videos))
    got = both.compare_videos
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (1, 9, 32, 96, 3)
    print(f"pipeline compare cot={cot}: {int((got != want.numpy()).sum())} differing bytes of {got.size}")
    assert np.array_equal(got, want.numpy())
    assert np.array_equal(got[:, :, :, 48:], both.edit_videos) and not np.array_equal(got[0, :, :, :48], fr.numpy())
    assert len(np.unique(got[:, :, :, 48:])) > 16
