"""-m gpu: the clip statistics on the device (wan_clip_stats behind video_io.clip_stats / ops.clip_stats) against
``reference_clip_stats``, the numpy definition that tests/test_clip_stats_host.py checks.  EQUALITY of every word: both sides count in
integers, and the one division of an SSIM window is the same IEEE double division on both.

The byte histogram walks a frame in runs of 16 pixels and tiles of 4096, the smoothed histogram in tiles of 32 x 64 pixels with a
border of up to 7, SSIM in tiles of 8 x 32 blocks of 4 x 4 pixels of which 7 x 31 windows are owned; a workgroup takes several tiles
of its frame.  So the shapes cover a frame inside one tile, remainders in every axis, more tiles than workgroups, a window larger
than the frame, frames without SSIM windows and a base at an odd address."""
import numpy as np
import pytest
import torch

from videocof_amd import (AutoencoderKLWan, ClipStats, change_mask, clip_stats, ops, reference_clip_stats, vae_roundtrip_frames)
from videocof_amd.weights import deterministic_vae_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLD = 10
FIELDS = ("diff_hist", "smooth_hist", "ssim_sum", "ssim_windows")


def clips(shape, seed=0):
    """A random source and an edit of it: noise of +-3 everywhere (below THRESHOLD), and per frame one repainted block and a few
    repainted single pixels at seeded places, so every step of the mask has edges inside the frame and at its borders."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (*shape, 3), generator=g, dtype=torch.uint8)
    edit = (src.long() + torch.randint(-3, 4, src.shape, generator=g)).clamp(0, 255)
    T, H, W = shape[-3:]
    flat_s, flat_e = src.view(-1, H, W, 3), edit.view(-1, H, W, 3)
    for n in range(flat_s.shape[0]):
        if n % 2 == 0 or T == 1:
            y, x = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
            flat_e[n, y:y + 4, x:x + 6] = 255 - flat_s[n, y:y + 4, x:x + 6].long()
            for _ in range(3):
                y, x = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
                flat_e[n, y, x] = 255 - flat_s[n, y, x].long()
    return src, edit.to(torch.uint8)


def same(got: ClipStats, want: ClipStats, what=""):
    assert got.smooth == want.smooth
    bad = {}
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == np.int64 and g.shape == w.shape, (f, g.dtype, g.shape, w.shape)
        bad[f] = int((g != w).sum())
    print(f"clip_stats {what}: words that differ {bad}; ssim_sum {want.ssim_sum.ravel()[:4].tolist()} windows "
          f"{want.ssim_windows.ravel()[:4].tolist()}")
    assert not any(bad.values()), bad


def check(a, b, alpha=None, smooth=2, dev=None):
    want = reference_clip_stats(a, b, alpha, smooth=smooth)
    da, db, dal = dev if dev is not None else (a.to(DEV), b.to(DEV), None if alpha is None else alpha.to(DEV))
    got = clip_stats(da, db, dal, smooth=smooth)
    same(got, want, f"{tuple(a.shape)} smooth={smooth} alpha={'no' if alpha is None else 'yes'}")
    return want


@pytest.mark.parametrize("smooth", [0, 2, 7])
@pytest.mark.parametrize("shape", [(3, 19, 37), (4, 70, 200)])
def test_clip_stats_equal_the_definition(shape, smooth):
    want = check(*clips(shape, seed=shape[1]), smooth=smooth)
    assert not want.diff_hist[:, 1].any() and (want.diff_hist[:, 0].sum(-1) == 3 * shape[1] * shape[2]).all()


@pytest.mark.parametrize("smooth", [0, 2, 7])
@pytest.mark.parametrize("shape", [(3, 19, 37), (4, 70, 200)])
def test_clip_stats_under_a_change_mask(shape, smooth):
    src, edit = clips(shape, seed=shape[1])
    alpha = change_mask(src, edit, threshold=THRESHOLD, smooth=2, grow=3, grow_t=1, feather=2).cpu()
    want = check(src, edit, alpha, smooth=smooth)
    if shape == (4, 70, 200):                                                        # both regions occur, in every statistic
        for f in FIELDS:
            assert (getattr(want, f).reshape(4, 2, -1).sum(-1) != 0).all(), f
        assert (want.max_diff(region=1)[::2] > 200).all()                            # frames 0 and 2: the mask covers the repainted block


def test_window_larger_than_the_frame_and_no_ssim_windows():
    src, edit = clips((1, 5, 7), seed=2)
    want = check(src, edit, smooth=7)
    assert not want.ssim_windows.any() and not want.ssim_sum.any() and want.smooth_hist.sum() == 35


@pytest.mark.parametrize("shape", [(1, 8, 8), (1, 9, 13)])
def test_one_and_two_windows(shape):
    src, edit = clips(shape, seed=3)
    want = check(src, edit)
    assert want.ssim_windows[0, 0] == 3 * ((shape[1] >> 2) - 1) * ((shape[2] >> 2) - 1)
    alpha = torch.zeros(shape, dtype=torch.uint8)
    alpha[0, 7, 7] = 1
    check(src, edit, alpha, smooth=1)


def test_misaligned_batch_and_host_inputs():
    src, edit = clips((2, 3, 19, 37), seed=4)
    alpha = (torch.rand(2, 3, 19, 37, generator=torch.Generator().manual_seed(5)) < 0.3).to(torch.uint8) * 255
    views = []
    for fr in (src, edit, alpha):
        flat = torch.zeros(fr.numel() + 1, dtype=torch.uint8, device=DEV)
        flat[1:] = fr.to(DEV).view(-1)
        views.append(flat[1:].view(fr.shape))
        assert views[-1].data_ptr() % 2 == 1
    want = check(src, edit, alpha, dev=views)
    one = reference_clip_stats(src[1], edit[1], alpha[1])
    for f in FIELDS:
        assert np.array_equal(getattr(want, f)[1], getattr(one, f)), f               # a sample of a batch is that sample alone
    same(clip_stats(views[0][1], views[1][1], views[2][1]), one, "sample 1 alone")
    same(clip_stats(src.numpy(), edit, alpha.numpy()), want, "host inputs")
    same(clip_stats(src, edit), reference_clip_stats(src, edit), "host inputs, no alpha")


def test_every_bin_with_a_count_of_its_own():
    """One 256 x 300 frame: in row v the first v + 1 pixels differ by exactly v in all channels, the rest are equal.  Bin v > 0 of the
    byte histogram holds 3 (v + 1), a count no other bin has, so a shifted or merged bin cannot cancel."""
    v = torch.arange(256).view(256, 1, 1)
    on = torch.arange(300).view(1, 300, 1) <= v
    a = torch.randint(0, 256, (256, 300, 3), generator=torch.Generator().manual_seed(6)) % (256 - v)       # room for + v
    b = torch.where(on, a + v, a)
    assert int(a.min()) >= 0 and int(b.max()) <= 255
    a, b = a.to(torch.uint8)[None], b.to(torch.uint8)[None]
    want = check(a, b, smooth=0)
    expect = 3 * (torch.arange(256) + 1)
    expect[0] = 3 * 256 * 300 - int(expect[1:].sum())
    assert want.diff_hist[0, 0].tolist() == expect.tolist() and len(set(expect.tolist())) == 256
    assert want.smooth_hist[0, 0].tolist() == (expect // 3).tolist()                # smooth = 0: s is d
    check(a, b, smooth=2)


@pytest.mark.parametrize("far", [False, True])
def test_every_byte_in_one_bin(far):
    """1024 x 1024 with a == b (everything in bin 0) and with a = 0, b = 255 (everything in bin 255): the two ways of counting, the
    registers and the LDS atomics, under full contention.  The counts are known without a reference."""
    a = torch.zeros(1, 1024, 1024, 3, dtype=torch.uint8, device=DEV)
    if not far:
        a.copy_(torch.randint(0, 256, a.shape, generator=torch.Generator().manual_seed(7), dtype=torch.uint8))
    b = torch.full_like(a, 255) if far else a.clone()
    s = clip_stats(a, b, smooth=2)
    bin_, windows = (255 if far else 0), 3 * 255 * 255
    assert s.diff_hist[0, 0, bin_] == 3 << 20 and s.diff_hist.sum() == 3 << 20
    assert s.smooth_hist[0, 0, bin_] == 1 << 20 and s.smooth_hist.sum() == 1 << 20
    assert s.ssim_windows.tolist() == [[windows, 0]]
    if far:                                                                          # s1 = 0, s2 = 64 * 255, ss = 64 * 255^2: vars = covar = 0
        q = int(np.rint(416.0 * 235963.0 / ((16320.0 ** 2 + 416.0) * 235963.0) * 2.0 ** 20))
        assert s.ssim_sum.tolist() == [[windows * q, 0]]
    else:
        assert s.ssim_sum.tolist() == [[windows << 20, 0]] and s.ssim()[0] == 1.0 and np.isposinf(s.psnr()[0])


def test_out_is_overwritten_and_nothing_beside_it():
    src, edit = clips((1, 3, 19, 37), seed=8)
    alpha = (torch.rand(1, 3, 19, 37, generator=torch.Generator().manual_seed(9)) < 0.5).to(torch.uint8)
    want = reference_clip_stats(src, edit, alpha)
    sentinel, n = -0x0123456789abcdef, 3 * 2 * ops.CLIP_STATS_WORDS
    buf = torch.full((3 * n,), sentinel, dtype=torch.int64, device=DEV)
    out = buf[n:2 * n].view(1, 3, 2, ops.CLIP_STATS_WORDS)
    for call in range(2):                                                            # the second call finds the first one's words
        res = ops.clip_stats(src.to(DEV), edit.to(DEV), alpha.to(DEV), 2, out=out)
        assert res.data_ptr() == out.data_ptr()
        w = out.cpu().numpy()
        got = ClipStats(w[0, ..., :256], w[0, ..., 256:512], w[0, ..., 512], w[0, ..., 513], 2)
        same(got, ClipStats(*(getattr(want, f)[0] for f in FIELDS), 2), f"out=, call {call}")
        assert bool((buf[:n] == sentinel).all()) and bool((buf[2 * n:] == sentinel).all())
    with pytest.raises(ValueError, match="out"):
        ops.clip_stats(src.to(DEV), edit.to(DEV), None, 2, out=torch.empty(1, 3, 2, 513, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("t", [0, 3, THRESHOLD, 100])
def test_smoothed_histogram_and_change_mask_agree_on_the_device(t):
    src, edit = clips((4, 70, 200), seed=70)
    s = clip_stats(src.to(DEV), edit.to(DEV), smooth=2)
    mask = change_mask(src.to(DEV), edit.to(DEV), threshold=t, smooth=2, grow=0, grow_t=0, feather=0)
    assert int(s.smooth_hist[:, :, t + 1:].sum()) == int((mask == 255).sum()) > 0


def test_argument_errors():
    src, edit = clips((1, 8, 8), seed=10)
    with pytest.raises(ValueError, match="differ in shape"):
        clip_stats(src, edit[:, :4])
    with pytest.raises(ValueError, match="smooth=8"):
        clip_stats(src, edit, smooth=8)
    with pytest.raises(ValueError, match="alpha"):
        clip_stats(src, edit, torch.zeros(1, 8, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        clip_stats(src.float(), edit.float())


def test_vae_roundtrip_frames():
    vae = AutoencoderKLWan()
    vae.load_state_dict(deterministic_vae_state_dict(), device=DEV)
    frames = torch.randint(0, 256, (5, 32, 48, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8)
    got = vae_roundtrip_frames(vae, frames)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (5, 32, 48, 3)
    video = ops.frames_u8_to_video(frames.to(DEV)[None], vae.dtype)
    want = ops.video_to_frames_u8(vae.decode(vae.encode(video)[0].mode().to(vae.dtype)).sample)
    assert torch.equal(got, want[0])
    assert torch.equal(vae_roundtrip_frames(vae, frames.to(DEV)[None]), want)        # a device batch of one
    s = clip_stats(frames, got)
    t = s.threshold_for()
    print(f"vae round trip of random frames (deterministic weights): psnr {s.psnr(per_frame=False):.2f} dB, ssim "
          f"{s.ssim(per_frame=False):.4f}, threshold_for() = {t}")
    assert isinstance(t, int) and 0 <= t <= 254
    same(s, reference_clip_stats(frames, got), "vae round trip")
