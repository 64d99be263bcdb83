"""The definition of the clip statistics (``reference_clip_stats`` and the methods of ``ClipStats``) on the
host: properties of the definition itself, its tie to ``reference_change_mask``, and the argument checks of the C entry point, which
return before anything is launched.  tests/test_gpu_clip_stats.py holds the kernels to this definition word for word."""
import math

import numpy as np
import pytest
import torch

from videocof_amd import ClipStats, _lib, reference_change_mask, reference_clip_stats


def noisy(shape, seed=0, repaint=4):
    """A random clip and a copy with +-3 noise everywhere and, per frame, `repaint` pixels set to their complement."""
    g = np.random.default_rng(seed)
    a = g.integers(0, 256, (*shape, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + g.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
    fa, fb = a.reshape(-1, *shape[-2:], 3), b.reshape(-1, *shape[-2:], 3)
    for n in range(fa.shape[0]):
        for _ in range(repaint):
            y, x = int(g.integers(0, shape[-2])), int(g.integers(0, shape[-1]))
            fb[n, y, x] = 255 - fa[n, y, x]
    return a, b


@pytest.mark.parametrize("shape", [(3, 19, 37), (2, 3, 9, 13)])
def test_histograms_count_every_byte_and_every_pixel_once(shape):
    a, b = noisy(shape, seed=1)
    H, W = shape[-2:]
    alpha = (np.random.default_rng(2).random(shape) < 0.3).astype(np.uint8) * 200
    for al in (None, alpha):
        s = reference_clip_stats(a, b, al, smooth=2)
        assert isinstance(s, ClipStats) and s.smooth == 2
        assert s.diff_hist.shape == (*shape[:-2], 2, 256) and s.smooth_hist.shape == s.diff_hist.shape
        assert s.ssim_sum.shape == (*shape[:-2], 2) and s.ssim_windows.shape == s.ssim_sum.shape
        assert all(x.dtype == np.int64 for x in (s.diff_hist, s.smooth_hist, s.ssim_sum, s.ssim_windows))
        assert (s.diff_hist.sum((-1, -2)) == 3 * H * W).all() and (s.smooth_hist.sum((-1, -2)) == H * W).all()
        assert (s.ssim_windows.sum(-1) == 3 * ((H >> 2) - 1) * ((W >> 2) - 1)).all()
        if al is None:
            assert not s.diff_hist[..., 1, :].any() and not s.smooth_hist[..., 1, :].any()
            assert not s.ssim_sum[..., 1].any() and not s.ssim_windows[..., 1].any()
        else:
            assert (s.diff_hist[..., 1, :].sum(-1) == 3 * (alpha != 0).sum((-1, -2))).all()
            assert (s.smooth_hist[..., 1, :].sum(-1) == (alpha != 0).sum((-1, -2))).all()
            whole = reference_clip_stats(a, b, None, smooth=2)                     # the regions partition the unmasked statistics
            for name in ("diff_hist", "smooth_hist", "ssim_sum", "ssim_windows"):
                assert np.array_equal(getattr(s, name).sum(-2 if "hist" in name else -1),
                                      getattr(whole, name)[..., 0, :] if "hist" in name else getattr(whole, name)[..., 0])


def test_identical_clips():
    a, _ = noisy((2, 16, 24), seed=3)
    s = reference_clip_stats(a, a)
    assert (s.diff_hist[:, 0, 0] == 3 * 16 * 24).all() and s.diff_hist.sum() == 2 * 3 * 16 * 24
    assert (s.smooth_hist[:, 0, 0] == 16 * 24).all() and s.smooth_hist.sum() == 2 * 16 * 24
    assert (s.ssim_sum[:, 0] == s.ssim_windows[:, 0] << 20).all() and (s.ssim_windows[:, 0] == 3 * 3 * 5).all()
    assert np.isposinf(s.psnr()).all() and np.isposinf(s.psnr(per_frame=False))
    assert (s.ssim() == 1.0).all() and s.ssim(per_frame=False) == 1.0 and (s.ssim(region=0) == 1.0).all()
    assert (s.mae() == 0.0).all() and (s.max_diff() == 0).all() and (s.quantile(1.0) == 0).all()
    assert np.isnan(s.psnr(region=1)).all() and np.isnan(s.ssim(region=1)).all() and np.isnan(s.mae(region=1)).all()
    assert s.threshold_for() == 0


def test_psnr_mae_maximum_and_quantiles_equal_the_pixels():
    a, b = noisy((3, 19, 37), seed=4)
    alpha = np.zeros((3, 19, 37), np.uint8)
    alpha[:, 5:12, 8:30] = 9
    s = reference_clip_stats(a, b, alpha)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    m = alpha != 0

    def close(got, want):
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)

    for t in range(3):
        close(s.psnr()[t], 10 * math.log10(255.0 ** 2 / (d[t] ** 2).mean()))
        close(s.mae()[t], d[t].mean())
        close(s.psnr(region=1)[t], 10 * math.log10(255.0 ** 2 / (d[t][m[t]] ** 2).mean()))
        close(s.mae(region=0)[t], d[t][~m[t]].mean())
        assert s.max_diff()[t] == d[t].max() and s.max_diff(region=1)[t] == d[t][m[t]].max()
        for q in (0.0, 0.5, 0.99, 1.0):
            v = np.sort(d[t].ravel())
            assert s.quantile(q)[t] == v[max(math.ceil(q * v.size), 1) - 1] if q > 0 else s.quantile(q)[t] == 0
    close(s.psnr(per_frame=False), 10 * math.log10(255.0 ** 2 / (d ** 2).mean()))
    close(s.mae(region=1, per_frame=False), d[m].mean())
    assert s.max_diff(per_frame=False) == d.max()
    with pytest.raises(ValueError, match="region"):
        s.psnr(region=2)


@pytest.mark.parametrize("smooth", [0, 2, 7])
def test_smoothed_histogram_is_the_change_mask_before_its_threshold(smooth):
    a, b = noisy((3, 19, 37), seed=5, repaint=12)
    s = reference_clip_stats(a, b, smooth=smooth)
    for t in (0, 1, 2, 3, 10, 40, 254):
        mask = reference_change_mask(a, b, threshold=t, smooth=smooth, grow=0, grow_t=0, feather=0)
        assert set(np.unique(mask.numpy())) <= {0, 255}
        assert np.array_equal(s.smooth_hist[:, 0, t + 1:].sum(-1), (mask.numpy() == 255).sum((-1, -2))), t


def test_threshold_for_is_the_smallest_threshold_under_the_share():
    a, b = noisy((4, 40, 60), seed=6, repaint=3)               # 12 repainted pixels of 9600: their 5 x 5 windows exceed 1e-3 of the clip
    pixels, share = 4 * 40 * 60, 2e-2
    s = reference_clip_stats(a, b, smooth=2)
    t = s.threshold_for(share)
    assert isinstance(t, int) and 1 <= t <= 254

    def marked(thr):
        return int((reference_change_mask(a, b, threshold=thr, smooth=2, grow=0, grow_t=0, feather=0) == 255).sum())

    limit = math.floor(share * pixels)
    print(f"threshold_for({share}) = {t}: marks {marked(t)} of {pixels}, limit {limit}; {t - 1} marks {marked(t - 1)}")
    assert marked(t) <= limit < marked(t - 1)
    assert s.threshold_for(1.0) == 0 and s.threshold_for(0.0) == int(np.nonzero(s.smooth_hist.sum((0, 1)))[0].max())
    far = reference_clip_stats(np.zeros_like(a), np.full_like(a, 255))            # no threshold in 0..254 qualifies
    assert far.threshold_for(0.5) == 254


def test_ssim_shapes_and_sign():
    g = np.random.default_rng(7)
    a = g.integers(0, 256, (1, 8, 8, 3), dtype=np.uint8)
    s = reference_clip_stats(a, 255 - a)
    assert s.ssim_windows[0, 0] == 3 and s.ssim_sum[0, 0] < 0 and s.ssim()[0] < 0                   # one window per plane, signed
    board = (np.indices((8, 8)).sum(0) % 2 * 255).astype(np.uint8)
    board = np.repeat(board[None, :, :, None], 3, -1)
    assert reference_clip_stats(board, 255 - board).ssim_sum[0, 0] == 3 * -1044867
    # 9 x 13: h4 = 2, w4 = 3; row 8 and column 12 are not read
    a, b = noisy((2, 9, 13), seed=8)
    a2, b2 = a.copy(), b.copy()
    a2[:, 8], b2[:, :, 12] = 255 - a2[:, 8], 255 - b2[:, :, 12]
    s, s2 = reference_clip_stats(a, b), reference_clip_stats(a2, b2)
    assert (s.ssim_windows[:, 0] == 3 * 1 * 2).all()
    assert np.array_equal(s.ssim_sum, s2.ssim_sum) and not np.array_equal(s.diff_hist, s2.diff_hist)
    # 7 x 40: one row of blocks, no windows
    a, b = noisy((1, 7, 40), seed=9)
    s = reference_clip_stats(a, b)
    assert not s.ssim_windows.any() and not s.ssim_sum.any() and np.isnan(s.ssim()).all() and s.diff_hist.sum() == 3 * 7 * 40
    # a window belongs to region 1 if any of its 64 alpha bytes is set
    a, b = noisy((1, 12, 16), seed=10)
    alpha = np.zeros((1, 12, 16), np.uint8)
    alpha[0, 11, 15] = 1                                                             # the last block: the last window only
    s = reference_clip_stats(a, b, alpha)
    assert s.ssim_windows[0].tolist() == [3 * (2 * 3 - 1), 3]


def test_ssim_window_equals_the_formula_written_out():
    a, b = noisy((1, 8, 8), seed=11, repaint=20)
    want = 0
    for c in range(3):
        x, y = a[0, :, :, c].astype(np.int64), b[0, :, :, c].astype(np.int64)
        s1, s2, ss, s12 = int(x.sum()), int(y.sum()), int((x * x + y * y).sum()), int((x * y).sum())
        vars_, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
        q = (float(2 * s1 * s2 + 416) * float(2 * covar + 235963)) / (float(s1 * s1 + s2 * s2 + 416) * float(vars_ + 235963)) * 2.0 ** 20
        want += int(np.rint(q))
    assert reference_clip_stats(a, b).ssim_sum[0, 0] == want


def test_argument_errors():
    a, b = noisy((2, 8, 8), seed=12)
    with pytest.raises(ValueError, match="differ in shape"):
        reference_clip_stats(a, b[:1])
    with pytest.raises(ValueError, match="uint8"):
        reference_clip_stats(a.astype(np.int32), b.astype(np.int32))
    with pytest.raises(ValueError, match="smooth=8"):
        reference_clip_stats(a, b, smooth=8)
    with pytest.raises(ValueError, match="smooth=-1"):
        reference_clip_stats(a, b, smooth=-1)
    with pytest.raises(ValueError, match="alpha"):
        reference_clip_stats(a, b, np.zeros((2, 8, 9), np.uint8))
    with pytest.raises(ValueError, match="alpha"):
        reference_clip_stats(a, b, np.zeros((2, 8, 8), np.float32))
    assert reference_clip_stats(torch.from_numpy(a), torch.from_numpy(b), torch.zeros(2, 8, 8, dtype=torch.uint8)).smooth == 2


def test_the_entry_point_validates_before_it_launches():
    lib = _lib.load()
    p = 256                                                   # never dereferenced: every call below returns before a launch
    need = lib.wan_clip_stats_workspace_bytes(1, 8, 8)
    assert need > 0 and lib.wan_clip_stats_workspace_bytes(0, 8, 8) == 0
    for args in ((None, p, None, p, 1, 8, 8, 2, p, need, None), (p, None, None, p, 1, 8, 8, 2, p, need, None),
                 (p, p, None, None, 1, 8, 8, 2, p, need, None)):
        assert lib.wan_clip_stats(*args) == _lib.WAN_ERR_INVALID
    with pytest.raises(ValueError, match="null tensor"):
        _lib.check(_lib.WAN_ERR_INVALID, "wan_clip_stats")
    for smooth in (8, -1):
        assert lib.wan_clip_stats(p, p, None, p, 1, 8, 8, smooth, p, need, None) == _lib.WAN_ERR_INVALID
    for shape in ((0, 8, 8), (1, -8, 8), (1, 8, 0)):
        assert lib.wan_clip_stats(p, p, None, p, *shape, 2, p, need, None) == _lib.WAN_ERR_INVALID
    assert lib.wan_clip_stats(p, p, None, p, 1, 8, 8, 2, None, 0, None) == _lib.WAN_ERR_INVALID          # no workspace
    assert lib.wan_clip_stats(p, p, None, p, 1, 8, 8, 2, p, need - 1, None) == _lib.WAN_ERR_INVALID      # too small a one
    assert lib.wan_clip_stats(p, p, None, p, 65536, 8, 8, 2, p, 1 << 40, None) == _lib.WAN_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="65535 frames"):
        _lib.check(_lib.WAN_ERR_UNSUPPORTED, "wan_clip_stats")
