"""CPU: the geometry and the arithmetic of the clip fit (videocof_amd/video_io.py: fit_size, fit_plan, reference_fit_frames), and
the ABI of its kernel.  ``reference_fit_frames`` is what tests/test_gpu_frame_fit.py holds the kernel to bit for bit; here it is
pinned to Pillow's 8-bit BILINEAR resample (whose antialiased triangle it restates) followed by the crop, byte for byte."""
import ctypes
import math

import numpy as np
import pytest
import torch

import videocof_amd
from videocof_amd import _lib, video_io
from videocof_amd.video_io import fit_plan, fit_size, reference_fit_frames, resample_axis_table

# (clip height, width) -> (target height, width): odd sources, non-integer and 4x downscales, a 2x upscale, equal sizes, an
# upscale in one axis with a large crop in the other, windows clipped at both borders
PAIRS = [((37, 53), (32, 48)), ((135, 240), (48, 80)), ((130, 70), (16, 16)), ((24, 40), (48, 80)), ((48, 80), (48, 80)),
         ((270, 480), (120, 208)), ((50, 33), (32, 48)), ((17, 19), (16, 16))]


def random_frame(h, w, seed=0):
    return torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def test_fit_size_table():
    assert fit_size(1080, 1920) == (464, 848)
    assert fit_size(480, 854) == (464, 848)
    assert fit_size(480, 832) == (480, 832)
    assert fit_size(1920, 1080) == (848, 464)


def test_fit_size_properties():
    for h in list(range(1, 2300, 41)) + [480, 720, 1080, 2160]:
        for w in list(range(1, 4100, 59)) + [832, 854, 1280, 1920, 3840]:
            H, W = fit_size(h, w)
            assert H % 16 == 0 and W % 16 == 0 and H >= 16 and W >= 16 and H * W <= 480 * 832, (h, w, H, W)
            assert fit_size(w, h) == (W, H)
            if h % 16 == 0 and w % 16 == 0 and h * w <= 480 * 832:
                assert (H, W) == (h, w)
            if min(H, W) > 16:                       # the ratio, up to one grid step per side
                assert (H - 16) / (W + 16) <= h / w <= (H + 16) / (W - 16), (h, w, H, W)
    assert fit_size(96, 160, max_area=48 * 80) == (48, 80)
    assert fit_size(100, 100, max_area=64 * 64, multiple=32) == (64, 64)
    with pytest.raises(ValueError):
        fit_size(0, 10)


def test_fit_plan_is_the_training_loaders_geometry():
    """videox_fun/data/dataset_image_video.py:464-477 restated line by line."""
    for (h, w), (th, tw) in PAIRS + [((1080, 1920), (464, 848)), ((480, 854), (464, 848)), ((1920, 1080), (848, 464))]:
        scale = max(th / h, tw / w)
        new_h = int(round(h * scale))
        new_w = int(round(w * scale))
        y0 = max((new_h - th) // 2, 0)
        x0 = max((new_w - tw) // 2, 0)
        p = fit_plan(h, w, th, tw)
        assert (p.scale, p.new_height, p.new_width, p.y0, p.x0) == (scale, new_h, new_w, y0, x0)
        assert (p.height, p.width, p.out_height, p.out_width) == (h, w, th, tw)
        assert p.new_height >= th and p.new_width >= tw                 # the crop never runs out of picture
        y, x, wh, ww = p.source_window
        assert 0 <= y and 0 <= x and wh >= 1 and ww >= 1 and y + wh <= h and x + ww <= w
        assert abs(y - y0 / scale) <= 0.5 + 1e-9 and abs(x - x0 / scale) <= 0.5 + 1e-9
        assert abs(wh - th / scale) <= 1.0 and abs(ww - tw / scale) <= 1.0
    assert fit_plan(37, 53, 32, 48).source_window == (1, 0, 35, 53)
    assert fit_plan(48, 80, 48, 80).source_window == (0, 0, 48, 80)


@pytest.mark.parametrize("src,dst", PAIRS)
def test_reference_equals_pillow_bilinear_and_crop(src, dst):
    Image = pytest.importorskip("PIL.Image")
    fr = random_frame(*src, seed=src[0])
    fr[0, :16].view(-1)[:48] = torch.arange(48, dtype=torch.uint8) * 5        # some structure next to the noise
    p = fit_plan(*src, *dst)
    want = np.asarray(Image.fromarray(fr.numpy()).resize((p.new_width, p.new_height), Image.BILINEAR))
    want = want[p.y0:p.y0 + dst[0], p.x0:p.x0 + dst[1]]
    got = reference_fit_frames(fr, *dst).numpy()
    assert got.shape == want.shape and np.array_equal(got, want)


def test_constant_frames_stay_constant():
    vals = torch.arange(256, dtype=torch.uint8)
    for src, dst in PAIRS:
        fr = vals.view(256, 1, 1, 1).expand(256, src[0], src[1], 3)
        got = reference_fit_frames(fr, *dst)
        assert torch.equal(got, vals.view(256, 1, 1, 1).expand(256, dst[0], dst[1], 3)), (src, dst)


def test_identity_at_equal_size():
    fr = random_frame(48, 80, seed=3)[None].repeat(2, 1, 1, 1)
    assert torch.equal(reference_fit_frames(fr, 48, 80), fr)
    xmin, n, k = resample_axis_table(80, 80)
    assert np.array_equal(xmin, np.arange(80)) and np.array_equal(k[:, 0], np.full(80, 1 << 22)) and not k[:, 1:].any()


def test_tables_weights_sum_to_one_and_tiles_stay_inside_the_kernels_staging():
    """The coefficients are non-negative and sum to 2^22 up to their rounding (so a byte times the sum fits 32 bits); windows move
    monotonically, and a tile of 16 / 64 outputs spans no more source positions than the kernel sizes its LDS for from the tap
    count alone (span_bound in csrc/frame_fit.hip)."""
    def span_bound(tile, k):
        return (tile - 1) * ((k + 2) // 2) + k + 3
    for in_size in list(range(1, 200, 7)) + [480, 854, 1080, 1920, 4000]:
        for new in (1, 5, 16, 17, 33, 48, 100, 464, 848, 1000):
            xmin, n, k = resample_axis_table(in_size, new)
            taps = k.shape[1]
            assert (k >= 0).all() and (np.abs(k.sum(1) - (1 << 22)) <= taps).all()
            assert (n >= 1).all() and (xmin >= 0).all() and (xmin + n <= in_size).all() and taps == n.max()
            assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + n) >= 0).all()
            for tile in (16, 64):
                for s in range(0, new, tile):
                    e = min(s + tile, new) - 1
                    assert xmin[e] + n[e] - xmin[s] <= span_bound(tile, taps), (in_size, new, tile, s)
    assert resample_axis_table(128, 16)[2].shape[1] == 16 and resample_axis_table(130, 16)[2].shape[1] <= 19       # an 8x downscale
    sub = resample_axis_table(85, 240 * 85 // 240, 2, 80)
    full = resample_axis_table(85, 85)
    assert np.array_equal(sub[0], full[0][2:82])                    # a crop only selects output indices


def test_the_surface_is_exported():
    names = {"fit_size", "fit_plan", "fit_frames", "restore_frames", "reference_fit_frames"}
    assert names <= set(video_io.__all__)
    for name in names:
        assert getattr(videocof_amd, name) is getattr(video_io, name)
    with pytest.raises((RuntimeError, AssertionError, ValueError)):
        video_io.fit_frames(torch.zeros(2, 16, 16, 4, dtype=torch.uint8))          # not RGB frames: refused before any device work
    with pytest.raises(ValueError):
        video_io.fit_frames(torch.zeros(2, 16, 16, 3))                              # not bytes


def test_export_is_declared_exported_and_bound():
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "wan_hip.h")).read()
    for sym in ("wan_frames_u8_resample", "wan_frames_resample_table_bytes"):
        assert sym in _lib.SIGNATURES and hasattr(raw, sym) and f"{sym}(" in header
    assert _lib.ABI_VERSION == 11 and lib.wan_abi_version() == 11               # additive: no existing entry changed
    assert "#define WAN_RESAMPLE_MAX_TAPS 24" in header and video_io.MAX_TAPS == 24
    assert lib.wan_frames_resample_table_bytes(848, 5) == 848 * 7 * 4 and lib.wan_frames_resample_table_bytes(0, 5) == 0


def test_argument_errors_without_a_gpu():
    lib = _lib.load()
    f = lib.wan_frames_u8_resample
    assert f(None, None, 1, 1, 16, 16, 16, 16, None, 2, None, 2, None) == _lib.WAN_ERR_INVALID
    assert f(16, 16, 1, 1, 16, 16, 16, 16, None, 2, 16, 2, None) == _lib.WAN_ERR_INVALID                 # one null table
    with pytest.raises(ValueError, match="null tensor"):
        _lib.check(f(16, None, 1, 1, 16, 16, 16, 16, 16, 2, 16, 2, None), "wan_frames_u8_resample")
    assert f(16, 16, 1, 0, 16, 16, 16, 16, 16, 2, 16, 2, None) == _lib.WAN_ERR_INVALID                   # T = 0
    assert f(16, 16, 1, 1, 16, 16, 16, 16, 16, 0, 16, 2, None) == _lib.WAN_ERR_INVALID                   # no taps
    st = f(16, 16, 1, 1, 400, 16, 16, 16, 16, 2, 16, 25, None)                                           # 25 taps: beyond the build
    assert st == _lib.WAN_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="filter taps"):
        _lib.check(st, "wan_frames_u8_resample")
    st = f(16, 16, 2, 32768, 16, 16, 16, 16, 16, 2, 16, 2, None)                                         # 65536 frames
    assert st == _lib.WAN_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="at most 65535"):
        _lib.check(st, "wan_frames_u8_resample")
    with pytest.raises(RuntimeError, match="filter taps"):                                              # the host refuses it first
        video_io._device_table(1000, 16, 0, 16, "cpu")
