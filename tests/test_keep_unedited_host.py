"""CPU: the definitions of the change mask and the composite (videocof_amd/video_io.py: reference_change_mask,
reference_composite_frames), which tests/test_gpu_keep_unedited.py holds the kernels to byte for byte.  Here they are held to a second,
slower statement of DESIGN.md section 4.3.3 (one shifted copy of the plane per window offset instead of running sums) and to the
properties a caller relies on: a changed pixel is taken from the edit entirely, a pixel far from every change is the original's
byte, a batch's samples do not leak into each other, and outside the fit's window nothing but the original is ever written."""
import numpy as np
import pytest
import torch

from videocof_amd import _lib, change_mask, reference_change_mask, reference_composite_frames, reference_fit_frames
from videocof_amd.video_io import _resize_plan, fit_plan

THRESHOLD = 10
# (smooth, grow, grow_t, feather): nothing, the defaults, a small window (so that 19 x 37 has far pixels), the limits
PARAMS = [(0, 0, 0, 0), (2, 12, 1, 8), (1, 2, 0, 1), (1, 3, 1, 3), (7, 32, 4, 32)]


def clips(shape, seed=0, patches=((0, 4, 6, 3, 4), (2, 12, 25, 2, 2))):
    """A random source and an edit of it: noise of +-3 everywhere (below THRESHOLD) and repainted blocks (frame, y, x, h, w), in
    every sample of a batch."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (*shape, 3), generator=g, dtype=torch.uint8)
    noise = torch.randint(-3, 4, src.shape, generator=g)
    edit = (src.long() + noise).clamp(0, 255)
    for t, y, x, h, w in patches:
        if t < shape[-3] and y + h <= shape[-2] and x + w <= shape[-1]:
            edit[..., t, y:y + h, x:x + w, :] = 255 - src[..., t, y:y + h, x:x + w, :].long()
    return src, edit.to(torch.uint8)


def shifted(x, dy, dx, clamp):
    """x[..., y + dy, x + dx] with indices clamped to the frame, or 0 outside it."""
    H, W = x.shape[-2:]
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    out = x[..., np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]]
    if not clamp:
        out = out * (((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :])
    return out


def window_sum(x, r, clamp):
    return sum(shifted(x, dy, dx, clamp) for dy in range(-r, r + 1) for dx in range(-r, r + 1))


def slow_mask(src, edit, threshold, smooth, grow, grow_t, feather):
    """The definition, window offset by window offset -> (b, near, alpha); near = a b within grow + feather pixels and grow_t frames."""
    d = np.abs(edit.numpy().astype(np.int64) - src.numpy().astype(np.int64)).max(-1)
    n = (2 * smooth + 1) ** 2
    b = ((2 * window_sum(d, smooth, True) + n) // (2 * n) > threshold).astype(np.int64)
    T = b.shape[-3]

    def over_frames(p):
        out = np.zeros_like(p)
        for t in range(T):
            out[..., t, :, :] = p[..., max(t - grow_t, 0):min(t + grow_t, T - 1) + 1, :, :].max(-3)
        return out
    g = over_frames((window_sum(b, grow, False) > 0).astype(np.int64))
    m = (2 * feather + 1) ** 2
    alpha = (2 * 255 * window_sum(g, feather, True) + m) // (2 * m)
    near = over_frames((window_sum(b, min(grow + feather, max(b.shape[-2:])), False) > 0).astype(np.int64))
    return b, near, alpha


@pytest.mark.parametrize("shape", [(3, 19, 37), (2, 3, 19, 37)])
@pytest.mark.parametrize("params", PARAMS)
def test_mask_equals_the_slow_statement_and_keeps_its_promises(shape, params):
    src, edit = clips(shape, seed=len(shape))
    alpha = reference_change_mask(src, edit, threshold=THRESHOLD, smooth=params[0], grow=params[1], grow_t=params[2], feather=params[3])
    assert alpha.dtype == torch.uint8 and tuple(alpha.shape) == shape
    b, near, want = slow_mask(src, edit, THRESHOLD, *params)
    assert 0 < b.sum() < b.size
    assert np.array_equal(alpha.numpy(), want)
    assert (alpha.numpy()[b == 1] == 255).all()                  # b = 1 implies alpha = 255
    assert (alpha.numpy()[near == 0] == 0).all()                 # nothing within grow + feather pixels and grow_t frames: 0
    if params == (1, 2, 0, 1):
        assert (near == 0).sum() > b.size // 2 and 0 < (alpha.numpy() % 255 != 0).sum()      # far pixels and a feathered edge exist


def test_identical_clips_give_an_empty_mask_and_the_original():
    src, _ = clips((3, 19, 37), seed=3)
    alpha = reference_change_mask(src, src.clone(), threshold=0)
    assert int(alpha.max()) == 0
    other = torch.randint(0, 256, src.shape, generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    assert torch.equal(reference_composite_frames(other, src, alpha), other)


@pytest.mark.parametrize("grow_t", [1, 4])
def test_a_batch_keeps_its_samples_apart(grow_t):
    src, edit = clips((2, 3, 19, 37), seed=5, patches=((2, 8, 20, 3, 3),))            # the last frame of sample 0 borders sample 1
    edit[1] = src[1]
    alpha = reference_change_mask(src, edit, threshold=THRESHOLD, grow_t=grow_t)
    assert int(alpha[1].max()) == 0 and int(alpha[0].max()) == 255
    assert torch.equal(alpha[0], reference_change_mask(src[0], edit[0], threshold=THRESHOLD, grow_t=grow_t))


def test_windows_larger_than_the_frame():
    src, edit = clips((1, 5, 7), seed=6, patches=((0, 1, 2, 2, 2),))
    for params in [(0, 8, 0, 0), (7, 8, 2, 8), (2, 32, 4, 32)]:
        alpha = reference_change_mask(src, edit, threshold=THRESHOLD, smooth=params[0], grow=params[1], grow_t=params[2], feather=params[3])
        b, _, want = slow_mask(src, edit, THRESHOLD, *params)
        assert np.array_equal(alpha.numpy(), want), params
        if b.any():
            assert int(alpha.min()) == 255                       # one changed pixel and grow >= the frame: everything


@pytest.mark.parametrize("orig,fit", [((54, 100), (32, 48)), ((135, 240), (48, 80))])
def test_composite_with_a_plan(orig, fit):
    plan = fit_plan(*orig, *fit)
    y, x, wh, ww = plan.source_window
    assert (wh, ww) != orig and x > 0                            # the fit crops: part of the original never reached the model
    g = torch.Generator().manual_seed(orig[0])
    o = torch.randint(0, 256, (2, *orig, 3), generator=g, dtype=torch.uint8)
    e = torch.randint(0, 256, (2, *fit, 3), generator=g, dtype=torch.uint8)
    a = torch.randint(0, 256, (2, *fit), generator=g, dtype=torch.uint8)
    inside = torch.zeros(*orig, dtype=torch.bool)
    inside[y:y + wh, x:x + ww] = True
    got = reference_composite_frames(o, e, a, plan)
    assert got.dtype == torch.uint8 and got.shape == o.shape
    assert torch.equal(got[:, ~inside], o[:, ~inside]) and not torch.equal(got[:, inside], o[:, inside])
    full = reference_composite_frames(o, e, torch.full_like(a, 255), plan)
    assert torch.equal(full[:, y:y + wh, x:x + ww], reference_fit_frames(e, wh, ww, plan=_resize_plan(*fit, wh, ww)))
    assert torch.equal(full[:, ~inside], o[:, ~inside])
    assert torch.equal(reference_composite_frames(o, e, torch.zeros_like(a), plan), o)
    with pytest.raises(ValueError, match="plan"):
        reference_composite_frames(o, e, a, fit_plan(orig[0] + 1, orig[1], *fit))
    with pytest.raises(ValueError, match="FitPlan"):
        reference_composite_frames(o, e, a)


def test_same_size_composite_is_the_rounded_blend():
    a, e, o = np.meshgrid(np.arange(256), np.arange(0, 256, 5), np.arange(0, 256, 3), indexing="ij")
    shape = (1, a.shape[0], a.shape[1] * a.shape[2])
    planes = [torch.from_numpy(v.reshape(shape).astype(np.uint8)) for v in (a, e, o)]
    got = reference_composite_frames(planes[2][..., None].expand(*shape, 3), planes[1][..., None].expand(*shape, 3), planes[0])
    want = np.floor((a * e + (255 - a) * o) / 255.0 + 0.5 - 1e-9)                    # round to nearest; a half never occurs (255 is odd)
    assert np.array_equal(got[..., 0].numpy().reshape(a.shape), want.astype(np.uint8))


BAD = [dict(threshold=-1), dict(threshold=255), dict(smooth=8), dict(smooth=-1), dict(grow=33), dict(grow_t=5), dict(grow_t=-1),
       dict(grow=4, feather=5), dict(feather=-1)]


@pytest.mark.parametrize("bad", BAD)
def test_the_limits_raise(bad):
    src, edit = clips((1, 5, 7))
    with pytest.raises(ValueError, match="threshold="):
        reference_change_mask(src, edit, **bad)
    with pytest.raises(ValueError, match="threshold="):          # the device front end checks before it touches a device
        change_mask(src, edit, **bad)
    args = dict(threshold=16, smooth=2, grow=12, grow_t=1, feather=8)
    args.update(bad)
    lib = _lib.load()                                            # and so does the C entry, before anything is enqueued
    st = lib.wan_change_mask(8, 8, 8, 1, 1, 5, 7, args["threshold"], args["smooth"], args["grow"], args["grow_t"], args["feather"], 8, 1 << 20,
                             None)
    assert st == _lib.WAN_ERR_INVALID
    with pytest.raises(ValueError, match="threshold="):
        _lib.check(st, "wan_change_mask")


def test_entry_points_refuse_bad_geometry_before_launching():
    lib = _lib.load()
    assert lib.wan_change_mask_workspace_bytes(2, 3, 19, 37) == 2 * 4352 and lib.wan_change_mask_workspace_bytes(0, 3, 19, 37) == 0
    assert lib.wan_change_mask(8, 8, 8, 1, 3, 19, 37, 16, 2, 12, 1, 8, 8, 100, None) == _lib.WAN_ERR_INVALID          # workspace too small
    assert lib.wan_change_mask(None, 8, 8, 1, 3, 19, 37, 16, 2, 12, 1, 8, 8, 1 << 20, None) == _lib.WAN_ERR_INVALID
    assert lib.wan_frames_u8_composite(8, 8, 8, 8, 2, 54, 100, 0, 20, 54, 81, None) == _lib.WAN_ERR_INVALID           # 20 + 81 > 100
    with pytest.raises(ValueError, match="window"):
        _lib.check(_lib.WAN_ERR_INVALID, "wan_frames_u8_composite")
    assert lib.wan_frames_u8_composite(8, 8, 8, 8, 2, 54, 100, -1, 0, 54, 81, None) == _lib.WAN_ERR_INVALID
    assert lib.wan_plane_u8_resample(8, 8, 8, 2, 32, 48, 54, 81, 8, 25, 8, 2, None) == _lib.WAN_ERR_UNSUPPORTED       # 25 taps
    assert lib.wan_plane_u8_resample(8, None, 8, 2, 32, 48, 54, 81, 8, 2, 8, 2, None) == _lib.WAN_ERR_INVALID
