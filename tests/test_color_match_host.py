"""Colour match on the host: ``reference_color_stats`` / ``reference_color_coefficients`` / ``reference_frames_affine`` (the numpy /
Python-int definitions the kernels are held to) against a brute-force loop over pixels written from the
definition's text, the constructions whose answer is known in closed form, and the argument checks of the public functions, which
all run before anything touches a device."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from videocof_amd import (color_match, color_match_coefficients, reference_color_coefficients, reference_color_match,
                          reference_color_stats, reference_frames_affine)

ONE = 4096


def brute_stats(ref, edit, alpha):
    """[B, T, 16] by a loop over every pixel; ref / alpha may hold one frame per sample."""
    B, T, H, W, _ = edit.shape
    out = np.zeros((B, T, 16), np.int64)
    for b in range(B):
        for t in range(T):
            rt = t if ref.shape[1] == T else 0
            s = [0] * 16
            for y in range(H):
                for x in range(W):
                    if alpha is not None and int(alpha[b, rt, y, x]) != 0:
                        continue
                    s[0] += 1
                    for c in range(3):
                        r, e = int(ref[b, rt, y, x, c]), int(edit[b, t, y, x, c])
                        s[1 + 4 * c] += r
                        s[2 + 4 * c] += e
                        s[3 + 4 * c] += r * r
                        s[4 + 4 * c] += e * e
            out[b, t] = s
    return out


def brute_coef(stats, pool_t, gain, min_pixels):
    """The coefficients written a second way, from the definition's text and not from the reference's code: exact fractions for the two
    floors, a search for the largest g with g * g <= q instead of isqrt, a loop for the shift instead of bit_length."""
    B, T, _ = stats.shape
    out = np.zeros((B, T, 3, 2), np.int64)
    for b in range(B):
        pooled = np.zeros((T, 16), object)
        for t in range(T):
            for u in range(T):
                if abs(u - t) <= pool_t:
                    pooled[t] = pooled[t] + np.array([int(v) for v in stats[b, u]], object)
        for t in range(T):
            n = pooled[t, 0]
            for c in range(3):
                A, E, AA, EE = pooled[t, 1 + 4 * c:5 + 4 * c]
                if n < 1 or n < min_pixels:
                    out[b, t, c] = (ONE, 0)
                    continue
                g = ONE
                Vs, Ve = n * AA - A * A, n * EE - E * E
                if gain and Ve != 0:
                    k = 0
                    while max(Vs, Ve) >> k >= 1 << 38:
                        k += 1
                    vs, ve = Vs // 2 ** k, Ve // 2 ** k
                    if ve == 0:
                        g = 2 * ONE
                    else:
                        q = math.floor(Fraction(vs * 2 ** 24, ve))
                        lo, hi = 0, 1 << 32                                          # lo * lo <= q < hi * hi
                        while hi - lo > 1:
                            mid = (lo + hi) // 2
                            lo, hi = (mid, hi) if mid * mid <= q else (lo, mid)
                        g = sorted((ONE // 2, lo, 2 * ONE))[1]
                out[b, t, c] = (g, math.floor(Fraction(ONE * A - g * E + n // 2, n)))
    return out


def brute_affine(frames, coef):
    flat, k = frames.reshape(-1, *frames.shape[-3:]), coef.reshape(-1, 3, 2)
    out = np.zeros_like(flat)
    for f in range(flat.shape[0]):
        for idx in np.ndindex(*flat.shape[1:]):
            g, b = int(k[f, idx[2], 0]), int(k[f, idx[2], 1])
            out[(f,) + idx] = min(max((g * int(flat[(f,) + idx]) + b + ONE // 2) >> 12, 0), 255)
    return out.reshape(frames.shape)


def clips(B=2, T=3, H=5, W=7, seed=0):
    g = np.random.default_rng(seed)
    ref = g.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)
    edit = g.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)
    alpha = (g.random((B, T, H, W)) < 0.4).astype(np.uint8) * g.integers(1, 256, (B, T, H, W), dtype=np.uint8)
    return ref, edit, alpha


@pytest.mark.parametrize("with_alpha", [False, True])
@pytest.mark.parametrize("one_frame", [False, True])
def test_stats_equal_the_loop(with_alpha, one_frame):
    ref, edit, alpha = clips()
    if one_frame:
        ref, alpha = ref[:, :1], alpha[:, :1]
    a = alpha if with_alpha else None
    got = reference_color_stats(ref, edit, a)
    assert got.dtype == np.int64 and got.shape == (2, 3, 16)
    assert np.array_equal(got, brute_stats(ref, edit, a))
    assert not got[..., 13:].any()
    one = reference_color_stats(ref[1], edit[1], None if a is None else a[1])          # a sample of a batch is that sample alone
    assert np.array_equal(one, got[1])
    if one_frame:                                                                    # [H, W, 3] beside [T, H, W, 3]
        assert np.array_equal(reference_color_stats(ref[1, 0], edit[1], None if a is None else a[1, 0]), got[1])


def test_a_frame_with_nothing_counted():
    ref, edit, alpha = clips()
    alpha[0, 1] = 7
    got = reference_color_stats(ref, edit, alpha)
    assert not got[0, 1].any() and got[0, 0, 0] > 0
    coef = reference_color_coefficients(got, pool_t=0, min_pixels=0)
    assert coef[0, 1].tolist() == [[ONE, 0]] * 3


@pytest.mark.parametrize("pool_t", [0, 1, 2, 8])
@pytest.mark.parametrize("gain", [True, False])
def test_coefficients_equal_the_loop(pool_t, gain):
    ref, edit, alpha = clips(seed=1)
    stats = reference_color_stats(ref, edit, alpha)
    for min_pixels in (0, int(stats[0, 0, 0]), int(stats[..., 0].max()) + 1, 10 ** 6):
        got = reference_color_coefficients(stats, pool_t=pool_t, gain=gain, min_pixels=min_pixels)
        assert got.dtype == np.int32 and got.shape == (2, 3, 3, 2)
        assert np.array_equal(got, brute_coef(stats, pool_t, gain, min_pixels)), (pool_t, gain, min_pixels)
    if pool_t >= 2:                                                                  # one transform per sample, and the samples differ
        full = reference_color_coefficients(stats, pool_t=pool_t, gain=gain, min_pixels=0)
        assert (full[:, :1] == full).all() and not np.array_equal(full[0], full[1])


def test_affine_equals_the_loop():
    g = np.random.default_rng(2)
    frames = g.integers(0, 256, (2, 2, 4, 5, 3), dtype=np.uint8)
    coef = np.stack([g.integers(-3 * ONE, 3 * ONE, (2, 2, 3)), g.integers(-300 * ONE, 300 * ONE, (2, 2, 3))], -1)
    coef[0, 0] = [[2048, 0], [8192, -81920], [ONE, -255 * ONE]]
    got = reference_frames_affine(frames, coef)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), brute_affine(frames, coef))
    ident = np.broadcast_to(np.array([ONE, 0]), (2, 2, 3, 2))
    assert np.array_equal(reference_frames_affine(frames, ident).numpy(), frames)


@pytest.mark.parametrize("size", [(5, 7), (33, 130)])
def test_known_constructions_give_the_reference_back_exactly(size):
    g = np.random.default_rng(3)
    H, W = size
    u = g.integers(0, 118, (1, 2, H, W, 3), dtype=np.uint8)
    alpha = (g.random((1, 2, H, W)) < 0.7).astype(np.uint8) * 255
    alpha[0, 0, 0, :2] = 0                                                           # something is always counted
    alpha[0, 1, 0, :2] = 0
    for ref, edit, want in ((u, u + 20, (ONE, -20 * ONE)), (2 * u, u + 10, (2 * ONE, -20 * ONE))):
        coef = reference_color_coefficients(reference_color_stats(ref, edit, alpha), pool_t=0, min_pixels=1)
        assert (coef == np.array(want)).all(), coef
        assert np.array_equal(reference_color_match(edit, ref, alpha, pool_t=0, min_pixels=1).numpy(), ref)      # masked pixels too
    coef = reference_color_coefficients(reference_color_stats(u + 10, 2 * u, alpha), pool_t=0, min_pixels=1)
    assert (coef[..., 0] == ONE // 2).all()
    assert np.array_equal(reference_color_match(2 * u, u + 10, alpha, pool_t=0, min_pixels=1).numpy(), u + 10)


def test_sums_past_64_bits():
    """17 pooled frames of 3840 x 2160, half the pixels 255 and half 0 in ref, a quarter of that contrast in edit: n * AA needs 70
    bits, and the answer is known: the deviations are 127.5 and 31.875, gain 4 clamps to 2."""
    P = 3840 * 2160
    stats = np.zeros((1, 17, 16), np.int64)
    stats[..., 0] = P
    for c in range(3):
        stats[..., 1 + 4 * c] = P // 2 * 255
        stats[..., 2 + 4 * c] = P // 2 * 96 + P // 2 * 160
        stats[..., 3 + 4 * c] = P // 2 * 255 * 255
        stats[..., 4 + 4 * c] = P // 2 * 96 * 96 + P // 2 * 160 * 160
    assert (17 * P * int(stats[0, 0, 3]) * 17).bit_length() > 64
    coef = reference_color_coefficients(stats, pool_t=8)
    assert np.array_equal(coef, brute_coef(stats, 8, True, 1024))
    assert (coef[0, 8, :, 0] == 2 * ONE).all()
    stats[..., 2::4][..., :3] = P // 2 * 64 + P // 2 * 192                           # deviation 64: gain 127.5 / 64
    stats[..., 4::4][..., :3] = P // 2 * 64 * 64 + P // 2 * 192 * 192
    coef = reference_color_coefficients(stats, pool_t=8)
    assert np.array_equal(coef, brute_coef(stats, 8, True, 1024))
    assert (abs(coef[0, 8, :, 0] - ONE * 255 // 128) <= 1).all()                    # the shift to 38 bits costs at most the last place


def test_argument_errors():
    ref, edit, alpha = clips()
    for fn in (color_match, color_match_coefficients, reference_color_match):
        with pytest.raises(ValueError, match="pool_t"):
            fn(edit, ref, pool_t=9)
        with pytest.raises(ValueError, match="pool_t"):
            fn(edit, ref, pool_t=-1)
        with pytest.raises(ValueError, match="pool_t"):
            fn(edit, ref, pool_t=1.5)
        with pytest.raises(ValueError, match="min_pixels"):
            fn(edit, ref, min_pixels=-1)
        with pytest.raises(ValueError, match="gain"):
            fn(edit, ref, gain=2)
    for fn in (color_match, color_match_coefficients):
        with pytest.raises(ValueError, match="edit_u8"):
            fn(edit.astype(np.float32), ref)
        with pytest.raises(ValueError, match="edit_u8"):
            fn(edit[0, 0], ref[0, 0])
        with pytest.raises(ValueError, match="ref_u8"):
            fn(edit, ref[:, :2])
        with pytest.raises(ValueError, match="ref_u8"):
            fn(edit, ref.astype(np.int16))
        with pytest.raises(ValueError, match="ref_u8"):
            fn(edit, ref[0, 0])                                                      # [H, W, 3] beside a batch
        with pytest.raises(ValueError, match="alpha"):
            fn(edit, ref, alpha[:, :1])
        with pytest.raises(ValueError, match="alpha"):
            fn(edit, ref[:, :1], alpha)
        with pytest.raises(ValueError, match="alpha"):
            fn(edit, ref, alpha.astype(np.int32))
    with pytest.raises(ValueError, match="stats"):
        reference_color_coefficients(np.zeros((3, 15), np.int64))
    assert reference_color_coefficients(np.zeros((3, 16), np.int64)).shape == (3, 3, 2)
    with pytest.raises(ValueError, match="reference_frames_affine"):
        reference_frames_affine(edit, np.zeros((2, 2, 3, 2), np.int64))


class _NeverCalled:
    device = torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError(f"the pipeline touched .{name} before it checked `color_match`")


def test_pipeline_checks_the_switch_before_anything_runs():
    from videocof_amd import WanPipeline, WanPipelineOutput
    assert WanPipelineOutput(videos=None).color_match is None
    pipe = WanPipeline(transformer=_NeverCalled(), scheduler=_NeverCalled())
    frames = torch.zeros(9, 32, 48, 3, dtype=torch.uint8)
    mask = torch.zeros(9, 32, 48, dtype=torch.uint8)
    call = dict(height=32, width=48, source_frames=9)
    with pytest.raises(ValueError, match="color_match needs the uint8 source frames"):
        pipe(video=torch.zeros(1, 3, 9, 32, 48), output_type="uint8", color_match=True, **call)
    with pytest.raises(ValueError, match="color_match needs the uint8 source frames"):
        pipe(video=None, source_latents=torch.zeros(1, 16, 3, 4, 6), output_type="uint8", color_match=True, **call)
    for output_type in ("latent", "numpy"):
        with pytest.raises(ValueError, match="color_match .* needs output_type='uint8'"):
            pipe(video=frames, output_type=output_type, color_match=dict(pool_t=0), **call)
    with pytest.raises(ValueError, match="color_match with edit_region_vae_halo"):
        pipe(video=frames, output_type="uint8", color_match=True, edit_mask=mask, edit_region=True, edit_region_vae_halo=16, **call)
    with pytest.raises(ValueError, match="source_frames, height, width"):
        pipe(video=frames[:, :16], output_type="uint8", color_match=True, **call)
    for bad, match in ((dict(pool_t=9), "pool_t=9"), (dict(min_pixels=-1), "min_pixels"), (dict(gain=1), "gain"), (dict(pool=1), "unknown key"),
                       ("yes", "True, or a dict"), (1, "True, or a dict")):
        with pytest.raises(ValueError, match=match):
            pipe(video=frames, output_type="uint8", color_match=bad, **call)
