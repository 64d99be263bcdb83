"""-m gpu: colour match on the device -- wan_color_stats, wan_color_coef and wan_frames_u8_affine (behind ops.color_stats /
color_coef / frames_u8_affine, video_io.color_match / color_match_coefficients and WanPipeline(color_match=...)) against the
definitions in numpy and Python ints that tests/test_color_match_host.py checks.  EQUALITY of every word and byte: both sides are
integer arithmetic, and the kernels use no floating point at all.

Every operand is the interior of a ``kernel_bounds.Guarded`` buffer whose surroundings are poisoned and checked after every call,
at bases misaligned by 0, 1 and 3 bytes.  The sums kernel walks a frame in runs of 16 pixels and tiles of 4096, the transform in
runs of 48 bytes and tiles of 12288: 5 x 7 is one partial run, 33 x 130 one partial tile (two of the transform's), 264 x 256 more
tiles than one and the size from which the variances need the 38-bit shift."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import kernel_bounds as KB  # noqa: E402
from videocof_amd import (AutoencoderKLWan, FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel, color_match,  # noqa: E402
                          color_match_coefficients, ops, reference_color_coefficients, reference_color_match, reference_color_stats,
                          reference_compare_frames, reference_frames_affine)
from videocof_amd.weights import deterministic_dit_state_dict, deterministic_vae_state_dict, det_uniform  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ONE = 4096
SIZES = [(5, 7), (33, 130), (264, 256)]
B, T = 2, 3


def guarded(shape, dtype, off=0, fill=None):
    """A contiguous tensor of `shape` inside a poisoned buffer, its base `off` bytes past a 16-byte boundary (int64 as pairs of
    int32, which is as far as Guarded's element sizes go) -> (the Guarded, the tensor)."""
    n = int(np.prod(shape)) * (2 if dtype == torch.int64 else 1)
    held = torch.int32 if dtype == torch.int64 else dtype
    assert off == 0 or held == torch.uint8
    g = KB.Guarded((1, n), held, ld=(n + off + 64 + 15) // 16 * 16, rows_before=1, rows_after=1, cols_before=off, device=DEV)
    t = g.view[0]
    t = (t.view(torch.int64) if dtype == torch.int64 else t).view(shape)
    assert t.data_ptr() % 16 == off * t.element_size() and t.is_contiguous()
    if fill is not None:
        t.copy_(torch.as_tensor(fill))
    return g, t


@functools.lru_cache(maxsize=None)
def case(size):
    """ref, edit, alpha (frame [1, 1] with every alpha non-zero), and the definition's sums with and without alpha, for T and one
    ref frame per sample: computed once, shared, never written."""
    H, W = size
    g = np.random.default_rng(H * 1000 + W)
    ref = g.integers(0, 256, (B, T, H, W, 3), dtype=np.uint8)
    edit = np.clip(ref.astype(np.int64) * g.integers(60, 140, (B, T, 1, 1, 3)) // 100 + g.integers(-30, 30, (B, T, 1, 1, 3))
                   + g.integers(-3, 4, ref.shape), 0, 255).astype(np.uint8)
    alpha = (g.random((B, T, H, W)) < 0.5).astype(np.uint8) * g.integers(1, 256, (B, T, H, W), dtype=np.uint8)
    alpha[1, 1] = g.integers(1, 256, (H, W), dtype=np.uint8)
    stats = {(full, masked): reference_color_stats(ref if full else ref[:, :1], edit, (alpha if full else alpha[:, :1]) if masked else None)
             for full in (True, False) for masked in (True, False)}
    assert not stats[True, True][1, 1].any() and stats[True, True][0, 0, 0] > 0
    return ref, edit, alpha, stats


def run_stats(ref, edit, alpha, off):
    gs = [guarded(x.shape, torch.uint8, off, x) if x is not None else (None, None) for x in (ref, edit, alpha)]
    go, out = guarded((edit.shape[0], edit.shape[1], 16), torch.int64)
    out.fill_(-0x0123456789abcdef)                                                   # every word is overwritten
    res = ops.color_stats(gs[0][1], gs[1][1], gs[2][1], out=out)
    assert res.data_ptr() == out.data_ptr()
    for g, _ in gs + [(go, out)]:
        if g is not None:
            g.check()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the sums
@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_stats_equal_the_definition(size, off):
    ref, edit, alpha, stats = case(size)
    for full in (True, False):                                                       # a ref frame per edit frame; one per sample
        for masked in (False, True):
            got = run_stats(ref if full else ref[:, :1], edit, ((alpha if full else alpha[:, :1]) if masked else None), off)
            want = stats[full, masked]
            bad = int((got != want).sum())
            print(f"color_stats {size} off={off} ref_T={T if full else 1} alpha={masked}: {bad} differing words; n = {want[..., 0].ravel().tolist()}")
            assert bad == 0 and got.shape == (B, T, 16)
    assert stats[True, True][1, 1, 0] == 0                                           # the frame with nothing counted


def test_sums_of_squares_past_32_bits():
    x = np.full((1, 1, 264, 256, 3), 255, np.uint8)
    got = run_stats(x, x, None, 1)
    n = 264 * 256
    assert n * 255 * 255 > 2 ** 32
    assert got[0, 0].tolist() == [n] + [n * 255, n * 255, n * 255 * 255, n * 255 * 255] * 3 + [0, 0, 0]


# ------------------------------------------------------------------------------------------------ the coefficients
def run_coef(stats, pool_t, gain, min_pixels):
    gs, s = guarded(stats.shape, torch.int64, fill=stats)
    go, out = guarded(stats.shape[:2] + (3, 2), torch.int32)
    out.fill_(0x5a5a5a5a)
    res = ops.color_coef(s, pool_t, gain, min_pixels, out=out)
    assert res.data_ptr() == out.data_ptr()
    gs.check(), go.check()
    return out.cpu().numpy()


def check_coef(stats, what, pools=(0, 1, 2, 8), gains=(True, False), mins=(0, 1024)):
    seen = set()
    for pool_t in pools:
        for gain in gains:
            for min_pixels in mins:
                want = reference_color_coefficients(stats, pool_t=pool_t, gain=gain, min_pixels=min_pixels)
                got = run_coef(stats, pool_t, gain, min_pixels)
                assert got.dtype == np.int32 and np.array_equal(got, want), (what, pool_t, gain, min_pixels, got.tolist(), want.tolist())
                seen.update(want[..., 0].ravel().tolist())
    return seen


@pytest.mark.parametrize("size", SIZES)
def test_coefficients_of_the_stats_above(size):
    _, _, _, stats = case(size)
    for key, s in stats.items():
        gains = check_coef(s, (size, key), mins=(0, int(s[0, 0, 0]), int(s[0, 0, 0]) + 1))
        assert len(gains) > 3                                                        # real gains, not the fall-backs only
    s = stats[True, True]
    if size == (264, 256):                                                           # the 38-bit shift is taken
        assert (int(s[0, 0, 0]) * int(s[0, 0, 3]) - int(s[0, 0, 1]) ** 2).bit_length() > 38
    # pooling stays inside the sample: frame [1, 1] counts nothing, pool_t = 1 gives it frames [1, 0] and [1, 2], never [0, 2]
    alone = reference_color_coefficients(s[1:], pool_t=1, min_pixels=0)
    assert np.array_equal(run_coef(s, 1, True, 0)[1], alone[0])


def _two_level(n, lo, hi):
    """The sums of n pixels, half at `lo` and half at `hi`: (sum, sum of squares)."""
    return n // 2 * (lo + hi), n // 2 * (lo * lo + hi * hi)


def hand_made(n, ref, edit, frames=1):
    s = np.zeros((1, frames, 16), np.int64)
    s[..., 0] = n
    for c in range(3):
        s[..., 1 + 4 * c], s[..., 3 + 4 * c] = ref
        s[..., 2 + 4 * c], s[..., 4 + 4 * c] = edit
    return s


def test_coefficients_of_hand_made_stats():
    P = 3840 * 2160
    # 17 pooled frames of 3840 x 2160, half the pixels 255 and half 0: n AA needs 70 bits
    big = hand_made(P, _two_level(P, 0, 255), _two_level(P, 64, 192), frames=17)
    assert (17 * P * 17 * int(big[0, 0, 3])).bit_length() > 64
    seen = check_coef(big, "4K x 17", pools=(0, 8), mins=(1024,))
    assert ONE * 255 // 128 in {g - 1 for g in seen} | seen | {g + 1 for g in seen}
    # Ve == 0: a flat edit
    flat = hand_made(5000, _two_level(5000, 10, 200), (5000 * 77, 5000 * 77 * 77))
    assert check_coef(flat, "Ve == 0", pools=(0,)) == {ONE}
    # ve == 0 after the shift: Vs of 66 bits, Ve = n - 1 of 26
    n = 1 << 26
    tiny = hand_made(n, _two_level(n, 0, 255), (100 * n + 1, 10000 * n + 201))
    assert n * (10000 * n + 201) - (100 * n + 1) ** 2 == n - 1
    assert check_coef(tiny, "ve == 0", pools=(0,), gains=(True,), mins=(1,)) == {2 * ONE}
    # n just below and at min_pixels
    edge = np.concatenate([hand_made(m, _two_level(m - m % 2, 20, 120), _two_level(m - m % 2, 40, 90)) for m in (1023, 1024)], 0)
    got = run_coef(edge, 0, True, 1024)
    assert got[0, 0].tolist() == [[ONE, 0]] * 3 and got[1, 0, 0, 0] == 2 * ONE and got[1, 0, 0, 1] != 0
    check_coef(edge, "n at min_pixels", pools=(0,), mins=(1023, 1024, 1025))
    # gains on both clamps, and just inside them
    for ref, edit, g in (((0, 200), (50, 90), 2 * ONE), ((50, 90), (0, 200), ONE // 2), ((0, 198), (0, 100), None), ((0, 100), (0, 198), None)):
        seen = check_coef(hand_made(4096, _two_level(4096, *ref), _two_level(4096, *edit)), (ref, edit), pools=(0,), gains=(True,), mins=(1,))
        assert seen == {g} if g else ONE // 2 < min(seen) and max(seen) < 2 * ONE, seen


# ------------------------------------------------------------------------------------------------ the transform
FIXED = [(2048, 0), (8192, -81920), (4096, -1044480), (4096, 1044480)]


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("size", [(5, 7), (17, 19), (33, 130)])
def test_transform_equals_the_definition(size, off):
    H, W = size
    g = np.random.default_rng(H + off)
    N = len(FIXED) + 4
    frames = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    if H * W >= 256:
        frames.reshape(N, H * W, 3)[:, :256] = np.arange(256, dtype=np.uint8)[None, :, None]      # every byte value in every channel
    else:
        frames.reshape(N, -1)[:, :105] = np.arange(N * 105, dtype=np.int64).reshape(N, 105) * 37 % 256
    coef = np.zeros((N, 3, 2), np.int32)
    coef[:len(FIXED)] = np.array(FIXED)[:, None]
    coef[len(FIXED):len(FIXED) + 2] = np.stack([g.integers(0, 3 * ONE, (2, 3)), g.integers(-300 * ONE, 300 * ONE, (2, 3))], -1)
    coef[len(FIXED) + 2:] = np.stack([g.integers(-2 ** 21, 2 ** 21 + 1, (2, 3)), g.integers(-2 ** 30, 2 ** 30 + 1, (2, 3))], -1)
    want = reference_frames_affine(frames, coef)
    assert len(np.unique(want.numpy()[:len(FIXED) + 2])) > 100
    gc, k = guarded(coef.shape, torch.int32, fill=coef)
    gf, f = guarded(frames.shape, torch.uint8, off, frames)
    go, out = guarded(frames.shape, torch.uint8, off)
    res = ops.frames_u8_affine(f, k, out=out)                                        # out of place
    assert res.data_ptr() == out.data_ptr()
    for x in (gc, gf, go):
        x.check()
    differ = out.cpu() != want
    bad = int(differ.sum())
    print(f"frames_u8_affine {size} off={off}: {bad} differing bytes out of place, per frame {differ.sum((1, 2, 3)).tolist()}")
    assert bad == 0 and torch.equal(f.cpu(), torch.from_numpy(frames))
    ops.frames_u8_affine(f, k, out=f)                                                # in place
    gc.check(), gf.check()
    assert torch.equal(f.cpu(), want)
    assert torch.equal(ops.frames_u8_affine(out, k).cpu(), reference_frames_affine(want, coef))     # a fresh output


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("size", SIZES)
def test_known_shifts_are_undone_exactly(size):
    H, W = size
    g = np.random.default_rng(W)
    u = g.integers(0, 118, (B, T, H, W, 3), dtype=np.uint8)
    alpha = (g.random((B, T, H, W)) < 0.7).astype(np.uint8) * 255
    alpha[:, :, 0, :3] = 0                                                           # something is always counted
    da = torch.from_numpy(alpha).to(DEV)
    for name, ref, edit, want in (("offset", u, u + 20, (ONE, -20 * ONE)), ("gain 2", 2 * u, u + 10, (2 * ONE, -20 * ONE)),
                                  ("gain 1/2", u + 10, 2 * u, (ONE // 2, None))):
        dr, de = torch.from_numpy(ref).to(DEV), torch.from_numpy(edit).to(DEV)
        coef = color_match_coefficients(de, dr, da, min_pixels=1)
        assert coef.is_cuda and coef.dtype == torch.int32 and tuple(coef.shape) == (B, T, 3, 2)
        assert bool((coef[..., 0] == want[0]).all()) and (want[1] is None or bool((coef[..., 1] == want[1]).all())), (name, coef.cpu())
        out = color_match(de, dr, da, min_pixels=1)
        bad = int((out.cpu() != torch.from_numpy(ref)).sum())
        print(f"color_match {size} {name}: {bad} bytes differ from ref, masked pixels included")
        assert bad == 0
        assert torch.equal(out.cpu(), reference_color_match(edit, ref, alpha, min_pixels=1))
        garbage = np.where(alpha[..., None] != 0, g.integers(0, 256, edit.shape, dtype=np.uint8), edit)
        assert torch.equal(color_match_coefficients(torch.from_numpy(garbage).to(DEV), dr, da, min_pixels=1), coef)
        kept = torch.from_numpy(alpha == 0)
        assert torch.equal(color_match(garbage, ref, alpha, min_pixels=1).cpu()[kept], torch.from_numpy(ref)[kept])


def test_shapes_host_inputs_and_out():
    ref, edit, alpha, _ = case((33, 130))
    want = reference_color_match(edit, ref, alpha)
    assert torch.equal(color_match(edit, ref, alpha).cpu(), want)                    # numpy on the host
    assert torch.equal(color_match(torch.from_numpy(edit[1]), ref[1], alpha[1]).cpu(), want[1])
    one = reference_color_match(edit, ref[:, :1], alpha[:, :1], pool_t=0, gain=False, min_pixels=0)
    assert torch.equal(color_match(edit, ref[:, :1], alpha[:, :1], pool_t=0, gain=False, min_pixels=0).cpu(), one)
    assert torch.equal(color_match(edit[1], ref[1, 0], alpha[1, 0], pool_t=0, gain=False, min_pixels=0).cpu(), one[1])
    frame0 = color_match(edit[0], edit[0, :1], pool_t=8)                             # the reference's rule: every frame towards frame 0
    assert torch.equal(frame0.cpu(), reference_color_match(edit[0], edit[0, 0], pool_t=8))
    pinned = torch.empty(edit.shape, dtype=torch.uint8, pin_memory=True)
    got = color_match(edit, ref, alpha, out=pinned)
    assert got is pinned and torch.equal(pinned, want)
    with pytest.raises(ValueError, match="out"):
        color_match(edit, ref, alpha, out=torch.empty(edit.shape[1:], dtype=torch.uint8))
    with pytest.raises(ValueError, match="out"):
        ops.color_stats(torch.from_numpy(ref).to(DEV), torch.from_numpy(edit).to(DEV), None,
                        out=torch.empty(B, T, 15, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="pool_t"):
        ops.color_coef(torch.zeros(1, 1, 16, dtype=torch.int64, device=DEV), 9, True, 0)


def test_a_frame_range_of_a_longer_clip_is_matched_in_place():
    """What the pipeline does with a batch under cot=True: the edit segment is frames [1, 4) of a longer device clip, so the batch is not
    contiguous and the samples go one by one; one source / mask for both samples is paired with each.  The frames beside the range
    stay as they are."""
    from videocof_amd.video_io import _color_match_segment
    ref, edit, alpha, _ = case((33, 130))
    args = (1, True, 64)
    clip = torch.empty(B, T + 2, 33, 130, 3, dtype=torch.uint8, device=DEV)
    seg = clip[:, 1:1 + T]
    assert not seg.is_contiguous()
    for src, mask in ((ref, alpha), (ref[0], alpha[0]), (ref[1], None)):
        clip.fill_(0xA5)
        seg.copy_(torch.from_numpy(edit))
        coef = _color_match_segment(seg, torch.from_numpy(src), None if mask is None else torch.from_numpy(mask).to(DEV), args)
        r5 = src if src.ndim == 5 else np.ascontiguousarray(np.broadcast_to(src, ref.shape))
        a4 = None if mask is None else mask if mask.ndim == 4 else np.ascontiguousarray(np.broadcast_to(mask, alpha.shape))
        want = reference_color_match(edit, r5, a4, pool_t=1, gain=True, min_pixels=64)
        assert torch.equal(seg.cpu(), want)
        assert torch.equal(coef.cpu(), torch.from_numpy(reference_color_coefficients(reference_color_stats(r5, edit, a4), pool_t=1, min_pixels=64)))
        assert bool((clip[:, 0] == 0xA5).all()) and bool((clip[:, -1] == 0xA5).all())
    whole = torch.from_numpy(edit).to(DEV)                                            # contiguous: one call for the batch
    coef = _color_match_segment(whole, torch.from_numpy(ref).to(DEV), torch.from_numpy(alpha).to(DEV), args)
    assert torch.equal(whole.cpu(), reference_color_match(edit, ref, alpha, pool_t=1, gain=True, min_pixels=64))
    assert torch.equal(coef, color_match_coefficients(edit, ref, alpha, pool_t=1, min_pixels=64))


# ------------------------------------------------------------------------------------------------ the pipeline
TINY = dict(dim=256, ffn_dim=512, num_layers=1, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)


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
    kw.setdefault("output_type", "uint8")
    return pipe(video=video, prompt_embeds=ctx, height=32, width=48, source_frames=9, reasoning_frames=4, num_inference_steps=2,
                guidance_scale=1.0, shift=3, repeat_rope=True, cot=cot, generator=gen, weight_dtype=torch.bfloat16,
                return_dict=True, **kw)


FRAMES = torch.randint(0, 256, (9, 32, 48, 3), generator=torch.Generator().manual_seed(51), dtype=torch.uint8)
MASK = torch.zeros(9, 32, 48, dtype=torch.uint8)
MASK[2:7, 8:24, 16:40] = 255


@pytest.mark.parametrize("cot", [True, False])
@pytest.mark.parametrize("masked", [False, True])
def test_pipeline_color_match(pipe, cot, masked):
    kw = dict(edit_mask=MASK) if masked else {}
    args = dict(pool_t=1, gain=True, min_pixels=64)
    plain = run(pipe, FRAMES, cot, **kw)
    off = run(pipe, FRAMES, cot, color_match=False, **kw)
    assert plain.color_match is None and off.color_match is None
    assert torch.equal(plain.latents, off.latents) and np.array_equal(plain.videos, off.videos)
    for switch, by_hand in ((True, {}), (args, args)):
        got = run(pipe, FRAMES, cot, color_match=switch, compare=True, **kw)
        assert torch.equal(got.latents, plain.latents)
        edit = torch.from_numpy(plain.edit_videos)
        alpha = MASK[None] if masked else None
        want = color_match(edit, FRAMES[None], alpha, **by_hand).cpu()
        bad = int((torch.from_numpy(got.edit_videos) != want).sum())
        print(f"pipeline color_match cot={cot} masked={masked} {switch}: {bad} differing bytes; moved {int((want != edit).sum())} of {edit.numel()}")
        assert bad == 0 and torch.equal(want, reference_color_match(edit, FRAMES[None], alpha, **by_hand))
        coef = got.color_match
        assert coef.is_cuda and coef.dtype == torch.int32 and tuple(coef.shape) == (1, 9, 3, 2)
        assert torch.equal(coef, color_match_coefficients(edit, FRAMES[None], alpha, **by_hand))
        assert bool((coef.cpu() != torch.tensor([ONE, 0])).any())                    # something was estimated
        if cot:
            assert np.array_equal(got.ground_videos, plain.ground_videos) and np.shares_memory(got.videos, got.edit_videos)
            assert np.array_equal(got.videos[:, -9:], got.edit_videos)
        else:
            assert np.array_equal(got.videos, got.edit_videos)
        assert np.array_equal(got.compare_videos, reference_compare_frames(FRAMES[None], want).numpy())     # composed from the matched frames


def test_pipeline_refusals(pipe):
    for bad, match in ((dict(output_type="numpy"), "output_type='uint8'"), (dict(output_type="latent"), "output_type='uint8'"),
                       (dict(color_match=dict(pool=1)), "unknown key"), (dict(color_match=dict(pool_t=9)), "pool_t"),
                       (dict(color_match="yes"), "True, or a dict"),
                       (dict(edit_mask=MASK, edit_region=True, edit_region_vae_halo=16), "color_match with edit_region_vae_halo")):
        with pytest.raises(ValueError, match=match):
            run(pipe, FRAMES, False, **{"color_match": True, **bad})
    with pytest.raises(ValueError, match="needs the uint8 source frames"):
        run(pipe, torch.zeros(1, 3, 9, 32, 48), False, color_match=True)
    with pytest.raises(ValueError, match="source_frames, height, width"):
        run(pipe, FRAMES[:5], False, color_match=True)


def test_without_the_switch_the_bytes_are_the_parent_commits(pipe):
    """tests/golden/color_match_parent.json: sha256 of `videos` and the latents of the four calls above without the switch, recorded
    from the parent commit's tree and library on an MI355X (and equal, on the same box, to this tree's)."""
    import hashlib
    import json
    with open(os.path.join(HERE, "golden", "color_match_parent.json")) as f:
        golden = json.load(f)["sha256"]
    for cot in (True, False):
        for masked in (False, True):
            r = run(pipe, FRAMES, cot, **(dict(edit_mask=MASK) if masked else {}))
            h = hashlib.sha256()
            h.update(r.videos.tobytes())
            h.update(r.latents.float().cpu().numpy().tobytes())
            assert r.color_match is None and h.hexdigest() == golden[f"cot={cot},masked={masked}"], (cot, masked)
