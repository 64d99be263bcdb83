"""Temporal context windows on the host: the plan, the option conversion and the torch / numpy restatements of the two device
passes (videocof_amd/windows.py).  No GPU."""
import numpy as np
import pytest
import torch

import videocof_amd
from videocof_amd import window_plan, window_latent_frames, reference_window_gather, reference_window_blend


def ulp1(x):
    return float(np.spacing(np.float32(x)))


def column_sums(plan):
    return plan.alpha.astype(np.float64).sum(axis=0)


def raw_weight(j, n, o):
    return min(j + 1, n - j, o + 1)


def test_plan_7_4_2_has_three_way_coverage():
    p = window_plan(7, 4, 2)
    assert p.starts == (0, 2, 3) and p.K == 3 and p.n == 4 and p.frames == 7
    assert p.alpha.shape == (3, 7) and p.alpha.dtype == np.float32
    assert p.covering(3) == (0, 1, 2)
    assert [raw_weight(3 - a, 4, 2) for a in p.starts] == [1, 2, 1]
    np.testing.assert_array_equal(p.alpha[:, 3], np.array([0.25, 0.5, 0.25], dtype=np.float32))
    assert np.all(np.abs(column_sums(p) - 1.0) <= ulp1(1.0))
    for f in (0, 1, 6):
        assert len(p.covering(f)) == 1 and p.alpha[p.covering(f)[0], f] == np.float32(1.0)
    # 0 where a window does not cover the frame
    for k, a in enumerate(p.starts):
        outside = np.ones(7, dtype=bool)
        outside[a:a + 4] = False
        assert np.all(p.alpha[k, outside] == 0) and np.all(p.alpha[k, ~outside] > 0)


def test_plan_81_21_4_is_five_windows():
    p = window_plan(81, 21, 4)           # 321 frames in windows of 81 with 16 frames of overlap
    assert p.K == 5 and p.starts == (0, 17, 34, 51, 60) and p.starts[-1] == 60
    assert np.all(np.abs(column_sums(p) - 1.0) <= ulp1(1.0))


@pytest.mark.parametrize("frames,window", [(1, 2), (4, 4), (3, 21), (21, 21)])
def test_a_clip_that_fits_is_one_window(frames, window):
    p = window_plan(frames, window, 1)
    assert p.K == 1 and p.starts == (0,) and p.window == frames
    np.testing.assert_array_equal(p.alpha, np.ones((1, frames), dtype=np.float32))


def test_no_overlap_averages_only_where_the_last_window_was_pulled_back():
    p = window_plan(10, 4, 0)            # starts 0, 4, 6: frames 6 and 7 are shared by the last two windows
    assert p.starts == (0, 4, 6)
    for f in range(10):
        cov = p.covering(f)
        if f in (6, 7):
            assert cov == (1, 2) and p.alpha[1, f] == p.alpha[2, f] == np.float32(0.5)
        else:
            assert len(cov) == 1 and p.alpha[cov[0], f] == np.float32(1.0)
    q = window_plan(12, 4, 0)            # the windows tile the clip: nothing is averaged
    assert q.starts == (0, 4, 8) and set(np.unique(q.alpha)) == {np.float32(0.0), np.float32(1.0)}


@pytest.mark.parametrize("args", [(7, 1, 0), (7, 4, 4), (7, 4, -1), (0, 4, 1), (7.0, 4, 1), (7, 4, True), (7, "4", 1)])
def test_bad_plan_arguments_raise(args):
    with pytest.raises(ValueError, match="window_plan"):
        window_plan(*args)


def test_sweep_of_every_small_plan():
    """All (Fs <= 24, n, o): every frame covered, equal lengths inside the clip, ascending starts, the stride never above n - o,
    weights the normalised ramp, every column 1 within 1 ulp, exactly 1 under single coverage."""
    count = 0
    for Fs in range(1, 25):
        for n in range(2, 25):
            for o in range(0, n):
                p = window_plan(Fs, n, o)
                count += 1
                if Fs <= n:
                    assert p.K == 1 and p.window == Fs
                    continue
                s = n - o
                assert p.K == -(-(Fs - n) // s) + 1 and p.window == n
                assert p.starts[0] == 0 and p.starts[-1] == Fs - n
                assert all(0 < b - a <= s for a, b in zip(p.starts, p.starts[1:]))
                assert all(b - a == s for a, b in zip(p.starts[:-2], p.starts[1:-1]))
                cover = np.zeros(Fs, dtype=int)
                for a in p.starts:
                    assert 0 <= a and a + n <= Fs
                    cover[a:a + n] += 1
                assert cover.min() >= 1
                assert np.all(np.abs(column_sums(p) - 1.0) <= ulp1(1.0))
                for f in range(Fs):
                    cov = p.covering(f)
                    raw = [raw_weight(f - p.starts[k], n, o) for k in cov]
                    want = (np.array(raw, dtype=np.float64) / sum(raw)).astype(np.float32)
                    np.testing.assert_array_equal(p.alpha[list(cov), f], want)
                    if len(cov) == 1:
                        assert p.alpha[cov[0], f] == np.float32(1.0)
                assert np.count_nonzero(p.alpha) == p.K * n
    assert count == 24 * sum(range(2, 25))


def test_pixel_options_convert_like_source_frames():
    assert window_latent_frames(81, 16) == (21, 4)
    assert window_latent_frames(13, 8) == (4, 2)
    assert window_latent_frames(81, 0) == (21, 0)
    assert window_latent_frames(5, 4) == (2, 1)
    assert window_latent_frames(17, 8, ratio=8) == (3, 1)
    for tw, to, ratio in ((81, 16, 4), (33, 12, 4), (49, 0, 4)):
        n, o = window_latent_frames(tw, to, ratio)
        assert n == (tw - 1) // ratio + 1 and o == (to - 1) // ratio + 1


@pytest.mark.parametrize("tw,to,name", [(80, 16, "temporal_window=80"), (1, 0, "temporal_window=1"), (0, 0, "temporal_window=0"),
                                        (81.0, 16, "temporal_window=81.0"), (81, 15, "temporal_overlap=15"),
                                        (81, -4, "temporal_overlap=-4"), (81, 84, "temporal_overlap=84"), (13, 16, "temporal_overlap=16"),
                                        (81, None, "temporal_overlap=None")])
def test_bad_pixel_options_raise_and_name_the_value(tw, to, name):
    with pytest.raises(ValueError, match=name):
        window_latent_frames(tw, to)


class _Stop(Exception):
    pass


def test_pipeline_checks_the_options_before_it_runs_anything():
    """WanPipeline.__call__ validates the window options up front (the transformer here is never called)."""
    class T:
        device = torch.device("cpu")
        config = type("C", (), {"patch_size": (1, 2, 2)})()

    pipe = videocof_amd.WanPipeline(transformer=T(), scheduler=videocof_amd.FlowUniPCMultistepScheduler(shift=1))
    emb = [torch.zeros(3, 8)]
    common = dict(prompt_embeds=emb, guidance_scale=1.0, num_inference_steps=2, output_type="latent", device="cpu")
    lat = torch.zeros(1, 16, 15, 4, 4)
    with pytest.raises(ValueError, match="temporal_window=12"):
        pipe(latents=lat, source_frames=25, cot=True, temporal_window=12, **common)
    with pytest.raises(ValueError, match="temporal_overlap=6"):
        pipe(latents=lat, source_frames=25, cot=True, temporal_window=13, temporal_overlap=6, **common)
    with pytest.raises(ValueError, match="window_batch=0"):
        pipe(latents=lat, source_frames=25, cot=True, temporal_window=13, temporal_overlap=8, window_batch=0, **common)
    with pytest.raises(ValueError, match="has none"):          # a T2V call: no source segment to cut windows from
        pipe(source_frames=25, cot=True, temporal_window=13, temporal_overlap=8, **common)
    with pytest.raises(ValueError, match=r"not \[source \| grounding \| target\]"):
        pipe(latents=lat[:, :, :14], source_frames=25, cot=True, temporal_window=13, temporal_overlap=8, **common)
    with pytest.raises(NotImplementedError, match="capture_graph='loop'"):
        pipe(latents=lat, source_frames=25, cot=True, temporal_window=13, temporal_overlap=8, capture_graph="loop", **common)
    with pytest.raises(TypeError, match="temporal_windows"):   # a misspelt switch is still an unexpected keyword
        pipe(latents=lat, source_frames=25, cot=True, temporal_windows=13, **common)


# ---------------------------------------------------------------- gather / blend restatements
def np_gather(state, starts, n, G, k0, k1, rep):
    K = len(starts)
    Fs = (state.shape[2] - K * G) // 2
    wins = [np.concatenate([state[:, :, a:a + n], state[:, :, Fs + k * G:Fs + (k + 1) * G],
                            state[:, :, Fs + K * G + a:Fs + K * G + a + n]], axis=2) for k, a in list(enumerate(starts))[k0:k1]]
    return np.concatenate(wins * rep)


def np_blend(pred, plan, G, dtype=np.float32):
    """The blend with every product and sum in `dtype` (float32: the kernel's definition; float64: the yardstick)."""
    K, n, Fs = plan.K, plan.window, plan.frames
    B = pred.shape[0] // K
    p = pred.reshape(K, B, *pred.shape[1:]).astype(dtype)
    out = np.zeros((B, pred.shape[1], 2 * Fs + K * G) + pred.shape[3:], dtype=dtype)
    for k in range(K):
        out[:, :, Fs + k * G:Fs + (k + 1) * G] = p[k][:, :, n:n + G]
    for f in range(Fs):
        acc = None
        for k in plan.covering(f):
            term = plan.alpha[k, f].astype(dtype) * p[k][:, :, n + G + f - plan.starts[k]]
            acc = term if acc is None else acc + term
        out[:, :, Fs + K * G + f] = acc
    return out


@pytest.mark.parametrize("Fs,n,o,G,B", [(7, 4, 2, 1, 2), (7, 4, 2, 0, 1), (10, 4, 0, 2, 1), (9, 5, 3, 1, 1)])
def test_gather_and_blend_restatements_agree(Fs, n, o, G, B):
    plan = window_plan(Fs, n, o)
    K = plan.K
    rng = np.random.default_rng(Fs * 100 + n * 10 + o)
    state = rng.standard_normal((B, 3, 2 * Fs + K * G, 2, 3)).astype(np.float32)
    for k0, k1, rep in ((0, K, 1), (0, K, 2), (1, K, 1), (K - 1, K, 2)):
        got = reference_window_gather(torch.from_numpy(state), plan, n, G, k0, k1, rep).numpy()
        want = np_gather(state, plan.starts, n, G, k0, k1, rep)
        assert got.shape == (rep * (k1 - k0) * B, 3, 2 * n + G, 2, 3)
        np.testing.assert_array_equal(got, want)
    # window k, sample b of the batch is [source[a:a+n] | ground_k | target[a:a+n]] of sample b
    full = reference_window_gather(torch.from_numpy(state), plan, n, G).numpy()
    for k, a in enumerate(plan.starts):
        for b in range(B):
            w = full[k * B + b]
            np.testing.assert_array_equal(w[:, :n], state[b, :, a:a + n])
            np.testing.assert_array_equal(w[:, n:n + G], state[b, :, Fs + k * G:Fs + (k + 1) * G])
            np.testing.assert_array_equal(w[:, n + G:], state[b, :, Fs + K * G + a:Fs + K * G + a + n])

    pred = rng.standard_normal((K * B, 3, 2 * n + G, 2, 3)).astype(np.float32)
    t32 = reference_window_blend(torch.from_numpy(pred), plan, G).numpy()
    np.testing.assert_array_equal(t32, np_blend(pred, plan, G, np.float32))          # torch float32 == numpy float32, bit for bit
    f64 = np_blend(pred, plan, G, np.float64)
    # float32 against float64: alpha carries half an ulp, every product and every sum half an ulp of a partial result that never
    # exceeds sum_k alpha_k |p_k| = S; with at most M covering windows that is (M products + (M - 1) sums + 1 for alpha) half-ulps of S
    p = pred.reshape(K, B, *pred.shape[1:])
    for f in range(Fs):
        cov = plan.covering(f)
        S = sum(float(plan.alpha[k, f]) * np.abs(p[k][:, :, n + G + f - plan.starts[k]].astype(np.float64)) for k in cov)
        bound = 2 * len(cov) * 2.0 ** -24 * S * (1 + 2.0 ** -20)
        err = np.abs(t32[:, :, Fs + K * G + f].astype(np.float64) - f64[:, :, Fs + K * G + f])
        assert np.all(err <= bound), (f, float(err.max()), float(bound.min()))
        if len(cov) == 1:                    # single coverage: the window's prediction unchanged
            np.testing.assert_array_equal(t32[:, :, Fs + K * G + f], p[cov[0]][:, :, n + G + f - plan.starts[cov[0]]])
    assert not t32[:, :, :Fs].any()                                                 # the CoF mask
    for k in range(K):
        np.testing.assert_array_equal(t32[:, :, Fs + k * G:Fs + (k + 1) * G], p[k][:, :, n:n + G])
    # bf16 in, bf16 out: the float32 sum rounded once
    pb = torch.from_numpy(pred).bfloat16()
    tb = reference_window_blend(pb, plan, G)
    assert tb.dtype == torch.bfloat16
    want = torch.from_numpy(np_blend(pb.float().numpy(), plan, G, np.float32)).bfloat16()
    assert torch.equal(tb, want)
