"""Spatial context windows, host side (no GPU): TilePlan's indexing and weights, the partition of unity of the float32 weights,
spatial_window_cells, and the torch restatements of wan_tile_gather / wan_tile_blend against a slow per-element float64 loop.
Bounds and observed values: docs/TEST_BOUNDS.md, "Spatial context windows"."""
import numpy as np
import pytest
import torch

from videocof_amd import (TilePlan, reference_tile_blend, reference_tile_gather, reference_window_blend, reference_window_gather,
                          spatial_window_cells, window_plan)
from videocof_amd.weights import det_uniform


def _plan(t, y, x):
    return TilePlan(window_plan(*t), window_plan(*y), window_plan(*x))


SMALL = ((7, 4, 2), (6, 4, 2), (7, 4, 2))
TRIPLES = [SMALL, ((21, 21, 4), (135, 60, 12), (240, 104, 16)), ((81, 21, 4), (90, 60, 12), (160, 104, 16))]


# ------------------------------------------------------------------------------------------------ (a)
def test_a_indexing_and_shape():
    p = _plan(*SMALL)
    assert (p.Kt, p.Ky, p.Kx, p.K) == (3, 2, 3, 18)
    assert p.shape == (4, 4, 4) and p.extent == (7, 6, 7)
    assert p.t.starts == (0, 2, 3) and p.y.starts == (0, 2) and p.x.starts == (0, 2, 3)
    seen = []
    for kt in range(p.Kt):
        for ky in range(p.Ky):
            for kx in range(p.Kx):
                k = p.index(kt, ky, kx)
                assert k == (kt * p.Ky + ky) * p.Kx + kx and p.split(k) == (kt, ky, kx)
                assert p.origin(k) == (p.t.starts[kt], p.y.starts[ky], p.x.starts[kx])
                seen.append(k)
    assert seen == list(range(p.K))
    with pytest.raises(IndexError):
        p.split(p.K)
    assert p.covering(3, 2, 3) == tuple(range(18))                       # the middle of the clip: every tile
    assert p.covering(0, 0, 0) == (0,) and p.covering(6, 5, 6) == (17,)
    # 1080 rows are 135 latent rows: no multiple of the patch, and tiled all the same
    assert window_plan(135, 60, 12).starts == (0, 48, 75)
    # an axis whose extent fits its window: one window of the whole extent
    q = _plan((21, 21, 4), (60, 60, 12), (240, 104, 16))
    assert (q.Kt, q.Ky, q.Kx) == (1, 1, 3) and q.shape == (21, 60, 104)


def test_a_one_tile_per_spatial_axis_has_the_temporal_weights():
    p = _plan((7, 4, 2), (6, 6, 2), (7, 8, 2))
    assert (p.Ky, p.Kx, p.K) == (1, 1, 3)
    for k in range(p.K):
        w = p.weights(k)
        assert w.dtype == np.float32 and w.shape == (7, 6, 7)
        assert np.array_equal(w, np.broadcast_to(p.t.alpha[k][:, None, None], w.shape))          # bit for bit
        assert np.array_equal(p.weights(k, ground=True), np.ones((6, 7), np.float32))


@pytest.mark.parametrize("triple", TRIPLES)
def test_a_a_lone_tile_has_weight_one(triple):
    p = _plan(*triple)
    count = sum((p.weights(k) != 0).astype(np.int32) for k in range(p.K))
    assert count.min() >= 1
    for k in range(p.K):
        w = p.weights(k)
        a, y0, x0 = p.origin(k)
        n, th, tw = p.shape
        inside = np.zeros(w.shape, bool)
        inside[a:a + n, y0:y0 + th, x0:x0 + tw] = True
        assert not w[~inside].any() and (w[inside] > 0).all()
        assert (w[inside & (count == 1)] == np.float32(1.0)).all()


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("triple", TRIPLES)
def test_b_partition_of_unity(triple):
    """The float64 sum of the float32 weights over the covering tiles is within 5 * 2^-24 of 1: three roundings of the axis weights
    (each at most 2^-24 relative: 2^-25 for a value below 1, doubled for slack at the binade's edge) and two of the products."""
    p = _plan(*triple)
    total = sum(p.weights(k).astype(np.float64) for k in range(p.K))
    ground = [sum(p.weights(p.index(kt, ky, kx), ground=True).astype(np.float64) for ky in range(p.Ky) for kx in range(p.Kx))
              for kt in range(p.Kt)]
    worst = max(float(np.abs(total - 1).max()), max(float(np.abs(g - 1).max()) for g in ground))
    print(f"partition of unity {triple}: K = {p.K}, worst |sum - 1| = {worst:.3e}")
    assert worst <= 5 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ (c)
def test_c_spatial_window_cells():
    assert spatial_window_cells((480, 832), (96, 128)) == ((60, 104), (12, 16))
    assert spatial_window_cells((16, 16), (0, 8)) == ((2, 2), (0, 1))
    assert spatial_window_cells([32, 48], (24, 40)) == ((4, 6), (3, 5))                       # the largest overlap: n - 1 cells
    assert spatial_window_cells((np.int64(32), 32), (16, np.int32(16))) == ((4, 4), (2, 2))
    assert spatial_window_cells((64, 64), (16, 16), ratio=16, patch=1) == ((4, 4), (1, 1))
    for bad in (480, (480,), (480, 832, 3), "ab", None, (480.0, 832), (True, 832)):
        with pytest.raises(ValueError, match="spatial_window"):
            spatial_window_cells(bad, (96, 128))
    for bad in ((0, 832), (8, 832), (480, 840), (488, 832), (-16, 832)):
        with pytest.raises(ValueError, match="spatial_window="):
            spatial_window_cells(bad, (96, 128))
    for bad in (96, (96,), (96.0, 128), (False, 128)):
        with pytest.raises(ValueError, match="spatial_overlap"):
            spatial_window_cells((480, 832), bad)
    for bad in ((-8, 128), (96, 100), (4, 128), (480, 128), (96, 832)):
        with pytest.raises(ValueError, match="spatial_overlap="):
            spatial_window_cells((480, 832), bad)
    with pytest.raises(ValueError, match="no stride"):
        spatial_window_cells((32, 32), (32, 16))


# ------------------------------------------------------------------------------------------------ (d)
G, B, C = 1, 2, 2


def _slow_gather(state, p, k0, k1, rep):
    (n, th, tw), (Fs, _, _) = p.shape, p.extent
    out = torch.empty(rep * (k1 - k0) * B, C, 2 * n + G, th, tw, dtype=state.dtype)
    for r in range(rep):
        for k in range(k0, k1):
            kt = p.split(k)[0]
            a, y0, x0 = p.origin(k)
            for wf in range(2 * n + G):
                F = a + wf if wf < n else Fs + kt * G + wf - n if wf < n + G else Fs + p.Kt * G + a + wf - n - G
                for b in range(B):
                    for c in range(C):
                        for y in range(th):
                            for x in range(tw):
                                out[(r * (k1 - k0) + k - k0) * B + b, c, wf, y, x] = state[b, c, F, y0 + y, x0 + x]
    return out


def _slow_blend(pred, p):
    """float64 throughout: the exact weighted sum of the float32 weights and predictions."""
    (n, th, tw), (Fs, H, W), Kt = p.shape, p.extent, p.Kt
    w = [p.weights(k).astype(np.float64) for k in range(p.K)]
    wg = [p.weights(k, ground=True).astype(np.float64) for k in range(p.K)]
    x = pred.double().reshape(p.K, B, C, 2 * n + G, th, tw)
    out = torch.zeros(B, C, 2 * Fs + Kt * G, H, W, dtype=torch.float64)
    for y in range(H):
        for xx in range(W):
            for kt in range(Kt):
                for g in range(G):
                    ks = [p.index(kt, ky, kx) for ky in p.y.covering(y) for kx in p.x.covering(xx)]
                    out[:, :, Fs + kt * G + g, y, xx] = sum(wg[k][y, xx] * x[k][:, :, n + g, y - p.origin(k)[1], xx - p.origin(k)[2]]
                                                            for k in ks)
            for f in range(Fs):
                out[:, :, Fs + Kt * G + f, y, xx] = sum(
                    w[k][f, y, xx] * x[k][:, :, n + G + f - p.origin(k)[0], y - p.origin(k)[1], xx - p.origin(k)[2]]
                    for k in p.covering(f, y, xx))
    return out


def test_d_the_torch_restatements_against_a_per_element_loop():
    p = _plan(*SMALL)
    assert p.x.starts == (0, 2, 3)                # the pulled-back last window overlaps its neighbour by more than asked
    (n, th, tw), (Fs, H, W) = p.shape, p.extent
    state = det_uniform("tiles.host.state", (B, C, 2 * Fs + p.Kt * G, H, W), 2.0)
    for k0, k1, rep in ((0, p.K, 1), (5, 11, 2), (17, 18, 1)):
        assert torch.equal(reference_tile_gather(state, p, G, k0, k1, rep), _slow_gather(state, p, k0, k1, rep))
    assert torch.equal(reference_tile_gather(state, p, G), _slow_gather(state, p, 0, p.K, 1))
    pred = det_uniform("tiles.host.pred", (p.K * B, C, 2 * n + G, th, tw), 2.0)
    got, want = reference_tile_blend(pred, p, G), _slow_blend(pred, p)
    assert got.shape == want.shape and got.dtype == torch.float32
    rel = float((got.double() - want).norm() / want.norm())
    print(f"reference_tile_blend vs float64 loop: rel-L2 {rel:.3e}")
    assert rel < 1e-6
    assert not bool(got[:, :, :Fs].any())
    # where one tile covers a position the prediction passes through unchanged
    assert torch.equal(got[:, :, Fs + p.Kt * G, 0, 0], pred.view(p.K, B, C, 2 * n + G, th, tw)[0][:, :, n + G, 0, 0])
    bf = reference_tile_blend(pred.bfloat16(), p, G)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf, reference_tile_blend(pred.bfloat16().float(), p, G).bfloat16())


def test_d_one_tile_per_spatial_axis_is_the_temporal_restatement():
    p = _plan((7, 4, 2), (6, 6, 2), (7, 8, 2))
    state = det_uniform("tiles.host.state1", (B, C, 2 * 7 + 3 * G, 6, 7), 2.0)
    assert torch.equal(reference_tile_gather(state, p, G, 1, 3, 2), reference_window_gather(state, p.t, 4, G, 1, 3, 2))
    pred = det_uniform("tiles.host.pred1", (3 * B, C, 2 * 4 + G, 6, 7), 2.0)
    assert torch.equal(reference_tile_blend(pred, p, G), reference_window_blend(pred, p.t, G))
