"""The VAE part of tests/kernel_bounds.py checked on the CPU (the companion of tests/test_kernel_bounds_host.py):

* conv_cl_im2col -- the reference every conv test is judged against -- agrees with torch's fp64 conv3d / conv2d in every mode of
  wan_conv_cl (1e-12 relative: fp64 against fp64);
* honest emulations of the kernels' arithmetic (fp32 accumulation tap-major, channel-chunk-major, in 16 / 32 / 64-wide groups,
  one rounding to nearest even, with and without the residual) stay inside conv_bound / rmsnorm_silu_bound / softmax_rows_bound;
* thirteen mutants -- each a way the index arithmetic of videocof_amd/csrc/vae_conv.hip could be wrong -- fall outside, and the
  failure names their pixels.  For each the verdict of the old limit (whole-tensor rel-L2 < 4e-3) at the same shape is recorded.
"""
import math
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_bounds as KB  # noqa: E402

BF = torch.bfloat16
OLD_LIMIT = 4e-3


def bf(x):
    return x.to(BF)


def _truncate_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def _rel_l2(x, ref):
    return float((x.double() - ref).norm() / ref.norm())


def _cf(t):          # [T, H, W, C] -> [1, C, T, H, W] fp64
    return t.double().permute(3, 0, 1, 2)[None]


def _rows(y):        # [1, C, T, H, W] -> [T*H*W, C]
    return y[0].permute(1, 2, 3, 0).reshape(-1, y.shape[1])


# ------------------------------------------------------------------------------------------------ the reference itself
# (mode, cin, cout, T, H, W, nh)
MODES = [("causal", 8, 12, 2, 5, 7, 0), ("causal", 8, 12, 2, 5, 7, 1), ("causal", 16, 8, 3, 4, 9, 2),
         ("1x1", 16, 8, 2, 3, 5, 0),
         ("down2d", 8, 8, 2, 12, 20, 0), ("down2d", 8, 8, 1, 13, 21, 0),
         ("up2d", 8, 12, 2, 5, 7, 0),
         ("time", 8, 16, 3, 3, 5, 0), ("time", 8, 16, 2, 4, 6, 2),
         ("down3d", 8, 8, 4, 5, 7, 1), ("down3d", 8, 8, 5, 3, 5, 1)]


def mode_geometry(mode, T, H, W):
    return KB.conv_geometry(mode, T, H, W)[:5]


def torch_conv(mode, P, T, H, W, nh):
    """The same convolution by torch's fp64 conv3d / conv2d, the padding made explicit: [M, cout] without the bias."""
    x, hist, wt = P["x"], P["hist"], P["wt"].double()
    cin = x.shape[-1]
    if mode in ("causal", "time"):
        fr = torch.cat([torch.zeros(2 - nh, H, W, cin, dtype=BF)] + ([hist] if nh else []) + [x])
        return _rows(F.conv3d(_cf(fr), wt, padding=(0, 1, 1) if mode == "causal" else 0))
    if mode == "1x1":
        return _rows(F.conv3d(_cf(x), wt))
    if mode == "down3d":
        fr = torch.cat([torch.zeros(1 - nh, H, W, cin, dtype=BF)] + ([hist] if nh else []) + [x])
        return _rows(F.conv3d(_cf(fr), wt, stride=(2, 1, 1)))
    img = x.double().permute(0, 3, 1, 2)                                  # [T, C, H, W]
    if mode == "down2d":
        y = F.conv2d(F.pad(img, (0, 1, 0, 1)), wt[:, :, 0], stride=2)
    else:
        y = F.conv2d(F.interpolate(img, scale_factor=2.0, mode="nearest-exact"), wt[:, :, 0], padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


@pytest.mark.parametrize("mode,cin,cout,T,H,W,nh", MODES, ids=[f"{m[0]}-{m[1]}x{m[2]}-{m[3]}x{m[4]}x{m[5]}-h{m[6]}" for m in MODES])
def test_im2col_reference_agrees_with_torch_fp64(mode, cin, cout, T, H, W, nh):
    kernel, stride, pad, out_thw, ups = mode_geometry(mode, T, H, W)
    P = KB.conv_operands(cin, cout, kernel, T, H, W, nh, seed=T * 100 + H + W + nh)
    A = KB.conv_cl_im2col(P["x"], P["hist"], kernel, stride, pad, out_thw, ups)
    assert A.shape == (out_thw[0] * out_thw[1] * out_thw[2], P["K"]) and A.dtype == torch.float64
    got = A @ P["w"].double()[:, :P["K"]].t()
    want = torch_conv(mode, P, T, H, W, nh)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_time_interleave_is_the_reference_rearrangement():
    To, Ho, Wo, C = 2, 3, 4, 16
    conv = torch.arange(To * Ho * Wo * C, dtype=torch.float64).view(To * Ho * Wo, C)
    out = KB.time_interleave(conv, (To, Ho, Wo)).view(2 * To, Ho, Wo, C // 2)
    c4 = conv.view(To, Ho, Wo, C)
    for t in range(To):
        for half in range(2):
            assert torch.equal(out[2 * t + half], c4[t, :, :, half * 8:(half + 1) * 8])


# ------------------------------------------------------------------------------------------------ honest emulations
def _acc_chunks(A, w, K, chunk):
    acc = torch.zeros(A.shape[0], w.shape[0])
    for k0 in range(0, K, chunk):
        acc = acc + A[:, k0:k0 + chunk].float() @ w[:, k0:min(k0 + chunk, K)].float().t()
    return acc


def _acc_channel_chunk_major(A, w, cin, ntaps, cc=32):
    """The patch kernel's order: for each 32-channel chunk, all taps."""
    acc = torch.zeros(A.shape[0], w.shape[0])
    for c0 in range(0, cin, cc):
        for tap in range(ntaps):
            k0 = tap * cin + c0
            acc = acc + A[:, k0:k0 + cc].float() @ w[:, k0:k0 + cc].float().t()
    return acc


def _finish(acc, bias, resid):
    v = acc + bias
    if resid is not None:
        v = v + resid.float()
    return bf(v)


@pytest.fixture(scope="module")
def causal():
    """Causal 3x3x3, (cin, cout, T, H, W) = (32, 96, 3, 9, 33), two history frames, residual: M = 891 pixels, K = 864."""
    cin, cout, T, H, W, nh = 32, 96, 3, 9, 33, 2
    kernel, stride, pad, out_thw, _ = mode_geometry("causal", T, H, W)
    P = KB.conv_operands(cin, cout, kernel, T, H, W, nh, seed=5, resid_shape=(T * H * W, cout))
    A = KB.conv_cl_im2col(P["x"], P["hist"], kernel, stride, pad, out_thw)
    ref, bound = KB.conv_bound(A, P["w"], P["bias"], P["resid"], P["K"])
    ref_nr, bound_nr = KB.conv_bound(A, P["w"], P["bias"], None, P["K"])
    return dict(P, A=A, ref=ref, bound=bound, ref_nr=ref_nr, bound_nr=bound_nr, cin=cin, cout=cout, T=T, H=H, W=W, nh=nh,
                geo=(kernel, stride, pad, out_thw))


def test_honest_conv_emulations_stay_inside(causal):
    c = causal
    A, w, K = c["A"], c["w"], c["K"]
    worst = 0.0
    accs = {"tap-major": _acc_chunks(A, w, K, c["cin"]), "channel-chunk-major": _acc_channel_chunk_major(A, w, c["cin"], 27),
            "16-wide": _acc_chunks(A, w, K, 16), "32-wide": _acc_chunks(A, w, K, 32), "64-wide": _acc_chunks(A, w, K, 64)}
    for name, acc in accs.items():
        worst = max(worst, KB.assert_within(_finish(acc, c["bias"], c["resid"]), c["ref"], c["bound"], f"{name}, residual"))
        worst = max(worst, KB.assert_within(_finish(acc, c["bias"], None), c["ref_nr"], c["bound_nr"], name))
    print(f"[bound] honest conv emulations: peak |err|/bound = {worst:.3f}")
    assert 0.5 < worst <= 1.0, worst          # the half-ulp term of the one rounding is sharp


RECORD = {}          # mutant -> does the old limit (rel-L2 < 4e-3) let it through at this shape


def _record(name, out, ref):
    RECORD[name] = _rel_l2(out, ref) < OLD_LIMIT
    print(f"[mutant] {name}: rel-L2 {_rel_l2(out, ref):.2e} -> old limit {'passes it' if RECORD[name] else 'rejects it'}")
    return RECORD[name]


def _rejected(name, out, ref, bound, rows):
    """The mutant is outside the bound, the failure names exactly the pixel range `rows` = (lo, hi); records the old limit's verdict."""
    passes_old = _record(name, out, ref)
    with pytest.raises(AssertionError, match="outside the bound") as e:
        KB.assert_within(out, ref, bound, name)
    m = re.search(r"rows (\d+)-(\d+)", str(e.value))
    assert m and (int(m.group(1)), int(m.group(2))) == tuple(rows), (name, str(e.value), rows)
    return passes_old


def _mut_out(c, A_mut=None, ref_nb=None):
    """fp64 reference of a mutated gather, honestly finished: + bias, + residual in fp32, one rounding."""
    if ref_nb is None:
        ref_nb = A_mut @ c["w"].double()[:, :c["K"]].t()
    return _finish(ref_nb.float(), c["bias"], c["resid"])


def test_conv_gather_mutants_are_rejected_and_named(causal):
    c = causal
    A, ref, bound, cin, T, H, W, nh = c["A"], c["ref"], c["bound"], c["cin"], c["T"], c["H"], c["W"], c["nh"]
    kernel, stride, pad, out_thw = c["geo"]
    HW = H * W
    KB.assert_within(_mut_out(c, A), ref, bound, "unmutated")
    frames = torch.cat([c["hist"], c["x"]]).double()
    # 1. W-edge wrap: the pixel at (to, ho, wo) = (1, 3, 0) takes its left neighbours (wi = -1, hi inside the image) at their flat
    #    address -- the last pixel of the previous image row -- instead of zero
    to, ho = 1, 3
    m = (to * H + ho) * W
    Am = A.clone()
    for kt in range(3):
        for kh in range(3):
            tap = (kt * 3 + kh) * 3                                          # kw = 0
            Am[m, tap * cin:(tap + 1) * cin] = frames[to - 2 + kt + nh, ho - 1 + kh - 1, W - 1]
    _rejected("1 W-edge wrap", _mut_out(c, Am), ref, bound, (m, m))
    # 2. history frames -2 and -1 exchanged: output frames 0 (taps kt = 0, 1) and 1 (tap kt = 0) read history
    Am = KB.conv_cl_im2col(c["x"], c["hist"].flip(0), kernel, stride, pad, out_thw)
    _rejected("2 history frames exchanged", _mut_out(c, Am), ref, bound, (0, 2 * HW - 1))
    # 3. history read as zero for the first output frame only
    Am = A.clone()
    Am[:HW] = KB.conv_cl_im2col(c["x"], None, kernel, stride, pad, out_thw)[:HW]
    _rejected("3 no history in frame 0", _mut_out(c, Am), ref, bound, (0, HW - 1))
    # 7. one 8-channel chunk of one tap dropped for the pixels of one 8-row piece of a tile (tile 3, piece 5)
    m0 = 3 * 128 + 5 * 8
    Am = A.clone()
    Am[m0:m0 + 8, 13 * cin + 8:13 * cin + 16] = 0.0
    _rejected("7 one chunk of one tap dropped", _mut_out(c, Am), ref, bound, (m0, m0 + 7))
    # 9. the residual added after the bf16 rounding (two roundings)
    acc = _acc_chunks(A, c["w"], c["K"], 64)
    out = bf(bf(acc + c["bias"]).float() + c["resid"].float())
    passes_old = _record("9 residual after the rounding", out, ref)
    with pytest.raises(AssertionError, match="outside the bound") as e:
        KB.assert_within(out, ref, bound, "9 residual after the rounding")
    assert int(str(e.value).split(": ")[1].split(" of ")[0]) > 1000 and passes_old          # not marginal, and the old limit passes it
    # 10. a truncating store
    out = _truncate_bf16(acc + c["bias"] + c["resid"].float())
    _rejected("10 truncating store", out, ref, bound, (0, T * HW - 1))
    # 11. the bias of one 4-column group taken from its neighbour
    b2 = c["bias"].clone()
    b2[44:48] = c["bias"][40:44]
    out = _finish(acc, b2, c["resid"])
    _record("11 bias of the neighbouring group", out, ref)
    with pytest.raises(AssertionError, match=rf"rows 0-{T * HW - 1}, cols 44-47"):
        KB.assert_within(out, ref, bound, "11 bias of the neighbouring group")


def test_k_padding_mutant_is_rejected():
    """8. Cin = 8: K = 216, Kpad = 256 -- forty K-padding columns; read as non-zero (against the A columns a wrapped tap index would
    fetch) they move every pixel."""
    cin, cout, T, H, W = 8, 96, 2, 9, 33
    kernel, stride, pad, out_thw, _ = mode_geometry("causal", T, H, W)
    P = KB.conv_operands(cin, cout, kernel, T, H, W, 2, seed=8)
    A = KB.conv_cl_im2col(P["x"], P["hist"], kernel, stride, pad, out_thw)
    ref, bound = KB.conv_bound(A, P["w"], P["bias"], None, P["K"])
    KB.assert_within(_finish(_acc_chunks(A, P["w"], P["K"], 64), P["bias"], None), ref, bound, "honest, Cin = 8")
    g = torch.Generator().manual_seed(9)
    wpad = bf(torch.randn(cout, P["Kpad"] - P["K"], generator=g) / math.sqrt(P["K"])).double()
    mut = A @ P["w"].double()[:, :P["K"]].t() + A[:, :P["Kpad"] - P["K"]] @ wpad.t()
    P["resid"] = None
    _rejected("8 K padding read as non-zero", _mut_out(P, ref_nb=mut), ref, bound, (0, T * H * W - 1))


def test_resample_and_interleave_mutants_are_rejected():
    # 4. the upsample source is (hi + 1) >> 1: the same conv over an explicitly (wrongly) upsampled plane
    cin, cout, T, H, W = 16, 96, 2, 5, 7
    kernel, stride, pad, out_thw, ups = mode_geometry("up2d", T, H, W)
    P = KB.conv_operands(cin, cout, kernel, T, H, W, 0, seed=4)
    P["resid"] = None
    A = KB.conv_cl_im2col(P["x"], None, kernel, stride, pad, out_thw, True)
    ref, bound = KB.conv_bound(A, P["w"], P["bias"], None, P["K"])
    h2, w2 = torch.arange(2 * H), torch.arange(2 * W)
    up_ok = P["x"][:, h2 >> 1][:, :, w2 >> 1]
    assert torch.equal(KB.conv_cl_im2col(up_ok, None, kernel, stride, pad, out_thw, False), A)          # the honest plane, explicitly
    up_bad = P["x"][:, ((h2 + 1) >> 1).clamp_max(H - 1)][:, :, ((w2 + 1) >> 1).clamp_max(W - 1)]
    Am = KB.conv_cl_im2col(up_bad, None, kernel, stride, pad, out_thw, False)
    KB.assert_within(_mut_out(P, A), ref, bound, "honest upsample")
    # (the last pixel reads only clamped sources in both planes: the one pixel the mutant leaves right)
    _rejected("4 upsample source (hi + 1) >> 1", _mut_out(P, Am), ref, bound, (0, A.shape[0] - 2))
    # 5. stride-2 padding at the top / left instead of the bottom / right
    cin, cout, T, H, W = 16, 96, 2, 12, 20
    kernel, stride, pad, out_thw, _ = mode_geometry("down2d", T, H, W)
    P = KB.conv_operands(cin, cout, kernel, T, H, W, 0, seed=5)
    P["resid"] = None
    A = KB.conv_cl_im2col(P["x"], None, kernel, stride, pad, out_thw)
    ref, bound = KB.conv_bound(A, P["w"], P["bias"], None, P["K"])
    Am = KB.conv_cl_im2col(P["x"], None, kernel, stride, (0, 1, 1), out_thw)
    KB.assert_within(_mut_out(P, A), ref, bound, "honest stride 2")
    _rejected("5 stride-2 padding top / left", _mut_out(P, Am), ref, bound, (0, A.shape[0] - 1))
    # 6. the interleave halves swapped
    cin, cout, T, H, W = 16, 32, 2, 4, 6
    kernel, stride, pad, out_thw, _ = mode_geometry("time", T, H, W)
    P = KB.conv_operands(cin, cout, kernel, T, H, W, 2, seed=6)
    A = KB.conv_cl_im2col(P["x"], P["hist"], kernel, stride, pad, out_thw)
    ref, bound = KB.conv_bound(A, P["w"], P["bias"], None, P["K"])
    ref_i, bound_i = KB.time_interleave(ref, out_thw), KB.time_interleave(bound, out_thw)
    honest = _finish(_acc_chunks(A, P["w"], P["K"], 16), P["bias"], None)
    KB.assert_within(KB.time_interleave(honest, out_thw), ref_i, bound_i, "honest interleave")
    swapped = KB.time_interleave(torch.cat([honest[:, 16:], honest[:, :16]], dim=1), out_thw)
    _rejected("6 interleave halves swapped", swapped, ref_i, bound_i, (0, 2 * A.shape[0] - 1))


# ------------------------------------------------------------------------------------------------ row kernels
def _rmsnorm_silu_f32(x, gamma, silu, ss=None):
    xf = x.float()
    ss = xf.pow(2).sum(dim=-1, keepdim=True) if ss is None else ss
    scale = torch.tensor(float(x.shape[-1])).sqrt() / ss.sqrt().clamp_min(1e-12)
    a = xf * scale * gamma
    return a / (1.0 + torch.exp(-a)) if silu else a


@pytest.mark.parametrize("C", [8, 64, 96, 192, 384, 512])
def test_honest_rmsnorm_silu_emulation_stays_inside_and_mutants_fall_outside(C):
    g = torch.Generator().manual_seed(C)
    rows = 67
    x = bf(torch.randn(rows, C, generator=g) * 1.5)
    x[5] = 0
    gamma = torch.rand(C, generator=g) + 0.5
    for silu in (False, True):
        ref, bound = KB.rmsnorm_silu_bound(x, gamma, silu)
        assert float(ref[5].abs().max()) == 0.0
        y = _rmsnorm_silu_f32(x, gamma, silu)
        # the lane-grouped sum: 8 per lane, then a tree
        ss = x.float().pow(2).view(rows, C // 8, 8).sum(dim=-1).flip(-1).sum(dim=-1, keepdim=True)
        assert KB.assert_within(bf(y), ref, bound, "rmsnorm_silu") <= 1.0
        assert KB.assert_within(bf(_rmsnorm_silu_f32(x, gamma, silu, ss)), ref, bound, "rmsnorm_silu, grouped sum") <= 1.0
        with pytest.raises(AssertionError, match="outside the bound"):
            KB.assert_within(_truncate_bf16(y), ref, bound, "rmsnorm_silu truncated")
        # 12b. one pixel's scale used for its neighbour in the wave
        ss2 = x.float().pow(2).sum(dim=-1, keepdim=True)
        ss2[21] = ss2[20]
        out = bf(_rmsnorm_silu_f32(x, gamma, silu, ss2))
        _record(f"12b neighbour's scale, C={C}, silu={silu}", out, ref)
        with pytest.raises(AssertionError, match=r"rows 21-21, "):
            KB.assert_within(out, ref, bound, "neighbour's scale")
    if C == 96:
        # 12a. the sum of squares over the whole 16-lane group: lanes 12 .. 15 are not zero but hold the next pixel's first 32 channels
        ref, bound = KB.rmsnorm_silu_bound(x, gamma, True)
        nxt = torch.roll(x, -1, 0)[:, :32].float()
        ss = x.float().pow(2).sum(dim=-1, keepdim=True) + nxt.pow(2).sum(dim=-1, keepdim=True)
        out = bf(_rmsnorm_silu_f32(x, gamma, True, ss))
        _record("12a sum over the 16-lane group", out, ref)
        with pytest.raises(AssertionError, match=rf"rows 0-{rows - 1}, "):
            KB.assert_within(out, ref, bound, "sum over the 16-lane group")


def _softmax_f32(s, n, scale, sum_upto=None):
    sf = s[:, :n].float()
    e = torch.exp((sf - sf.max(dim=-1, keepdim=True).values) * scale)
    # 256 strided partial sums, then their sum: the kernel's order
    pad = (-n) % 256
    part = F.pad(e if sum_upto is None else e[:, :sum_upto], (0, pad if sum_upto is None else (-sum_upto) % 256)).view(s.shape[0], -1, 256).sum(dim=1)
    return e * (1.0 / part.sum(dim=-1, keepdim=True))


@pytest.mark.parametrize("rows,n", [(3, 1), (5, 100), (4, 256), (3, 257), (2, 1000)])
@pytest.mark.parametrize("scale", [0.3, 1.0 / math.sqrt(384.0)])
def test_honest_softmax_emulation_stays_inside_and_mutants_fall_outside(rows, n, scale):
    g = torch.Generator().manual_seed(n)
    s = torch.randn(rows, n, generator=g) * 5
    s[0, n // 2] = 60.0                                                     # one dominant entry
    ref, bound = KB.softmax_rows_bound(s, n, scale)
    assert abs(float(ref.sum(dim=-1).max()) - 1.0) < 1e-12
    assert KB.assert_within(bf(_softmax_f32(s, n, scale)), ref, bound, "softmax_rows") <= 1.0
    assert KB.assert_within(bf(torch.softmax(s.float() * scale, dim=-1)), ref, bound, "softmax_rows, torch fp32") <= 1.0
    if n > 1:
        with pytest.raises(AssertionError, match="outside the bound"):
            KB.assert_within(_truncate_bf16(_softmax_f32(s, n, scale)), ref, bound, "softmax_rows truncated")
    if n > 256:
        # 13. elements >= 256 left out of the row sum
        out = bf(_softmax_f32(s, n, scale, sum_upto=256))
        _record(f"13 sum stops at 256, n={n}, scale={scale:.3f}", out, ref)
        # (row 0's dominant entry sits below 256: where it takes nearly all the mass the lost terms hide behind it)
        with pytest.raises(AssertionError, match=rf"rows [01]-{rows - 1}, "):
            KB.assert_within(out, ref, bound, "sum stops at 256")
