"""-m gpu: the VAE's three convolution kernels (conv_cl_kernel, conv3_patch_kernel, conv3_head_kernel) and its two row kernels
(rmsnorm_silu_cl, softmax_rows) judged PER ELEMENT against fp64 references built by plain indexing (kernel_bounds.conv_cl_im2col)
under the derived bounds of tests/kernel_bounds.py (docs/TEST_BOUNDS.md), every operand and result inside poisoned guard bands.

tests/test_gpu_vae.py holds these kernels to whole-tensor rel-L2 limits, which pass a pixel that wraps around the W edge, exchanged
history frames in a corner case, a dropped 8-channel chunk, a truncating store (tests/test_vae_bounds_host.py).  Here the gather
kernel runs every mode of wan_conv_cl at small shapes on both address paths (conv_fast 1 / 0) and both tile orders (conv_xcd 1 / 0)
-- results must be bit-identical, only addresses differ -- with output row strides ldo = channels + 8 and + 4.
Every comparison prints its worst |err| / bound; the limit is 1.
"""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_bounds as KB  # noqa: E402
from videocof_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
TUNING_KEYS = ("conv_fast", "conv_xcd", "conv_patch", "conv_head", "conv_mfma")


class _Tuning:
    """Sets tuning keys; restores EVERY conv key to what it was on entry, whatever happens inside."""

    def __init__(self, **values):
        self.values = values

    def __enter__(self):
        self.old = {k: ops.get_tuning(k) for k in TUNING_KEYS}
        for k, v in self.values.items():
            ops.set_tuning(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            ops.set_tuning(k, v)


def _report(tag, worst):
    print(f"[bound] {tag}: worst |err|/bound = {worst:.3f}")
    return worst


@functools.lru_cache(maxsize=2)
def _problem(mode, cin, cout, T, H, W, nh, resid, zero_rows=0):
    """Operands, fp64 reference and bound of one case, on the CPU, computed once and left unchanged.  zero_rows: that many trailing
    weight rows are zero (the head's padding channel)."""
    kernel, stride, pad, out_thw, ups, il = KB.conv_geometry(mode, T, H, W)
    M = out_thw[0] * out_thw[1] * out_thw[2]
    ch = cout // 2 if il else cout
    rows = 2 * M if il else M
    P = KB.conv_operands(cin, cout, kernel, T, H, W, nh, seed=cin + cout + 7 * T + 13 * H + W + nh, resid_shape=(rows, ch) if resid else None)
    if zero_rows:
        P["w"][cout - zero_rows:] = 0
    A = KB.conv_cl_im2col(P["x"], P["hist"], kernel, stride, pad, out_thw, ups)
    assert 2 * A.shape[0] * P["K"] * cout < 2e9
    assert not (il and resid)
    ref, bound = KB.conv_bound(A, P["w"], P["bias"], P["resid"], P["K"])
    if il:
        ref, bound = KB.time_interleave(ref, out_thw), KB.time_interleave(bound, out_thw)
    P.update(ref=ref, bound=bound, geo=(kernel, stride, pad, out_thw, ups, il), rows=rows, ch=ch, cout=cout, T=T, H=H, W=W, cin=cin, nh=nh)
    return P


class _DeviceOperands:
    """x, hist, w, bias of a case inside NaN poison on the device: guard rows before and after the contiguous tensors; w with
    ldw = Kpad + 16, poison right of Kpad, zeros in [K, Kpad) as the ABI demands."""

    def __init__(self, P):
        T, H, W, cin, nh = P["T"], P["H"], P["W"], P["cin"], P["nh"]
        self.g = {}
        self.x = self._put("x", P["x"].view(T * H * W, cin)).view(T, H, W, cin)
        self.hist = self._put("hist", P["hist"].view(nh * H * W, cin)).view(nh, H, W, cin) if nh else None
        self.bias = self._put("bias", P["bias"][None])[0]
        gw = KB.Guarded(tuple(P["w"].shape), BF, ld=P["Kpad"] + 16, device=DEV)
        self.g["w"] = gw
        self.w = gw.fill(P["w"].to(DEV))
        assert float(self.w[:, P["K"]:].abs().max() if P["Kpad"] > P["K"] else 0.0) == 0.0

    def _put(self, name, t):
        gd = KB.Guarded(tuple(t.shape), t.dtype, device=DEV)
        self.g[name] = gd
        return gd.fill(t.to(DEV))

    def check(self, tag):
        for name, gd in self.g.items():
            gd.check(f"{tag}: guard band of {name}")


def _run(P, D, extra, tag):
    """One wan_conv_cl call into a Guarded output of row stride ldo = channels + extra (the residual, if any, at the same stride).
    Returns the [rows, ch] result on the device; every guard is checked."""
    kernel, stride, pad, out_thw, ups, il = P["geo"]
    rows, ch = P["rows"], P["ch"]
    To = 2 * out_thw[0] if il else out_thw[0]
    go = KB.Guarded((rows, ch), BF, ld=ch + extra, device=DEV)
    resid = None
    if P["resid"] is not None:
        gr = KB.Guarded((rows, ch), BF, ld=ch + extra, device=DEV)
        resid = gr.fill(P["resid"].to(DEV)).view(To, out_thw[1], out_thw[2], ch)
    out = ops.conv_cl(D.x, D.w, D.bias, P["cout"], kernel, stride=stride, pad=pad, out_thw=out_thw, hist=D.hist, upsample2x=ups,
                      time_interleave=il, resid=resid, out=go.view.view(To, out_thw[1], out_thw[2], ch))
    assert out.data_ptr() == go.view.data_ptr()
    torch.cuda.synchronize()
    go.check(f"{tag}, ldo = channels + {extra}: guard band of out")
    if resid is not None:
        gr.check(f"{tag}: guard band of resid")
    D.check(tag)
    return go.view


# ------------------------------------------------------------------------------------------------ gather kernel
# (mode, cin, cout, T, H, W, residual, history frame counts) -- tiles = tiles_m x tiles_n of conv_cl_kernel (128 pixels x BN channels)
GATHER = [
    ("causal", 8, 96, 2, 9, 33, False, (0, 1, 2)),        # K = 216, Kpad = 256: eight taps share a K tile; NT = 3; 5 x 1 = 5 tiles
    ("causal", 96, 96, 3, 13, 37, True, (0, 1, 2)),       # 12 x 1 = 12 tiles: a remainder of 4 over the 8 XCD slabs
    ("causal", 32, 192, 1, 8, 16, False, (0, 1, 2)),      # exactly one 128-pixel tile, NT = 6; 1 tile
    ("causal", 32, 192, 2, 16, 32, False, (0, 1, 2)),     # 8 x 1 = 8 tiles: a multiple of 8
    ("causal", 64, 128, 2, 7, 19, False, (0, 1, 2)),      # NT = 4, one whole N tile; 3 x 1 = 3 tiles
    ("causal", 32, 320, 1, 5, 27, False, (0, 1, 2)),      # NT = 4, two whole N tiles and a ragged third; 2 x 3 = 6 tiles
    ("causal", 96, 64, 1, 11, 13, False, (0, 1, 2)),      # NT = 3 with masked columns; 2 tiles
    ("causal", 96, 16, 2, 6, 10, False, (0, 1, 2)),       # NT = 1; 1 tile
    ("causal", 96, 4, 2, 9, 33, False, (0, 1, 2)),        # NT = 1, the head's shape with conv_head = 0; 5 tiles
    ("1x1", 384, 1152, 1, 3, 5, False, (0,)),             # 1 x 6 = 6 tiles
    ("1x1", 384, 384, 2, 3, 5, True, (0,)),               # 1 x 2 = 2 tiles
    ("1x1", 16, 16, 3, 4, 6, False, (0,)),                # 1 tile
    ("down2d", 96, 96, 2, 12, 20, False, (0,)),           # the bottom / right zero tap is read; 1 tile
    ("down2d", 96, 96, 1, 13, 21, False, (0,)),           # ... is not read; 1 tile
    ("down2d", 192, 192, 1, 6, 10, False, (0,)),          # 1 tile
    ("up2d", 192, 96, 2, 5, 7, False, (0,)),              # 280 output pixels: 3 tiles
    ("up2d", 384, 192, 1, 3, 5, False, (0,)),             # 1 tile
    ("time", 384, 768, 3, 3, 5, False, (0, 2)),           # 1 x 4 = 4 tiles
    ("time", 96, 192, 2, 4, 6, False, (0, 2)),            # 1 tile
    ("down3d", 96, 96, 4, 5, 7, False, (1,)),             # T_out = 2; 1 tile
    ("down3d", 192, 192, 5, 3, 5, False, (1,)),           # odd T, T_out = 2; 1 tile
]
GATHER_CASES = [(m, ci, co, T, H, W, r, nh) for (m, ci, co, T, H, W, r, nhs) in GATHER for nh in nhs]


@pytest.mark.parametrize("mode,cin,cout,T,H,W,resid,nh", GATHER_CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}x{c[4]}x{c[5]}-h{c[7]}{'-r' if c[6] else ''}" for c in GATHER_CASES])
def test_gather_kernel_every_mode_per_element(mode, cin, cout, T, H, W, resid, nh):
    P = _problem(mode, cin, cout, T, H, W, nh, resid)
    D = _DeviceOperands(P)
    tag = f"conv gather {mode} {cin}->{cout} {T}x{H}x{W} hist {nh}{' +resid' if resid else ''}"
    outs = {}
    with _Tuning(conv_patch=0, conv_head=0) as tune:
        for fast in (1, 0):
            for xcd in (1, 0):
                ops.set_tuning("conv_fast", fast)
                ops.set_tuning("conv_xcd", xcd)
                outs[(fast, xcd)] = _run(P, D, 8, f"{tag} fast {fast} xcd {xcd}").clone()
        ops.set_tuning("conv_fast", tune.old["conv_fast"])
        ops.set_tuning("conv_xcd", tune.old["conv_xcd"])
        narrow = _run(P, D, 4, tag).clone()
    _report(tag, KB.assert_within(outs[(1, 1)], P["ref"], P["bound"], tag))
    outs["ldo = channels + 4"] = narrow
    for key, o in outs.items():          # only addresses differ between the four settings and the two row strides
        if not torch.equal(o, outs[(1, 1)]):
            KB.assert_within(o, P["ref"], P["bound"], f"{tag}, (conv_fast, conv_xcd) = {key}")          # names the pixels, if outside
            raise AssertionError(f"{tag}: (conv_fast, conv_xcd) = {key} differs from (1, 1) in {int((o != outs[(1, 1)]).sum())} elements")


def test_conv_cl_out_is_validated():
    x = torch.zeros(1, 4, 4, 8, device=DEV, dtype=BF)
    w = torch.zeros(16, 64, device=DEV, dtype=BF)
    call = lambda out: ops.conv_cl(x, w, None, 16, (1, 1, 1), out_thw=(1, 4, 4), out=out)
    buf = torch.zeros(16, 24, device=DEV, dtype=BF)
    assert call(buf[:, :16].view(1, 4, 4, 16)).data_ptr() == buf.data_ptr()
    with pytest.raises(ValueError, match="ldo % 4"):
        call(torch.zeros(16, 18, device=DEV, dtype=BF)[:, :16].view(1, 4, 4, 16))
    with pytest.raises(ValueError, match="shape"):
        call(torch.zeros(1, 4, 4, 12, device=DEV, dtype=BF))
    with pytest.raises(ValueError, match="dense rows"):
        call(torch.zeros(1, 8, 4, 16, device=DEV, dtype=BF)[:, ::2])
    with pytest.raises(ValueError, match="bfloat16"):
        call(torch.zeros(1, 4, 4, 16, device=DEV))
    # the packed 16-bit tap coordinates hold pads below 4096, along W as along H
    for pad in ((0, 4096, 0), (0, 0, 4096)):
        with pytest.raises(ValueError, match="bad stride/pad"):
            ops.conv_cl(x, w, None, 16, (1, 1, 1), pad=pad, out_thw=(1, 4, 4))


# ------------------------------------------------------------------------------------------------ patch kernel
# the four shapes of test_lds_patch_conv_vs_torch_and_vs_gather_kernel, one column past a tile, one row past two tiles
PATCH = [(32, 96, 1, 8, 32, 0, False), (96, 96, 3, 13, 37, 1, True), (64, 192, 2, 21, 70, 2, False), (96, 384, 1, 9, 33, 2, True),
         (32, 96, 2, 8, 33, 1, False), (96, 192, 1, 17, 32, 2, True)]


@pytest.mark.parametrize("cin,cout,T,H,W,nh,resid", PATCH, ids=[f"{c[0]}x{c[1]}-{c[2]}x{c[3]}x{c[4]}-h{c[5]}{'-r' if c[6] else ''}" for c in PATCH])
def test_patch_kernel_per_element(cin, cout, T, H, W, nh, resid):
    P = _problem("causal", cin, cout, T, H, W, nh, resid)
    D = _DeviceOperands(P)
    tag = f"conv patch {cin}->{cout} {T}x{H}x{W} hist {nh}{' +resid' if resid else ''}"
    with _Tuning(conv_patch=2):
        for mfma in (32, 16):
            ops.set_tuning("conv_mfma", mfma)
            out = _run(P, D, 8, f"{tag} mfma {mfma}")
            _report(f"{tag} mfma {mfma}", KB.assert_within(out, P["ref"], P["bound"], f"{tag} mfma {mfma}"))
        # rows 8-byte aligned only: the 16-byte stores of the patch kernel do not apply (dispatch rule ldo % 8), the gather kernel runs
        ops.set_tuning("conv_mfma", 32)
        narrow = _run(P, D, 4, f"{tag} ldo + 4").clone()
        _report(f"{tag} ldo + 4 (gather fallback)", KB.assert_within(narrow, P["ref"], P["bound"], f"{tag} ldo + 4"))
        ops.set_tuning("conv_patch", 0)
        assert torch.equal(_run(P, D, 4, f"{tag} gather"), narrow), (tag, "ldo % 8 != 0 must run the gather kernel")


# ------------------------------------------------------------------------------------------------ head kernel
HEAD = [(96, 1, 8, 32, 0), (96, 3, 13, 37, 1), (32, 2, 21, 70, 2), (96, 5, 9, 65, 2), (32, 1, 8, 33, 2)]


@pytest.mark.parametrize("cin,T,H,W,nh", HEAD, ids=[f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-h{c[4]}" for c in HEAD])
def test_head_kernel_per_element(cin, T, H, W, nh):
    P = _problem("causal", cin, 4, T, H, W, nh, False, 1)          # three real channels, the fourth weight row is zero
    D = _DeviceOperands(P)
    tag = f"conv head {cin}->4 {T}x{H}x{W} hist {nh}"
    with _Tuning(conv_head=1):
        out = _run(P, D, 4, tag)                                      # ldo = 8
        _report(tag, KB.assert_within(out, P["ref"], P["bound"], tag))
        assert torch.equal(out[:, 3].cpu(), P["bias"][3].to(BF).expand(P["rows"])), (tag, "column 3 is its bias, rounded once")


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("C", [8, 64, 96, 192, 384, 512])          # LPP = 8, 8, 16 (12 lanes active), 32, 64, 64
@pytest.mark.parametrize("rows", [1, 63, 257])                     # below, across and not a multiple of rows_per_wg (128 / 64 / 32 / 16)
def test_rmsnorm_silu_cl_per_element(C, rows):
    g = torch.Generator().manual_seed(C + rows)
    x = (torch.randn(rows, C, generator=g) * 1.5).to(BF)
    if rows > 1:
        x[rows // 2] = 0                                           # the eps path: max(||x||, 1e-12)
    gamma = torch.rand(C, generator=g) + 0.5
    gx = KB.Guarded((rows, C), BF, device=DEV)
    gg = KB.Guarded((1, C), torch.float32, device=DEV)
    gx.fill(x.to(DEV))
    gg.fill(gamma[None].to(DEV))
    lib = _lib.load()
    for silu in (False, True):
        go = KB.Guarded((rows, C), BF, device=DEV)
        _lib.check(lib.wan_rmsnorm_silu_cl(ops._p(gx.view), ops._p(gg.view), ops._p(go.view), rows, C, int(silu), ops._stream()),
                   "wan_rmsnorm_silu_cl")
        torch.cuda.synchronize()
        tag = f"rmsnorm_silu_cl C {C} rows {rows} silu {int(silu)}"
        go.check(f"{tag}: guard band of out")
        gx.check(f"{tag}: guard band of x")
        gg.check(f"{tag}: guard band of gamma")
        ref, bound = KB.rmsnorm_silu_bound(x, gamma, silu)
        _report(tag, KB.assert_within(go.view, ref, bound, tag))
        if rows > 1:
            assert float(go.view[rows // 2].abs().max()) == 0.0


@pytest.mark.parametrize("rows,n,npad", [(3, 1, 64), (5, 100, 128), (4, 256, 256), (3, 257, 320), (2, 1000, 1024)])
@pytest.mark.parametrize("scale", [0.3, 1.0 / math.sqrt(384.0)])
def test_softmax_rows_per_element(rows, n, npad, scale):
    g = torch.Generator().manual_seed(n)
    s = torch.randn(rows, n, generator=g) * 5
    s[0, n // 2] = 60.0                                            # one row with a single dominant entry
    gs = KB.Guarded((rows, n), torch.float32, ld=n + 8, device=DEV)          # lds > n, poison right of n
    gs.fill(s.to(DEV))
    gp = KB.Guarded((rows, npad), BF, ld=npad + 8, device=DEV)
    lib = _lib.load()
    _lib.check(lib.wan_softmax_rows(ops._p(gs.view), gs.view.stride(0), ops._p(gp.view), gp.view.stride(0), rows, n, npad, float(scale),
                                    ops._stream()), "wan_softmax_rows")
    torch.cuda.synchronize()
    tag = f"softmax_rows rows {rows} n {n} npad {npad} scale {scale:.4f}"
    gp.check(f"{tag}: guard band of p")
    gs.check(f"{tag}: guard band of scores")
    ref, bound = KB.softmax_rows_bound(s, n, scale)
    _report(tag, KB.assert_within(gp.view[:, :n], ref, bound, tag))
    if npad > n:
        assert float(gp.view[:, n:].float().abs().max()) == 0.0 and not bool(torch.isnan(gp.view[:, n:].float()).any())
