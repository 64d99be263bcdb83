"""-m gpu: the fp8 (OCP e4m3) kernels judged PER ELEMENT on the operands they are handed -- against fp64 references under the derived
bounds of tests/kernel_bounds.py, or with torch.equal where the result has an exact definition -- with poisoned guard bands around
every operand and result (docs/TEST_BOUNDS.md, "The fp8 kernels").  tests/test_gpu_fp8.py keeps the MODE statements (error against the
bf16 operands, calibration, graphs, LoRA order); this module is the KERNEL statement: the fp8 mode is lossy because of the
quantisation, and on its e4m3 operands every kernel is as exact as its bf16 sibling.

What the whole-tensor limits could not see and this module does: a truncating store, a row or column scale taken from the neighbour,
a 16x16 sub-tile that misses a K tile, a store past N / M / ldo, a read past an operand that reaches a result (operands sit in NaN:
0x7F bytes), one key admitted past k_len (the rows of k8 behind it hold a key that would take all the mass) or lost, two keys of a
tile exchanged (decisive-key inputs), a V scale byte of the wrong key half, the MX edges of P (block sums many binades below the row's
largest, scale word 0).  Every comparison prints its worst |err| / bound; the limit is 1.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_bounds as KB  # noqa: E402
from oracle import wan_oracle as O  # noqa: E402
from videocof_amd import _lib, ops  # noqa: E402
from videocof_amd._lib import RopeParams  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F8, U8 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8


def _report(tag, worst):
    print(f"[bound] {tag}: worst |err|/bound = {worst:.3f}")
    return worst


def _fill8(gd, t):
    """Copy an e4m3 (or uint8 code) tensor into a one-byte Guarded view, byte for byte."""
    gd.view.view(U8).copy_(t.view(U8).to(gd.raw.device))
    return gd


def _vec(t, dtype=torch.float32, aligned=False):
    """A 1-D vector as the interior of a poisoned buffer, 16 bytes into its row, NaN before and behind.  The vector is 16-byte aligned
    only when its byte size is a multiple of 16 (one guard row of the same length precedes it); `aligned`: the kernel demands it."""
    n = t.numel()
    lead = 16 // torch.empty((), dtype=dtype).element_size()
    gd = KB.Guarded((1, n), dtype, ld=n + 2 * lead, rows_before=1, rows_after=1, cols_before=lead, device=DEV)
    gd.view[0].copy_(t.to(DEV))
    assert not aligned or gd.view[0].data_ptr() % 16 == 0, (n, dtype)
    return gd


def _codes(t):
    return t.contiguous().view(U8).cpu()


# ------------------------------------------------------------------------------------------------ GEMM
GEMM_DEFAULTS = {"gemm_pk": 1, "gemm_pk_min_units": 0}
# family -> (tuning, wan_gemm_fp8_ws_plan): the 8-wave per-tile kernel; the persistent stream-K kernel's e4m3 instantiation ("schedule P")
# with the stream-K cut at a quarter of a tile's K range (as tests/test_gpu_fp8.py sets it) and with the plan's own choice
FAMILIES = {"tile": ({"gemm_pk": 0}, 1), "pkq": ({"gemm_pk": 2, "gemm_pk_min_units": "quarter"}, 3), "pkown": ({"gemm_pk": 2, "gemm_pk_min_units": 0}, 3)}
# one K tile (per-tile only: the persistent plan needs K % 256 == 0); split tiles; three 256-units with ragged M and N; many tiles, shallow K
SHAPES = [(300, 256, 128), (1100, 520, 512), (3000, 1164, 768), (4100, 2100, 256)]
GEMM_CASES = [(f, s) for s in SHAPES for f in (("tile",) if s[2] % 256 else ("tile", "pkq", "pkown"))]


class _Tuning:
    def __init__(self, values, K):
        self.values = {k: (max(1, (K // 256 + 3) // 4) if v == "quarter" else v) for k, v in values.items()}

    def __enter__(self):
        for k, v in self.values.items():
            ops.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            ops.set_tuning(k, GEMM_DEFAULTS[k])


@functools.lru_cache(maxsize=1)
def _gemm_problem(M, N, K):
    """Operands quantised on the CPU by the exact definition (no kernel under test takes part), fp64 reference and terms, once per shape."""
    g = torch.Generator().manual_seed(M + N + K)
    acodes, sa = KB.quantize_rows_fp8_ref((torch.randn(M, K, generator=g) * 2).to(BF))
    wcodes, sw = KB.quantize_rows_fp8_ref((torch.randn(N, K, generator=g) * 0.05).to(BF))
    aq, wq = acodes.view(F8), wcodes.view(F8)
    bias = torch.randn(N, generator=g) * 0.5
    x0 = torch.randn(M, N, generator=g) * (10.0 ** torch.randint(-3, 4, (M, N), generator=g).float())
    rpb = (M + 1) // 2                                                   # a sample seam inside a wave's rows
    gate = torch.randn(2, N, generator=g)
    ref, term = KB.gemm_fp8_ref_and_term(aq, sa, wq, sw, bias, K)
    ref_nb, term_nb = KB.gemm_fp8_ref_and_term(aq, sa, wq, sw, None, K)
    return dict(aq=aq, sa=sa, wq=wq, sw=sw, bias=bias, x0=x0, rpb=rpb, gate=gate, ref=ref, term=term, ref_nb=ref_nb, term_nb=term_nb)


def _gemm_run(P, M, N, K):
    """Every epilogue once, operands and results in guard bands.  Returns the Guarded results and the operand guards."""
    A = KB.Guarded((M, K), F8, ld=K + 16, rows_before=1, rows_after=3, cols_before=16, device=DEV)
    W = KB.Guarded((N, K), F8, ld=K + 16, rows_before=1, rows_after=3, cols_before=16, device=DEV)
    _fill8(A, P["aq"]); _fill8(W, P["wq"])
    sa, sw, bias = _vec(P["sa"]), _vec(P["sw"], aligned=True), _vec(P["bias"])
    gate = KB.Guarded((2, N), torch.float32, device=DEV)
    gate.fill(P["gate"].to(DEV))
    args = (A.view, sa.view[0], W.view, sw.view[0])
    o = {}
    o["bf16"] = KB.Guarded((M, N), BF, ld=N + 8, device=DEV)
    ops.gemm_fp8(*args, bias.view[0], ops.EPI_BF16, out=o["bf16"].view)
    o["gelu"] = KB.Guarded((M, N), BF, ld=N + 4, device=DEV)
    ops.gemm_fp8(*args, bias.view[0], ops.EPI_GELU_BF16, out=o["gelu"].view)
    o["f32"] = KB.Guarded((M, N), torch.float32, ld=N + 4, device=DEV)
    ops.gemm_fp8(*args, None, ops.EPI_F32, out=o["f32"].view)
    o["f32b"] = KB.Guarded((M, N), torch.float32, ld=N + 8, device=DEV)
    ops.gemm_fp8(*args, bias.view[0], ops.EPI_F32, out=o["f32b"].view)
    o["resid"] = KB.Guarded((M, N), torch.float32, ld=N + 8, device=DEV)
    o["resid"].fill(P["x0"].to(DEV))
    ops.gemm_fp8(*args, bias.view[0], ops.EPI_RESID_F32, out=o["resid"].view, gate=gate.view, rows_per_batch=P["rpb"])
    for pad in (8, 4):           # transposed: the columns [M, ldo) are guard band (contract: NOT written, include/wan_hip.h)
        o[f"T{pad}"] = KB.Guarded((N, M), BF, ld=ops.round_up(M, 64) + pad, device=DEV)
        ops.gemm_fp8(*args, bias.view[0], ops.EPI_BF16_T, out=o[f"T{pad}"].view)
    torch.cuda.synchronize()
    return o, {"A": A, "W": W, "sa": sa, "sw": sw, "bias": bias, "gate": gate}


@functools.lru_cache(maxsize=1)
def _per_tile_f32(M, N, K):
    """EPI_F32 (with bias) of the per-tile kernel on the problem's operands: what the persistent families must agree with."""
    P = _gemm_problem(M, N, K)
    with _Tuning(FAMILIES["tile"][0], K):
        out = ops.gemm_fp8(P["aq"].to(DEV), P["sa"].to(DEV), P["wq"].to(DEV), P["sw"].to(DEV), P["bias"].to(DEV), ops.EPI_F32)
    return out.cpu()


@pytest.mark.parametrize("family,shape", GEMM_CASES, ids=[f"{f}-{s[0]}x{s[1]}x{s[2]}" for f, s in GEMM_CASES])
def test_gemm_fp8_per_element_and_guard_bands(family, shape):
    M, N, K = shape
    tune, plan = FAMILIES[family]
    P = _gemm_problem(M, N, K)
    lib = _lib.load()
    tag = f"gemm_fp8 {family} {M}x{N}x{K}"
    with _Tuning(tune, K):
        assert lib.wan_gemm_fp8_ws_plan(M, N, K) == plan, (family, shape, lib.wan_gemm_fp8_ws_plan(M, N, K))
        ws = ops.gemm_workspace(torch.device(DEV), M, N, K, fp8=True)
        assert (ws is not None) == (plan == 3)
        if ws is not None:
            ws.fill_(0xFF)
        o, guards = _gemm_run(P, M, N, K)
        if ws is not None:                                # garbage of another kind in the workspace: bitwise the same results
            ws.fill_(0xA5)
            o2, guards2 = _gemm_run(P, M, N, K)
            for k in o:
                assert torch.equal(o[k].view, o2[k].view), f"{tag} {k}: not bitwise reproducible over workspace contents"
                o2[k].check(f"{tag} {k} (second run)")
            for name, gd in guards2.items():
                gd.check(f"{tag} operand {name} (second run)")
    for name, gd in guards.items():
        gd.check(f"{tag} operand {name}")
    worst = {}
    ref, term = P["ref"], P["term"]
    b16 = KB.gemm_bound(None, None, None, K, BF, ref, term)
    worst["bf16"] = KB.assert_within(o["bf16"].view, ref, b16, tag + " EPI_BF16")
    g_ref, g_bound = KB.gelu_bound(ref, term)
    worst["gelu"] = KB.assert_within(o["gelu"].view, g_ref, g_bound, tag + " EPI_GELU_BF16")
    a_ref, a_bound = KB.gelu_from_acc_bound(o["f32b"].view)
    worst["gelu_acc"] = KB.assert_within(o["gelu"].view, a_ref, a_bound, tag + " EPI_GELU_BF16 vs g(own EPI_F32 accumulator)")
    worst["f32b"] = KB.assert_within(o["f32b"].view, ref, KB.gemm_bound(None, None, None, K, torch.float32, ref, term), tag + " EPI_F32 with bias")
    worst["f32"] = KB.assert_within(o["f32"].view, P["ref_nb"], KB.gemm_bound(None, None, None, K, torch.float32, P["ref_nb"], P["term_nb"]),
                                    tag + " EPI_F32")
    # the accumulation term alone (no output-rounding term): what docs/TEST_BOUNDS.md records about the matrix pipe's adder
    worst["acc_only"] = KB.assert_within(o["f32"].view, P["ref_nb"], P["term_nb"], tag + " EPI_F32 against the accumulation term alone")
    r_ref, r_bound = KB.resid_bound(ref, term, P["gate"][torch.arange(M) // P["rpb"]], P["x0"])
    worst["resid"] = KB.assert_within(o["resid"].view, r_ref, r_bound, f"{tag} EPI_RESID_F32 rows_per_batch {P['rpb']}")
    for pad in (8, 4):
        worst[f"T{pad}"] = KB.assert_within(o[f"T{pad}"].view.t(), ref, b16, f"{tag} EPI_BF16_T ldo roundup(M, 64) + {pad} (rows = tokens)")
    for k, gd in o.items():
        gd.check(f"{tag} {k}" + (": pad columns [M, ldo) must be left alone" if k[0] == "T" else ""))
    if family != "tile":                                  # same products, another summation order: within twice the accumulation term
        tile = _per_tile_f32(M, N, K)
        worst["vs_tile"] = KB.assert_within(o["f32b"].view, tile.double(), 2.0 * term, tag + " EPI_F32 vs the per-tile kernel")
        print(f"        differs from the per-tile kernel's EPI_F32 in {int((o['f32b'].view.cpu() != tile).sum())} of {M * N} elements")
    _report(tag, max(worst.values()))
    print("        " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ quantisers
@pytest.mark.parametrize("rows,cols", [(37, 256), (5, 5120), (3, 8)])
def test_quantize_rows_fp8_is_its_exact_definition(rows, cols):
    g = torch.Generator().manual_seed(rows + cols)
    x = (torch.randn(rows, cols, generator=g) * torch.rand(rows, 1, generator=g) * 5).to(BF)
    x[0] = 0.0                                                      # a row of zeros: the scale floor
    x[1] = (x[1].float() * 1e-3).to(BF)
    x[1, cols // 2] = 3.0e38                                        # one huge element
    den = torch.tensor([2.0 ** -130, -2.0 ** -133, 0.0, 2.0 ** -127, -2.0 ** -128, 2.0 ** -131, 0.0, 2.0 ** -129]).to(BF)
    x[2] = den.repeat(cols // 8)                                    # bf16 denormals
    X = KB.Guarded((rows, cols), BF, ld=cols + 8, cols_before=4, device=DEV)
    X.fill(x.to(DEV))
    Q = KB.Guarded((rows, cols), F8, ld=cols + 12, cols_before=4, device=DEV)
    S = _vec(torch.zeros(rows))
    ops.quantize_rows_fp8(X.view, out=Q.view, out_scale=S.view[0])
    torch.cuda.synchronize()
    want_q, want_s = KB.quantize_rows_fp8_ref(x)
    got_q, got_s = _codes(Q.view), S.view[0].cpu()
    assert torch.equal(got_s, want_s), (got_s, want_s)
    diff = (got_q != want_q).nonzero()
    assert diff.shape[0] == 0, f"{diff.shape[0]} codes differ, first at {diff[0].tolist()}: {int(got_q[tuple(diff[0])])} vs {int(want_q[tuple(diff[0])])}"
    for gd in (X, Q, S):
        gd.check(f"quantize_rows_fp8 {rows}x{cols}")


@pytest.mark.parametrize("rows", [1, 5, 333])
@pytest.mark.parametrize("dim", [256, 1536, 5120])
def test_ln_modulate_fp8_per_element(dim, rows):
    """The inputs of the bf16 module's ln_modulate test: batch seams inside a workgroup's rows."""
    g = torch.Generator().manual_seed(dim + rows)
    x = torch.randn(rows, dim, generator=g) * 2 + 0.3
    rpb = 1 if rows == 1 else (3 if rows == 5 else 111)
    nb = (rows + rpb - 1) // rpb
    sc, sh = torch.randn(nb, dim, generator=g) * 0.5, torch.randn(nb, dim, generator=g) * 0.5
    sel = torch.arange(rows) // rpb
    Q = KB.Guarded((rows, dim), F8, device=DEV, rows_before=2, rows_after=4)
    S = _vec(torch.zeros(rows))
    xg = KB.Guarded((rows, dim), torch.float32, device=DEV, rows_before=1, rows_after=4)
    xg.fill(x.to(DEV))
    sg = KB.Guarded((nb, dim), torch.float32, device=DEV); sg.fill(sc.to(DEV))
    hg = KB.Guarded((nb, dim), torch.float32, device=DEV); hg.fill(sh.to(DEV))
    ops.ln_modulate_fp8(xg.view, sg.view, hg.view, True, rpb, 1e-6, out=Q.view, out_scale=S.view[0])
    torch.cuda.synchronize()
    y, bound, s_ref, s_tol = KB.ln_modulate_fp8_bound(x, sc[sel], sh[sel], True, 1e-6)
    s = S.view[0].cpu().double()
    bad = ((s - s_ref).abs() > s_tol).nonzero().flatten().tolist()
    assert not bad, f"ln_modulate_fp8 dim {dim}: row scales of rows {bad[:8]} outside max|y| / 448 +- the fp32 ln term"
    w = KB.assert_within(Q.view.float().cpu().double() * s[:, None], y, bound, f"ln_modulate_fp8 dim {dim} rows {rows} rows_per_batch {rpb}")
    for gd in (Q, S, xg, sg, hg):
        gd.check(f"ln_modulate_fp8 dim {dim} rows {rows}")
    _report(f"ln_modulate_fp8 dim {dim} rows {rows}", w)


def _vt_case(B, H, Lk, seed, extreme=True):
    """V^T [B, C, pad] bf16 (columns [Lk, pad) zero) with rows of very different magnitude, an all-zero block and a block of denormals."""
    g = torch.Generator().manual_seed(seed)
    C, pad = H * 128, ops.round_up(Lk, 64)
    vt = torch.zeros(B, C, pad, dtype=BF)
    vt[:, :, :Lk] = (torch.randn(B, C, Lk, generator=g) * torch.rand(B, C, 1, generator=g) * 4).to(BF)
    if extreme:
        n = min(32, Lk)
        vt[0, 3, :n] = 0.0
        vt[B - 1, 5, :n] = (torch.full((n,), 2.0 ** -130) * (torch.arange(n) % 5 - 2)).to(BF)
        if Lk > 40:
            vt[0, 7, 32:min(64, Lk)] = 0.0
    return vt


def _vt_buffers(vt, H, Lk):
    B, C, pad = vt.shape
    Vt = KB.Guarded((B, C, pad), BF, ld=pad + 8, device=DEV)                     # ldvt > roundup(Lk, 64): NaN beyond
    Vt.fill(vt.to(DEV))
    V8 = KB.Guarded((B, C, pad), F8, ld=pad + 16, device=DEV)
    S8 = _vec(torch.zeros(B * H * (pad // 64) * 256, dtype=U8), U8, aligned=True)
    return Vt, V8, S8


def _vt_quantise_checked(Vt, V8, S8, vt, H, Lk, tag):
    """wan_vt_quantize_mx into the guarded buffers, held with torch.equal against the exact definition.  Returns its de-quantisation."""
    ops.vt_quantize_mx(Vt.view, H, Lk, v8=V8.view, scales=S8.view[0])
    torch.cuda.synchronize()
    want_v8, want_sc, deq = KB.vt_quantize_mx_ref(vt, H, Lk)
    got_sc = S8.view[0].cpu()
    d = (got_sc != want_sc).nonzero()
    assert d.shape[0] == 0, f"{tag}: {d.shape[0]} scale bytes differ, first at {int(d[0])}: {int(got_sc[int(d[0])])} vs {int(want_sc[int(d[0])])}"
    got = _codes(V8.view)
    d = (got != want_v8).nonzero()
    assert d.shape[0] == 0, (f"{tag}: {d.shape[0]} codes differ (batch, channel, stored position) first {d[0].tolist()}: "
                             f"{int(got[tuple(d[0])])} vs {int(want_v8[tuple(d[0])])}")
    for gd in (Vt, V8, S8):
        gd.check(tag)
    return deq


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("Lk", [8, 63, 64, 65, 200])
def test_vt_quantize_mx_is_its_exact_definition(Lk, H):
    B = 2
    vt = _vt_case(B, H, Lk, seed=Lk + H)
    Vt, V8, S8 = _vt_buffers(vt, H, Lk)
    assert S8.view[0].numel() == _lib.load().wan_vt_mx_scale_bytes(B, H, Lk)
    _vt_quantise_checked(Vt, V8, S8, vt, H, Lk, f"vt_quantize_mx B{B} H{H} Lk{Lk}")


def test_rmsnorm_rope_fp8_is_the_e4m3_cast_of_the_bf16_result_in_guard_bands():
    """tests/test_gpu_fp8.py's exact statement with every operand and result in a guard band."""
    g = torch.Generator(device=DEV).manual_seed(5)
    rows, H = 3 * 4 * 6 + 5, 3
    C = H * 128
    wide = KB.Guarded((rows, 2 * C), BF, ld=2 * C + 16, cols_before=8, rows_before=2, rows_after=4, device=DEV)
    wide.fill((torch.randn(rows, 2 * C, device=DEV, generator=g) * 2).bfloat16())
    qk = wide.view
    nq, nk = torch.rand(C, device=DEV, generator=g) + 0.5, torch.rand(C, device=DEV, generator=g) + 0.5
    NQ, NK = _vec(nq), _vec(nk)
    ang = O.rope_angles(128).to(DEV)
    rope = (torch.cos(ang).float().contiguous(), torch.sin(ang).float().contiguous())
    rp = RopeParams(3, 4, 6, 2, 1, 2, 0, rows, ang.shape[0])
    qs = ops.q_prescale(128)
    Q8 = KB.Guarded((rows, C), F8, rows_before=2, rows_after=4, device=DEV)
    K8 = KB.Guarded((rows, C), F8, rows_before=2, rows_after=4, device=DEV)
    before = qk.clone()
    ops.rmsnorm_rope_fp8(qk[:, :C], NQ.view[0], qk[:, C:], NK.view[0], 128, 1e-6, rope, rp, Q8.view, K8.view, x0_scale=qs * 32.0, x1_scale=4.0)
    torch.cuda.synchronize()
    assert torch.equal(qk, before)
    for gd in (wide, NQ, NK, Q8, K8):
        gd.check("rmsnorm_rope_fp8")
    ref = before.clone()
    ops.rmsnorm_rope_(ref[:, :C], nq, ref[:, C:], nk, 128, 1e-6, rope, rp, x0_scale=qs)
    want_q = (ref[:, :C].float() * 32.0).clamp(-448, 448).to(F8)
    want_k = (ref[:, C:].float() * 4.0).clamp(-448, 448).to(F8)
    assert torch.equal(Q8.view.view(U8), want_q.view(U8))
    assert torch.equal(K8.view.view(U8), want_k.view(U8))


@pytest.mark.parametrize("valid", [1, 127, 129, 650])
def test_col_mean_and_qk_quantise_in_guard_bands(valid):
    """The two kernels behind K smoothing.  valid_rows 1 / 127 / 129 leave some of the column mean's 128 row chunks empty.
    Column mean: n fp32 additions in a fixed two-stage order, the rounded 1 / n and one multiply:  |err| <= (n + 4) 2^-24 mean|x|.
    The quantiser: torch's e4m3 cast of the same fp32 values, exactly."""
    g = torch.Generator(device=DEV).manual_seed(9)
    B, Ll, C = 2, 700, 1536
    wide = KB.Guarded((B * Ll, 2 * C), BF, ld=2 * C + 16, cols_before=8, rows_before=2, rows_after=4, device=DEV)
    x = (torch.randn(B * Ll, 2 * C, device=DEV, generator=g) * 1.5 + 0.3).bfloat16()
    x[:, C + 5] += 40.0                                          # a channel with a large common offset
    wide.fill(x)
    qk = wide.view
    k = qk[:, C:]
    need = int(_lib.load().wan_col_mean_workspace_bytes(B, C)) // 4
    WS = _vec(torch.zeros(need), aligned=True)
    Mn = KB.Guarded((B, C), torch.float32, device=DEV)
    ops.col_mean(k, Ll, valid, B, out=Mn.view, workspace=WS.view[0])
    torch.cuda.synchronize()
    mean = Mn.view.clone()
    kd = x[:, C:].double().view(B, Ll, C)[:, :valid]
    want = kd.mean(dim=1)
    bound = (valid + 4) * KB.U_F32 * kd.abs().mean(dim=1) + 2.0 ** -120
    w = KB.assert_within(mean, want.cpu(), bound.cpu(), f"col_mean valid_rows {valid} (rows = samples)")
    ops.col_mean(k, Ll, valid, B, out=Mn.view, workspace=WS.view[0])
    assert torch.equal(mean, Mn.view)
    Q8 = KB.Guarded((B * Ll, C), F8, rows_before=2, rows_after=4, device=DEV)
    K8 = KB.Guarded((B * Ll, C), F8, rows_before=2, rows_after=4, device=DEV)
    ops.qk_quantize_fp8(qk[:, :C], k, Ll, Mn.view, 32.0, 4.0, Q8.view, K8.view)
    torch.cuda.synchronize()
    want_q = (x[:, :C].float() * 32.0).clamp(-448, 448).to(F8)
    want_k = ((x[:, C:].float().view(B, Ll, C) - mean[:, None, :]) * 4.0).clamp(-448, 448).view(-1, C).to(F8)
    assert torch.equal(Q8.view.view(U8), want_q.view(U8))
    assert torch.equal(K8.view.view(U8), want_k.view(U8))
    ops.qk_quantize_fp8(qk[:, :C], k, Ll, None, 32.0, 4.0, Q8.view, K8.view)
    assert torch.equal(K8.view.view(U8), (x[:, C:].float() * 4.0).clamp(-448, 448).to(F8).view(U8))
    for gd in (wide, WS, Mn, Q8, K8):
        gd.check(f"col_mean / qk_quantize_fp8 valid_rows {valid}")
    _report(f"col_mean valid_rows {valid}", w)


# ------------------------------------------------------------------------------------------------ attention
QE, KE = 5, 2
Q_PER_WG = 256           # kQPerWG of videocof_amd/csrc/attn_fwd.hip: the query rows of one workgroup (one max-free verdict each)


def _attn8_buffers(samples, q_idx, Lk, H):
    """samples: one dict of kernel_bounds.decisive_qkv_e4m3 / wide_range_qkv_e4m3 per batch entry; q_idx: the query rows used (or None).
    q8 rows past Lq: NaN (0x7F).  k8 gets 64 more rows: the guard key in every head behind k_len, NaN behind those.  vt columns
    [Lk, roundup(Lk, 64)) zero, NaN beyond.  out: ldo = C + 8."""
    B, C = len(samples), H * 128
    q8 = torch.stack([s["q8"].view(U8) if q_idx is None else s["q8"].view(U8)[q_idx] for s in samples]).reshape(B, -1, C)
    Lq = q8.shape[1]
    Q = KB.Guarded((B, Lq, C), F8, ld=C + 32, cols_before=16, device=DEV)
    _fill8(Q, q8)
    K = KB.Guarded((B, Lk + 64, C), F8, ld=C + 32, cols_before=16, device=DEV)
    kk = torch.stack([torch.cat([s["k8"].reshape(Lk, C).view(U8), s["guard"].view(U8).repeat(H)[None].expand(64, C)]) for s in samples])
    _fill8(K, kk)
    pad = ops.round_up(Lk, 64)
    vt = torch.zeros(B, C, pad, dtype=BF)
    for b, s in enumerate(samples):
        vt[b, :, :Lk] = s["v"].reshape(Lk, C).t()
    Out = KB.Guarded((B, Lq, C), BF, ld=C + 8, device=DEV)
    return Q, K, vt, Out, Lq


def _refs(samples, q_idx, Lk, H, v_of, bound_fn):
    """(ref, bound) [B, Lq, H, 128] from bound_fn per (sample, head); v_of(b, h): that head's V [Lk, 128]."""
    refs, bounds = [], []
    for b, s in enumerate(samples):
        rb, bb = [], []
        for h in range(H):
            r, bd = bound_fn(s["qd"][:, h], s["kd"][:, h], v_of(b, h), Lk)          # on the unique query rows ...
            rb.append(r if q_idx is None else r[q_idx])                              # ... repeated as the call repeats them
            bb.append(bd if q_idx is None else bd[q_idx])
        refs.append(torch.stack(rb, dim=1)); bounds.append(torch.stack(bb, dim=1))
    return torch.stack(refs), torch.stack(bounds)


def _run_qk8(tag, samples, q_idx, Lk, H):
    B = len(samples)
    Q, K, vt, Out, Lq = _attn8_buffers(samples, q_idx, Lk, H)
    Vt = KB.Guarded(tuple(vt.shape), BF, ld=vt.shape[2] + 8, device=DEV)
    Vt.fill(vt.to(DEV))
    ops.attention_fwd_qk8(Q.view, K.view, Vt.view, H, QE, KE, k_len=Lk, out=Out.view, workspace=ops.AttentionWorkspace())
    variant = ops.get_tuning("last_attn_variant")
    torch.cuda.synchronize()
    assert variant & 15 == 4, variant
    ref, bound = _refs(samples, q_idx, Lk, H, lambda b, h: samples[b]["v"][:, h], KB.attention_qk8_bound)
    o = Out.view.float().cpu().reshape(B, Lq, H, 128)
    worst = 0.0
    for b in range(B):
        for h in range(H):
            worst = max(worst, KB.assert_within(o[b, :, h], ref[b, :, h], bound[b, :, h], f"{tag} sample {b} head {h} (rows = queries)"))
    for name, gd in (("q8", Q), ("k8", K), ("vt", Vt), ("out", Out)):
        gd.check(f"{tag} {name}")
    _report(tag, worst)
    return variant


def _run_f8(tag, samples, q_idx, Lk, H, tail_from=None, all_redone=False):
    """wan_attention_fwd_f8 judged per workgroup: every group of 256 query rows of a (sample, head) lies entirely inside the f8 bound
    (de-quantised V: the max-free attempt held) or entirely inside the qk8 bound (bf16 V: it was redone by the fp8-QK^T lazy kernel);
    the groups that satisfy only the second may not outnumber scratch header word [1].  tail_from: first query block of the split-KV
    tail round, which runs the fp8-QK^T form on the bf16 V by design and is not counted by the header: its groups must lie inside the
    qk8 bound.  all_redone: the case is built so that EVERY workgroup fails its max-free check -- header word [1] must equal the number
    of groups and every group must lie inside the qk8 bound (the f8 bound's 2^-4 p |v| is as wide as the e4m3 rounding of V, so a redone
    group usually lies inside the f8 bound as well and "inside the qk8 bound only" alone would constrain nothing there).
    How word [1] is counted (attn_fwd.hip): the attempt's workgroup 0 clears it, every workgroup of the FIX-UP launch whose flag is set
    adds one; when more than an eighth of a launch was redone the fix-up also sets the sticky word [0], which makes the attempt of LATER
    calls on the same scratch flag every workgroup without computing -- those are still counted by their fix-up.  Every case here
    uses a fresh workspace, so the attempt really runs.  Returns (variant, redone, only_qk8)."""
    B = len(samples)
    Q, K, vt, Out, Lq = _attn8_buffers(samples, q_idx, Lk, H)
    Vt, V8, S8 = _vt_buffers(vt, H, Lk)
    deq = _vt_quantise_checked(Vt, V8, S8, vt, H, Lk, tag + " vt_quantize_mx")             # the key order of v8, bit for bit
    site = ops.AttentionWorkspace()
    ops.attention_fwd_f8(Q.view, K.view, V8.view, S8.view[0], Vt.view, H, QE, KE, k_len=Lk, out=Out.view, workspace=site)
    variant = ops.get_tuning("last_attn_variant")
    torch.cuda.synchronize()
    assert variant & 15 == 5, variant
    redone = int(site.buf[:16].view(torch.int32)[1])
    ref8, bound8 = _refs(samples, q_idx, Lk, H, lambda b, h: samples[b]["v"][:, h], KB.attention_qk8_bound)
    reff, boundf = _refs(samples, q_idx, Lk, H, lambda b, h: deq[b, h * 128:(h + 1) * 128, :Lk].t(), KB.attention_f8_bound)
    o = Out.view.float().cpu().reshape(B, Lq, H, 128).double()
    assert bool(torch.isfinite(o).all()), f"{tag}: non-finite outputs"
    rf, r8 = (o - reff).abs() / boundf.clamp_min(1e-300), (o - ref8).abs() / bound8.clamp_min(1e-300)
    only_qk8, worst_f, worst_8, groups = 0, 0.0, 0.0, 0
    for b in range(B):
        for h in range(H):
            for g0 in range(0, Lq, Q_PER_WG):
                sl = slice(g0, min(g0 + Q_PER_WG, Lq))
                wf, w8 = float(rf[b, sl, h].max()), float(r8[b, sl, h].max())
                groups += 1
                if all_redone or (tail_from is not None and g0 // Q_PER_WG >= tail_from):        # computed on the bf16 V: the qk8 bound
                    worst_8 = max(worst_8, KB.assert_within(o[b, sl, h], ref8[b, sl, h], bound8[b, sl, h],
                                                            f"{tag} sample {b} head {h} query rows {sl.start}-{sl.stop - 1} (redone / tail group); qk8 bound"))
                    continue
                if wf <= 1.0:
                    worst_f = max(worst_f, wf)
                elif w8 <= 1.0:
                    worst_8 = max(worst_8, w8)
                    if tail_from is None or g0 // Q_PER_WG < tail_from:
                        only_qk8 += 1
                else:                                    # neither: let the f8 bound name the rows
                    KB.assert_within(o[b, sl, h], reff[b, sl, h], boundf[b, sl, h],
                                     f"{tag} sample {b} head {h} query rows {sl.start}-{sl.stop - 1} (inside neither bound; vs qk8 bound {w8:.3g}); f8 bound")
    for name, gd in (("q8", Q), ("k8", K), ("vt", Vt), ("v8", V8), ("v8 scales", S8), ("out", Out)):
        gd.check(f"{tag} {name}")
    print(f"[redone] {tag}: header word [1] = {redone}, workgroups inside the qk8 bound only = {only_qk8}")
    assert only_qk8 <= redone, (tag, only_qk8, redone)
    if all_redone:
        assert redone == groups, (tag, redone, groups)
    else:
        _report(tag + " (f8 bound)", worst_f)
    if worst_8:
        _report(tag + " (redone / tail groups, qk8 bound)", worst_8)
    return variant, redone, only_qk8


ATTN_L = [8, 63, 64, 65, 191, 192, 193, 1025]
KERNELS = ["qk8", "f8"]


def _decisive(B, L, H, seed):
    return [KB.decisive_qkv_e4m3(L, H, seed + 1000 * b, QE, KE) for b in range(B)]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("L", ATTN_L)
def test_fp8_attention_decisive_keys_per_element(L, kernel):
    """Lq = Lk around the 64-key tile and at 1025: key i decides row i on the e4m3 operands, the guard key waits behind the last one."""
    i = ATTN_L.index(L) + KERNELS.index(kernel)
    B, H = 1 + i % 2, (1, 3, 5)[i % 3]
    samples = _decisive(B, L, H, seed=L)
    tag = f"attention_{kernel} decisive B{B} H{H} L{L}"
    if kernel == "qk8":
        _run_qk8(tag, samples, None, L, H)
    else:
        _, redone, _ = _run_f8(tag, samples, None, L, H)
        assert redone == 0, redone                       # scores <= 15 in log2 units: the max-free attempt holds


@pytest.mark.parametrize("kernel", KERNELS)
def test_fp8_attention_more_queries_than_keys(kernel):
    Lq, Lk, H = 257, 8, 3
    samples = _decisive(1, Lk, H, seed=257)
    (_run_qk8 if kernel == "qk8" else _run_f8)(f"attention_{kernel} Lq{Lq} Lk{Lk} H{H}", samples, torch.arange(Lq) % Lk, Lk, H)


@pytest.mark.parametrize("tail", [1, 0])
@pytest.mark.parametrize("kernel", KERNELS)
def test_fp8_attention_split_tail_decisive_keys(kernel, tail):
    """87 query blocks x 3 heads = 261 workgroups = one round + 5: the last 2 query blocks run split over the keys + a merge
    (attn_tail = 1; the fp8-QK^T form on the bf16 V for both kernels) or as a second round (0).  The queries repeat the 1100 decisive
    rows, so reference and bound are evaluated once per unique row and every row of the call is judged."""
    Lq, Lk, H = 86 * 256 + 10, 1100, 3
    samples = _decisive(1, Lk, H, seed=9)
    q_idx = torch.arange(Lq) % Lk
    ops.set_tuning("attn_tail", tail)
    try:
        tag = f"attention_{kernel} split tail={tail}"
        if kernel == "qk8":
            variant = _run_qk8(tag, samples, q_idx, Lk, H)
        else:
            variant, _, _ = _run_f8(tag, samples, q_idx, Lk, H, tail_from=85 if tail else None)
    finally:
        ops.set_tuning("attn_tail", 1)
    assert bool(variant & _lib.ATTN_VARIANT_SPLIT_TAIL) == bool(tail), variant


@pytest.mark.parametrize("kernel", KERNELS)
def test_fp8_attention_wide_range_rows(kernel):
    """One key at +20 log2 units, whole 32-key blocks at -96 ... -128: MX blocks of P whose sums are 116 - 148 binades below the row's
    largest probability, denormal or zero (scale word 0) in the max-free form."""
    Lq, Lk = 300, 520
    samples = [KB.wide_range_qkv_e4m3(Lq, Lk, seed=31, q_exp=QE, k_exp=KE)]
    (_run_qk8 if kernel == "qk8" else _run_f8)(f"attention_{kernel} wide range Lq{Lq} Lk{Lk}", samples, None, Lk, 1)


@pytest.mark.parametrize("kernel", KERNELS)
def test_fp8_attention_heavy_key_half_without_v(kernel):
    """The two MX blocks of a 64-key tile 2^10 ... 2^15 apart in mass, the heavy one with V = 0 (tile 0: key half 0, tile 1: key half 1):
    the output is carried by the light halves.  A P scale taken per 64-key tile instead of per 32-key block flushes their probabilities
    to e4m3 subnormals of the tile scale and falls outside in every row (tests/test_fp8_bounds_host.py shows it on the emulation)."""
    Lq, Lk = 300, 200
    samples = [KB.heavy_half_qkv_e4m3(Lq, Lk, seed=41, q_exp=QE, k_exp=KE)]
    tag = f"attention_{kernel} heavy key half without V Lq{Lq} Lk{Lk}"
    if kernel == "qk8":
        _run_qk8(tag, samples, None, Lk, 1)
    else:
        _, redone, _ = _run_f8(tag, samples, None, Lk, 1)
        assert redone == 0, redone                       # scores <= 25: the max-free attempt holds, so the f8 P path is what is judged


@pytest.mark.parametrize("kernel", KERNELS)
def test_fp8_attention_large_scores_force_the_redo(kernel):
    """q std 30: exp2-domain scores of +-100 and more.  The lazy reference has to be repaired (qk8); every workgroup of the all-fp8
    kernel fails its max-free check and is redone by the fp8-QK^T lazy kernel on the bf16 V."""
    Lq, Lk, H = 300, 1000, 2
    g = torch.Generator().manual_seed(30)
    c = 128 ** -0.5 * KB.LOG2E
    qp = (torch.randn(Lq, H, 128, generator=g) * 30 * c).to(BF)
    k = torch.randn(Lk, H, 128, generator=g).to(BF)
    v = (torch.randn(Lk, H, 128, generator=g) + torch.linspace(-1, 1, 128)).to(BF)
    qp[..., 0], k[..., 0] = 1.0, 0.0                                     # the guard channel: score 64 with the key behind k_len
    q8 = (qp.float() * 2.0 ** QE).clamp(-448, 448).to(F8)
    k8 = (k.float() * 2.0 ** KE).clamp(-448, 448).to(F8)
    guard = torch.zeros(128)
    guard[0] = 256.0
    s = dict(q8=q8, k8=k8, v=v, guard=guard.to(F8), qd=KB.dq_pow2(q8, QE), kd=KB.dq_pow2(k8, KE))
    tag = f"attention_{kernel} q std 30 Lq{Lq} Lk{Lk} H{H}"
    if kernel == "qk8":
        _run_qk8(tag, [s], None, Lk, H)
    else:
        _run_f8(tag, [s], None, Lk, H, all_redone=True)
