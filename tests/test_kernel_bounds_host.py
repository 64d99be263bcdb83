"""The bounds of tests/kernel_bounds.py checked on the CPU: honest emulations of the kernels' arithmetic (bf16 operands, fp32
accumulation in several orders, one rounding) stay inside, every mutant a rel-L2 limit lets through is rejected and the failure
names the right rows.  A constant loosened later fails here, without a GPU."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_bounds as KB  # noqa: E402

BF = torch.bfloat16


def bf(x):
    return x.to(BF)


def _operands(M, N, K, seed=None):
    g = torch.Generator().manual_seed(M + N + K if seed is None else seed)
    a, w = bf(torch.randn(M, K, generator=g)), bf(torch.randn(N, K, generator=g) * 0.1)
    bias = torch.randn(N, generator=g) * 0.5
    return a, w, bias


def _acc_f32(a, w, bias, chunk, reverse=False):
    """fp32 accumulation of exact bf16 products, K cut into `chunk`-wide pieces summed forward or backward, bias last."""
    K = a.shape[1]
    acc = torch.zeros(a.shape[0], w.shape[0])
    starts = list(range(0, K, chunk))
    for k0 in (reversed(starts) if reverse else starts):
        acc = acc + a[:, k0:k0 + chunk].float() @ w[:, k0:k0 + chunk].float().t()
    return acc + bias if bias is not None else acc


def _truncate_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def _gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


@pytest.mark.parametrize("M,N,K", [(1100, 520, 512), (3000, 1164, 384), (2304, 1536, 896), (129, 1536, 192), (255, 260, 64)])
def test_honest_gemm_emulations_stay_inside(M, N, K):
    a, w, bias = _operands(M, N, K)
    ref = KB.gemm_ref(a, w, bias)
    acc_term = KB.gemm_acc_term(a, w, bias, K)
    b16 = KB.gemm_bound(a, w, bias, K, BF, ref, acc_term)
    b32 = KB.gemm_bound(a, w, bias, K, torch.float32, ref, acc_term)
    g_ref, g_bound = KB.gelu_bound(ref, acc_term)
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(M, N, generator=g) * (10.0 ** torch.randint(-3, 3, (M, 1), generator=g).float())
    gate = torch.randn(2, N, generator=g)
    gate_rows = gate[torch.arange(M) // ((M + 1) // 2)]
    r_ref, r_bound = KB.resid_bound(ref, acc_term, gate_rows, x0)
    worst16 = worst32 = 0.0
    for chunk, rev in ((32, False), (64, False), (128, True), (K, False), (64, True)):
        acc = _acc_f32(a, w, bias, chunk, rev)
        worst16 = max(worst16, KB.assert_within(bf(acc), ref, b16, f"bf16 chunk {chunk}"))
        worst32 = max(worst32, KB.assert_within(acc, ref, b32, f"fp32 chunk {chunk}"))
        x = acc
        KB.assert_within(bf(0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))), g_ref, g_bound, "gelu")
        KB.assert_within(x0 + acc * gate_rows, r_ref, r_bound, "resid")
        KB.assert_within(torch.addcmul(x0, acc, gate_rows), r_ref, r_bound, "resid fma")
    assert 0.5 < worst16 <= 1.0 and worst32 < 0.05, (worst16, worst32)       # the half-ulp term is sharp; fp32 far inside


@pytest.fixture(scope="module")
def case():
    M, N, K = 3000, 1164, 384
    a, w, bias = _operands(M, N, K)
    ref = KB.gemm_ref(a, w, bias)
    acc_term = KB.gemm_acc_term(a, w, bias, K)
    acc = _acc_f32(a, w, bias, 64)
    return dict(M=M, N=N, K=K, a=a, w=w, bias=bias, ref=ref, acc_term=acc_term, acc=acc, good=bf(acc),
                bound=KB.gemm_bound(a, w, bias, K, BF, ref, acc_term))


def _rel_l2(x, ref):
    return float((x.double() - ref).norm() / ref.norm())


def test_truncation_mutant_is_rejected(case):
    out = _truncate_bf16(case["acc"])
    assert _rel_l2(out, case["ref"]) < 4e-3                       # the old limit lets it through
    with pytest.raises(AssertionError, match=r"rows 0-2999, cols 0-1163") as e:
        KB.assert_within(out, case["ref"], case["bound"], "truncation")
    n = int(str(e.value).split(": ")[1].split(" of ")[0])
    # every element whose dropped bits exceed half an ulp (+ the accumulation slack): 457 507 of 3 492 000 on the operands this
    # count was first taken with; the seed moves it by a fraction of a percent, a drifted bound or emulation by far more
    assert 440000 < n < 475000, n


def test_gelu_mutants_are_rejected(case):
    g_ref, g_bound = KB.gelu_bound(case["ref"], case["acc_term"])
    x = case["acc"]
    honest = 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    KB.assert_within(bf(honest), g_ref, g_bound, "tanh gelu")
    # the kernel's own formulation x / (1 + 2^a) in fp32
    k1 = -2.0 * 0.7978845608028654 * 1.4426950408889634
    sig = x * (1.0 / (1.0 + torch.exp2((x * x * (k1 * 0.044715) + k1) * x)))
    KB.assert_within(bf(sig), g_ref, g_bound, "sigmoid-form gelu")
    # erf-GELU differs from the tanh form by at most 4.8e-4 (near |x| = 2.2).  At K = 384 the accumulation term of this case is
    # ~1.1e-3 per element -- the fp32 sum itself may be that far off -- so no bound that admits every honest order can tell the two
    # apart here; it can at K = 64 (term ~3e-5).  At K = 384 the erf form is rejected by the second check below (gelu_from_acc_bound).
    erf = bf(_gelu_erf(x))
    assert _rel_l2(erf, g_ref) < 5e-3
    a2, w2, bias2 = _operands(1100, 520, 64)
    ref2, term2 = KB.gemm_ref(a2, w2, bias2), KB.gemm_acc_term(a2, w2, bias2, 64)
    g2_ref, g2_bound = KB.gelu_bound(ref2, term2)
    x2 = _acc_f32(a2, w2, bias2, 32)
    KB.assert_within(bf(KB.gelu_tanh(x2).float()), g2_ref, g2_bound, "tanh gelu, K = 64")
    assert _rel_l2(bf(_gelu_erf(x2)), g2_ref) < 5e-3                # the old limit lets it through
    with pytest.raises(AssertionError, match="outside the bound"):
        KB.assert_within(bf(_gelu_erf(x2)), g2_ref, g2_bound, "erf gelu")
    with pytest.raises(AssertionError, match="outside the bound"):
        KB.assert_within(_truncate_bf16(honest), g_ref, g_bound, "truncated gelu")
    # ... and at (3000, 1164, 384) itself by the second check, against g of the kernel's own fp32 accumulator (here: the emulation's)
    a_ref, a_bound = KB.gelu_from_acc_bound(x)
    KB.assert_within(bf(honest), a_ref, a_bound, "tanh gelu vs own accumulator")
    KB.assert_within(bf(sig), a_ref, a_bound, "sigmoid-form gelu vs own accumulator")
    with pytest.raises(AssertionError, match="outside the bound") as e:
        KB.assert_within(erf, a_ref, a_bound, "erf gelu vs own accumulator")
    assert int(str(e.value).split(": ")[1].split(" of ")[0]) > 100000                  # not a marginal rejection
    with pytest.raises(AssertionError, match="outside the bound"):
        KB.assert_within(_truncate_bf16(honest), a_ref, a_bound, "truncated gelu vs own accumulator")


def test_tile_and_store_mutants_are_rejected_and_named(case):
    a, w, ref, bound, good = case["a"], case["w"], case["ref"], case["bound"], case["good"]
    # one 16x16 MFMA sub-tile misses one 32-wide K step
    acc = case["acc"].clone()
    acc[2944:2960, 1136:1152] -= a[2944:2960, 96:128].float() @ w[1136:1152, 96:128].float().t()
    assert _rel_l2(bf(acc), ref) < 4e-3
    with pytest.raises(AssertionError, match=r"rows 2944-2959, cols 1136-1151"):
        KB.assert_within(bf(acc), ref, bound, "sub-tile")
    # one 8-element row segment stored from the neighbouring row
    out = good.clone()
    out[1501, 640:648] = good[1500, 640:648]
    assert _rel_l2(out, ref) < 4e-3
    with pytest.raises(AssertionError, match=r"rows 1501-1501, cols 64\d-647"):
        KB.assert_within(out, ref, bound, "row segment")
    # 8 scattered elements stored as zero
    g = torch.Generator().manual_seed(3)
    cand = (ref.abs() > 0.5).nonzero()
    pick = cand[torch.randperm(cand.shape[0], generator=g)[:8]]
    out = good.clone()
    out[pick[:, 0], pick[:, 1]] = 0
    assert _rel_l2(out, ref) < 4e-3
    with pytest.raises(AssertionError, match=r"^zeroed: 8 of "):
        KB.assert_within(out, ref, bound, "zeroed")
    # rows m and m + 1 swapped
    out = good.clone()
    out[[2047, 2048]] = good[[2048, 2047]]
    with pytest.raises(AssertionError, match=r"rows 2047-2048, cols "):
        KB.assert_within(out, ref, bound, "rows swapped")
    # the bias of the last 4-column group taken from the group before
    b2 = case["bias"].clone()
    b2[-4:] = case["bias"][-8:-4]
    out = bf(_acc_f32(a, w, b2, 64))
    with pytest.raises(AssertionError, match=r"cols 116\d-1163"):
        KB.assert_within(out, ref, bound, "bias group")
    # one element off by two bf16 ulps
    out = good.clone()
    out.view(torch.int16)[777, 333] += 2
    with pytest.raises(AssertionError, match=r"^two ulps: 1 of .*rows 777-777, cols 333-333"):
        KB.assert_within(out, ref, bound, "two ulps")
    # NaN is a violation, not a pass
    out = good.clone()
    out[5, 7] = float("nan")
    with pytest.raises(AssertionError, match=r"rows 5-5, cols 7-7"):
        KB.assert_within(out, ref, bound, "nan")
    KB.assert_within(good, ref, bound, "honest")


# ------------------------------------------------------------------------------------------------ attention
def _attn_emulated(q, k, v, scale, k_len=None, p_dtype=BF):
    """The kernels' arithmetic: fp32 scores and exponentials, l from the fp32 p, P rounded to bf16 for P.V, fp32 sums, one rounding."""
    if k_len is not None:
        k, v = k[:k_len], v[:k_len]
    s = (q.float() @ k.float().t()) * (scale * 1.4426950408889634)
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    l = p.sum(dim=-1, keepdim=True)
    return bf((p.to(p_dtype).float() @ v.float()) / l)


def test_honest_attention_emulation_stays_inside():
    g = torch.Generator().manual_seed(0)
    Lq, Lk = 300, 1000
    scale = 128 ** -0.5
    for qs in (1.0, 3.0):
        q, k = bf(torch.randn(Lq, 128, generator=g) * qs), bf(torch.randn(Lk, 128, generator=g))
        v = bf(torch.randn(Lk, 128, generator=g) + torch.arange(128) * 0.01)
        ref, bound = KB.attention_bound(q, k, v, scale)
        worst = KB.assert_within(_attn_emulated(q, k, v, scale), ref, bound, "random attention")
        assert worst <= 1.0
        ref, bound = KB.attention_bound(q, k, v, scale, 937)
        KB.assert_within(_attn_emulated(q, k, v, scale, 937), ref, bound, "random attention, k_len")
        ref, bound = KB.attention_bound(q, k, v, scale)
        for nsplit in (1, 3, 16):
            w2 = KB.assert_within(_attn_emulated_tiled(q, k, v, scale, nsplit), ref, bound, f"tiled lazy reference, {nsplit} splits")
            assert w2 <= 1.0
        KB.assert_within(_attn_emulated_tiled(q, k, v, scale, 2, window=1.5), ref, bound, "tiled, reference raised often")
        # P TRUNCATED to bf16 (output still rounded to nearest): on broad random rows p @ |v| >> |ref| and the one-sided loss
        # of ~0.7 2^-8 stays inside c = 1 -- stated, not hidden; the decisive-key inputs below are where it shows
        KB.assert_within(_attn_p_truncated(q, k, v, scale), ref, bound, "P truncated, random inputs: not visible")


def _attn_p_truncated(q, k, v, scale):
    s = (q.float() @ k.float().t()) * (scale * 1.4426950408889634)
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    return bf((_truncate_bf16(p).float() @ v.float()) / p.sum(dim=-1, keepdim=True))           # output rounded to nearest even


def _attn_emulated_tiled(q, k, v, scale, nsplit=1, window=2.0 ** 16):
    """The kernels' bookkeeping rather than a one-shot softmax: 64-key tiles, a LAZY reference (the row max of a split's first tile,
    raised -- O and l rescaled -- only when a tile's p leaves the window, so p may exceed 1), P rounded to bf16 per tile, fp32 O and
    l; `nsplit` key ranges merged as attn_combine_kernel does (w_s = 2^(m_s - M), num / den)."""
    c = scale * 1.4426950408889634
    Lk = k.shape[0]
    tiles = [(t, min(t + 64, Lk)) for t in range(0, Lk, 64)]
    per = (len(tiles) + nsplit - 1) // nsplit
    parts = []
    for sp in range(0, len(tiles), per):
        m = O = l = None
        for t0, t1 in tiles[sp:sp + per]:
            st = (q.float() @ k[t0:t1].float().t()) * c
            if m is None:
                m = st.max(dim=-1, keepdim=True).values
                O, l = torch.zeros(q.shape[0], v.shape[1]), torch.zeros(q.shape[0], 1)
            over = (st - m).max(dim=-1, keepdim=True).values > math.log2(window)
            m_new = torch.where(over, torch.maximum(m, st.max(dim=-1, keepdim=True).values), m)
            alpha = torch.exp2(m - m_new)
            m = m_new
            p = torch.exp2(st - m)
            O = O * alpha + bf(p).float() @ v[t0:t1].float()
            l = l * alpha + p.sum(dim=-1, keepdim=True)
        parts.append((m, O, l))
    M = torch.stack([m for m, _, _ in parts]).max(dim=0).values
    num = sum(O * torch.exp2(m - M) for m, O, _ in parts)
    den = sum(l * torch.exp2(m - M) for m, _, l in parts)
    return bf(num / den)


def _gross_rows(out, ref, bound):
    """Rows in which more than half of the elements violate.  A softer statement than "row L - 1 and no other": a lost key also
    grazes the rows it held a little mass of, and the bound is tight enough to see that, so the failure message's row range starts
    wherever the first grazed row is (the regex below pins only its end).  What is pinned exactly is the set of GROSS rows."""
    bad = ~((out.double() - ref).abs() <= bound)
    return (bad.sum(dim=-1) > bad.shape[-1] // 2).nonzero().flatten().tolist()


@pytest.mark.parametrize("L", [191, 640, 1025])
def test_decisive_key_inputs_expose_single_key_mutants(L):
    scale = 128 ** -0.5
    q, k, v, t = KB.decisive_qkv(L, 1, seed=L)
    q, k, v = q[:, 0], k[:, 0], v[:, 0]
    ref, bound = KB.attention_bound(q, k, v, scale)
    p = KB.attention_ref(q, k, v, scale)[1]
    assert 0.5 <= float(p.diagonal().min()) and float(p.diagonal().max()) <= 0.99
    KB.assert_within(_attn_emulated(q, k, v, scale), ref, bound, "decisive, honest")
    for nsplit in (1, 4, 16):
        KB.assert_within(_attn_emulated_tiled(q, k, v, scale, nsplit), ref, bound, f"decisive, tiled lazy reference, {nsplit} splits")
    # a truncating P conversion (output still rounded to nearest) is NOT rejected, here or on random inputs: its loss is at most
    # 2^-7 of one p_j, the bound grants 2^-8 for P plus 2^-8 for the output, and a row whose decisive p sits at the top of its
    # truncation interval is rare.  Known blind spot of c = 1 (docs/TEST_BOUNDS.md); the ratio moves from ~0.5 towards 1.
    w_trunc = KB.assert_within(_attn_p_truncated(q, k, v, scale), ref, bound, "P truncated, decisive inputs")
    assert w_trunc > KB.assert_within(_attn_emulated(q, k, v, scale), ref, bound, "decisive, honest")
    # the last key dropped: row L - 1 is grossly wrong and no other (rows that held a little of its mass are grazed)
    with pytest.raises(AssertionError, match=rf"rows \d+-{L - 1}, "):
        KB.assert_within(_attn_emulated(q, k, v, scale, L - 1), ref, bound, "last key dropped")
    assert _gross_rows(_attn_emulated(q, k, v, scale, L - 1), ref, bound) == [L - 1]
    # one padding key admitted: the row of k behind the last key as the GPU tests lay it out (KB.heavy_key), value 0
    k_ext = torch.cat([k, KB.heavy_key()[None]])
    v_ext = torch.cat([v, torch.zeros(1, 128, dtype=BF)])
    with pytest.raises(AssertionError, match=rf"rows 0-{L - 1}, "):
        KB.assert_within(_attn_emulated(q, k_ext, v_ext, scale), ref, bound, "padding key admitted")
    # keys 64 j - 1 and 64 j swapped (k only: the tile seam hands a key the neighbour's value)
    j = 64 * (L // 128 + 1)
    if j < L:
        k_sw = k.clone()
        k_sw[[j - 1, j]] = k[[j, j - 1]]
        with pytest.raises(AssertionError, match="outside the bound"):
            KB.assert_within(_attn_emulated(q, k_sw, v, scale), ref, bound, "keys swapped at a tile edge")
        assert _gross_rows(_attn_emulated(q, k_sw, v, scale), ref, bound) == [j - 1, j]
    # a key duplicated at a tile edge (key j counted twice)
    if j < L:
        k_dup, v_dup = torch.cat([k, k[j:j + 1]]), torch.cat([v, v[j:j + 1]])
        with pytest.raises(AssertionError, match="outside the bound"):
            KB.assert_within(_attn_emulated(q, k_dup, v_dup, scale), ref, bound, "key duplicated")


def test_random_inputs_do_not_expose_a_padding_key_but_the_guard_key_does():
    """The hole the decisive inputs close: on unit-variance inputs an admitted zero key changes nothing a bound can see."""
    g = torch.Generator().manual_seed(2)
    q, k, v = (bf(torch.randn(n, 128, generator=g)) for n in (300, 1000, 1000))
    scale = 128 ** -0.5
    ref, bound = KB.attention_bound(q, k, v, scale)
    zero_key = torch.cat([k, torch.zeros(1, 128, dtype=BF)]), torch.cat([v, torch.zeros(1, 128, dtype=BF)])
    KB.assert_within(_attn_emulated(q, *zero_key, scale), ref, bound, "zero pad key: invisible")     # passes -- that is the point
    q[:, 0] = 1.0
    k[:, 0] = 0.0
    ref, bound = KB.attention_bound(q, k, v, scale)
    heavy = torch.cat([k, KB.heavy_key()[None]]), zero_key[1]
    with pytest.raises(AssertionError, match=r"rows 0-299, "):
        KB.assert_within(_attn_emulated(q, *heavy, scale), ref, bound, "heavy pad key")


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("dim", [256, 1536, 5120, 640])
def test_honest_row_kernel_emulations_stay_inside(dim):
    g = torch.Generator().manual_seed(dim)
    rows = 37
    x = torch.randn(rows, dim, generator=g) * 2 + 0.3
    sc, sh = torch.randn(rows, dim, generator=g) * 0.5, torch.randn(rows, dim, generator=g) * 0.5
    ref, bound = KB.ln_modulate_bound(x, sc, sh, True, 1e-6)
    mean = x.mean(dim=-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + 1e-6)
    y = (x - mean) * rstd * (1 + sc) + sh
    assert KB.assert_within(bf(y), ref, bound, "ln_modulate") <= 1.0
    with pytest.raises(AssertionError):
        KB.assert_within(_truncate_bf16(y), ref, bound, "ln_modulate truncated")
    bad = bf(y).clone()
    bad[20] = bf((x[20] - mean[20]) * rstd[20] * (1 + sc[21]) + sh[21])             # the batch seam one row late
    with pytest.raises(AssertionError, match=r"rows 20-20, "):
        KB.assert_within(bad, ref, bound, "ln_modulate seam")
    # RMSNorm + rotation
    xb = bf(torch.randn(rows, dim, generator=g))
    w = torch.rand(dim, generator=g) + 0.5
    ang = torch.rand(rows, 64, generator=g, dtype=torch.float64) * 6.0
    cos, sin = ang.cos(), ang.sin()
    ref, bound = KB.rmsnorm_rope_bound(xb, w, 1e-6, 0.1275, (cos, sin))
    yf = xb.float() * torch.rsqrt(xb.float().pow(2).mean(dim=-1, keepdim=True) + 1e-6) * w * 0.1275
    yh = yf.view(rows, dim // 128, 64, 2)
    c32, s32 = cos.float()[:, None, :], sin.float()[:, None, :]
    rot = torch.stack([yh[..., 0] * c32 - yh[..., 1] * s32, yh[..., 0] * s32 + yh[..., 1] * c32], dim=-1).reshape(rows, dim)
    assert KB.assert_within(bf(rot), ref, bound, "rmsnorm_rope") <= 1.0
    with pytest.raises(AssertionError):
        KB.assert_within(_truncate_bf16(rot), ref, bound, "rmsnorm_rope truncated")
    rot2 = rot.clone()
    # a row rotated by its neighbour's angle
    yh12 = yh[11]
    rot2[11] = torch.stack([yh12[..., 0] * c32[12] - yh12[..., 1] * s32[12], yh12[..., 0] * s32[12] + yh12[..., 1] * c32[12]], dim=-1).reshape(dim)
    with pytest.raises(AssertionError, match=r"rows 11-11, "):
        KB.assert_within(bf(rot2), ref, bound, "rope angle of the next row")
    ref, bound = KB.rmsnorm_rope_bound(xb, w, 1e-6)
    KB.assert_within(bf(xb.float() * torch.rsqrt(xb.float().pow(2).mean(dim=-1, keepdim=True) + 1e-6) * w), ref, bound, "rmsnorm")


# ------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_guarded_catches_single_bytes(dtype):
    gd = KB.Guarded((5, 12), dtype, ld=16, rows_before=2, rows_after=3, cols_before=0)
    assert gd.view.shape == (5, 12) and gd.view.stride(0) == 16 and torch.isnan(gd.view.float()).all()
    gd.fill(torch.ones(5, 12))
    gd.check()
    raw8 = gd.raw.view(torch.uint8)
    esz = gd.esize
    row_bytes = 16 * esz
    # one byte, one element past the end of row 1
    off = (2 + 1) * row_bytes + 12 * esz
    keep = int(raw8.view(-1)[off])
    raw8.view(-1)[off] = keep ^ 0x40
    with pytest.raises(AssertionError, match=r"rows 1-1 of 5, cols 12-12 of 12"):
        gd.check()
    raw8.view(-1)[off] = keep
    gd.check()
    # one byte, one row past the last
    off = (2 + 5) * row_bytes + 3 * esz + (esz - 1)
    keep = int(raw8.view(-1)[off])
    raw8.view(-1)[off] = 0
    with pytest.raises(AssertionError, match=r"rows 5-5 of 5, cols 3-3 of 12"):
        gd.check()
    raw8.view(-1)[off] = keep
    # the row before the first, and a column left of the view
    gl = KB.Guarded((2, 4, 8), dtype, ld=24, rows_before=1, rows_after=1, cols_before=8)
    assert gl.view.shape == (2, 4, 8)
    gl.view.zero_()
    gl.check()
    keep = gl.raw.clone()
    gl.raw.view(dtype)[1, 0, 9] = 0.0
    with pytest.raises(AssertionError, match=r"batch 1-1, rows -1--1 of 4, cols 1-1 of 8"):
        gl.check()
    gl.raw.copy_(keep)
    gl.raw.view(dtype)[0, 2, 7] = 1.0
    with pytest.raises(AssertionError, match=r"batch 0-0, rows 1-1 of 4, cols -1--1 of 8"):
        gl.check()
