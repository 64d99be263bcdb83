"""-m gpu: the kernels of the umT5 text encoder -- rmsnorm_rows_kernel<NV, OUT_F32>, t5_softmax_bias_kernel, the blockIdx.y form of
the 128x128 GEMM (wan_gemm_bf16_batched), mul_bf16_kernel, embedding_rows_kernel -- judged PER ELEMENT against fp64 references under the
derived bounds of tests/kernel_bounds.py (docs/TEST_BOUNDS.md, "The text encoder"), every operand and result inside poisoned guard bands,
and the encoder's exact invariants (masked ids, internal padding, batch neighbours) with torch.equal.

tests/test_gpu_t5.py holds these kernels to whole-tensor rel-L2 limits at a handful of shapes; tests/test_t5_bounds_host.py shows what
those let through.  Every comparison prints its worst |err| / bound; the limit is 1.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_bounds as KB  # noqa: E402
from oracle.gen_golden_t5 import TINY  # noqa: E402
from videocof_amd import _lib, ops  # noqa: E402
from videocof_amd.wan_text_encoder import WanT5EncoderModel, relative_position_buckets  # noqa: E402
from videocof_amd.weights import deterministic_t5_state_dict, random_t5_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32
EPS = 1e-6
NB = 32


def _report(tag, worst):
    print(f"[bound] {tag}: worst |err|/bound = {worst:.3f}")
    return worst


def _guarded(t, **kw):
    """A 2-D tensor copied into the interior of a poisoned device buffer -> (Guarded, view)."""
    gd = KB.Guarded(tuple(t.shape), t.dtype, device=DEV, **kw)
    return gd, gd.fill(t.to(DEV))


# ------------------------------------------------------------------------------------------------ rmsnorm_rows
# NV = ceil(dim / 1024) float4 chunks per thread: 4, 8, 1000, 1024 -> 1; 1028 -> 2 with ONE lane in the second chunk; 2052 -> 3 ... 7172 -> 8,
# each with a ragged last chunk; 4096 and 8192 the full ones
RMS_DIMS = [4, 8, 1000, 1024, 1028, 2052, 3076, 4096, 4100, 5124, 6148, 7172, 8192]


@pytest.mark.parametrize("rows", [3, 67])
@pytest.mark.parametrize("dim", RMS_DIMS)
def test_rmsnorm_rows_per_element(dim, rows):
    g = torch.Generator().manual_seed(dim + rows)
    x = torch.randn(rows, dim, generator=g) * 3
    w = torch.rand(dim, generator=g) + 0.5
    x[0] = 0                                                        # exactly 0 out
    x[1] = torch.randn(dim, generator=g) * 1e-20                    # eps dominates: rstd = 1 / sqrt(eps), the squares are denormal
    x[2] = torch.randn(dim, generator=g) * 1e15                     # squares of 1e30, a sum of 1e34
    gx, xd = _guarded(x)
    gw, wd = _guarded(w[None])
    assert xd.is_contiguous()
    for dt in (BF, F32):
        go = KB.Guarded((rows, dim), dt, device=DEV)
        out = ops.rmsnorm_rows(xd, wd[0], EPS, out_dtype=dt, out=go.view)
        torch.cuda.synchronize()
        tag = f"rmsnorm_rows dim {dim} rows {rows} {str(dt)[6:]}"
        assert out.data_ptr() == go.view.data_ptr()
        go.check(f"{tag}: guard band of out")
        gx.check(f"{tag}: guard band of x")
        gw.check(f"{tag}: guard band of w")
        ref, bound = KB.rmsnorm_rows_bound(x, w, EPS, dt)
        _report(tag, KB.assert_within(go.view, ref, bound, tag))
        assert float(go.view[0].float().abs().max()) == 0.0, (tag, "the all-zero row")


# ------------------------------------------------------------------------------------------------ t5_softmax_bias
@functools.lru_cache(maxsize=None)
def _lut(L):
    return relative_position_buckets(L, NB)


LUT_POISON = 0x0001          # 16-bit pattern; as int32 0x00010001 = 65537: a bucket far outside the table
TABLE_BAND = 65537 + 64      # guard rows behind the table: table[65537 * H + h] is NaN poison, inside the buffer

# (H, L, k_len, extra columns of npad beyond roundup(L, 64))
SOFTMAX = [(1, 4, 1, 0), (1, 4, 4, 0), (3, 72, 1, 0), (3, 72, 37, 0), (3, 72, 37, 64), (2, 260, 256, 0), (2, 260, 257, 0), (5, 600, 333, 0),
           (2, 2048, 2048, 0), (2, 2048, 1, 0), (2, 2048, 1793, 0), (64, 128, 19, 0)]


@pytest.mark.parametrize("guard", [False, True], ids=["random", "guard-scores"])
@pytest.mark.parametrize("H,L,k_len,extra", SOFTMAX, ids=[f"{c[0]}x{c[1]}-k{c[2]}{'-wide' if c[3] else ''}" for c in SOFTMAX])
def test_t5_softmax_bias_per_element(H, L, k_len, extra, guard):
    lut = _lut(L)
    s, table = KB.t5_softmax_inputs(H, L, k_len, seed=L + k_len, lut=lut, guard=guard, num_buckets=NB)
    npad = ops.round_up(L, 64) + extra
    assert npad <= 2048 and (extra == 0 or npad > ops.round_up(L, 64))
    gs, sd = _guarded(s.view(H * L, L))
    gt, td = _guarded(table, rows_after=TABLE_BAND)
    gl, ld = _guarded(lut[None], poison=LUT_POISON)
    assert int(gl.raw.view(torch.int32)[0, 0, 0]) * H >= NB * H + 2 * H and (int(gl.raw.view(torch.int32)[0, 0, 0]) + 1) * H <= (NB + TABLE_BAND) * H
    gp = KB.Guarded((H * L, npad), BF, ld=npad + 8, device=DEV)
    P = gp.view.unflatten(0, (H, L))                                 # strides (L ldp, ldp, 1), ldp = npad + 8 > npad
    out = ops.t5_softmax_bias(sd.view(H, L, L), td, ld[0], H, k_len, npad, out=P)
    torch.cuda.synchronize()
    tag = f"t5_softmax_bias {(H, L, k_len)} npad {npad}{' guard scores' if guard else ''}"
    assert out.data_ptr() == P.data_ptr()
    gp.check(f"{tag}: guard band of p")
    gs.check(f"{tag}: guard band of scores")
    gt.check(f"{tag}: guard band of table")
    gl.check(f"{tag}: guard band of lut")
    ref, bound = KB.t5_softmax_bias_bound(s, table, lut, H, k_len)
    Pc = P.cpu()
    _report(tag, KB.assert_within(Pc[:, :, :k_len], ref, bound, tag))
    if k_len < npad:
        tail = Pc[:, :, k_len:].float()
        assert float(tail.abs().max()) == 0.0 and not bool(torch.isnan(tail).any()), (tag, "columns [k_len, npad) must be exactly 0")
    if k_len == 1:
        assert bool((Pc[:, :, 0] == 1.0).all()), (tag, "one key: p is exactly 1")


def test_t5_softmax_bias_out_is_validated():
    H, L, npad = 2, 8, 64
    s = torch.zeros(H, L, L, device=DEV)
    table = torch.zeros(NB, H, device=DEV)
    lut = _lut(L).to(DEV)
    call = lambda out: ops.t5_softmax_bias(s, table, lut, H, L, npad, out=out)
    wide = torch.zeros(H * L, npad + 8, device=DEV, dtype=BF)
    assert call(wide[:, :npad].unflatten(0, (H, L))).data_ptr() == wide.data_ptr()
    assert call(torch.zeros(H, L, npad + 64, device=DEV, dtype=BF)).shape == (H, L, npad + 64)          # wider than npad is allowed
    with pytest.raises(ValueError, match=r"\[H, Lq, >= npad\]"):
        call(torch.zeros(H, L, npad - 8, device=DEV, dtype=BF))
    with pytest.raises(ValueError, match=r"\[H, Lq, >= npad\]"):
        call(torch.zeros(H, L + 1, npad, device=DEV, dtype=BF))
    with pytest.raises(ValueError, match=r"\[H, Lq, >= npad\]"):
        call(torch.zeros(H * L, npad, device=DEV, dtype=BF))
    with pytest.raises(ValueError, match="strides"):                 # a gap between the heads: row (h, i) is addressed at (h Lq + i) ldp
        call(torch.zeros(H, L + 2, npad, device=DEV, dtype=BF)[:, :L])
    with pytest.raises(ValueError, match="contiguous"):
        call(torch.zeros(H, L, 2 * npad, device=DEV, dtype=BF)[:, :, ::2])
    with pytest.raises(ValueError, match="bfloat16"):
        call(torch.zeros(H, L, npad, device=DEV))


# ------------------------------------------------------------------------------------------------ batched GEMM
GEMM = [(1, 4), (2, 72), (3, 132), (2, 260), (64, 128), (5, 516)]


@pytest.mark.parametrize("H,L", GEMM, ids=[f"{h}x{l}" for h, l in GEMM])
def test_gemm_batched_as_the_encoder_calls_it(H, L):
    """S_h = q_h k_h^T from the interleaved q | k rows (the neighbour of a head's 64 columns is another head's data), then
    o_h = P_h v_h into the head's 64 columns of [L, A]: per element, per head."""
    D, A = 64, 64 * H
    Lp = ops.round_up(L, 64)
    k_len = max(1, L - L // 3)
    g = torch.Generator().manual_seed(H * L)
    qk = torch.randn(L, 2 * A, generator=g).to(BF)
    gq, qb = _guarded(qk)                                            # NaN rows above and below
    # ---- scores: ldo = L + 4, two guard rows between the heads
    gS = KB.Guarded((H, L, L), F32, ld=L + 4, rows_before=1, rows_after=1, device=DEV)
    S = gS.view
    assert S.stride(0) == (L + 2) * (L + 4) and S.stride(1) == L + 4
    ops.gemm_batched(qb[:, :D], D, qb[:, A:A + D], D, S[0], S.stride(0), L, L, D, H, ops.EPI_F32)
    torch.cuda.synchronize()
    tag = f"gemm_batched scores H {H} L {L}"
    gS.check(f"{tag}: guard band of S")
    gq.check(f"{tag}: guard band of q | k")
    Sc = S.cpu()
    worst = 0.0
    for h in range(H):
        q_h, k_h = qk[:, h * D:(h + 1) * D], qk[:, A + h * D:A + (h + 1) * D]
        worst = max(worst, KB.assert_within(Sc[h], KB.gemm_ref(q_h, k_h), KB.gemm_bound(q_h, k_h, None, D, F32), f"{tag}, head {h}"))
    _report(f"{tag} EPI_F32", worst)
    # ---- P @ V: P columns [k_len, Lp) and vt columns [L, Lp) zero, as the encoder leaves them; o with ldo = A + 8
    Pm = torch.zeros(H, L, Lp)
    Pm[:, :, :k_len] = torch.rand(H, L, k_len, generator=g)
    Pm = Pm.to(BF)
    vt = torch.zeros(A, Lp)
    vt[:, :L] = torch.randn(A, L, generator=g)
    vt = vt.to(BF)
    gP, Pd = _guarded(Pm.view(H * L, Lp))
    gv, vd = _guarded(vt)
    go = KB.Guarded((L, A), BF, ld=A + 8, device=DEV)
    o = go.view
    ops.gemm_batched(Pd[:L], L * Lp, vd[:D], D * Lp, o[:, :D], D, L, D, Lp, H, ops.EPI_BF16)
    torch.cuda.synchronize()
    tag = f"gemm_batched P @ V H {H} L {L}"
    go.check(f"{tag}: guard band of o")
    gP.check(f"{tag}: guard band of P")
    gv.check(f"{tag}: guard band of vt")
    oc = o.cpu()
    worst = 0.0
    for h in range(H):
        P_h, v_h = Pm[h], vt[h * D:(h + 1) * D]
        worst = max(worst, KB.assert_within(oc[:, h * D:(h + 1) * D], KB.gemm_ref(P_h, v_h), KB.gemm_bound(P_h, v_h, None, Lp, BF), f"{tag}, head {h}"))
    _report(f"{tag} EPI_BF16", worst)
    # ---- batch = 1 with non-zero strides (the gridDim.y == 1 branch) for the LAST head: the other heads' columns are not touched
    z = H - 1
    o.fill_(1.25)
    ops.gemm_batched(Pd[z * L:(z + 1) * L], L * Lp, vd[z * D:(z + 1) * D], D * Lp, o[:, z * D:(z + 1) * D], D, L, D, Lp, 1, ops.EPI_BF16)
    torch.cuda.synchronize()
    go.check(f"{tag}, batch 1: guard band of o")
    o1 = o.cpu()
    assert torch.equal(o1[:, z * D:(z + 1) * D], oc[:, z * D:(z + 1) * D]), (tag, "one head alone must equal the same head of the batched launch")
    if H > 1:
        assert bool((o1[:, :z * D] == 1.25).all()), (tag, "the columns of the other heads were written")
    S.fill_(-3.0)
    ops.gemm_batched(qb[:, z * D:(z + 1) * D], D, qb[:, A + z * D:A + (z + 1) * D], D, S[z], S.stride(0), L, L, D, 1, ops.EPI_F32)
    torch.cuda.synchronize()
    gS.check(f"{tag}, batch 1: guard band of S")
    S1 = S.cpu()
    assert torch.equal(S1[z], Sc[z]) and (H == 1 or bool((S1[:z] == -3.0).all()))


# ------------------------------------------------------------------------------------------------ mul_bf16
def _mul_operands(n, seed):
    """Randoms, with the first eight products special: a bf16 denormal times 3, -0 and +0 (signs kept), inf, two products that
    overflow to +-inf, a product that is an fp32 denormal (1e-20 x 1e-20), the largest denormal halved.  No inf x 0."""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a[:8] = torch.tensor([1e-40, -0.0, 0.0, float("inf"), 3e38, -3e38, 1e-20, 1.17e-38])
    b[:8] = torch.tensor([3.0, 5.0, -7.0, 2.0, 10.0, 10.0, 1e-20, 0.5])
    a, b = a.to(BF), b.to(BF)
    want = (a.float() * b.float()).to(BF)
    assert bool(torch.isinf(want[3:6]).all()) and not bool(torch.isnan(want).any()) and float(a[0]) != 0.0 and float(want[0]) != 0.0
    return a, b, want


@pytest.mark.parametrize("mode", ["out-of-place", "in-place-a", "in-place-b"])
@pytest.mark.parametrize("n", [8, 2056, 77 * 320])
def test_mul_bf16_bitwise_and_in_place(n, mode):
    """The encoder calls it in place on the second operand (ops.mul_bf16(f, g, out=g)): every element is read and written by the
    same thread, once."""
    a, b, want = _mul_operands(n, n)
    ga, ad = _guarded(a[None])
    gb, bd = _guarded(b[None])
    go = KB.Guarded((1, n), BF, device=DEV)
    dst = {"out-of-place": go.view, "in-place-a": ad, "in-place-b": bd}[mode]
    out = ops.mul_bf16(ad, bd, out=dst)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.data_ptr()
    for name, gd in (("a", ga), ("b", gb), ("out", go)):
        gd.check(f"mul_bf16 n {n} {mode}: guard band of {name}")
    got = dst.cpu()[0]
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (n, mode, int((got.view(torch.int16) != want.view(torch.int16)).sum()))
    if mode != "in-place-a":
        assert torch.equal(ad.cpu()[0].view(torch.int16), a.view(torch.int16))
    if mode != "in-place-b":
        assert torch.equal(bd.cpu()[0].view(torch.int16), b.view(torch.int16))
    if mode == "out-of-place":
        assert bool((go.raw == go.poison).sum() == go.raw.numel() - n)


def test_mul_bf16_grid_stride_loop():
    """n / 8 > 65536 * 256: the only case in which a thread takes a second element.  134 M elements, 268 MB per operand, compared on
    the device with the same torch expression; out of place into a buffer with a sentinel tail, then in place on b."""
    n = 8 * (65536 * 256 + 257)
    torch.manual_seed(5)
    a = torch.randn(n, device=DEV, dtype=BF)
    b = torch.randn(n, device=DEV, dtype=BF)
    want = (a.float() * b.float()).to(BF)
    buf = torch.full((n + 64,), 7.0, device=DEV, dtype=BF)
    ops.mul_bf16(a, b, out=buf[:n])
    assert torch.equal(buf[:n], want) and bool((buf[n:] == 7.0).all())
    del buf
    ops.mul_bf16(a, b, out=b)
    assert torch.equal(b, want)


def test_mul_bf16_and_rmsnorm_rows_out_is_validated():
    a = torch.zeros(4, 16, device=DEV, dtype=BF)
    with pytest.raises(ValueError, match="mul_bf16.out"):
        ops.mul_bf16(a, a, out=torch.zeros(4, 8, device=DEV, dtype=BF))
    with pytest.raises(ValueError, match="mul_bf16.out"):
        ops.mul_bf16(a, a, out=torch.zeros(8, 16, device=DEV, dtype=BF)[::2])
    with pytest.raises(ValueError, match="mul_bf16.out"):
        ops.mul_bf16(a, a, out=torch.zeros(64, device=DEV, dtype=BF))
    assert ops.mul_bf16(a, a, out=a).data_ptr() == a.data_ptr()
    x = torch.ones(4, 16, device=DEV)
    w = torch.ones(16, device=DEV)
    for dt in (BF, F32):
        with pytest.raises(ValueError, match="rmsnorm_rows.out"):
            ops.rmsnorm_rows(x, w, EPS, out_dtype=dt, out=torch.zeros(4, 32, device=DEV, dtype=dt)[:, :16])
        with pytest.raises(ValueError, match="rmsnorm_rows.out"):
            ops.rmsnorm_rows(x, w, EPS, out_dtype=dt, out=torch.zeros(2, 16, device=DEV, dtype=dt))
        with pytest.raises(ValueError, match="rmsnorm_rows.out"):
            ops.rmsnorm_rows(x, w, EPS, out_dtype=dt, out=torch.zeros(8, 16, device=DEV, dtype=dt)[::2])
    with pytest.raises(ValueError, match="expected"):
        ops.rmsnorm_rows(x, w, EPS, out_dtype=BF, out=torch.zeros(4, 16, device=DEV))


# ------------------------------------------------------------------------------------------------ embedding_rows
@pytest.mark.parametrize("vocab,dim", [(256384, 64), (600, 4096)], ids=["umt5-vocabulary", "dim-4096"])
def test_embedding_rows_real_vocabulary_bitwise(vocab, dim):
    """The real vocabulary: ids up to 256 383, id * dim in 64-bit.  ids, table and output sit between guards."""
    torch.manual_seed(vocab)
    gt = KB.Guarded((vocab, dim), BF, device=DEV)
    table = gt.fill(torch.randn(vocab, dim, device=DEV).to(BF))
    g = torch.Generator().manual_seed(dim)
    fixed = [0, vocab - 1, vocab - 1, 0, vocab // 2, vocab // 2 - 1, vocab - 2, 1, 0, vocab - 1]
    ids = torch.cat([torch.tensor(fixed), torch.randint(0, vocab, (40,), generator=g)])
    n = ids.numel()
    idbuf = torch.full((n + 16,), 1 << 40, dtype=torch.int64, device=DEV)          # a neighbour read as an id is clamped to the last row
    idbuf[8:8 + n] = ids.to(DEV)
    go = KB.Guarded((n, dim), F32, device=DEV)
    _lib.check(_lib.load().wan_embedding_rows(ops._p(idbuf[8:8 + n]), ops._p(table), vocab, ops._p(go.view), n, dim, ops._stream()),
               "wan_embedding_rows")
    torch.cuda.synchronize()
    go.check(f"embedding_rows {vocab} x {dim}: guard band of out")
    gt.check(f"embedding_rows {vocab} x {dim}: guard band of table")
    assert torch.equal(go.view, table[ids.to(DEV)].float())
    assert torch.equal(ops.embedding_rows(ids.to(DEV), table), go.view)


# ------------------------------------------------------------------------------------------------ encoder invariants
MID = dict(vocab=1000, dim=512, dim_attn=512, dim_ffn=1280, num_heads=8, num_layers=3, num_buckets=32)


@pytest.fixture(scope="module", params=["tiny", "dim-512"])
def encoder(request):
    if request.param == "tiny":
        cfg, sd, L, lens = TINY, deterministic_t5_state_dict(**TINY), 72, [37, 11, 72]
    else:
        cfg, sd, L, lens = MID, random_t5_state_dict("cpu", seed=1, **MID), 512, [300, 41, 512]
    m = WanT5EncoderModel(shared_pos=False, **cfg)
    m.load_state_dict(sd, device=DEV)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, cfg["vocab"], (3, L), generator=g)
    mask = torch.zeros(3, L, dtype=torch.long)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    zeroed = ids * mask
    return dict(m=m, ids=ids.to(DEV), zeroed=zeroed.to(DEV), mask=mask.to(DEV), lens=lens, L=L, out=m(zeroed.to(DEV), mask.to(DEV))[0])


def test_encoder_valid_rows_ignore_the_ids_behind_the_mask(encoder):
    e = encoder
    assert bool(torch.isfinite(e["out"].float()).all())
    out_rand = e["m"](e["ids"], e["mask"])[0]                          # random ids behind the mask instead of 0
    assert bool(torch.isfinite(out_rand.float()).all())
    for b, n in enumerate(e["lens"]):
        assert torch.equal(out_rand[b, :n], e["out"][b, :n]), (b, n, "a masked key reached a valid row")
    if min(e["lens"]) < e["L"]:
        b = e["lens"].index(min(e["lens"]))
        assert not torch.equal(out_rand[b, e["lens"][b]:], e["out"][b, e["lens"][b]:])          # the padded rows do see their own ids


def test_encoder_internal_padding_equals_an_explicit_mask(encoder):
    """L = 30 is padded to 32 inside forward() with masked positions: the same as 32 ids (whatever the last two are) with a mask of 30."""
    e, m = encoder, encoder["m"]
    ids32 = e["ids"][:, :32]
    mask30 = torch.zeros(3, 32, dtype=torch.long, device=DEV)
    mask30[:, :30] = 1
    short = m(ids32[:, :30].contiguous())[0]
    assert short.shape[:2] == (3, 30)
    assert torch.equal(short, m(ids32.contiguous(), mask30)[0][:, :30])
    assert torch.equal(short, m(ids32[:, :30].contiguous(), mask30[:, :30].contiguous())[0])


def test_encoder_batch_of_three_equals_three_solo_calls(encoder):
    e, m = encoder, encoder["m"]
    for b, n in enumerate(e["lens"]):
        solo = m(e["zeroed"][b:b + 1], e["mask"][b:b + 1])[0]
        assert torch.equal(solo[0, :n], e["out"][b, :n]), (b, n, "a sample's valid rows depend on its batch neighbours")
