"""The umT5 text encoder part of tests/kernel_bounds.py checked on the CPU (the companion of tests/test_vae_bounds_host.py and
tests/test_fp8_bounds_host.py):

* honest fp32 emulations of rmsnorm_rows_kernel and t5_softmax_bias_kernel (videocof_amd/csrc/t5_kernels.hip) -- per-thread strided
  partial sums, a 64-lane xor tree, four wave sums, one rounding to nearest even -- stay inside rmsnorm_rows_bound /
  t5_softmax_bias_bound, and their worst |err| / bound is printed;
* twelve mutants -- each a way the index arithmetic, the masks or a reduction of these kernels (and of the batched GEMM between them)
  could be wrong -- are applied to the fp64 reference, finished honestly, fall outside their bound, and the failure names their rows /
  columns.  For each the verdict of the old limits of tests/test_gpu_t5.py at the old shapes is recorded and asserted (OLD_LIMIT_PASSES);
* the input builders' own properties (every bucket used, the guard score decisive) are asserted on the CPU.
"""
import functools
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_bounds as KB  # noqa: E402
from videocof_amd.wan_text_encoder import relative_position_buckets  # noqa: E402

BF = torch.bfloat16
F32 = torch.float32
EPS = 1e-6

# What the limits of tests/test_gpu_t5.py say about each mutant at that module's own shapes (True: the mutant passes them).
# rmsnorm: rel-L2 < 4e-3 (bf16) and < 1e-5 (fp32);  softmax: rel-L2 < 4e-3, |row sum - 1| < 1e-2, columns >= k_len exactly 0;
# batched GEMM: rel-L2 < 1e-5 (fp32 scores) / < 4e-3 (bf16 output).  Recorded results, asserted so that they stay true.
OLD_LIMIT_PASSES = {
    "1 truncating store, rmsnorm bf16 (5, 4096)": True,
    "1 truncating store, softmax (5, 600, 333)": True,
    "2 ragged chunk left out, bf16 limit at dim 1028": True,
    "2 ragged chunk left out, fp32 limit at dim 1028": False,
    "3 mean over roundup(dim, 1024), bf16 (64, 1000)": False,
    "3 mean over roundup(dim, 1024), fp32 (64, 1000)": False,
    "4 eps after the root, bf16 (37, 256)": True,
    "4 eps after the root, fp32 (37, 256)": True,
    "5 key k_len admitted, rel-L2 and row sum (5, 600, 333)": False,
    "5 key k_len admitted, zero columns (5, 600, 333)": False,
    "6 bucket of i - j (2, 72, 37)": False,
    "7 lut offset Lq (2, 72, 37)": False,
    "8 table indexed [h nb + bucket] (2, 72, 37)": False,
    "9 row sum stops at 256 (5, 600, 333)": False,
    "10 maximum of the first wave only (5, 600, 333)": False,
    "11 head z reads head z + 1's k (2, 72)": False,
    "12 output stride L L + 4 (2, 72)": False,
}
RECORD = {}


def bf(x):
    return x.to(BF)


def _truncate_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def _rel_l2(x, ref):
    return float((x.double() - ref.double()).norm() / ref.double().norm())


def _record(name, passes, detail=""):
    RECORD[name] = bool(passes)
    print(f"[mutant] {name}: {detail}-> old limit {'passes it' if passes else 'rejects it'}")
    assert RECORD[name] == OLD_LIMIT_PASSES[name], (name, detail, "the recorded old-limit verdict no longer holds")


def _rejected(name, out, ref, bound, where):
    """`out` is outside the bound and the failure names `where` (a regular expression over "dim0 a-b, rows c-d, cols e-f")."""
    with pytest.raises(AssertionError, match="outside the bound") as e:
        KB.assert_within(out, ref, bound, name)
    assert re.search(where, str(e.value)), (name, str(e.value), where)
    return str(e.value)


@functools.lru_cache(maxsize=None)
def _lut(L):
    return relative_position_buckets(L, 32)


def _xor_tree(v):
    """v [..., 64]: the shuffle tree of wave_sum (offsets 32 ... 1); every lane ends with the same sum, lane 0 is taken."""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def _block_sum(per_thread):
    """per_thread fp32 [..., 256] -> block_sum<4>: xor tree per wave, then 0 + the four wave sums in order."""
    waves = _xor_tree(per_thread.reshape(*per_thread.shape[:-1], 4, 64))
    t = torch.zeros_like(waves[..., 0])
    for i in range(4):
        t = t + waves[..., i]
    return t


# ------------------------------------------------------------------------------------------------ rmsnorm_rows
def _rms_inputs(rows, dim, seed, special=True):
    """x of std 3, w in [0.5, 1.5); with `special` one all-zero row, one of magnitude 1e-20 (eps dominates), one of 1e15."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, dim, generator=g) * 3
    w = torch.rand(dim, generator=g) + 0.5
    if special:
        assert rows >= 3
        x[0] = 0
        x[1] = torch.randn(dim, generator=g) * 1e-20
        x[2] = torch.randn(dim, generator=g) * 1e15
    return x, w


def _rms_emulate(x, w, eps):
    """rmsnorm_rows_kernel<NV> in fp32: thread t squares and adds float4 chunks t, t + 256, ...; block_sum; / dim + eps; rsqrt; two
    multiplies."""
    rows, dim = x.shape
    nchunk = dim // 4
    nv = (nchunk + 255) // 256
    c = F.pad(x.float().view(rows, nchunk, 4), (0, 0, 0, nv * 256 - nchunk)).view(rows, nv, 256, 4)
    sq = c * c
    chunk = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
    ss = torch.zeros(rows, 256)
    for i in range(nv):
        ss = ss + chunk[:, i]
    arg = _block_sum(ss) / torch.tensor(float(dim)) + torch.tensor(eps, dtype=F32)
    return x.float() * torch.rsqrt(arg)[:, None] * w.float()


def _rms_mutant(x, w, eps, ss=None, count=None, eps_after=False):
    """The fp64 reference with one thing changed -- the sum of squares, the divisor, or where eps enters -- finished honestly: rounded
    once to fp32 (the caller rounds that once more to bf16)."""
    xd = x.double()
    ss = (xd * xd).sum(dim=-1, keepdim=True) if ss is None else ss
    ms = ss / (x.shape[1] if count is None else count)
    rstd = 1.0 / (torch.sqrt(ms) + eps) if eps_after else 1.0 / torch.sqrt(ms + eps)
    return (xd * rstd * w.double()).float()


RMS_DIMS = [4, 8, 1000, 1024, 1028, 2052, 3076, 4096, 4100, 5124, 6148, 7172, 8192]


@pytest.mark.parametrize("dim", RMS_DIMS)
def test_honest_rmsnorm_rows_emulation_stays_inside(dim):
    x, w = _rms_inputs(5, dim, seed=dim)
    y = _rms_emulate(x, w, EPS)
    for dt, out in ((BF, bf(y)), (F32, y)):
        ref, bound = KB.rmsnorm_rows_bound(x, w, EPS, dt)
        worst = KB.assert_within(out, ref, bound, f"rmsnorm_rows emulation, dim {dim}, {dt}")
        print(f"[bound] rmsnorm_rows emulation dim {dim} {str(dt)[6:]}: worst |err|/bound = {worst:.3f}")
        assert float(out[0].abs().max()) == 0.0 and float(ref[0].abs().max()) == 0.0          # the all-zero row
        assert worst <= 1.0 and (dt == F32 or worst > 0.5)                                    # the bf16 half ulp is sharp
    # the eps-dominated row: rstd is 1 / sqrt(eps) there, the 1e15 row comes out at unit scale
    ref, _ = KB.rmsnorm_rows_bound(x, w, EPS, F32)
    assert abs(float((ref[1] / (x[1].double() * w.double())).mean()) / 1e3 - 1.0) < 1e-6
    assert 0.1 < float(ref[2].abs().max()) < 20.0


def test_rmsnorm_rows_mutants_are_rejected_and_named():
    # 1. truncating store (bf16), judged by the old limit at the old shape (5, 4096)
    x, w = _rms_inputs(5, 4096, seed=11, special=False)
    ref, bound = KB.rmsnorm_rows_bound(x, w, EPS, BF)
    out = _truncate_bf16(_rms_emulate(x, w, EPS))
    _rejected("1 truncating store", out, ref, bound, r"rows 0-4, cols 0-4095")
    _record("1 truncating store, rmsnorm bf16 (5, 4096)", _rel_l2(out, ref) < 4e-3, f"rel-L2 {_rel_l2(out, ref):.2e} ")

    # 2. dim 1028 = 257 float4 chunks: chunk 256 (thread 0's second) left out of the sum of squares.  No shape of the old module
    #    reaches a second chunk per thread with a ragged end, so its limits are applied at this dim
    x, w = _rms_inputs(5, 1028, seed=12)
    ss = (x.double()[:, :1024] ** 2).sum(dim=-1, keepdim=True)
    y = _rms_mutant(x, w, EPS, ss=ss)
    for dt, out in ((BF, bf(y)), (F32, y)):
        ref, bound = KB.rmsnorm_rows_bound(x, w, EPS, dt)
        KB.assert_within(_rms_mutant(x, w, EPS).to(dt), ref, bound, "unmutated")
        _rejected("2 ragged chunk left out", out, ref, bound, r"rows 2-4, ")         # row 0 is zero, row 1 is all eps: both unmoved
    x, w = _rms_inputs(64, 1028, seed=12, special=False)                             # 64 random rows, as the old module draws them
    y = _rms_mutant(x, w, EPS, ss=(x.double()[:, :1024] ** 2).sum(dim=-1, keepdim=True))
    for dt, out in ((BF, bf(y)), (F32, y)):
        ref, bound = KB.rmsnorm_rows_bound(x, w, EPS, dt)
        _rejected("2 ragged chunk left out", out, ref, bound, r"rows 0-63, ")
        _record(f"2 ragged chunk left out, {'bf16' if dt == BF else 'fp32'} limit at dim 1028", _rel_l2(out, ref) < (4e-3 if dt == BF else 1e-5),
                f"rel-L2 {_rel_l2(out, ref):.2e} ")

    # 3. the mean taken over roundup(dim, 1024) (the padded thread count) instead of dim; old shape (64, 1000)
    x, w = _rms_inputs(64, 1000, seed=13, special=False)
    y = _rms_mutant(x, w, EPS, count=1024)
    for dt, out in ((BF, bf(y)), (F32, y)):
        ref, bound = KB.rmsnorm_rows_bound(x, w, EPS, dt)
        _rejected("3 mean over roundup(dim, 1024)", out, ref, bound, r"rows 0-63, cols 0-999")
        _record(f"3 mean over roundup(dim, 1024), {'bf16' if dt == BF else 'fp32'} (64, 1000)", _rel_l2(out, ref) < (4e-3 if dt == BF else 1e-5),
                f"rel-L2 {_rel_l2(out, ref):.2e} ")

    # 4. eps added after the root, 1 / (sqrt(mean) + eps).  On unit-scale rows the difference is 3e-7 relative -- inside every bound
    #    that admits a dim-term sum, and inside the old limits at the old shape (37, 256); the eps-dominated row shows it
    x, w = _rms_inputs(37, 256, seed=14, special=False)
    y = _rms_mutant(x, w, EPS, eps_after=True)
    for dt, out in ((BF, bf(y)), (F32, y)):
        ref, _ = KB.rmsnorm_rows_bound(x, w, EPS, dt)
        _record(f"4 eps after the root, {'bf16' if dt == BF else 'fp32'} (37, 256)", _rel_l2(out, ref) < (4e-3 if dt == BF else 1e-5),
                f"rel-L2 {_rel_l2(out, ref):.2e} ")
    x, w = _rms_inputs(37, 256, seed=14)
    y = _rms_mutant(x, w, EPS, eps_after=True)
    for dt, out in ((BF, bf(y)), (F32, y)):
        ref, bound = KB.rmsnorm_rows_bound(x, w, EPS, dt)
        _rejected("4 eps after the root", out, ref, bound, r"rows 1-1, ")


# ------------------------------------------------------------------------------------------------ t5_softmax_bias
def _full(ref, bound, npad):
    """Reference and bound over all npad columns: [k_len, npad) is exactly zero."""
    pad = npad - ref.shape[-1]
    return F.pad(ref, (0, pad)), F.pad(bound, (0, pad))


def _softmax_emulate(s, table, lut, k_len, npad):
    """t5_softmax_bias_kernel in fp32: v = s + bias (one rounding), masked keys -inf; the row maximum; e = exp(v - mx); thread t adds
    e[t], e[t + 256], ...; block_sum; inv = 1 / sum; p = bf16(e * inv) over npad columns."""
    H, L, _ = s.shape
    v = torch.full((H, L, 2048), float("-inf"))
    v[:, :, :k_len] = (s + KB.t5_bias(table, lut, L).float())[:, :, :k_len]
    mx = v.max(dim=-1, keepdim=True).values
    e = torch.exp(v - mx)
    per_thread = torch.zeros(H, L, 256)
    for t in range(8):
        per_thread = per_thread + e[:, :, 256 * t:256 * t + 256]
    inv = 1.0 / _block_sum(per_thread)
    return bf(e * inv[..., None])[:, :, :npad]


def _softmax_mutant(s, table, lut, k_len, npad, admit=0, flip=False, lut_off=0, table_t=False, sum_upto=None, first_wave_max=False):
    """The fp64 reference with one thing changed, finished honestly (fp32 exponentials where the mutant is about their range, one
    rounding to bf16).  Returns bf16 [H, L, npad]."""
    H, L, _ = s.shape
    i = torch.arange(L)
    off = (i[:, None] - i[None, :] if flip else i[None, :] - i[:, None]) + L - 1 + lut_off
    bucket = lut.long()[off.clamp(0, 2 * L - 2)]                           # [L, L]
    flat = table.double().reshape(-1)
    nb = table.shape[0]
    h = torch.arange(H)[:, None, None]
    bias = flat[h * nb + bucket[None]] if table_t else flat[bucket[None] * H + h]
    n = k_len + admit
    t = (s.double() + bias)[:, :, :n]
    if first_wave_max:
        # wave 0 holds j = lane + 256 t: its maximum only; the exponentials in fp32, where they overflow
        j = torch.arange(n)
        mx = t[:, :, (j % 256) < 64].max(dim=-1, keepdim=True).values
        e = torch.exp((t - mx).float())
        p = e * (1.0 / e.sum(dim=-1, keepdim=True))
    else:
        e = torch.exp(t - t.max(dim=-1, keepdim=True).values)
        p = e / (e if sum_upto is None else e[:, :, :sum_upto]).sum(dim=-1, keepdim=True)
    return bf(F.pad(p.float(), (0, npad - n)))


def _old_softmax_limits(P, ref_full, L, k_len):
    """(rel-L2 < 4e-3 and |row sum - 1| < 1e-2, columns >= k_len exactly zero): the three assertions of test_t5_softmax_bias_vs_oracle."""
    rel = _rel_l2(P[:, :, :L], ref_full[:, :, :L])
    rowsum = float((P[:, :, :L].float().sum(-1) - 1).abs().max())
    zero = float(P[:, :, k_len:].float().abs().max()) == 0.0 if k_len < P.shape[-1] else True
    return rel < 4e-3 and rowsum < 1e-2, zero, f"rel-L2 {rel:.2e}, row sum off by {rowsum:.1e} "


SOFTMAX_SHAPES = [(1, 4, 1), (1, 4, 4), (3, 72, 1), (3, 72, 37), (2, 260, 256), (2, 260, 257), (5, 600, 333), (2, 1028, 1028), (2, 1028, 1)]


@pytest.mark.parametrize("H,L,k_len", SOFTMAX_SHAPES)
@pytest.mark.parametrize("guard", [False, True])
def test_honest_softmax_bias_emulation_stays_inside(H, L, k_len, guard):
    lut = _lut(L)
    s, table = KB.t5_softmax_inputs(H, L, k_len, seed=L + k_len, lut=lut, guard=guard)
    npad = (L + 63) // 64 * 64
    ref, bound = _full(*KB.t5_softmax_bias_bound(s, table, lut, H, k_len), npad)
    assert abs(float(ref.sum(dim=-1).max()) - 1.0) < 1e-12
    out = _softmax_emulate(s, table, lut, k_len, npad)
    worst = KB.assert_within(out, ref, bound, f"t5_softmax_bias emulation {(H, L, k_len)}")
    print(f"[bound] t5_softmax_bias emulation {(H, L, k_len)}{' guard scores' if guard else ''}: worst |err|/bound = {worst:.3f}")
    if k_len == 1:
        assert bool((out[:, :, 0] == 1.0).all())
    if guard and k_len < L:
        # the guard score is decisive: one admitted key takes (1 - 1e-15) of every row
        full = torch.softmax(s.double() + KB.t5_bias(table, lut, L), dim=-1)
        assert float(full[:, :, k_len:].sum(dim=-1).min()) > 1.0 - 1e-12


def test_softmax_bias_mutants_are_rejected_and_named():
    # ---- the old module's small shape
    H, L, k_len, npad = 2, 72, 37, 128
    lut = _lut(L)
    s, table = KB.t5_softmax_inputs(H, L, k_len, seed=L + k_len, lut=lut)
    ref, bound = _full(*KB.t5_softmax_bias_bound(s, table, lut, H, k_len), npad)
    KB.assert_within(_softmax_mutant(s, table, lut, k_len, npad), ref, bound, "unmutated")
    for name, kw, where in (("6 bucket of i - j", dict(flip=True), r"dim0 0-1, rows 0-71, "),
                            ("7 lut offset Lq", dict(lut_off=1), r"dim0 0-1, rows 0-71, "),
                            ("8 table indexed [h nb + bucket]", dict(table_t=True), r"dim0 0-1, rows 0-71, ")):
        out = _softmax_mutant(s, table, lut, k_len, npad, **kw)
        _rejected(name, out, ref, bound, where)
        ok, zero, detail = _old_softmax_limits(out, ref, L, k_len)
        _record(f"{name} (2, 72, 37)", ok and zero, detail)

    # ---- the old module's (5, 600, 333): a key among hundreds
    H, L, k_len, npad = 5, 600, 333, 640
    lut = _lut(L)
    s, table = KB.t5_softmax_inputs(H, L, k_len, seed=L + k_len, lut=lut)
    ref, bound = _full(*KB.t5_softmax_bias_bound(s, table, lut, H, k_len), npad)
    # 1. truncating store
    p32 = F.pad(torch.softmax((s.double() + KB.t5_bias(table, lut, L))[:, :, :k_len], dim=-1).float(), (0, npad - k_len))
    out = _truncate_bf16(p32)
    _rejected("1 truncating store", out, ref, bound, r"dim0 0-4, rows 0-599, ")
    ok, zero, detail = _old_softmax_limits(out, ref, L, k_len)
    _record("1 truncating store, softmax (5, 600, 333)", ok and zero, detail)
    # 5. key k_len admitted (mask j <= k_len) on RANDOM scores.  With logits of std 3.6 a row's mass sits on a handful of keys, so one
    #    more key among 333 moves the whole tensor by 7.5e-2: the old limits see it here, and the old module also sees the non-zero
    #    column k_len.  Per element the column is named; the guard scores make the same mutant a total loss of every row
    out = _softmax_mutant(s, table, lut, k_len, npad, admit=1)
    msg = _rejected("5 key k_len admitted, random scores", out, ref, bound, r"dim0 0-4, rows 0-599, cols \d+-333")
    ok, zero, detail = _old_softmax_limits(out, ref, L, k_len)
    _record("5 key k_len admitted, rel-L2 and row sum (5, 600, 333)", ok, detail)
    _record("5 key k_len admitted, zero columns (5, 600, 333)", zero, "column k_len is not zero ")
    # ... and on the guard scores it takes every row whole
    sg, tg = KB.t5_softmax_inputs(H, L, k_len, seed=L + k_len, lut=lut, guard=True)
    refg, boundg = _full(*KB.t5_softmax_bias_bound(sg, tg, lut, H, k_len), npad)
    KB.assert_within(_softmax_mutant(sg, tg, lut, k_len, npad), refg, boundg, "unmutated, guard scores")
    outg = _softmax_mutant(sg, tg, lut, k_len, npad, admit=1)
    _rejected("5 key k_len admitted, guard scores", outg, refg, boundg, r"dim0 0-4, rows 0-599, cols 0-333")
    assert float(outg[:, :, k_len].float().min()) == 1.0 and _rel_l2(outg[:, :, :k_len], refg[:, :, :k_len]) > 0.999
    assert "cols" in msg
    # 9. scores at j >= 256 left out of the row sum
    out = _softmax_mutant(s, table, lut, k_len, npad, sum_upto=256)
    _rejected("9 row sum stops at 256", out, ref, bound, r"dim0 0-4, rows 0-599, ")
    ok, zero, detail = _old_softmax_limits(out, ref, L, k_len)
    _record("9 row sum stops at 256 (5, 600, 333)", ok and zero, detail)
    # 10. the row maximum from the first wave only; the maximum sits at j = 100 and exceeds the rest by more than exp can hold
    s10 = s.clone()
    s10[:, :, 100] = 200.0
    ref10, bound10 = _full(*KB.t5_softmax_bias_bound(s10, table, lut, H, k_len), npad)
    worst = KB.assert_within(_softmax_emulate(s10, table, lut, k_len, npad), ref10, bound10, "honest emulation, one score of 200")
    assert worst <= 1.0
    out = _softmax_mutant(s10, table, lut, k_len, npad, first_wave_max=True)
    assert bool(torch.isnan(out[:, :, 100].float()).all())
    _rejected("10 maximum of the first wave only", out, ref10, bound10, r"dim0 0-4, rows 0-599, cols 100-100")
    ok, zero, detail = _old_softmax_limits(out, ref10, L, k_len)
    _record("10 maximum of the first wave only (5, 600, 333)", ok and zero, detail)


# ------------------------------------------------------------------------------------------------ batched GEMM
def test_batched_gemm_mutants_are_rejected_and_named():
    """S_h = q_h k_h^T from the interleaved [L, 2A] rows, the old module's (H, L) = (2, 72) and three heads at L = 132."""
    for H, L in ((2, 72), (3, 132)):
        D, A = 64, 64 * H
        g = torch.Generator().manual_seed(H * L)
        qk = bf(torch.randn(L, 2 * A, generator=g))
        q = [qk[:, h * D:(h + 1) * D] for h in range(H)]
        k = [qk[:, A + h * D:A + (h + 1) * D] for h in range(H)]
        ref = torch.stack([KB.gemm_ref(q[h], k[h]) for h in range(H)])
        bound = torch.stack([KB.gemm_bound(q[h], k[h], None, D, F32) for h in range(H)])
        honest = torch.stack([q[h].float() @ k[h].float().t() for h in range(H)])
        worst = KB.assert_within(honest, ref, bound, f"batched GEMM emulation {(H, L)}")
        print(f"[bound] batched GEMM EPI_F32 emulation {(H, L)}: worst |err|/bound = {worst:.3f}")
        # 11. head z reads head z + 1's k columns (the last one wraps into q's columns of the next row group: here, head 0's)
        out = torch.stack([q[h].float() @ k[(h + 1) % H].float().t() for h in range(H)])
        _rejected("11 head z reads head z + 1's k", out, ref, bound, rf"dim0 0-{H - 1}, rows 0-{L - 1}, cols 0-{L - 1}")
        if (H, L) == (2, 72):
            _record("11 head z reads head z + 1's k (2, 72)", _rel_l2(out, ref) < 1e-5, f"rel-L2 {_rel_l2(out, ref):.2e} ")
        # 12. head z stored at z (L L + 4): read back at the stride the caller gave, every head but the first is shifted
        flat = torch.full((H * (L * L + 4),), float("nan"))
        for h in range(H):
            flat[h * (L * L + 4):h * (L * L + 4) + L * L] = honest[h].reshape(-1)
        out = flat[:H * L * L].view(H, L, L)
        _rejected("12 output stride L L + 4", out, ref, bound, rf"dim0 1-{H - 1}, rows 0-{L - 1}, cols 0-{L - 1}")
        if (H, L) == (2, 72):
            _record("12 output stride L L + 4 (2, 72)", _rel_l2(out, ref) < 1e-5, f"rel-L2 {_rel_l2(out, ref):.2e} ")

