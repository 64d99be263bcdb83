"""-m gpu: the GEMM families, the attention forms and the row kernels judged PER ELEMENT against fp64 references under the derived
bounds of tests/kernel_bounds.py (docs/TEST_BOUNDS.md), with poisoned guard bands around every operand and result.

What a whole-tensor rel-L2 cannot see and this module does: a wrong 16x16 sub-tile, a row segment stored from the neighbouring
row, a truncating bf16 conversion, a store past column N or row M, a read past the end that reaches a result (operands sit in NaN),
one key admitted past Lk or lost at a tile seam (decisive-key inputs; the rows of k behind the last key hold a key that would take
all the mass).  Every comparison prints its worst |err| / bound; the limit is 1.
"""
import functools
import math
import os
import random
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
BF = torch.bfloat16

GEMM_DEFAULTS = {"gemm_variant": 0, "gemm_w4": 1, "gemm_pk": 1, "gemm_pk_form": 31, "gemm_pk_min_units": 0, "gemm_splitk": 1,
                 "sp_reserve_cus": 0}
# family -> (tuning, wan_gemm_ws_plan, wan_gemm_ws_splits or None); "quarter" = the stream-K cut at a quarter of a tile's K range
FAMILIES = {
    "128":        ({"gemm_variant": 1, "gemm_pk": 0, "gemm_splitk": 0}, 0, 1),
    "splitk2":    ({"gemm_variant": 1, "gemm_pk": 0, "gemm_splitk": 2}, 0, 2),
    "splitk3":    ({"gemm_variant": 1, "gemm_pk": 0, "gemm_splitk": 3}, 0, 3),
    "256w8":      ({"gemm_variant": 2, "gemm_w4": 0, "gemm_pk": 0}, 1, None),
    "256w4":      ({"gemm_variant": 2, "gemm_w4": 3, "gemm_pk": 0}, 2, None),
    "pk31":       ({"gemm_pk": 2, "gemm_pk_form": 31, "gemm_pk_min_units": "quarter"}, 3, None),
    "pk0":        ({"gemm_pk": 2, "gemm_pk_form": 0, "gemm_pk_min_units": "quarter"}, 3, None),
    "pk31own":    ({"gemm_pk": 2, "gemm_pk_form": 31, "gemm_pk_min_units": 0}, 3, None),
    "pk31rsv":    ({"gemm_pk": 2, "gemm_pk_form": 31, "gemm_pk_min_units": "quarter", "sp_reserve_cus": 16}, 3, None),
}
# (M, N, K): M at tile - 1 / tile / tile + 1 / a prime, M % 8 != 0 (the transposed store's last 8-token group), N % 8 == 4 (the 8-byte
# store path) and N % 8 == 0, N one 4-column group past a tile, K from one K tile up
SHAPES_128 = [(127, 132, 64), (128, 128, 192), (129, 260, 64), (521, 520, 320)]
SHAPES_SPLITK = [(131, 132, 1024), (515, 196, 4096), (1000, 520, 2048)]
SHAPES_256 = [(255, 260, 128), (256, 256, 256), (257, 516, 384), (1031, 520, 512)]
# the persistent kernel needs one whole 256^2 tile each way (M = 255 belongs to the per-tile kernels); existing shapes of
# tests/test_gpu_kernels.py; (2304, 1536, 1536): a 1.3B Linear, 54 tiles on one worker per CU -- the short launch whose leftover tiles
# go whole (tests/test_gemm_pk_plan.py)
SHAPES_PK = [(256, 256, 128), (257, 516, 384), (1031, 520, 512), (3000, 1164, 384), (2900, 1672, 640), (4100, 2100, 256),
             (2304, 1536, 1536)]
GEMM_CASES = ([("128", s) for s in SHAPES_128] + [(f, s) for s in SHAPES_SPLITK for f in ("splitk2", "splitk3")]
              + [(f, s) for s in SHAPES_256 for f in ("256w8", "256w4")]
              + [(f, s) for s in SHAPES_PK for f in ("pk31", "pk0")]
              + [("pk31own", s) for s in SHAPES_PK[3:]] + [("pk31rsv", (3000, 1164, 384)), ("pk31rsv", (2304, 1536, 1536))])
GEMM_CASES.sort(key=lambda c: c[1])            # cases of one shape run back to back: the fp64 reference is computed once


class _Tuning:
    def __init__(self, values, K):
        self.values = {k: (max(1, (K // 128 + 3) // 4) if v == "quarter" else v) for k, v in values.items()}

    def __enter__(self):
        for k, v in self.values.items():
            ops.set_tuning(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            ops.set_tuning(k, GEMM_DEFAULTS[k])


def _poisoned_operand(t, rows_after=3):
    """`t` as the interior of a poisoned buffer: 8 NaN columns left, 8 right, NaN rows above and below."""
    gd = KB.Guarded(tuple(t.shape), t.dtype, ld=t.shape[-1] + 16, rows_before=1, rows_after=rows_after, cols_before=8, device=DEV)
    gd.fill(t.to(DEV))
    return gd


@functools.lru_cache(maxsize=1)
def _gemm_problem(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    a, w = torch.randn(M, K, generator=g).to(BF), (torch.randn(N, K, generator=g) * 0.1).to(BF)
    bias = torch.randn(N, generator=g) * 0.5
    # residual stream of mixed magnitude: the read-modify-write add matters at 1e-3 and at 1e3
    x0 = torch.randn(M, N, generator=g) * (10.0 ** torch.randint(-3, 4, (M, N), generator=g).float())
    ref = KB.gemm_ref(a, w, bias)
    term = KB.gemm_acc_term(a, w, bias, K)
    return dict(a=a, w=w, bias=bias, x0=x0, ref=ref, term=term, ref_nb=ref - bias.double(), term_nb=KB.gemm_acc_term(a, w, None, K),
                gen=g)


def _report(tag, worst):
    print(f"[bound] {tag}: worst |err|/bound = {worst:.3f}")
    return worst


@pytest.mark.parametrize("family,shape", GEMM_CASES, ids=[f"{f}-{s[0]}x{s[1]}x{s[2]}" for f, s in GEMM_CASES])
def test_gemm_family_per_element_and_guard_bands(family, shape):
    M, N, K = shape
    tune, plan, splits = FAMILIES[family]
    P = _gemm_problem(M, N, K)
    lib = _lib.load()
    A, W = _poisoned_operand(P["a"]), _poisoned_operand(P["w"])
    bias = P["bias"].to(DEV)
    tag = f"gemm {family} {M}x{N}x{K}"
    worst = {}
    with _Tuning(tune, K):
        assert lib.wan_gemm_ws_plan(M, N, K) == plan, (family, shape, lib.wan_gemm_ws_plan(M, N, K))
        if splits is not None:
            assert lib.wan_gemm_ws_splits(M, N, K) == splits, (family, shape, lib.wan_gemm_ws_splits(M, N, K))
        # row-major epilogues: output rows 8-byte aligned only (ldo = N + 4) or 16-byte aligned (N + 8)
        o_bf = KB.Guarded((M, N), BF, ld=N + 8, device=DEV)
        o_ge = KB.Guarded((M, N), BF, ld=N + 4, device=DEV)
        o_f = KB.Guarded((M, N), torch.float32, ld=N + 4, device=DEV)
        ops.gemm(A.view, W.view, bias, ops.EPI_BF16, out=o_bf.view)
        ops.gemm(A.view, W.view, bias, ops.EPI_GELU_BF16, out=o_ge.view)
        ops.gemm(A.view, W.view, None, ops.EPI_F32, out=o_f.view)
        o_fb = KB.Guarded((M, N), torch.float32, ld=N + 8, device=DEV)
        ops.gemm(A.view, W.view, bias, ops.EPI_F32, out=o_fb.view)
        # read-modify-write: a gate seam at a row that is not a multiple of 8, samples shorter than a wave's 128 rows, no gate
        resid = []
        rpb_odd = max(129, ((M + 1) // 2) | 1)
        for rpb in (rpb_odd, 100, None):
            if rpb == 100 and M < 200:
                continue
            o_r = KB.Guarded((M, N), torch.float32, ld=N + 8, device=DEV)
            o_r.fill(P["x0"].to(DEV))
            gate = None
            if rpb is not None:
                gate = torch.randn((M + rpb - 1) // rpb, N, generator=torch.Generator().manual_seed(rpb))
            ops.gemm(A.view, W.view, bias, ops.EPI_RESID_F32, out=o_r.view, gate=None if gate is None else gate.to(DEV),
                     rows_per_batch=rpb or 0)
            resid.append((rpb, gate, o_r))
        # transposed: ldo = roundup(M, 64) + 8 and + 4; the columns [M, ldo) are guard band (contract: NOT written, include/wan_hip.h)
        o_t = [KB.Guarded((N, M), BF, ld=ops.round_up(M, 64) + pad, device=DEV) for pad in (8, 4)]
        for t in o_t:
            ops.gemm(A.view, W.view, bias, ops.EPI_BF16_T, out=t.view)
        torch.cuda.synchronize()
    A.check(tag + " A"); W.check(tag + " W")
    b16 = KB.gemm_bound(None, None, None, K, BF, P["ref"], P["term"])
    worst["bf16"] = KB.assert_within(o_bf.view, P["ref"], b16, tag + " EPI_BF16")
    o_bf.check(tag + " EPI_BF16")
    g_ref, g_bound = KB.gelu_bound(P["ref"], P["term"])
    worst["gelu"] = KB.assert_within(o_ge.view, g_ref, g_bound, tag + " EPI_GELU_BF16")
    o_ge.check(tag + " EPI_GELU_BF16")
    # the second GELU check: against g of the kernel's own fp32 accumulator (no K-sized term: sees an erf-form epilogue at every K)
    a_ref, a_bound = KB.gelu_from_acc_bound(o_fb.view)
    worst["gelu_acc"] = KB.assert_within(o_ge.view, a_ref, a_bound, tag + " EPI_GELU_BF16 vs g(own EPI_F32 accumulator)")
    worst["f32b"] = KB.assert_within(o_fb.view, P["ref"], KB.gemm_bound(None, None, None, K, torch.float32, P["ref"], P["term"]),
                                     tag + " EPI_F32 with bias")
    o_fb.check(tag + " EPI_F32 with bias")
    worst["f32"] = KB.assert_within(o_f.view, P["ref_nb"], KB.gemm_bound(None, None, None, K, torch.float32, P["ref_nb"], P["term_nb"]),
                                    tag + " EPI_F32")
    o_f.check(tag + " EPI_F32")
    for rpb, gate, o_r in resid:
        rows = None if gate is None else gate[torch.arange(M) // rpb]
        r_ref, r_bound = KB.resid_bound(P["ref"], P["term"], rows, P["x0"])
        worst[f"resid{rpb}"] = KB.assert_within(o_r.view, r_ref, r_bound, f"{tag} EPI_RESID_F32 rows_per_batch {rpb}")
        o_r.check(f"{tag} EPI_RESID_F32 rows_per_batch {rpb}")
    for t in o_t:
        worst[f"T{t.ld}"] = KB.assert_within(t.view.t(), P["ref"], b16, f"{tag} EPI_BF16_T ldo {t.ld} (rows = tokens, cols = channels)")
        t.check(f"{tag} EPI_BF16_T ldo {t.ld}: pad columns [M, ldo) must be left alone")
    _report(tag, max(worst.values()))
    print("        " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


def test_gemm_sp_shard_short_launch_sampled_rows():
    """M = 8385 = 67 080 / 8 (the 8-way shard, profiles/r01/gemm_sp_shard_shapes.txt), N = K = 5120: 660 tiles on one worker per CU,
    the launch the "leftover tiles go whole" rule was written for.  An fp64 reference of the whole product is beyond what a CPU test
    may cost, so the rows at every 256-row tile seam (last / first two) and the ragged last tile are judged per element, all columns;
    every other element must have been written with a finite value, and the guard bands cover the whole result."""
    M, N, K = 8385, 5120, 5120
    g = torch.Generator(device=DEV).manual_seed(8)
    a = torch.randn(M, K, device=DEV, generator=g).to(BF)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.02).to(BF)
    bias = torch.randn(N, device=DEV, generator=g) * 0.5
    A, W = _poisoned_operand(a), _poisoned_operand(w)
    rows = sorted({r for s in range(256, M, 256) for r in (s - 2, s - 1, s, s + 1)} | set(range(M - 130, M)) | {0, 1})
    rows_t = torch.tensor(rows)
    assert _lib.load().wan_gemm_ws_plan(M, N, K) == 3
    o_bf = KB.Guarded((M, N), BF, ld=N + 8, device=DEV)
    o_t = KB.Guarded((N, M), BF, ld=ops.round_up(M, 64) + 8, device=DEV)
    ops.gemm(A.view, W.view, bias, ops.EPI_BF16, out=o_bf.view)
    ops.gemm(A.view, W.view, bias, ops.EPI_BF16_T, out=o_t.view)
    torch.cuda.synchronize()
    a_s = a[rows_t.to(DEV)].cpu()
    ref = KB.gemm_ref(a_s, w.cpu(), bias.cpu())
    bound = KB.gemm_bound(a_s, w.cpu(), bias.cpu(), K, BF, ref)
    w1 = KB.assert_within(o_bf.view[rows_t.to(DEV)], ref, bound, f"gemm pk 8385x5120x5120 EPI_BF16, sampled rows (index into {rows[:4]}..)")
    w2 = KB.assert_within(o_t.view[:, rows_t.to(DEV)].t(), ref, bound, "gemm pk 8385x5120x5120 EPI_BF16_T, sampled rows")
    # every other row: written (the interiors started as NaN poison) and finite
    assert bool(torch.isfinite(o_bf.view).all()) and bool(torch.isfinite(o_t.view).all())
    o_bf.check("8385x5120x5120 EPI_BF16"); o_t.check("8385x5120x5120 EPI_BF16_T"); A.check("A"); W.check("W")
    _report("gemm pk 8385x5120x5120", max(w1, w2))


# ------------------------------------------------------------------------------------------------ attention
C_LOG2E = 1.4426950408889634


def _attn_buffers(q, k, v, k_lens, ld_pad=8):
    """q [B, Lq, H, D], k / v [B, Lk, H, D] (CPU bf16) -> guarded device operands.  k gets 64 more rows per sample; rows
    [k_lens[b], k_lens[b] + 64) hold KB.heavy_key() in every head, later rows NaN.  vt columns [k_lens[b], roundup(k_lens[b], 64)) are
    zero (the ABI's demand), later ones NaN.  q rows past Lq, everything beside the tensors: poison."""
    B, Lq, H, D = q.shape
    Lk, C = k.shape[1], H * D
    Q = KB.Guarded((B, Lq, C), BF, ld=C + ld_pad, device=DEV)
    Q.fill(q.reshape(B, Lq, C).to(DEV))
    Kb = KB.Guarded((B, Lk + 64, C), BF, ld=C + ld_pad, device=DEV)
    ldv = ops.round_up(Lk, 64)
    Vt = KB.Guarded((B, C, ldv), BF, ld=ldv + 8, device=DEV)
    kk = torch.full((B, Lk + 64, C), float("nan"), dtype=BF)
    vv = torch.full((B, C, ldv), float("nan"), dtype=BF)
    for b in range(B):
        n = k_lens[b]
        kk[b, :n] = k[b, :n].reshape(n, C)
        kk[b, n:n + 64] = KB.heavy_key(D).repeat(H)
        vv[b, :, :n] = v[b, :n].reshape(n, C).t()
        vv[b, :, n:ops.round_up(n, 64)] = 0
    Kb.fill(kk.to(DEV))
    Vt.fill(vv.to(DEV))
    Out = KB.Guarded((B, Lq, C), BF, ld=C + ld_pad, device=DEV)
    return Q, Kb, Vt, Out


def _check_attention(tag, out, q_eff, k, v, k_lens, guards):
    """out [B, Lq, C] against attention_bound per (sample, head); q_eff fp64 [B, Lq, H, D]."""
    B, Lq, H, D = q_eff.shape
    worst = 0.0
    o = out.float().cpu().reshape(B, Lq, H, D)
    for b in range(B):
        for h in range(H):
            ref, bound = KB.attention_bound(q_eff[b, :, h], k[b, :, h], v[b, :, h], D ** -0.5, k_lens[b])
            worst = max(worst, KB.assert_within(o[b, :, h], ref, bound, f"{tag} sample {b} head {h} (rows = queries)"))
    for name, gd in guards.items():
        gd.check(f"{tag} {name}")
    return _report(tag, worst)


def _run_attention(q, k, v, H, mode, k_lens=None, varlen=False):
    """mode: 'lazy' (attn_fast = 0, plain q), 'lazy_pre' (attn_fast = 0, pre-scaled q), 'maxfree' (attn_fast = 2, pre-scaled q),
    'default' (the dispatcher's own choice, plain q).  Returns (out Guarded, q_eff fp64, guards, variant)."""
    B, Lq = q.shape[:2]
    Lk = k.shape[1]
    k_lens = k_lens or [Lk] * B
    pre = mode in ("lazy_pre", "maxfree")
    c = ops.q_prescale(128)
    q_in = (q.float() * c).to(BF) if pre else q
    q_eff = q_in.double() / c if pre else q_in.double()
    Q, Kb, Vt, Out = _attn_buffers(q_in, k, v, k_lens)
    if mode != "default":
        ops.set_tuning("attn_fast", 2 if mode == "maxfree" else 0)
    try:
        if varlen:
            kw = dict(k_len=Lk, k_lens=torch.tensor(k_lens, device=DEV, dtype=torch.int32))
        else:
            assert len(set(k_lens)) == 1
            kw = dict(k_len=k_lens[0])
        ops.attention_fwd(Q.view, Kb.view, Vt.view, H, out=Out.view, q_prescaled=pre, workspace=ops.AttentionWorkspace(), **kw)
        variant = ops.get_tuning("last_attn_variant")
        torch.cuda.synchronize()
    finally:
        ops.set_tuning("attn_fast", 1)
    if mode != "default":
        assert variant & 15 == (2 if mode == "maxfree" else 1), (mode, variant)         # WAN_ATTN_VARIANT_W4_MAXFREE / _W4_LAZY
    if not varlen:
        plan = _lib.load().wan_attention_plan(B, Lq, k_lens[0], H, 128, 1 if pre else 0, 1 << 30)
        assert mode != "default" or plan == variant, (plan, variant)
    return Out, q_eff, {"q": Q, "k": Kb, "vt": Vt, "out": Out}, variant


def _decisive(B, L, H, seed):
    qs, ks, vs = zip(*[KB.decisive_qkv(L, H, seed + 1000 * b)[:3] for b in range(B)])
    return torch.stack(qs), torch.stack(ks), torch.stack(vs)


ATTN_L = [63, 64, 65, 191, 192, 193, 1025]


@pytest.mark.parametrize("mode", ["lazy", "lazy_pre", "maxfree"])
@pytest.mark.parametrize("L", ATTN_L)
def test_attention_decisive_keys_per_element(L, mode):
    """Lq = Lk at 64 j - 1 / 64 j / 64 j + 1 and 1025: key i decides row i, a heavy key waits behind the last one."""
    i = ATTN_L.index(L) + ["lazy", "lazy_pre", "maxfree"].index(mode)
    B, H = 1 + i % 2, (1, 3, 5)[i % 3]
    q, k, v = _decisive(B, L, H, seed=L)
    Out, q_eff, guards, variant = _run_attention(q, k, v, H, mode)
    _check_attention(f"attention {mode} B{B} H{H} L{L} [{_lib.ATTN_VARIANT_NAMES.get(variant & 15)}]", Out.view, q_eff, k, v, [L] * B, guards)
    # Lq != Lk: the query set truncated, and repeated past Lk
    idx = torch.cat([torch.arange(max(1, L - 37)), torch.arange(min(L, 50))])
    q2 = q[:, idx]
    Out, q_eff, guards, _ = _run_attention(q2, k, v, H, mode)
    _check_attention(f"attention {mode} B{B} H{H} Lq{len(idx)} Lk{L}", Out.view, q_eff, k, v, [L] * B, guards)


@pytest.mark.parametrize("mode", ["lazy", "maxfree"])
def test_attention_varlen_decisive_keys(mode):
    """wan_attention_fwd_varlen: per-sample key counts from device memory; behind each sample's last key 64 heavy keys, then NaN."""
    B, L, H = 2, 700, 3
    q, k, v = _decisive(B, L, H, seed=7)
    k_lens = [700, 321]
    Out, q_eff, guards, _ = _run_attention(q, k, v, H, mode, k_lens=k_lens, varlen=True)
    _check_attention(f"attention varlen {mode} k_lens {k_lens}", Out.view, q_eff, k, v, k_lens, guards)


@pytest.mark.parametrize("tail", [1, 0])
@pytest.mark.parametrize("mode", ["lazy_pre", "maxfree"])
def test_attention_split_tail_decisive_keys(mode, tail):
    """87 query blocks x 3 heads = 261 workgroups = one round + 5: the last blocks run split over the keys + a merge (attn_tail = 1)
    or as a second round (0).  Keys 1100 (17 full tiles + 12): the decisive key of a tail row sits in any of the splits."""
    Lq, Lk, H = 86 * 256 + 10, 1100, 3
    q, k, v = _decisive(1, Lk, H, seed=9)
    q = q[:, torch.arange(Lq) % Lk]
    ops.set_tuning("attn_tail", tail)
    try:
        Out, q_eff, guards, variant = _run_attention(q, k, v, H, mode)
    finally:
        ops.set_tuning("attn_tail", 1)
    assert bool(variant & _lib.ATTN_VARIANT_SPLIT_TAIL) == bool(tail), variant
    _check_attention(f"attention split tail={tail} {mode}", Out.view, q_eff, k, v, [Lk], guards)


@pytest.mark.parametrize("persist", [1, 0])
def test_cross_attention_persistent_form_decisive_keys(persist):
    """Lk = 512, 21 query blocks x 16 (batch, head) pairs: more blocks than CUs -> the persistent form walks them (attn_persist = 1);
    0: one workgroup per block.  Also with a key count that ends inside a tile (k_len = 300)."""
    B, Lq, Lk, H = 2, 256 * 20 + 37, 512, 8
    q, k, v = _decisive(B, Lk, H, seed=11)
    q = q[:, torch.arange(Lq) % Lk]
    assert ops.get_tuning("attn_persist") == 1
    ops.set_tuning("attn_persist", persist)
    try:
        for mode, kl in (("default", 512), ("lazy_pre", 512), ("default", 300)):
            Out, q_eff, guards, variant = _run_attention(q, k, v, H, mode, k_lens=[kl] * B)
            _check_attention(f"cross-attention persist={persist} {mode} k_len {kl}", Out.view, q_eff, k, v, [kl] * B, guards)
    finally:
        ops.set_tuning("attn_persist", 1)


def test_attention_random_shapes_per_element():
    """The cases of tests/test_gpu_fuzz.py::test_attention_random_shapes (same generator) under attention_bound: broad softmax rows."""
    rnd = random.Random(1)
    g = torch.Generator().manual_seed(1)
    worst = 0.0
    for _ in range(16):
        B = rnd.choice([1, 2])
        H = rnd.choice([1, 2, 5])
        Lq = rnd.choice([1, 31, 32, 33, 255, 256, 257, 700])
        Lk = rnd.choice([1, 63, 64, 65, 127, 128, 129, 512, 1000, 1025, 1600])
        q = (torch.randn(B, Lq, H, 128, generator=g) * rnd.choice([0.5, 1.0, 3.0])).to(BF)
        k = torch.randn(B, Lk, H, 128, generator=g).to(BF)
        v = torch.randn(B, Lk, H, 128, generator=g).to(BF)
        q[..., 0], k[..., 0] = 1.0, 0.0                       # channel 0 belongs to the heavy guard key (kernel_bounds.decisive_qkv)
        Out, q_eff, guards, _ = _run_attention(q, k, v, H, "default")
        worst = max(worst, _check_attention(f"attention random B{B} H{H} Lq{Lq} Lk{Lk}", Out.view, q_eff, k, v, [Lk] * B, guards))
    _report("attention random shapes", worst)


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("rows", [1, 5, 333])
@pytest.mark.parametrize("dim", [256, 1536, 5120, 640])
def test_ln_modulate_per_element(dim, rows):
    """Batch seams inside a workgroup's rows (rows_per_batch odd: the default kernel owns 2 rows per workgroup)."""
    g = torch.Generator().manual_seed(dim + rows)
    x = torch.randn(rows, dim, generator=g) * 2 + 0.3
    rpb = 1 if rows == 1 else (3 if rows == 5 else 111)
    nb = (rows + rpb - 1) // rpb
    sc, sh = torch.randn(nb, dim, generator=g) * 0.5, torch.randn(nb, dim, generator=g) * 0.5
    sel = torch.arange(rows) // rpb
    # x, scale, shift must be contiguous: guard ROWS before and after each
    Out = KB.Guarded((rows, dim), BF, device=DEV, rows_before=2, rows_after=4)
    xg = KB.Guarded((rows, dim), torch.float32, device=DEV, rows_before=1, rows_after=4)
    xg.fill(x.to(DEV))
    sg = KB.Guarded((nb, dim), torch.float32, device=DEV); sg.fill(sc.to(DEV))
    hg = KB.Guarded((nb, dim), torch.float32, device=DEV); hg.fill(sh.to(DEV))
    ops.ln_modulate(xg.view, sg.view, hg.view, True, rpb, 1e-6, out=Out.view)
    torch.cuda.synchronize()
    ref, bound = KB.ln_modulate_bound(x, sc[sel], sh[sel], True, 1e-6)
    w1 = KB.assert_within(Out.view, ref, bound, f"ln_modulate dim {dim} rows {rows} rows_per_batch {rpb}")
    for gd in (Out, xg, sg, hg):
        gd.check(f"ln_modulate dim {dim} rows {rows}")
    Out2 = KB.Guarded((rows, dim), BF, device=DEV)
    ops.ln_modulate(xg.view, sg.view[:1], hg.view[:1], False, rows, 1e-6, out=Out2.view)
    ref, bound = KB.ln_modulate_bound(x, sc[:1].expand(rows, dim), sh[:1].expand(rows, dim), False, 1e-6)
    w2 = KB.assert_within(Out2.view, ref, bound, f"ln affine dim {dim} rows {rows}")
    Out2.check("ln affine")
    _report(f"ln_modulate dim {dim} rows {rows}", max(w1, w2))


def _row_rotation(rows, grid, mode_args, token_offset, rows_per_batch):
    """cos / sin [rows, 64] fp64 of every row of the call, from the oracle's own rope_apply applied to the pairs (1, 0)."""
    F, Hp, Wp = grid
    fs, gr = mode_args
    basis = torch.zeros(rows_per_batch, 1, 128, dtype=torch.float64)
    basis[..., 0::2] = 1.0
    rot = O.rope_apply(basis, grid, O.rope_angles(128), fs, gr, token_offset=token_offset, total_tokens=F * Hp * Wp)
    cos, sin = rot[:, 0, 0::2].double(), rot[:, 0, 1::2].double()
    reps = (rows + rows_per_batch - 1) // rows_per_batch
    return cos.repeat(reps, 1)[:rows], sin.repeat(reps, 1)[:rows]


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("dim,rows,two", [(256, 1, True), (1536, 5, True), (5120, 333, True), (640, 333, False), (1536, 333, False)])
def test_rmsnorm_rope_per_element(dim, rows, two, rope):
    """In place on strided views inside one wide guarded buffer: [8 poison | x0 | 8 poison | x1 | 8 poison]; x0_scale; CoF rope map
    with token_offset > 0 and rows past the grid (not rotated), or no tables (the cross-attention form)."""
    g = torch.Generator().manual_seed(dim + rows + two)
    width = 2 * dim + 8 if two else dim                     # the guarded view spans x0, the 8 columns between, and x1
    wide = KB.Guarded((rows, width), BF, ld=width + 16, cols_before=8, rows_before=2, rows_after=4, device=DEV)
    x0 = torch.randn(rows, dim, generator=g).to(BF)
    x1 = (torch.randn(rows, dim, generator=g) * 3).to(BF)
    w0, w1 = torch.rand(dim, generator=g) + 0.5, torch.rand(dim, generator=g) + 0.5
    v0 = wide.view[:, :dim]
    v0.copy_(x0.to(DEV))
    v1 = None
    if two:
        v1 = wide.view[:, dim + 8:2 * dim + 8]
        v1.copy_(x1.to(DEV))
    c = ops.q_prescale(128)
    rp, tables, rot = None, None, None
    if rope:
        grid, fs, gr, off = (3, 3, 5), 1, (1, 2), 4
        rpb = rows if rows < 200 else 111
        rp = RopeParams(*grid, 2, fs, gr[1], off, rpb, 1024)
        ang = O.rope_angles(128)
        tables = (ang.cos().float().contiguous().to(DEV), ang.sin().float().contiguous().to(DEV))
        rot = _row_rotation(rows, grid, (fs, gr), off, rpb)
    ops.rmsnorm_rope_(v0, w0.to(DEV), v1, None if v1 is None else w1.to(DEV), 128, 1e-6, tables, rp, x0_scale=c)
    torch.cuda.synchronize()
    ref, bound = KB.rmsnorm_rope_bound(x0, w0, 1e-6, c, rot)
    worst = KB.assert_within(v0, ref, bound, f"rmsnorm_rope x0 dim {dim} rows {rows} rope {rope}")
    if two:
        ref, bound = KB.rmsnorm_rope_bound(x1, w1, 1e-6, 1.0, rot)
        worst = max(worst, KB.assert_within(v1, ref, bound, f"rmsnorm_rope x1 dim {dim} rows {rows} rope {rope}"))
    # the columns between and beside the two views
    if two:
        assert bool((wide.view[:, dim:dim + 8].contiguous().view(torch.int16) == KB.POISON16).all()), "columns between x0 and x1 were written"
    wide.check(f"rmsnorm_rope dim {dim} rows {rows}")
    _report(f"rmsnorm_rope dim {dim} rows {rows} two {two} rope {rope}", worst)
