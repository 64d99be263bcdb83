"""-m gpu: the folded cross-attention branch (include/wan_hip.h a9f, videocof_amd/csrc/cross_fold.hip).

* wan_cross_probs and wan_cross_fold_values, element by element, against a float64 evaluation of the same formula on the same
  bf16 inputs, with bounds DERIVED from the number formats and the operation counts (docs/TEST_BOUNDS.md, "The cross-attention
  fold"); the text rows are built the reference's way -- zero rows behind every prompt BEFORE the embedding -- so the rows behind
  the longest prompt are truly identical; q / k carry one large same-sign channel per head (bench.py --attn-stress);
* the branch on one model, tuning key "cross_fold" = 2 against 0: both against the fp32 oracle block, the folded path no further
  from it than the plain path plus the bound of the swapped rounding; composite == per-op bit for bit with the fold on; B = 2
  with unequal prompts; a 64-token prompt stays on the plain branch.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_bounds as KB  # noqa: E402
from oracle import wan_oracle as O  # noqa: E402
from videocof_amd import WanTransformer3DModel, ops  # noqa: E402
from videocof_amd.weights import deterministic_dit_state_dict, det_uniform  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 512
QS = ops.q_prescale(128)          # softmax_scale * log2(e): what wan_rmsnorm_rope's x0_scale leaves in the cross-attention q
SENTINEL = -7.0          # guard rows / columns of the output buffers: no kernel result is negative (P) or needs this value

# (prompt lengths of the batch, kept): kept >= the longest prompt, kept + 1 <= 64.  (62, 62) with kept = 63 scores one padding row
# on its own in front of the representative -- "63 -> 62".
CASES = [((1,), 1), ((1, 37), 37), ((62, 63), 63), ((62, 62), 63)]


def text_kv(H, lens, seed):
    """Text k [B, 512, C] and v^T [B, C, 512] (bf16, CPU) from prompts zero-padded BEFORE an embedding with a bias, as
    text_embedding does: every row behind a prompt is the embedding of a zero row.  Channel 5 of every head of k is 12."""
    C, g = 128 * H, torch.Generator().manual_seed(seed)
    raw = torch.zeros(len(lens), T, 32, dtype=torch.float64)
    for b, n in enumerate(lens):
        raw[b, :n] = torch.randn(n, 32, generator=g, dtype=torch.float64)
    w0, b0 = torch.randn(32, C, generator=g, dtype=torch.float64) / math.sqrt(32), torch.randn(C, generator=g, dtype=torch.float64)
    ctx = torch.tanh(raw @ w0 + b0)
    wk, wv = (torch.randn(C, C, generator=g, dtype=torch.float64) / math.sqrt(C) * 1.5 for _ in range(2))
    k, v = ctx @ wk, ctx @ wv + 0.3
    k.view(len(lens), T, H, 128)[..., 5] = 12.0
    k, v = k.to(torch.bfloat16), v.to(torch.bfloat16)
    for b, n in enumerate(lens):
        assert bool((k[b, n:] == k[b, n]).all()) and bool((v[b, n:] == v[b, n]).all())
    return k, v.transpose(1, 2).contiguous()


def queries(B, L, H, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, L, H, 128, generator=g, dtype=torch.float64) * 1.3 * QS
    q[..., 5] = 12.0 * QS              # same sign as k's channel 5: a common term of 144 * scale * log2(e) ~ 18 in every score
    return q.reshape(B, L, H * 128).to(torch.bfloat16)


def probs_ref(q, k, H, kept):
    """fp64: softmax over keys 0..kept of every head in the exp2 domain, key `kept` counted T - kept times.
    Returns (p [B, L, H, kept + 1], S [B, L, H, 1] = the largest sum_d |q_d k_d| + log2(T - kept) of the row)."""
    B, L, _ = q.shape
    qd, kd = q.double().view(B, L, H, 128), k.double()[:, :kept + 1].reshape(B, kept + 1, H, 128)
    s = torch.einsum("blhd,bjhd->blhj", qd, kd)
    s[..., kept] += math.log2(T - kept)
    mag = torch.einsum("blhd,bjhd->blhj", qd.abs(), kd.abs()).max(dim=-1, keepdim=True).values + math.log2(T - kept)
    return torch.softmax(s * math.log(2.0), dim=-1), mag


def probs_bound(p, S):
    """Per element  p (2^-8 + s + f) + 2^-120  (docs/TEST_BOUNDS.md):
    * 2^-8 p: the ONE rounding of the normalised fp32 probability to bf16 (RNE);
    * s = 2 (2^d - 1), d = 2^-23 (132 S + 4): a score is a 128-term fp32 MFMA sum (128 2^-23 sum_d |q_d k_d|, as gemm_acc_term), the
      representative's gets log2f(pad_count) (1 ulp, <= 9 2^-23) added (one rounding), and the subtraction of the row maximum rounds
      once more (both <= 2^-24 2 S) -- d bounds the log2-domain error of s_j - m; every exp2 moves by a factor within 2^(+-d), the
      numerator and the row sum both;
    * f = 2^-24 (2 + 64 + 2 + 1): v_exp_f32 (1 ulp), 64 additions of non-negative terms into the row sum in any order, v_rcp_f32
      (1 ulp), the final multiply;
    * 2^-120: exp2 results below the normal range are flushed."""
    d = 2.0 ** -23 * (132.0 * S + 4.0)
    s = 2.0 * (torch.exp2(d) - 1.0)
    return p * (KB.U_BF16 + s + KB.U_F32 * 69.0) + 2.0 ** -120


@pytest.fixture(scope="module")
def kv_cache():
    cache = {}

    def get(H, lens):
        if (H, lens) not in cache:
            cache[H, lens] = text_kv(H, lens, seed=100 * H + sum(lens))
        return cache[H, lens]
    return get


@pytest.mark.parametrize("lens,kept", CASES)
@pytest.mark.parametrize("L", [8, 264, 520])
@pytest.mark.parametrize("H", [2, 8])
def test_cross_probs_elementwise(H, L, lens, kept, kv_cache):
    B = len(lens)
    k, _ = kv_cache(H, lens)
    q = queries(B, L, H, seed=L + H)
    ref, S = probs_ref(q, k, H, kept)
    # guard band: 8 sentinel rows behind the result and 8 sentinel columns beside it (ldp = H * 64 + 8)
    buf = torch.full((B * L + 8, H * 64 + 8), SENTINEL, device=DEV, dtype=torch.bfloat16)
    out = ops.cross_probs(q.to(DEV), k.to(DEV), H, kept, T - kept, out=buf[:B * L, :H * 64])
    torch.cuda.synchronize()
    full = buf.cpu()
    assert bool((full[B * L:] == SENTINEL).all()) and bool((full[:, H * 64:] == SENTINEL).all()), "write outside the result"
    got = out.cpu().reshape(B, L, H, 64)
    assert bool((got[..., kept + 1:] == 0).all()), "columns above kept must be exact zeros"
    err = (got[..., :kept + 1].double() - ref).abs()
    bound = probs_bound(ref, S)
    worst = float((err / bound).max())
    print(f"cross_probs H={H} L={L} lens={lens} kept={kept}: max err/bound {worst:.3f}, max |err| {float(err.max()):.3e}, "
          f"row sums in [{float(got.double().sum(-1).min()):.5f}, {float(got.double().sum(-1).max()):.5f}]")
    assert worst <= 1.0
    # the representative carries the mass of all T - kept identical rows: against the plain 512-key softmax of the same inputs
    kd = k.double().view(B, T, H, 128)
    p512 = torch.softmax(torch.einsum("blhd,bjhd->blhj", q.double().view(B, L, H, 128), kd) * math.log(2.0), dim=-1)
    assert float((p512[..., kept:].sum(-1) - ref[..., kept]).abs().max()) < 1e-12
    assert float((p512[..., :kept] - ref[..., :kept]).abs().max()) < 1e-12


@pytest.mark.parametrize("lens,kept", CASES)
@pytest.mark.parametrize("H", [2, 8])
def test_cross_fold_values_elementwise(H, lens, kept, kv_cache):
    B, C = len(lens), 128 * H
    _, vt = kv_cache(H, lens)
    g = torch.Generator().manual_seed(7 + H)
    w = (torch.randn(C, C, generator=g) / math.sqrt(C)).to(torch.bfloat16)
    buf = torch.full((B, C + 8, H * 64 + 8), SENTINEL, device=DEV, dtype=torch.bfloat16)
    out = ops.cross_fold_values(w.to(DEV), vt.to(DEV), H, kept, out=buf[:, :C, :H * 64])
    torch.cuda.synchronize()
    full = buf.cpu()
    assert bool((full[:, C:] == SENTINEL).all()) and bool((full[:, :, H * 64:] == SENTINEL).all()), "write outside the result"
    got = out.cpu().reshape(B, C, H, 64)
    assert bool((got[..., kept + 1:] == 0).all()), "columns above kept must be exact zeros"
    worst = 0.0
    for b in range(B):
        for h in range(H):
            wh = w[:, h * 128:(h + 1) * 128]                              # [C, 128]
            vh = vt[b, h * 128:(h + 1) * 128, :kept + 1].t()               # [kept + 1, 128]
            ref = KB.gemm_ref(wh, vh)
            # one bf16 rounding + fp32 accumulation over 128 terms (tests/kernel_bounds.py, gemm_bound)
            bound = KB.gemm_bound(wh, vh, None, 128, torch.bfloat16, ref=ref)
            worst = max(worst, float(((got[b, :, h, :kept + 1].double() - ref).abs() / bound).max()))
    print(f"cross_fold_values H={H} lens={lens} kept={kept}: max err/bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ the branch
def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def small_model():
    dims = dict(dim=256, ffn_dim=512, num_layers=1, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64)
    m.load_state_dict(deterministic_dit_state_dict(**dims), device=DEV)
    yield m
    ops.set_tuning("cross_fold", 1)


def _block_inputs(m, lens):
    B, L, C = len(lens), 420, 256
    context = [det_uniform(f"cf.c{b}", (n, 64), 1.0).to(DEV) for b, n in enumerate(lens)]
    ctx = m._text_embed(context).view(B, T, C).float()                      # zero rows padded BEFORE text_embedding
    x = det_uniform("cf.x", (B, L, C), 1.0).to(DEV)
    e = det_uniform("cf.e", (B, 6, C), 0.3).to(DEV)
    return x, e, ctx


def _run(m, x, e, ctx, kept, mode, composite):
    ops.set_tuning("cross_fold", mode)
    m.use_block_composite = composite
    try:
        out = m.block_forward(x, e, ctx, (7, 6, 10), 0, [3] * x.shape[0], [(3, 4)] * x.shape[0], text_kept=kept)
        torch.cuda.synchronize()
        return out.clone(), m.last_cross_fold
    finally:
        m.use_block_composite = True
        ops.set_tuning("cross_fold", 1)


def swapped_rounding_bound(m, x, e, ctx, kept, ref):
    """What the two branches may differ by, relative to |ref|, to first order -- DERIVED from the weights and the inputs, in fp64:
    the plain branch rounds the attention output `att` to bf16 (|d c| <= 2^-8 |att| |W_co|^T), the folded branch rounds V' instead
    (|d c| <= 2^-8 P |V'|); swapping removes the first and adds the second, and in the worst case the removed one was cancelling an
    error, so both are allowed.  A perturbation d c of the cross-attention term reaches the block output as d c + J_ffn d c with
    |J_ffn|_2 <= max|gate| |W2|_2 1.13 |W0|_2 max|1 + scale| max rstd (GELU slope 1.13; LayerNorm's Jacobian is bounded by rstd)."""
    sd = {k_: v.detach().double().cpu() for k_, v in m.state_dict().items()}
    B, L, C = x.shape
    H, pre = 2, "blocks.0"
    cfg = O.DiTConfig(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64)
    num = 0.0
    lip = 0.0
    for b in range(B):
        xb, eb, cb = x[b].double().cpu(), e[b].double().cpu(), ctx[b].double().cpu()
        em = sd[pre + ".modulation"][0] + eb
        h = O.ln_modulate(xb, em[1], em[0], cfg.eps)
        y = O.self_attention(h, sd, pre + ".self_attn", cfg, (7, 6, 10), O.rope_angles(128), 3, (3, 4), L)
        x1 = xb + y * em[2]
        h3 = O.layer_norm(x1, cfg.eps, sd[pre + ".norm3.weight"], sd[pre + ".norm3.bias"])
        ca = pre + ".cross_attn"
        q = O.rms_norm(O.linear(h3, sd, ca + ".q"), sd[ca + ".norm_q.weight"], cfg.eps).view(L, H, 128)
        k = O.rms_norm(O.linear(cb, sd, ca + ".k"), sd[ca + ".norm_k.weight"], cfg.eps).view(T, H, 128)
        v = O.linear(cb, sd, ca + ".v").view(T, H, 128)
        p = torch.softmax(torch.einsum("lhd,jhd->lhj", q, k) / math.sqrt(128), dim=-1)            # [L, H, 512]
        att = torch.einsum("lhj,jhd->lhd", p, v).reshape(L, C)
        wo = sd[ca + ".o.weight"]
        d_att = KB.U_BF16 * (att.abs() @ wo.abs().t())
        vfold = torch.einsum("jhd,nhd->hjn", v, wo.view(C, H, 128))                               # V' [H, 512, C]
        d_v = KB.U_BF16 * torch.einsum("lhj,hjn->ln", p, vfold.abs())
        num += float((d_att + d_v).norm() ** 2)
        x2 = x1 + att @ wo.t() + sd[ca + ".o.bias"]
        rstd = 1.0 / torch.sqrt(x2.var(dim=-1, unbiased=False) + cfg.eps)
        lip = max(lip, float(em[5].abs().max() * torch.linalg.matrix_norm(sd[pre + ".ffn.2.weight"], ord=2) * KB.GELU_SLOPE
                             * torch.linalg.matrix_norm(sd[pre + ".ffn.0.weight"], ord=2) * (1.0 + em[4]).abs().max() * rstd.max()))
    return math.sqrt(num) * (1.0 + lip) / float(ref.double().norm())


@pytest.mark.parametrize("lens", [(37,), (5, 37)])
def test_branch_against_the_oracle_and_composite_is_bitwise(small_model, lens):
    m = small_model
    x, e, ctx = _block_inputs(m, lens)
    kept = max(lens)
    plain, ran0 = _run(m, x, e, ctx, kept, 0, True)
    fold_c, ran_c = _run(m, x, e, ctx, kept, 2, True)
    fold_p, ran_p = _run(m, x, e, ctx, kept, 2, False)
    by_rule, ran1 = _run(m, x, e, ctx, kept, 1, True)
    assert (ran0, ran_c, ran_p, ran1) == (False, True, True, False)      # the rule keeps H * 64 = 128 and 420 rows on the plain branch
    assert torch.equal(fold_c, fold_p), "composite and per-op launches must be bit-identical with the fold on"
    assert torch.equal(by_rule, plain)
    cfg = O.DiTConfig(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64)
    osd = {k_: v.detach().float() for k_, v in m.state_dict().items()}
    ref = torch.stack([O.block_forward(x[b], e[b], ctx[b], osd, 0, cfg, (7, 6, 10), O.rope_angles(128), 3, (3, 4), 420)
                       for b in range(len(lens))])
    r_plain, r_fold = rel_l2(plain, ref), rel_l2(fold_c, ref)
    allow = swapped_rounding_bound(m, x, e, ctx, kept, ref)
    print(f"block vs fp32 oracle, lens={lens}: plain rel-L2 {r_plain:.4e}, folded rel-L2 {r_fold:.4e}, swapped-rounding bound {allow:.4e}, "
          f"folded vs plain {rel_l2(fold_c, plain):.4e}")
    assert r_fold <= r_plain + allow
    assert r_plain < 1e-2 and r_fold < 1e-2


def test_a_64_token_prompt_takes_the_plain_branch(small_model):
    m = small_model
    x, e, ctx = _block_inputs(m, (64,))
    x63, e63, ctx63 = _block_inputs(m, (63,))
    for composite in (True, False):
        _, ran = _run(m, x, e, ctx, 64, 2, composite)           # 65 distinct keys per head
        assert ran is False
        _, ran = _run(m, x63, e63, ctx63, 63, 2, composite)     # 64 distinct keys: the largest prompt that folds
        assert ran is True
        if composite:
            assert ops.get_tuning("last_cross_fold") == 1       # what wan_dit_block_forward itself reports
    _, ran = _run(m, x, e, ctx, None, 2, True)                  # prompt length not known
    assert ran is False
    assert ops.get_tuning("last_cross_fold") == 0


def test_forward_passes_the_prompt_lengths(small_model):
    """WanTransformer3DModel.forward hands the longest prompt of the call to the blocks (forward composite and block loop alike):
    with "cross_fold" = 2 the model folds and stays within the oracle tolerance of __graft_entry__.smoke()."""
    m = small_model
    lat = det_uniform("cf.lat", (2, 16, 7, 12, 20), 1.0).to(DEV)
    ctx = [det_uniform("cf.p0", (37, 64), 1.0).to(DEV), det_uniform("cf.p1", (5, 64), 1.0).to(DEV)]
    t = torch.tensor([899, 899], device=DEV)
    kw = dict(frame_split_indices=[3, 3], ground_frame_indices=[(3, 4), (3, 4)])
    plain = m(lat, t, ctx, 420, **kw).float()
    assert m.last_cross_fold is False
    ops.set_tuning("cross_fold", 2)
    try:
        folded = m(lat, t, ctx, 420, **kw).float()
        assert m.last_cross_fold is True and m._text_kept == 37
        m.use_forward_composite = False
        folded_loop = m(lat, t, ctx, 420, **kw).float()
        assert m.last_cross_fold is True
    finally:
        m.use_forward_composite = True
        ops.set_tuning("cross_fold", 1)
    assert torch.equal(folded, folded_loop)
    cfg = O.DiTConfig(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64)
    sd = {k_: v.detach().float().cpu() for k_, v in m.state_dict().items()}
    ref = O.dit_forward(sd, cfg, lat.cpu(), t.cpu(), [c.cpu() for c in ctx], 420, [3, 3], [(3, 4), (3, 4)])
    r_plain, r_fold = rel_l2(plain.cpu(), ref), rel_l2(folded.cpu(), ref)
    print(f"forward vs fp32 oracle: plain rel-L2 {r_plain:.3e}, folded rel-L2 {r_fold:.3e}")
    assert r_plain < 2e-2 and r_fold < 2e-2
