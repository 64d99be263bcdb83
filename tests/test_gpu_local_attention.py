"""-m gpu: local self-attention -- wan_attention_fwd_sparse per element against fp64 attention over the gathered keys of
every query block's list (bounds: tests/kernel_bounds.py), bit for bit against the dense kernel where every tile is listed, and the
model / pipeline switches around it.  Inputs are the decisive-key inputs of kernel_bounds: key i decides query row i, and a key that
would take all the mass of every row (heavy_key) sits wherever the kernel must not read -- behind the last key, and in one physical
tile that no list names."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_bounds as KB  # noqa: E402
from videocof_amd import (FlowUniPCMultistepScheduler, GraphedLoop, WanPipeline, WanTransformer3DModel, _lib, ops)  # noqa: E402
from videocof_amd.local_attention import (LocalAttentionPlan, local_attention_plan, plan_from_blocks, reference_sparse_attention)  # noqa: E402
from videocof_amd.weights import deterministic_dit_state_dict, det_uniform  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
D = 128


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


@functools.lru_cache(maxsize=None)
def _decisive(B, L, H, seed):
    """Computed once per shape, shared by the tests that use it, never written to."""
    qs, ks, vs = zip(*[KB.decisive_qkv(L, H, seed + 1000 * b)[:3] for b in range(B)])
    return torch.stack(qs), torch.stack(ks), torch.stack(vs)


def _lists_plan(rows, Lq, Lk):
    blocks = np.zeros((-(-Lq // 256), -(-Lk // 64)), dtype=bool)
    for i, row in enumerate(rows):
        blocks[i, list(row)] = True
    return plan_from_blocks(blocks, Lq, Lk)


def _device_plan(host: LocalAttentionPlan):
    return ops.AttnSparsePlan(host.row_ptr, host.tiles, host.q_len, host.k_len, DEV)


def _buffers(q, k, v, Lk):
    """q [B, Lq, H, D], k / v [B, Lk, H, D] (CPU bf16) -> guarded device operands: k has 64 more rows holding heavy_key() in every
    head, V^T's pad columns [Lk, roundup(Lk, 64)) are zero (the ABI's demand), everything beside the tensors is poison (NaN)."""
    B, Lq, H, _ = q.shape
    C = H * D
    Q = KB.Guarded((B, Lq, C), BF, ld=C + 8, device=DEV)
    Q.fill(q.reshape(B, Lq, C).to(DEV))
    Kb = KB.Guarded((B, Lk + 64, C), BF, ld=C + 8, device=DEV)
    ldv = ops.round_up(Lk, 64)
    Vt = KB.Guarded((B, C, ldv), BF, ld=ldv + 8, device=DEV)
    kk = torch.empty(B, Lk + 64, C, dtype=BF)
    kk[:, :Lk] = k.reshape(B, Lk, C)
    kk[:, Lk:] = KB.heavy_key(D).repeat(H)
    vv = torch.zeros(B, C, ldv, dtype=BF)
    vv[:, :, :Lk] = v.reshape(B, Lk, C).transpose(1, 2)
    Kb.fill(kk.to(DEV))
    Vt.fill(vv.to(DEV))
    Out = KB.Guarded((B, Lq, C), BF, ld=C + 8, device=DEV)
    return Q, Kb, Vt, Out


def _prescale(q, pre):
    """(the q the kernel is given, the fp64 q it therefore computes with at scale 1 / sqrt(D))"""
    if not pre:
        return q, q.double()
    c = ops.q_prescale(D)
    q_in = (q.float() * c).to(BF)
    return q_in, q_in.double() / c


def _check_blocks(tag, out, q_eff, k, v, host, Lk):
    """out [B, Lq, C] per (sample, head, query block) against attention_bound over the block's gathered keys."""
    B, Lq, H, _ = q_eff.shape
    o = out.float().cpu().reshape(B, Lq, H, D)
    worst = 0.0
    for i in range(host.n_qblocks):
        keys = (torch.as_tensor(host.row(i).astype(np.int64))[:, None] * 64 + torch.arange(64)[None, :]).reshape(-1)
        keys = keys[keys < Lk]
        r0, r1 = i * 256, min((i + 1) * 256, Lq)
        for b in range(B):
            for h in range(H):
                ref, bound = KB.attention_bound(q_eff[b, r0:r1, h], k[b, keys, h], v[b, keys, h], D ** -0.5)
                worst = max(worst, KB.assert_within(o[b, r0:r1, h], ref, bound, f"{tag} sample {b} head {h} block {i} lists {list(host.row(i))}"))
    print(f"{tag}: worst |err| / bound = {worst:.3f}")
    return worst


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("pre", [False, True], ids=["plain_q", "prescaled_q"])
def test_full_list_equals_the_dense_kernel_bit_for_bit(pre):
    """B = 2, H = 3, Lq = Lk = 1 100: 17 full tiles + 12 keys, 5 query blocks with a tail.  The dense call is the one-launch lazy form
    (which is what this shape is given: asserted)."""
    B, H, L = 2, 3, 1100
    q, k, v = _decisive(B, L, H, 11)
    q_in, _ = _prescale(q, pre)
    Q, Kb, Vt, Out = _buffers(q_in, k, v, L)
    dense = ops.attention_fwd(Q.view, Kb.view, Vt.view, H, k_len=L, q_prescaled=pre, workspace=ops.AttentionWorkspace())
    assert ops.get_tuning("last_attn_variant") & ~_lib.ATTN_VARIANT_XCD_PINNED == 1           # WAN_ATTN_VARIANT_W4_LAZY, no split tail
    host = _lists_plan([range(18)] * 5, L, L)
    plan = _device_plan(host)
    assert plan.listed == 5 * 18 and plan.density == 1.0
    got = ops.attention_fwd_sparse(Q.view, Kb.view, Vt.view, H, plan, k_len=L, q_prescaled=pre, out=Out.view)
    variant = ops.get_tuning("last_attn_variant")
    torch.cuda.synchronize()
    assert variant & 15 == 1 and variant & _lib.ATTN_VARIANT_SPARSE
    assert got.data_ptr() == Out.view.data_ptr() and torch.equal(Out.view, dense)
    for g in (Q, Kb, Vt, Out):
        g.check("full list")


# query block -> (the physical tiles its 256 queries are drawn from, the tiles it lists).  Lk = 1 100: tiles 0..16 full, tile 17 holds
# 12 keys.  1, 2, 3, 4 and 5 listed tiles (peeled-only, odd and even steady-state counts), non-consecutive lists, lists that end on the
# partial physical tile (blocks 2, 4) and lists that do not; tiles 7 and 11 are listed by nobody and tile 7 holds heavy keys.
HAND = [((2,), (2,)), ((5, 6), (5, 6)), ((9,), (3, 9, 17)), ((12, 13), (0, 4, 12, 13)), ((16, 17), (1, 8, 14, 16, 17)), ((10,), (10, 15))]
HAND_LQ, HAND_LK, UNLISTED = 5 * 256 + 100, 1100, 7


@pytest.mark.parametrize("pre", [False, True], ids=["plain_q", "prescaled_q"])
def test_hand_made_lists_per_element(pre):
    B, H = 2, 3
    q, k, v = _decisive(B, HAND_LK, H, 11)
    idx = []
    for i, (own, _) in enumerate(HAND):
        keys = torch.cat([torch.arange(64 * t, min(64 * t + 64, HAND_LK)) for t in own])
        rows = min(256, HAND_LQ - 256 * i)
        idx.append(keys[torch.arange(rows) % keys.numel()])              # every query's decisive key lies in a diagonal tile
    q = q[:, torch.cat(idx)]
    k = k.clone()
    k[:, 64 * UNLISTED:64 * UNLISTED + 64] = KB.heavy_key(D)             # read by a wrong tile address, it takes every row
    assert all(UNLISTED not in lists for _, lists in HAND)
    q_in, q_eff = _prescale(q, pre)
    Q, Kb, Vt, Out = _buffers(q_in, k, v, HAND_LK)
    host = _lists_plan([lists for _, lists in HAND], HAND_LQ, HAND_LK)
    assert sorted(np.diff(host.row_ptr)) == [1, 2, 2, 3, 4, 5]
    plan = _device_plan(host)
    ops.attention_fwd_sparse(Q.view, Kb.view, Vt.view, H, plan, k_len=HAND_LK, q_prescaled=pre, out=Out.view)
    torch.cuda.synchronize()
    _check_blocks(f"hand-made lists ({'pre-scaled' if pre else 'plain'} q)", Out.view, q_eff, k, v, host, HAND_LK)
    for g in (Q, Kb, Vt, Out):
        g.check("hand-made lists")


def test_the_plan_of_a_small_cof_grid_per_element():
    """Grid (11, 6, 20), n = 5, G = 1, window (1, 2): L = 1 320 (20 full tiles + 40 keys), 6 query blocks listing 14..21 tiles."""
    H, L = 2, 1320
    host = local_attention_plan((11, 6, 20), [5], [(5, 6)], 1, 2)
    assert (host.n_qblocks, host.n_ktiles, int(np.diff(host.row_ptr).min())) == (6, 21, 14)
    q, k, v = _decisive(1, L, H, 23)
    q_in, q_eff = _prescale(q, True)
    Q, Kb, Vt, Out = _buffers(q_in, k, v, L)
    plan = _device_plan(host)
    assert abs(plan.density - 0.88095) < 1e-5
    ops.attention_fwd_sparse(Q.view, Kb.view, Vt.view, H, plan, k_len=L, q_prescaled=True, out=Out.view)
    torch.cuda.synchronize()
    _check_blocks("plan (11, 6, 20) / (1, 2)", Out.view, q_eff, k, v, host, L)
    for g in (Q, Kb, Vt, Out):
        g.check("small CoF plan")


def test_calls_that_do_not_fit_the_plan_are_refused():
    H, L = 1, 300
    plan = _device_plan(_lists_plan([(0, 1), (4,)], L, L))
    q = torch.zeros(1, L, H * D, device=DEV, dtype=BF)
    vt = torch.zeros(1, H * D, 320, device=DEV, dtype=BF)
    with pytest.raises(ValueError, match="the plan was made for"):
        ops.attention_fwd_sparse(q[:, :200], q, vt, H, plan)
    with pytest.raises(ValueError, match="the plan was made for"):
        ops.attention_fwd_sparse(q, q, vt, H, plan, k_len=299)
    with pytest.raises(ValueError, match="beyond the last"):
        ops.AttnSparsePlan([0, 1, 2], [0, 5], L, L, DEV)
    plan.close()
    with pytest.raises(ValueError, match="live"):
        ops.attention_fwd_sparse(q, q, vt, H, plan)


# ------------------------------------------------------------------------------------------------ model
TINY = dict(dim=256, ffn_dim=512, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)
GRID, N_SRC, SEQ = (11, 6, 20), 5, 1320
# a bf16 forward against the same forward with fp32 math in one place: the bound of the forward against the fp32 oracle
# (__graft_entry__.smoke, tests/test_gpu_dit.py: rel-L2 < 2e-2)
MODEL_TOL = 2e-2


@pytest.fixture(scope="module")
def sd():
    return deterministic_dit_state_dict(**TINY)


@pytest.fixture()
def model(sd):
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    m.load_state_dict(sd, device=DEV)
    ops.set_tuning("attn_fast", 0)            # no max-free attempt: the dense launches are the lazy form the sparse one is
    yield m
    ops.set_tuning("attn_fast", 1)


def _forward(m):
    lat = det_uniform("local.lat", (1, 16, GRID[0], 2 * GRID[1], 2 * GRID[2]), 1.0).to(DEV)
    ctx = [det_uniform("local.ctx", (37, 64), 1.0).to(DEV)]
    return m(lat, torch.tensor([749], device=DEV), ctx, SEQ, frame_split_indices=[N_SRC], ground_frame_indices=[(N_SRC, N_SRC + 1)])


def test_model_full_windows_equal_the_dense_forward(model):
    dense = _forward(model)
    model.use_forward_composite = model.use_block_composite = False
    per_kernel = _forward(model)
    model.use_forward_composite = model.use_block_composite = True
    model.enable_local_attention(N_SRC, GRID[1])
    assert model.local_attention == dict(window_frames=N_SRC, window_rows=GRID[1], sink_frames=1, dense_layers=())
    local = _forward(model)
    assert ops.get_tuning("last_attn_variant") & 15 == 1                      # (the last launch of a forward is the cross-attention)
    plan = model._local_plan_last
    assert plan.density == 1.0 and (plan.n_qblocks, plan.n_ktiles) == (6, 21)
    assert torch.equal(local, per_kernel) and torch.equal(local, dense)
    model.disable_local_attention()
    assert model.local_attention is None and torch.equal(_forward(model), dense)


def test_model_narrow_window_is_the_reference_over_the_listed_keys(model):
    from videocof_amd import wan_transformer3d as W
    dense = _forward(model)
    model.enable_local_attention(1, 1)
    seen = []
    real = ops.attention_fwd_sparse

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append(ops.get_tuning("last_attn_variant"))
        return out

    class Proxy:
        def __init__(self, fn):
            self.attention_fwd_sparse = fn

        def __getattr__(self, name):
            return getattr(ops, name)

    def reference(q, k, vt, H, plan, k_len=None, out=None, q_prescaled=False):
        """q carries softmax_scale * log2(e): exp2(q.k) = exp(q.k ln 2)"""
        assert q_prescaled and out is not None
        host = local_attention_plan(GRID, [N_SRC], [(N_SRC, N_SRC + 1)], 1, 1, q_len=q.shape[1])
        assert host.listed == plan.listed
        v = vt[:, :, :k_len].transpose(1, 2)
        out.copy_(reference_sparse_attention(q, k[:, :k_len], v, host, math.log(2.0)).to(BF))
        return out

    try:
        W.ops = Proxy(spy)
        local = _forward(model)
        W.ops = Proxy(reference)
        want = _forward(model)
    finally:
        W.ops = ops
    assert len(seen) == 2 and all(v & 15 == 1 and v & _lib.ATTN_VARIANT_SPARSE for v in seen)       # both layers
    assert model._local_plan_last.density < 0.9
    r_dense, r_ref = rel_l2(local, dense), rel_l2(local, want)
    print(f"window (1, 1): density {model._local_plan_last.density:.4f}, rel-L2 vs dense {r_dense:.3e}, vs the reference over the listed keys {r_ref:.3e}")
    assert not torch.equal(local, dense) and r_dense > r_ref
    assert r_ref < MODEL_TOL
    model.enable_local_attention(1, 1, dense_layers=(0, 1))
    assert torch.equal(_forward(model), dense)
    model.enable_local_attention(1, 1, dense_layers=(1,))
    one = _forward(model)
    assert not torch.equal(one, dense) and not torch.equal(one, local)


def test_model_refusals_and_graph_capture(model):
    from videocof_amd import GraphedForward
    model.enable_local_attention(1, 1)
    eager = _forward(model)
    model.enable_fp8_linear(("attn",))
    with pytest.raises(NotImplementedError, match="fp8"):
        _forward(model)
    model.disable_fp8_linear()
    model.force_ulysses = True
    from videocof_amd.dist import EmulatedRank
    model._sp, sp = EmulatedRank(0, 1), model._sp
    try:
        with pytest.raises(NotImplementedError, match="Ulysses"):
            _forward(model)
    finally:
        model.force_ulysses, model._sp = False, sp
    with pytest.raises(NotImplementedError, match="capture_graph='loop'"):
        GraphedLoop(model)((), torch.zeros(1, device=DEV), [], lambda x, c: x)
    with pytest.raises(ValueError):
        model.enable_local_attention(1, 1, dense_layers=(2,))
    # one hipGraph per forward: the eager warm-up call builds the plan, the capture and the replays read it
    g = GraphedForward(model)
    outs = [_forward(g) for _ in range(3)]
    assert g.replays == 2 and all(torch.equal(o, eager) for o in outs)
    model.disable_local_attention()
    assert not torch.equal(_forward(g), eager)                                # another key: not the local graph


# ------------------------------------------------------------------------------------------------ pipeline
def _pipe_run(model, **kw):
    pipe = WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))
    lat = torch.cat([det_uniform("local.src", (1, 16, N_SRC, 12, 40), 1.0), det_uniform("local.noise", (1, 16, N_SRC + 1, 12, 40), 1.0)], dim=2)
    ctx = det_uniform("local.pctx", (37, 64), 1.0)
    return pipe(latents=lat.to(DEV), prompt_embeds=[ctx.to(DEV)], source_frames=4 * (N_SRC - 1) + 1, reasoning_frames=4, num_inference_steps=2,
                guidance_scale=1.0, shift=3.0, repeat_rope=True, cot=True, output_type="latent", weight_dtype=torch.float32, **kw).latents


def test_pipeline_switches_local_attention_per_step(model):
    variants = []
    real = model._self_attention

    def spy(*a, **kw):
        out = real(*a, **kw)
        variants.append((model.current_steps, ops.get_tuning("last_attn_variant") & _lib.ATTN_VARIANT_SPARSE))
        return out
    model._self_attention = spy
    model.use_block_composite = False          # every layer's self-attention from Python, dense steps too: the spy sees all of them
    dense = _pipe_run(model, skip_source_prediction=False)
    assert variants == [(0, 0), (0, 0), (1, 0), (1, 0)]
    del variants[:]
    late = _pipe_run(model, skip_source_prediction=False, local_attention=(1, 1), local_attention_from_step=1)
    assert variants == [(0, 0), (0, 0), (1, 64), (1, 64)]                      # step 0 dense, step 1 through the lists
    assert model.local_attention is None                                       # the model's own setting is back
    del variants[:]
    model.enable_local_attention(2, 2, sink_frames=0)
    every = _pipe_run(model, skip_source_prediction=False, local_attention=dict(window_frames=1, window_rows=1, dense_layers=(0,)))
    assert variants == [(0, 0), (0, 64), (1, 0), (1, 64)]
    assert model.local_attention == dict(window_frames=2, window_rows=2, sink_frames=0, dense_layers=())
    assert not torch.equal(late, dense) and not torch.equal(every, late)
    with pytest.raises(NotImplementedError, match="capture_graph='loop'"):
        _pipe_run(model, local_attention=(1, 1), capture_graph="loop")
    with pytest.raises(ValueError, match="local_attention"):
        _pipe_run(model, local_attention=(1, 1, 1))
    with pytest.raises(ValueError, match="from_step"):
        _pipe_run(model, local_attention=(1, 1), local_attention_from_step=-1)


def test_a_windowed_step_plans_for_the_windows_grid(model):
    """Temporal context windows sit in front of the token path: every forward is a batch of windows of 4 + 1 + 4 frames, and the plan is
    made for THAT grid (9 x 2 x 2 tokens: one block, one tile -- every key listed, so the launches differ and the bits do not)."""
    pipe = WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))
    lat = torch.cat([det_uniform("local.wsrc", (1, 16, 7, 4, 4), 1.0), det_uniform("local.wnoise", (1, 16, 8, 4, 4), 1.0)], dim=2).to(DEV)
    ctx = det_uniform("local.wctx", (37, 64), 1.0).to(DEV)
    kw = dict(latents=lat, prompt_embeds=[ctx], source_frames=25, reasoning_frames=4, num_inference_steps=2, guidance_scale=1.0, shift=3.0,
              repeat_rope=True, cot=True, output_type="latent", weight_dtype=torch.float32, temporal_window=13, temporal_overlap=8)
    plain = pipe(**kw).latents
    assert not model._local_plans
    local = pipe(local_attention=(1, 0), **kw).latents
    (key,) = model._local_plans
    assert key[0] == (9, 2, 2) and key[1:3] == (4, (4, 5)) and model._local_plan_last.density == 1.0
    assert torch.equal(local, plain) and model.local_attention is None
