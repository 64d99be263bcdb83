"""-m gpu: the concurrent-exchange emulation (videocof_amd.dist.EmulatedRank(concurrent=True), wan_sp_channel_copy) and the CUs the
persistent grids leave to communication kernels (tuning key sp_reserve_cus).

* the channel copy moves bytes exactly, whatever the size, alignment, channel count and workgroup size, and nothing beside them;
* a rank whose exchanges run on a side stream computes the SAME BITS as the rank whose exchanges are inline copies -- with the
  receive buffers poisoned at every hand-over, so that a consumer that does not wait reads NaN (one run per case: this is a
  dependency check, not a race hunt);
* with 32 CUs reserved the persistent GEMM and the persistent cross-attention form stay within the bounds their own tests
  (tests/test_gpu_kernels.py) assert against fp64 / fp32 references at the same shapes;
* a graph captured in concurrent mode replays the bits of the eager run."""
import math

import pytest
import torch

from oracle import wan_oracle as O
from videocof_amd import _lib, ops
from videocof_amd.attention_utils import attention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def bf(x):
    return x.to(torch.bfloat16)


@pytest.fixture
def reserve_cus():
    """sp_reserve_cus for one test, back at 0 afterwards whatever happened in between."""
    def set_(n):
        ops.set_tuning("sp_reserve_cus", n)
    yield set_
    ops.set_tuning("sp_reserve_cus", 0)
    assert ops.get_tuning("sp_reserve_cus") == 0


@pytest.fixture
def sp_teardown():
    from videocof_amd import dist as vdist
    yield vdist
    vdist.destroy_sequence_parallel()
    assert ops.get_tuning("sp_reserve_cus") == 0


# ------------------------------------------------------------------------------------------------ the channel copy
GUARD = 64


def _copy_case(nbytes, channels, threads, dst_off=0, src_off=0, seed=0):
    """dst / src start `*_off` bytes behind a 16-byte boundary; GUARD bytes of a known pattern on either side of dst."""
    g = torch.Generator(device=DEV).manual_seed(seed + nbytes % 9973)
    src_buf = torch.randint(0, 256, (src_off + nbytes,), device=DEV, dtype=torch.uint8, generator=g)
    src = src_buf[src_off:]
    dst_buf = torch.full((GUARD + dst_off + nbytes + GUARD,), 0xA5, device=DEV, dtype=torch.uint8)
    dst = dst_buf[GUARD + dst_off:GUARD + dst_off + nbytes]
    assert src_buf.data_ptr() % 16 == 0 and dst_buf.data_ptr() % 16 == 0
    want = src.clone()
    ops.sp_channel_copy(dst, src, channels, threads)
    torch.cuda.synchronize()
    assert torch.equal(dst, want), (nbytes, channels, threads, dst_off, src_off)
    assert torch.equal(src, want)
    assert bool((dst_buf[:GUARD + dst_off] == 0xA5).all()) and bool((dst_buf[GUARD + dst_off + nbytes:] == 0xA5).all()), "guard bytes written"


@pytest.mark.parametrize("threads", [256, 512])
@pytest.mark.parametrize("channels", [1, 8, 16, 32])
@pytest.mark.parametrize("nbytes", [16, 4096 + 3, 1 << 20, (256 << 20) + 5], ids=["16B", "4KiB+3", "1MiB", "256MiB+5"])
def test_channel_copy_is_byte_exact(nbytes, channels, threads):
    _copy_case(nbytes, channels, threads)


@pytest.mark.parametrize("threads", [256, 512])
@pytest.mark.parametrize("channels", [1, 7, 32])
def test_channel_copy_unaligned_buffers_and_uneven_shares(channels, threads):
    """Heads and tails: both buffers 3 bytes off a 16-byte boundary (a head of 13 bytes, then vector accesses), buffers misaligned
    AGAINST each other (byte accesses), fewer 16-byte words than channels, one byte, and word counts that do not divide evenly."""
    for nbytes, d_off, s_off in ((4096 + 3, 3, 3), (4096 + 3, 1, 2), (100003, 5, 12), (5, 3, 3), (1, 0, 0), (1, 15, 15), (16 * 5, 0, 0),
                                 (16 * 33 + 15, 0, 0), (16 * 1000 + 7, 8, 8), (12, 9, 9)):
        _copy_case(nbytes, channels, threads, d_off, s_off, seed=channels)


def test_channel_copy_takes_any_dtype_and_refuses_what_it_cannot_do():
    a = torch.randn(3, 1001, device=DEV).bfloat16()
    b = torch.zeros_like(a)
    assert ops.sp_channel_copy(b, a) is b
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="same number of bytes"):
        ops.sp_channel_copy(torch.zeros(8, device=DEV), torch.zeros(9, device=DEV))
    with pytest.raises(ValueError, match="contiguous"):
        ops.sp_channel_copy(torch.zeros(8, 8, device=DEV).t(), torch.zeros(8, 8, device=DEV))
    with pytest.raises(ValueError, match="overlapping"):
        ops.sp_channel_copy(a.view(-1)[:64], a.view(-1)[32:96])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sp_channel_copy(torch.zeros(8), torch.zeros(8))


def test_concurrent_exchange_interface_orders_producer_copy_and_consumer(sp_teardown):
    """The raw calls: a producer on the compute stream right before the hand-over, the copy on the side stream, a consumer right
    behind wait(); async and blocking forms; the all-gather; more exchanges in flight than the event ring holds."""
    vdist = sp_teardown
    sp = vdist.init_sequence_parallel(backend="emulated", rank=0, world_size=4, concurrent=True, channels=8, threads=256, poison=True)
    a = torch.arange(1 << 22, device=DEV, dtype=torch.int32)
    send = a * 3
    recv = torch.zeros_like(send)
    wait = sp.exchange(recv, send, async_op=True)
    wait()
    got = recv + 1
    assert torch.equal(got, a * 3 + 1)
    assert sp._side is not None and sp._side != torch.cuda.current_stream()
    assert sp.exchange(recv, a) is None and torch.equal(recv, a)
    y = torch.randn(2, 5, 3, device=DEV)
    gth = sp.all_gather_tokens(y)
    assert gth.shape == (2, 20, 3) and all(torch.equal(gth[:, 5 * r:5 * r + 5], y) for r in range(4))
    pairs = [(torch.zeros(4096, device=DEV), torch.full((4096,), float(i), device=DEV)) for i in range(40)]
    waits = [sp.exchange(r, s, async_op=True) for r, s in pairs]
    for w in waits:
        w()
    assert all(float(r.min()) == float(r.max()) == float(i) for i, (r, _) in enumerate(pairs))
    with pytest.raises(ValueError, match="divisible"):
        sp.exchange(torch.zeros(10, device=DEV), torch.zeros(10, device=DEV))


# ------------------------------------------------------------------------------------------------ concurrent == serial
def _tiny_dit(heads, layers=2):
    from videocof_amd import WanTransformer3DModel
    from videocof_amd.weights import deterministic_dit_state_dict, det_uniform
    cfgd = dict(dim=128 * heads, ffn_dim=1024, num_layers=layers, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)
    m = WanTransformer3DModel(dim=128 * heads, ffn_dim=1024, num_heads=heads, num_layers=layers, text_dim=64)
    m.load_state_dict(deterministic_dit_state_dict(**cfgd), device=DEV)
    lat = det_uniform("sp.lat", (2, 16, 7, 12, 20), 1.0).to(DEV)
    ctx = [det_uniform("sp.c0", (37, 64), 1.0).to(DEV), det_uniform("sp.c1", (5, 64), 1.0).to(DEV)]
    t = torch.tensor([749, 749], device=DEV)
    kw = dict(frame_split_indices=[3, 3], ground_frame_indices=[(3, 4), (3, 4)])
    return m, (lat, t, ctx, 420), kw


@pytest.mark.parametrize("world,heads,channels,threads", [(2, 4, 16, 512), (4, 4, 8, 256), (8, 8, 32, 512), (2, 3, 16, 512), (8, 12, 1, 256)])
def test_concurrent_exchanges_compute_the_bits_of_the_serial_copy(sp_teardown, world, heads, channels, threads):
    """The sizes of tests/test_gpu_sp.py (a CFG batch of two, 420 -> padded tokens; (2, 3) and (8, 12): heads padded to a multiple of
    the degree), one rank of P = 2, 4, 8.  The same rank with every exchange as a channel copy on the side stream, receive buffers
    NaN-filled at each hand-over, must return exactly what the rank with inline copies returns: any missing wait_*() shows as NaN."""
    vdist = sp_teardown
    m, args, kw = _tiny_dit(heads)
    vdist.init_sequence_parallel(backend="emulated", rank=0, world_size=world)
    m.enable_multi_gpus_inference()
    assert m.sp_world_size == world
    serial = m(*args, **kw).clone()
    torch.cuda.synchronize()
    sp = vdist.init_sequence_parallel(backend="emulated", rank=0, world_size=world, concurrent=True, channels=channels, threads=threads,
                                      poison=True)
    m.enable_multi_gpus_inference()
    assert m._sp is sp and sp.concurrent and sp.poison
    conc = m(*args, **kw).clone()
    again = m(*args, **kw).clone()                         # the persistent wire buffers a second time (a reuse hazard shows here)
    torch.cuda.synchronize()
    assert sp._side is not None, "no exchange ran on the side stream"
    assert bool(torch.isfinite(serial.float()).all()) and bool(torch.isfinite(conc.float()).all())
    assert torch.equal(conc, serial), float((conc.float() - serial.float()).abs().max())
    assert torch.equal(again, serial)


def test_concurrent_mode_replays_from_a_step_graph_bit_identically(golden, sp_teardown):
    """WanPipeline(capture_graph="step") over a rank in concurrent mode: step 0 eager (side stream), step 1 captured (the copies are
    nodes of the capturing stream: no parallel branch) and replayed, later steps replayed -- the latents of the eager loop, bit for bit."""
    from videocof_amd import FlowUniPCMultistepScheduler, GraphedForward, WanPipeline, WanTransformer3DModel
    from videocof_amd.weights import deterministic_dit_state_dict
    vdist = sp_teardown
    heads = 4
    cfgd = dict(dim=128 * heads, ffn_dim=1024, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)
    m = WanTransformer3DModel(dim=128 * heads, ffn_dim=1024, num_heads=heads, num_layers=2, text_dim=64)
    m.load_state_dict(deterministic_dit_state_dict(**cfgd), device=DEV)
    g = golden("dit_g8_cof_loop")
    lat = torch.cat([torch.from_numpy(g["src"]), torch.from_numpy(g["noise"])], dim=2).to(DEV)
    ctx = torch.from_numpy(g["ctx"]).to(DEV)
    kw = dict(latents=lat, prompt_embeds=[ctx], source_frames=9, reasoning_frames=4, num_inference_steps=4, guidance_scale=1.0, shift=3,
              repeat_rope=True, cot=True, output_type="latent", weight_dtype=torch.float32)
    sp = vdist.init_sequence_parallel(backend="emulated", rank=0, world_size=2, concurrent=True, channels=16, threads=512, poison=True)
    m.enable_multi_gpus_inference()
    eager = WanPipeline(transformer=m, scheduler=FlowUniPCMultistepScheduler(shift=1))(capture_graph=False, **kw).latents.clone()
    graphed = WanPipeline(transformer=m, scheduler=FlowUniPCMultistepScheduler(shift=1))
    got = graphed(capture_graph="step", **kw).latents.clone()
    torch.cuda.synchronize()
    assert isinstance(graphed._graphed, GraphedForward) and graphed._graphed.replays == 3      # 1 eager + capture/replay + 2 replays
    assert sp._side is not None
    assert bool(torch.isfinite(eager.float()).all()) and torch.equal(got, eager)
    graphed._graphed.reset()


# ------------------------------------------------------------------------------------------------ 32 CUs reserved
@pytest.mark.parametrize("M,N,K", [(1100, 520, 512), (2304, 1536, 896), (9000, 5120, 640), (3000, 1164, 384)])
def test_persistent_gemm_with_reserved_cus_all_epilogues(reserve_cus, M, N, K):
    """tests/test_gpu_kernels.py::test_persistent_stream_k_gemm_all_epilogues at 32 reserved CUs (the product epilogue form; the forced
    stream-K cut and the plan's own): the same operands, the same fp64 reference, the same bounds; bitwise run to run."""
    g = torch.Generator().manual_seed(M + N + K)
    a, w = bf(torch.randn(M, K, generator=g)), bf(torch.randn(N, K, generator=g) * 0.1)
    bias = torch.randn(N, generator=g) * 0.5
    gate = torch.randn(2, N, generator=g)
    resid = torch.randn(M, N, generator=g)
    acc = a.double() @ w.double().t() + bias.double()
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)
    rpb = (M + 1) // 2
    lib = _lib.load()
    full = int(lib.wan_gemm_pk_grid(M, N))
    reserve_cus(32)
    ops.set_tuning("gemm_pk", 2)
    ops.set_tuning("gemm_pk_min_units", max(1, (K // 128 + 3) // 4))
    try:
        assert lib.wan_gemm_ws_plan(M, N, K) == 3 and int(lib.wan_gemm_pk_grid(M, N)) == full - 32
        ws = ops.gemm_workspace(ad.device, M, N, K)
        assert ws is not None and ws.numel() >= lib.wan_gemm_workspace_bytes(M, N, K)
        runs = []
        for rep in range(2):
            ws.fill_(0xA5 if rep else 0xFF)
            o_res = resid.to(DEV).clone()
            ops.gemm(ad, wd, bd, ops.EPI_RESID_F32, out=o_res, gate=gate.to(DEV), rows_per_batch=rpb)
            runs.append((ops.gemm(ad, wd, bd, ops.EPI_BF16), ops.gemm(ad, wd, bd, ops.EPI_GELU_BF16), ops.gemm(ad, wd, bd, ops.EPI_F32),
                         o_res, ops.gemm(ad, wd, None, ops.EPI_BF16_T)))
        ops.set_tuning("gemm_pk_min_units", 0)
        own = (ops.gemm(ad, wd, bd, ops.EPI_BF16), ops.gemm(ad, wd, bd, ops.EPI_F32))
        torch.cuda.synchronize()
    finally:
        ops.set_tuning("gemm_pk", 1)
        ops.set_tuning("gemm_pk_min_units", 0)
    assert rel_l2(own[0], acc) < 4e-3 and rel_l2(own[1], acc) < 1e-5
    o_bf, o_ge, o_f32, o_res, o_t = runs[0]
    assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[1]))
    assert rel_l2(o_bf, acc) < 4e-3 and rel_l2(o_f32, acc) < 1e-5
    x = acc.float().double()
    assert rel_l2(o_ge, 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))) < 5e-3
    gsel = gate.double()[torch.arange(M) // rpb]
    assert rel_l2(o_res, resid.double() + acc * gsel) < 1e-5
    assert o_t.shape[0] == N and rel_l2(o_t[:, :M].t(), acc - bias.double()) < 4e-3
    assert float(o_t[:, M:].abs().max()) == 0.0 if o_t.shape[1] > M else True


def test_persistent_cross_attention_with_reserved_cus(reserve_cus):
    """tests/test_gpu_kernels.py::test_cross_attention_persistent_form_walks_many_blocks at 32 reserved CUs: 336 query blocks walked by
    224 resident workgroups instead of 256 -- the same oracle bounds, and (a block's arithmetic does not depend on who walks it) the
    bits of the one-workgroup-per-block launch."""
    g = torch.Generator().manual_seed(11)
    B, Lq, Lk, H = 2, 256 * 20 + 37, 512, 8
    q = bf(torch.randn(B, Lq, H, 128, generator=g) * 2.0)
    k = bf(torch.randn(B, Lk, H, 128, generator=g))
    v = bf(torch.randn(B, Lk, H, 128, generator=g) + torch.arange(128) * 0.01)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    ref = torch.stack([O.attention(q[b].float(), k[b].float(), v[b].float(), None) for b in range(B)])
    ref300 = torch.stack([O.attention(q[b].float(), k[b].float(), v[b].float(), 300) for b in range(B)])
    assert ops.get_tuning("attn_persist") == 1
    reserve_cus(32)
    out = attention(qd, kd, vd)
    again = attention(qd, kd, vd)
    out300 = attention(qd, kd, vd, k_lens=torch.tensor([300, 300]))
    ops.set_tuning("attn_persist", 0)
    try:
        per_block = attention(qd, kd, vd)
    finally:
        ops.set_tuning("attn_persist", 1)
    torch.cuda.synchronize()
    assert rel_l2(out, ref) < 6e-3 and float((out.float().cpu() - ref).abs().max()) < 4e-2
    assert rel_l2(out300, ref300) < 6e-3
    assert torch.equal(out, again) and torch.equal(out, per_block)
