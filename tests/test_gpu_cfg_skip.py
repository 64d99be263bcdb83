"""-m gpu: ``enable_cfg_skip`` on the HIP model and pipeline against the fixtures captured from the reference
(tests/golden/dit_g16_cfg_skip_*.npz, tools/gen_golden_cfg_skip.py).  Tolerances are the ones of the existing tests of the same
kind: a forward as tests/test_gpu_dit.py::test_g6_forward_batch2_and_bf16_latents (rel-L2 < 1e-2, cosine > 0.9999), a CFG loop as
test_g8b_cfg_loop / test_pipeline_dpm_cfg_loop_matches_the_reference (rel-L2 < 5e-2, cosine > 0.999), a TeaCache forward as
test_g14_teacache_sequence (rel-L2 < 1.2e-2, cosine > 0.9999)."""
import numpy as np
import pytest
import torch

from videocof_amd import FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, WanPipeline, WanTransformer3DModel, ops
from videocof_amd.weights import deterministic_dit_state_dict, det_uniform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(dim=256, ffn_dim=512, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)
LOOPS = {"unipc_r25": "dit_g16_cfg_skip_loop_unipc_r25", "unipc_r50": "dit_g16_cfg_skip_loop_unipc_r50",
         "dpm_r25": "dit_g16_cfg_skip_loop_dpm_r25"}


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def cosine(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm()))


@pytest.fixture()
def model():
    m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
    m.load_state_dict(deterministic_dit_state_dict(**TINY), device=DEV)
    yield m
    m.disable_cfg_skip()
    m.disable_teacache()


def _fwd_inputs(g, B):
    lat = det_uniform("g16.lat", (3, 16, 7, 12, 20), 1.0)[:B].to(DEV)
    ctx = [det_uniform(f"g16.ctx{b}", (int(n), 64), 1.0).to(DEV) for b, n in enumerate(g["ctx_len"])]
    t = torch.from_numpy(g["t"]).to(DEV)
    return lat, t, ctx, dict(frame_split_indices=[3] * B, ground_frame_indices=[(3, 4)] * B)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("composite", [True, False])
def test_forward_with_the_switch_active_matches_the_reference(golden, model, B, composite):
    """Every (ratio, step) case of the fixture: the full result before the boundary, the conditional half twice behind it --
    the two halves bit-equal to each other and to a forward of the conditional samples alone on the same model."""
    g = golden(f"dit_g16_cfg_skip_fwd_b{B}")
    lat, t, ctx, kw = _fwd_inputs(g, B)
    model.use_forward_composite = composite
    half = B // 2
    alone = model(lat[half:], t[half:], ctx[half:], 420, frame_split_indices=[3] * (B - half), ground_frame_indices=[(3, 4)] * (B - half))
    for ratio, n, step, batch, halved, equal, rows in g["cases"].tolist():
        model.enable_cfg_skip(ratio, int(n))
        model.current_steps = int(step)
        out = model(lat, t, ctx, 420, **kw)
        assert out.shape[0] == int(rows)
        want = np.concatenate([g["out_half"]] * 2) if halved else g["out_full"]
        r, c = rel_l2(out, want), cosine(out, want)
        print(f"B={B} composite={composite} ratio={ratio} step={int(step)} halved={bool(halved)}: rel-L2 {r:.3e} cosine {c:.6f}")
        assert r < 1e-2 and c > 0.9999
        h = out.shape[0] // 2
        if halved:
            assert torch.equal(out[:h], out[h:]) and torch.equal(out[:h], alone)
        else:
            assert not torch.equal(out[:1], out[-1:])
    # bf16 latents: the doubled result in the latents' dtype, same rule
    model.enable_cfg_skip(0.5, 8)
    model.current_steps = 7
    out = model(lat.bfloat16(), t, ctx, 420, **kw)
    h = out.shape[0] // 2
    assert out.dtype == torch.bfloat16 and torch.equal(out[:h], out[h:])
    assert rel_l2(out.float(), np.concatenate([g["out_half"]] * 2)) < 1.5e-2
    # off again: the plain forward
    model.disable_cfg_skip()
    out = model(lat, t, ctx, 420, **kw)
    assert out.shape[0] == B and rel_l2(out, g["out_full"]) < 1e-2


@pytest.mark.parametrize("grid,patch,cout", [((3, 4, 8), (1, 2, 2), 16), ((2, 3, 5), (1, 2, 2), 16), ((2, 3, 3), (1, 1, 1), 5)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unpatchify_rep_writes_every_copy_in_one_pass(grid, patch, cout, dtype):
    """``wan_unpatchify_rep``: rep = 2 is ``torch.cat([y, y])`` of the rep = 1 result, with and without ``zero_frames``; rep = 1 is
    the existing entry point, bit for bit.  (W = 16: 16-byte chunks; W = 10 and W = 3: the element-wise form.)"""
    F, Hp, Wp = grid
    N = patch[0] * patch[1] * patch[2] * cout
    tok = det_uniform("g16.unp", (F * Hp * Wp + 5, N), 3.0).to(DEV)
    for zf in (0, 1):
        base = ops.unpatchify(tok, grid, patch, cout, dtype, zero_frames=zf)
        one = ops.unpatchify(tok, grid, patch, cout, dtype, zero_frames=zf, rep=1)
        assert one.shape == (1,) + base.shape and torch.equal(one[0], base)
        two = ops.unpatchify(tok, grid, patch, cout, dtype, zero_frames=zf, rep=2)
        assert torch.equal(two, torch.stack([base, base]))
        if zf:
            assert float(two[:, :, :zf].abs().max()) == 0.0 and float(two[:, :, zf:].abs().max()) > 0
        # a batch of 2 samples, copies one batch apart (the model's layout: slot k * B + b), into a poisoned buffer with a guard
        buf = torch.full((5,) + base.shape, 7.0, device=DEV, dtype=dtype)
        for b in range(2):
            ops.unpatchify(tok + b, grid, patch, cout, dtype, zero_frames=zf, out=buf[b], rep=2, rep_stride=2 * base.numel())
        b1 = ops.unpatchify(tok + 1, grid, patch, cout, dtype, zero_frames=zf)
        assert torch.equal(buf[:4], torch.stack([base, b1, base, b1])) and bool((buf[4] == 7.0).all())
        # a view that does not start on a 16-byte boundary takes the element-wise form: same bits
        flat = torch.full((2 * base.numel() + 3,), 7.0, device=DEV, dtype=dtype)
        ops.unpatchify(tok, grid, patch, cout, dtype, zero_frames=zf, out=flat[1:1 + base.numel()].view(base.shape), rep=2,
                       rep_stride=base.numel() + 1)
        assert torch.equal(flat[1:1 + base.numel()].view(base.shape), base)
        assert torch.equal(flat[2 + base.numel():2 + 2 * base.numel()].view(base.shape), base)
        assert float(flat[0]) == 7.0 and float(flat[1 + base.numel()]) == 7.0 and float(flat[-1]) == 7.0
    with pytest.raises(ValueError, match="do not fit"):
        ops.unpatchify(tok, grid, patch, cout, dtype, out=torch.empty(base.shape, device=DEV, dtype=dtype), rep=2)


def _pipe(model, kind):
    if kind.startswith("dpm"):
        return WanPipeline(transformer=model, scheduler=FlowDPMSolverMultistepScheduler(shift=1.0, solver_order=2))
    return WanPipeline(transformer=model, scheduler=FlowUniPCMultistepScheduler(shift=1))


def _loop_inputs(golden):
    g = golden("dit_g8_cof_loop")
    lat = torch.cat([torch.from_numpy(g["src"]), torch.from_numpy(g["noise"])], dim=2).to(DEV)
    return g, lat, torch.from_numpy(g["ctx"]).to(DEV), torch.from_numpy(golden("dit_g8b_cfg_loop")["neg"]).to(DEV)


def _run(pipe, lat, ctx, neg, steps=8, scale=5.0, steps_out=None, **kw):
    cb = None
    if steps_out is not None:
        cb = lambda p, i, t, d: steps_out.append(d["latents"].clone()) or {}
    return pipe(latents=lat, prompt_embeds=[ctx], negative_prompt_embeds=[neg] if scale > 1 else None, source_frames=9,
                reasoning_frames=4, num_inference_steps=steps, guidance_scale=scale, shift=5.0, repeat_rope=True, cot=True,
                output_type="latent", weight_dtype=torch.float32, callback_on_step_end=cb, **kw).latents


def _count_forwards(model):
    """Forwards by the batch size the token path really computes (the wrapper sits behind the model's rule)."""
    sizes, inner = [], model._forward

    def counted(x, *a, **k):
        sizes.append(len(x))
        return inner(x, *a, **k)
    model._forward = counted
    return sizes


@pytest.mark.parametrize("kind", sorted(LOOPS))
@pytest.mark.parametrize("literal", [False, True])
def test_pipeline_loop_matches_the_reference_loop(golden, model, kind, literal):
    want = golden(LOOPS[kind])
    g, lat, ctx, neg = _loop_inputs(golden)
    pipe = _pipe(model, kind)
    pipe._cfg_skip_literal = literal
    model.enable_cfg_skip(float(want["ratio"]), int(want["n"]))
    sizes, steps = _count_forwards(model), []
    out = _run(pipe, lat, ctx, neg, steps_out=steps)
    assert pipe.scheduler.timesteps.cpu().tolist() == want["timesteps"].tolist()
    assert len(steps) == 8 and torch.equal(steps[-1], out)
    figures = [(rel_l2(s, want["steps"][i]), cosine(s, want["steps"][i])) for i, s in enumerate(steps)]
    print(f"{kind} literal={literal}: per-step (rel-L2, cosine) " + " ".join(f"({r:.2e}, {c:.6f})" for r, c in figures))
    print(f"{kind} literal={literal}: forwards by batch size {sizes}, reference halved steps {want['halved_steps'].tolist()}")
    assert sizes.count(1) == len(want["halved_steps"]) and sizes.count(2) == 8 - len(want["halved_steps"]) and len(sizes) == 8
    assert [i for i, s in enumerate(sizes) if s == 1] == want["halved_steps"].tolist()
    for r, c in figures:
        assert r < 5e-2 and c > 0.999
    assert float((out[:, :, :3].cpu() - torch.from_numpy(g["src"])).abs().max()) < 1e-5
    assert model.cfg_skip_ratio == float(want["ratio"])                     # the caller's setting survives the call
    # no guidance: the switch has no effect (one sample per call, as in the reference)
    del model._forward
    sizes = _count_forwards(model)
    a = _run(pipe, lat, ctx, neg, scale=1.0)
    model.disable_cfg_skip()
    b = _run(pipe, lat, ctx, neg, scale=1.0)
    assert torch.equal(a, b) and sizes == [1] * 16


@pytest.mark.parametrize("kind", ["unipc_r50", "dpm_r25"])
def test_short_path_is_bit_identical_to_the_literal_path(golden, model, kind):
    """A skipped step without the doubled batch and without guidance arithmetic == the doubled batch through the model's rule,
    then guidance: nu + g * (nt - nu) with nt == nu is nu."""
    want = golden(LOOPS[kind])
    _, lat, ctx, neg = _loop_inputs(golden)
    model.enable_cfg_skip(float(want["ratio"]), 8)
    short, literal = _pipe(model, kind), _pipe(model, kind)
    literal._cfg_skip_literal = True
    s_steps, l_steps = [], []
    a, b = _run(short, lat, ctx, neg, steps_out=s_steps), _run(literal, lat, ctx, neg, steps_out=l_steps)
    assert all(torch.equal(x, y) for x, y in zip(s_steps, l_steps)) and torch.equal(a, b)
    model.disable_cfg_skip()
    assert not torch.equal(_run(short, lat, ctx, neg), a)                   # and the switch does change the loop


@pytest.mark.parametrize("graph", ["step", "loop"])
@pytest.mark.parametrize("literal", [False, True])
def test_graph_capture_with_the_switch_on_is_bit_identical(golden, model, graph, literal):
    """Both kinds of step captured once, replayed bit-identically; a call with another ratio gets its own steps (``step``: the
    B = 2 and B = 1 graphs in another order; ``loop``: another graph, the ratio is part of the key)."""
    _, lat, ctx, neg = _loop_inputs(golden)
    eager, graphed = _pipe(model, "unipc"), _pipe(model, "unipc")
    eager._cfg_skip_literal = graphed._cfg_skip_literal = literal
    want = {}
    for ratio in (0.5, 0.25, None):
        model.enable_cfg_skip(ratio, 8) if ratio else model.disable_cfg_skip()
        want[ratio] = _run(eager, lat, ctx, neg)
    assert not torch.equal(want[0.5], want[0.25]) and not torch.equal(want[0.25], want[None])
    for ratio in (0.5, 0.5, 0.5, 0.25, 0.25, None, 0.5):
        model.enable_cfg_skip(ratio, 8) if ratio else model.disable_cfg_skip()
        got = _run(graphed, lat, ctx, neg, capture_graph=graph)
        assert torch.equal(got, want[ratio]), ratio
    if graph == "step":
        assert len(graphed._graphed._entries) == 2                          # one graph per kind of step, whatever the ratio
        assert graphed._graphed.replays == 7 * 8 - 2                        # every forward but the two eager warm-ups
    else:
        assert len(graphed._graphed_loop._entries) == 3                     # one per (ratio) signature
        assert graphed._graphed_loop.replays == 2 + 1 + 0 + 1               # 0.5: capture + 2 replays ... second call onwards
    assert model._ctx_cache is None


def test_context_cache_serves_the_conditional_half_and_survives(golden, model):
    """cache_context on / off with the switch on: the same bits (the skipped steps read the right half of the hoisted K/V); the
    full entry is still there for the next full-batch call; a plain CFG call afterwards still matches its own fixture."""
    want = golden(LOOPS["unipc_r50"])
    _, lat, ctx, neg = _loop_inputs(golden)
    pipe = _pipe(model, "unipc")
    model.enable_cfg_skip(0.5, 8)
    a = _run(pipe, lat, ctx, neg, cache_context=True)
    b = _run(pipe, lat, ctx, neg, cache_context=False)
    assert torch.equal(a, b)
    # the model alone: full call, skipped call, full call on one cache entry
    model.cache_context = True
    try:
        x2, t2, kw = torch.cat([lat] * 2), torch.tensor([500, 500], device=DEV), dict(frame_split_indices=[3, 3], ground_frame_indices=[(3, 4)] * 2)
        model.current_steps = 0
        full = model(x2, t2, [neg, ctx], 420, **kw)
        entry = model._ctx_cache
        kv_ptr = entry[2][0][0].data_ptr()
        model.current_steps = 7
        skipped = model(x2, t2, [neg, ctx], 420, **kw)
        assert model._ctx_cache is entry and entry[2][0][0].data_ptr() == kv_ptr            # not rebuilt, not replaced
        tail = entry[3][1]
        assert tail[0][0].data_ptr() == kv_ptr + entry[2][0][0][0].numel() * 2               # a view one sample in: no copy
        assert torch.equal(skipped[0], skipped[1]) and rel_l2(skipped[1], full[1]) < 1e-2
        assert rel_l2(skipped[1], full[0]) > 10 * max(rel_l2(skipped[1], full[1]), 1e-4)        # the conditional half, not the other one
        model.current_steps = 0
        assert torch.equal(model(x2, t2, [neg, ctx], 420, **kw), full) and model._ctx_cache is entry
    finally:
        model.cache_context = False
        model.clear_context_cache()
    model.disable_cfg_skip()
    gb = golden("dit_g8b_cfg_loop")
    out = _run(pipe, lat, ctx, neg, steps=3)
    assert rel_l2(out, gb["steps"][2]) < 5e-2 and cosine(out, gb["steps"][2]) > 0.999


def test_teacache_together_with_cfg_skip_follows_the_reference(golden, model):
    """The reference runs both switches together (wan_transformer3d.py:956-1031 on the halved batch: the distance of the halved
    modulated input to the full one broadcasts, the full-batch residual is read from its end): same decisions, same outputs --
    step 3 of the fixture re-applies, on the conditional half, a residual taken at the full batch."""
    g = golden("dit_g16_cfg_skip_teacache")
    lat0 = det_uniform("g16.tea.lat", (2, 16, 5, 8, 12), 1.0).to(DEV)
    dl = det_uniform("g16.tea.dlat", (2, 16, 5, 8, 12), 0.15).to(DEV)
    ctx = [det_uniform(f"g16.ctx{b}", (n, 64), 1.0).to(DEV) for b, n in enumerate((9, 37))]
    n = len(g["ts"])
    assert g["calc"].tolist()[2:4] == [True, False] and g["halved"].tolist()[2:4] == [False, True]
    model.enable_teacache(g["coeff"].tolist(), n, float(g["thresh"]), num_skip_start_steps=1, offload=False)
    model.enable_cfg_skip(float(g["ratio"]), n)
    decisions = []
    for i, t in enumerate(g["ts"]):
        model.current_steps = i
        out = model(lat0 + i * dl, torch.tensor([int(t)] * 2, device=DEV), ctx, 120, frame_split_indices=[2, 2],
                    ground_frame_indices=[(2, 3), (2, 3)])
        decisions.append(bool(model.should_calc))
        assert out.shape[0] == 2 and bool(torch.equal(out[0], out[1])) == bool(g["halved"][i])
        want = np.concatenate([g[f"out{i}"]] * 2) if g["halved"][i] else g[f"out{i}"]
        r, c = rel_l2(out, want), cosine(out, want)
        print(f"teacache + cfg_skip step {i}: calc={decisions[-1]} halved={bool(g['halved'][i])} rel-L2 {r:.3e} cosine {c:.6f}")
        assert r < 1.2e-2 and c > 0.9999, i
    assert decisions == g["calc"].tolist() and model.teacache.cnt == 0


def test_sequence_parallel_branch_applies_the_same_rule(golden, model):
    """The Ulysses branch (one rank, library communicator, ``force_ulysses``): a skipped step equals the single-device one."""
    from videocof_amd import dist as vdist
    g = golden("dit_g16_cfg_skip_fwd_b2")
    lat, t, ctx, kw = _fwd_inputs(g, 2)
    model.enable_cfg_skip(0.5, 8)
    model.current_steps = 6
    want = model(lat, t, ctx, 420, **kw)
    vdist.init_sequence_parallel(backend="library", rank=0, world_size=1)
    try:
        model.enable_multi_gpus_inference()
        model.force_ulysses = True
        got = model(lat, t, ctx, 420, **kw)
        assert got.shape[0] == 2 and torch.equal(got[0], got[1])
        r = rel_l2(got, np.concatenate([g["out_half"]] * 2))
        print(f"Ulysses branch, skipped step: rel-L2 {r:.3e} vs the fixture, {rel_l2(got, want):.3e} vs the single-device path")
        assert r < 1e-2 and rel_l2(got, want) < 1e-2
    finally:
        model.force_ulysses = False
        vdist.destroy_sequence_parallel()
