"""cfg_skip on the host (no GPU): the switch's attributes, the activation rule against the flags captured from the reference
(tests/golden/dit_g16_cfg_skip_*.npz, tools/gen_golden_cfg_skip.py), the argument slicing of ``forward``, and the CPU oracle on
the conditional half, doubled, against the reference outputs."""
import numpy as np
import pytest
import torch

from oracle import wan_oracle as O
from videocof_amd import WanTransformer3DModel
from videocof_amd.wan_transformer3d import cfg_skip_active, cfg_skip_half
from videocof_amd.weights import deterministic_dit_state_dict, det_uniform

TINY = dict(dim=256, ffn_dim=512, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)
CFG = O.DiTConfig(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64)
LOOPS = ("dit_g16_cfg_skip_loop_unipc_r25", "dit_g16_cfg_skip_loop_unipc_r50", "dit_g16_cfg_skip_loop_dpm_r25")


def rel_l2(a, b):
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def tiny():
    return WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64)


def test_enable_share_disable_set_the_reference_attributes():
    """wan_transformer3d.py:752-771."""
    m, other = tiny(), tiny()
    m.current_steps = 5
    m.enable_cfg_skip(0.25, 8)
    assert (m.cfg_skip_ratio, m.current_steps, m.num_inference_steps) == (0.25, 0, 8)
    m.current_steps = 3
    other.share_cfg_skip(m)
    assert (other.cfg_skip_ratio, other.current_steps, other.num_inference_steps) == (0.25, 3, 8)
    m.disable_cfg_skip()
    assert (m.cfg_skip_ratio, m.current_steps, m.num_inference_steps) == (None, 0, None)
    assert other.cfg_skip_ratio == 0.25                                   # shared by value, as there
    m.enable_cfg_skip(1.0, 4)
    assert m.cfg_skip_ratio == 1.0
    m.enable_cfg_skip(0, 4)                                               # ratio 0: the switch is off
    assert (m.cfg_skip_ratio, m.current_steps, m.num_inference_steps) == (None, 0, None)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="cfg_skip_ratio"):
            m.enable_cfg_skip(bad, 8)
    with pytest.raises(NotImplementedError, match="RIFLEx"):              # the neighbouring refusal stays
        m.enable_riflex()


def test_activation_rule_agrees_with_the_reference_flags(golden):
    seen = 0
    for name in ("dit_g16_cfg_skip_fwd_b2", "dit_g16_cfg_skip_fwd_b3"):
        g = golden(name)
        assert g["case_fields"].tolist() == ["ratio", "n", "step", "batch", "halved", "halves_equal", "rows"]
        for ratio, n, step, batch, halved, equal, rows in g["cases"].tolist():
            n, step, batch = int(n), int(step), int(batch)
            assert cfg_skip_active(batch, ratio, step, n) == bool(halved), (ratio, n, step, batch)
            # odd batches follow the decorator: bs - bs // 2 samples computed, twice that returned
            assert rows == (2 * (batch - batch // 2) if halved else batch)
            assert bool(equal) == bool(halved)
            seen += 1
    assert seen == 12
    for name in LOOPS:
        g = golden(name)
        n, ratio = int(g["n"]), float(g["ratio"])
        assert [i for i in range(n) if cfg_skip_active(2, ratio, i, n)] == g["halved_steps"].tolist()
    g = golden("dit_g16_cfg_skip_teacache")
    assert [cfg_skip_active(2, float(g["ratio"]), i, len(g["ts"])) for i in range(len(g["ts"]))] == g["halved"].tolist()
    # no guidance batch, or the switch unset: never
    assert not cfg_skip_active(1, 1.0, 7, 8) and not cfg_skip_active(2, None, 7, None)


def test_forward_slices_every_batched_argument_and_asks_for_two_copies():
    """The decorator's slicing (cfg_optimization.py:10-26) on the model's own forward: positional or keyword, tensors, lists,
    tuples and ndarrays lose their first bs // 2 entries; ints pass."""
    m = tiny()
    calls = []
    m._forward = lambda *a, **k: calls.append((a, k)) or "out"
    x = torch.arange(3 * 2.0).view(3, 2)
    t = torch.tensor([7, 8, 9])
    ctx = ["c0", "c1", "c2"]
    m.enable_cfg_skip(0.5, 8)
    m.current_steps = 3
    assert m.forward(x, t, ctx, 420, frame_split_indices=[3, 3, 3], ground_frame_indices=((3, 4),) * 3) == "out"
    a, k = calls.pop()
    assert a[0] is x and a[2] is ctx and k.get("rep", 1) == 1            # before the boundary: untouched
    m.current_steps = 4
    m.forward(x, t, ctx, 420, frame_split_indices=np.array([3, 3, 3]), ground_frame_indices=((3, 4),) * 3)
    a, k = calls.pop()
    assert k == {"rep": 2}
    assert torch.equal(a[0], x[1:]) and torch.equal(a[1], t[1:]) and a[2] == ["c1", "c2"] and a[3] == 420
    assert tuple(a[4:9]) == (None,) * 5
    assert a[9] is True and a[10].tolist() == [3, 3] and a[11] == ((3, 4), (3, 4))
    m.forward(x=x[:2], t=t[:2], context=ctx[:2], seq_len=420)
    a, k = calls.pop()
    assert torch.equal(a[0], x[1:2]) and a[2] == ["c1"] and k == {"rep": 2}
    m.forward(x[:1], t[:1], ctx[:1], 420)                                 # one sample: no guidance pair, nothing to skip
    a, k = calls.pop()
    assert a[0].shape[0] == 1 and k.get("rep", 1) == 1
    assert cfg_skip_half(5, 1) == 5 and cfg_skip_half("ab", 1) == "ab"


def test_oracle_on_the_conditional_half_doubled_is_the_reference_output(golden):
    """fp32 restatement vs fp32 reference, the bound of tests/test_oracle_golden.py::test_g6_forward: rel-L2 < 1e-5."""
    sd = deterministic_dit_state_dict(**TINY)
    lat = det_uniform("g16.lat", (3, 16, 7, 12, 20), 1.0)
    for B in (2, 3):
        g = golden(f"dit_g16_cfg_skip_fwd_b{B}")
        ctx = [det_uniform(f"g16.ctx{b}", (int(n), 64), 1.0) for b, n in enumerate(g["ctx_len"])]
        t = torch.from_numpy(g["t"])
        half = B // 2
        out = O.dit_forward(sd, CFG, lat[half:B], t[half:], ctx[half:], 420, [3] * (B - half), [(3, 4)] * (B - half))
        want = np.concatenate([g["out_half"], g["out_half"]])
        r = rel_l2(torch.cat([out, out]), want)
        print(f"B={B}: oracle on x[{half}:] doubled vs reference, rel-L2 {r:.3e}")
        assert r < 1e-5
        full = O.dit_forward(sd, CFG, lat[:B], t, ctx, 420, [3] * B, [(3, 4)] * B)
        assert rel_l2(full, g["out_full"]) < 1e-5
        assert rel_l2(full[half:], g["out_half"]) < 1e-5                  # the halved result IS the conditional part of the full one
