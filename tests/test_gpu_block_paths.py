"""-m gpu: the launch sequence of a WanAttentionBlock on every host path that only tolerances pin otherwise -- fp8 Linears, fp8
attention, the suffix-only last block, Ulysses (head groups, tail composite, exposed-communication events, fp8) and padded heads --
equals, call for call, what the commit before the block path was restructured enqueued.

A trace is the list of `ops.*` calls made from videocof_amd/wan_transformer3d.py during ONE forward, interleaved with the calls of
the sequence-parallel group (`exchange`, `all_reduce_max`, `all_gather_tokens`) and of the wait handles `exchange` returned.  One
record is [name, positional arguments, keyword arguments]; a tensor argument is ("T", storage index, storage_offset, shape, stride,
dtype) with the storages numbered in order of first appearance within the forward (so no address is in the trace), an
AttentionWorkspace is the call site it belongs to, a float is its repr, everything else its value.  The recorder replaces the name
`ops` inside the module by a logging proxy and wraps the group's three methods; it touches nothing else, so the same file records
against any checkout.  Next to every trace the fixture holds the sha256 of the forward's output bytes (the kernels are bitwise
reproducible), and the tags of `_comm_events` where a configuration sets them.

tests/golden/dit_block_paths_parent.json was recorded on an MI355X from the parent commit's `videocof_amd` (its tree first on
sys.path, this tree's build of the unchanged library):
    PYTHONPATH=<parent checkout> WAN_HIP_LIB=<this build>/libwan_hip.so python tests/test_gpu_block_paths.py --record
"""
import ctypes
import hashlib
import json
import os
import socket
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.append(ROOT)          # (behind PYTHONPATH: --record imports the package of the checkout named there)
GOLDEN = os.path.join(ROOT, "tests", "golden", "dit_block_paths_parent.json")

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- the recorder
class _Trace:
    def __init__(self, model):
        self.log, self._storages = [], {}
        self._sites = {id(model._ws_self): "self", id(model._ws_cross): "cross", id(model._ws_self_sfx): "self_sfx",
                       id(model._ws_cross_sfx): "cross_sfx"}

    def enc(self, v):
        if torch.is_tensor(v):
            idx = self._storages.setdefault(v.untyped_storage().data_ptr(), len(self._storages))
            return ["T", idx, v.storage_offset(), list(v.shape), list(v.stride()), str(v.dtype)]
        if isinstance(v, (tuple, list)):
            return [self.enc(u) for u in v]
        if isinstance(v, float):
            return ["f", repr(v)]
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if id(v) in self._sites:
            return ["workspace", self._sites[id(v)]]
        if isinstance(v, ctypes.Structure):
            return [type(v).__name__] + [self.enc(getattr(v, f[0])) for f in v._fields_]
        if isinstance(v, (torch.dtype, torch.device)):
            return str(v)
        return ["object", type(v).__name__]

    def record(self, name, args, kwargs):
        self.log.append([name, [self.enc(a) for a in args], {k: self.enc(kwargs[k]) for k in sorted(kwargs)}])


class _OpsProxy:
    def __init__(self, real, trace):
        self._real, self._trace = real, trace

    def __getattr__(self, name):
        v = getattr(self._real, name)
        if not callable(v) or isinstance(v, type):
            return v

        def call(*args, **kwargs):
            self._trace.record(name, args, kwargs)
            return v(*args, **kwargs)
        return call


def traced_forward(model, call):
    """(trace, sha256 of the output) of `call()`, one forward of `model`."""
    from videocof_amd import wan_transformer3d as W
    trace, real_ops, sp = _Trace(model), W.ops, model._sp
    n_exchanges = [0]

    def logged(name, fn):
        def f(*args, **kwargs):
            trace.record("sp." + name, args, kwargs)
            out = fn(*args, **kwargs)
            if name != "exchange":
                return out
            k = n_exchanges[0]
            n_exchanges[0] += 1
            if out is None:
                return None

            def wait():
                trace.record("sp.wait", (k,), {})
                return out()
            return wait
        return f
    W.ops = _OpsProxy(real_ops, trace)
    try:
        if sp is not None:
            for name in ("exchange", "all_reduce_max", "all_gather_tokens"):
                setattr(sp, name, logged(name, getattr(sp, name)))
        out = call()
        torch.cuda.synchronize()
    finally:
        W.ops = real_ops
        if sp is not None:
            for name in ("exchange", "all_reduce_max", "all_gather_tokens"):
                sp.__dict__.pop(name, None)
    if model._comm_events is not None:
        trace.log.append(["comm_events", [tag for tag, _, _ in model._comm_events], {}])
    digest = hashlib.sha256(out.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
    return {"trace": json.loads(json.dumps(trace.log)), "sha256": digest}


# ---------------------------------------------------------------------------------------------------------------- the configurations
def _model(heads, ffn_dim):
    from videocof_amd import WanTransformer3DModel
    from videocof_amd.weights import deterministic_dit_state_dict
    m = WanTransformer3DModel(dim=128 * heads, ffn_dim=ffn_dim, num_heads=heads, num_layers=1, text_dim=64)
    m.load_state_dict(deterministic_dit_state_dict(dim=128 * heads, ffn_dim=ffn_dim, num_layers=1, in_dim=16, out_dim=16, text_dim=64,
                                                   freq_dim=256), device="cuda:0")
    return m


def _inputs(B, seq_len=420):
    from videocof_amd.weights import det_uniform
    lat = det_uniform("sp.lat", (2, 16, 7, 12, 20), 1.0).cuda()                    # grid (7, 6, 10): 420 tokens
    ctx = [det_uniform("sp.c0", (37, 64), 1.0).cuda(), det_uniform("sp.c1", (5, 64), 1.0).cuda()]
    t = torch.tensor([749, 749], device="cuda:0")
    kw = dict(frame_split_indices=[3, 3][:B], ground_frame_indices=[(3, 4), (3, 4)][:B])
    return lambda m: m(lat[:B], t[:B], ctx[:B], seq_len, **kw)


ALL_FP8 = ("qkv", "ffn", "o", "cross", "attn", "attn_pv")
# name -> (batch, seq_len, skip_source_frames, enable_fp8_linear layers, attn_smooth_k, _attn_events set)
SINGLE = {
    "bf16_b2": (2, 420, 0, None, True, False),
    "bf16_b1_pad_rows": (1, 448, 0, None, True, False),
    "bf16_b1_suffix": (1, 420, 3, None, True, False),
    "fp8_qkv_ffn": (2, 420, 0, ("qkv", "ffn"), True, False),
    "fp8_linears": (2, 420, 0, ("qkv", "ffn", "o", "cross"), True, False),
    "fp8_attn": (2, 420, 0, ("attn",), True, False),
    "fp8_attn_no_smooth_k": (2, 420, 0, ("attn",), False, False),
    "fp8_attn_pv": (2, 420, 0, ("attn", "attn_pv"), True, False),
    "fp8_all": (2, 420, 0, ALL_FP8, True, False),
    "fp8_qkv_ffn_b1_suffix": (1, 420, 3, ("qkv", "ffn"), True, False),
    "bf16_b2_attn_events": (2, 420, 0, None, True, True),          # (where _event_done sits: its ops.get_tuning call is in the trace)
}


def run_single(name):
    B, seq_len, skip, fp8, smooth_k, events = SINGLE[name]
    m = _model(heads=2, ffn_dim=512)
    m.use_block_composite = False
    m.skip_source_frames = skip
    if fp8:
        m.enable_fp8_linear(fp8, attn_smooth_k=smooth_k)
    call = _inputs(B, seq_len)
    call(m)                                  # the first forward calibrates the fp8 attention exponents; the trace is of the second
    if events:
        m._attn_events = []
    return traced_forward(m, lambda: call(m))


# name -> (sp_head_groups, use_block_composite, _comm_events set, _attn_events set, fp8 layers)
RCCL = {
    "groups2_composite": (2, True, False, False, None),
    "groups1_composite": (1, True, False, False, None),
    "groups2_per_op": (2, False, False, False, None),
    "groups1_per_op": (1, False, False, False, None),
    "groups2_comm_events": (2, True, True, False, None),
    "groups2_attn_events": (2, True, False, True, None),
    "fp8_linears": (2, True, False, False, ("qkv", "ffn", "o", "cross")),
    "fp8_attn_pv": (2, True, False, False, ("attn", "attn_pv")),
    "fp8_attn_pv_groups1": (1, True, False, False, ("attn", "attn_pv")),
}


def _rccl_child(port, out_path):
    """One rank, backend nccl (= RCCL), force_ulysses, 4 heads: every configuration of RCCL, written to `out_path`."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from videocof_amd import dist as vdist
        m = _model(heads=4, ffn_dim=1024)
        vdist.init_sequence_parallel()
        m.enable_multi_gpus_inference()
        m.force_ulysses = True
        call, res = _inputs(2), {}
        for name, (groups, composite, comm, events, fp8) in RCCL.items():
            m.sp_head_groups, m.use_block_composite = groups, composite
            if fp8:
                m.enable_fp8_linear(fp8)
            elif m._fp8:
                m.disable_fp8_linear()
            call(m)
            assert m._usp and m._bufs[m._bufs_last].vt is None          # really the wire-buffer branch
            m._comm_events, m._attn_events = ([] if comm else None), ([] if events else None)
            res[name] = traced_forward(m, lambda: call(m))
            m._comm_events = m._attn_events = None
        with open(out_path, "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


def _gloo_child(rank, world, port, out_path):
    """Two ranks on cuda:0 over gloo, 3 heads: padded heads (2 slots per rank, one dummy head).  bf16, tail composite on and off."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from videocof_amd import dist as vdist
        m = _model(heads=3, ffn_dim=1024)
        vdist.init_sequence_parallel()
        m.enable_multi_gpus_inference()
        assert m.sp_world_size == world and m.sp_world_rank == rank and m._sp_pad is not None
        call, res = _inputs(2), {}
        for name, composite in (("padded_heads_composite", True), ("padded_heads_per_op", False)):
            m.use_block_composite = composite
            call(m)
            res[name] = traced_forward(m, lambda: call(m))
        with open(out_path + f".{rank}", "w") as f:
            json.dump(res, f)
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


_CHILD_FAILED = []          # a child that did not exit 0 (a fault, a hang): this file starts nothing further on the GPU


def _join(procs, limit):
    for p in procs:
        p.join(limit)
    if any(p.exitcode != 0 for p in procs):
        _CHILD_FAILED.append([p.exitcode for p in procs])
        for p in procs:
            if p.is_alive():
                p.kill()
    assert not _CHILD_FAILED, f"child exit codes {_CHILD_FAILED[-1]}"


def run_rccl(tmp):
    import torch.multiprocessing as mp
    assert not _CHILD_FAILED, "an earlier child of this file did not exit 0"
    path = os.path.join(str(tmp), "rccl.json")
    p = mp.get_context("spawn").Process(target=_rccl_child, args=(_free_port(), path))
    p.start()
    _join([p], 300)
    with open(path) as f:
        return {"rccl1." + k: v for k, v in json.load(f).items()}


def run_gloo(tmp):
    import torch.multiprocessing as mp
    assert not _CHILD_FAILED, "an earlier child of this file did not exit 0"
    path, port, world = os.path.join(str(tmp), "gloo.json"), _free_port(), 2
    procs = [mp.get_context("spawn").Process(target=_gloo_child, args=(r, world, port, path)) for r in range(world)]
    for p in procs:
        p.start()
    _join(procs, 300)
    res = {}
    for r in range(world):
        with open(path + f".{r}") as f:
            res.update({f"gloo2.rank{r}.{k}": v for k, v in json.load(f).items()})
    return res


# ---------------------------------------------------------------------------------------------------------------- the tests
def _expected():
    with open(GOLDEN) as f:
        return json.load(f)["configs"]


def _check(name, got, want):
    a, b = got["trace"], want["trace"]
    for i, (ra, rb) in enumerate(zip(a, b)):
        if ra != rb:
            print(f"{name}: record {i} differs\n  parent: {json.dumps(rb)}\n  now:    {json.dumps(ra)}")
            break
    else:
        if len(a) != len(b):
            print(f"{name}: {len(a)} records, the parent made {len(b)}; first extra: {json.dumps((a + b)[min(len(a), len(b))])}")
    assert a == b, f"{name}: the launch trace differs from the parent's"
    assert got["sha256"] == want["sha256"], f"{name}: same launches, another output"


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_single_device_block_paths_launch_what_the_parent_launched(name):
    _check(name, run_single(name), _expected()["single." + name])


def test_ulysses_block_paths_over_rccl_launch_what_the_parent_launched(tmp_path):
    want, got = _expected(), run_rccl(tmp_path)
    assert set(got) == {k for k in want if k.startswith("rccl1.")}
    for name in sorted(got):
        _check(name, got[name], want[name])


def test_padded_head_block_paths_over_two_ranks_launch_what_the_parent_launched(tmp_path):
    want, got = _expected(), run_gloo(tmp_path)
    assert set(got) == {k for k in want if k.startswith("gloo2.")}
    for name in sorted(got):
        _check(name, got[name], want[name])


if __name__ == "__main__":
    import argparse
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", nargs="?", const=GOLDEN, required=True, metavar="PATH")
    out = ap.parse_args().record
    import videocof_amd
    configs = {"single." + name: run_single(name) for name in sorted(SINGLE)}
    with tempfile.TemporaryDirectory() as tmp:
        configs.update(run_rccl(tmp))
        configs.update(run_gloo(tmp))
    with open(out, "w") as f:
        json.dump({"configs": configs}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"package {os.path.dirname(os.path.abspath(videocof_amd.__file__))}: {len(configs)} configurations, {sum(len(c['trace']) for c in configs.values())} records -> {out}")
