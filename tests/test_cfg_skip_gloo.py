"""cfg_skip under sequence parallelism on CPU with gloo, world_size 2: every rank applies the same rule to the same call, so
the ranks stay in lockstep (the same sample count in the collectives of a step) and a skipped step gives what the single process
gives.  The token path itself needs a GPU (tests/test_gpu_cfg_skip.py); here it is replaced by a stand-in with the forward's
sequence-parallel structure -- this rank's token rows, a per-sample function of (x, t, context), the all-gather of
``videocof_amd.dist`` -- so what is under test is the rule in ``WanTransformer3DModel.forward`` and the exchange layer."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _stand_in(sp, rank, world):
    """``_forward`` with the shape of the real one: tokens [B, L, N] sharded by rows, gathered, returned ``rep`` times."""
    def fwd(x, t, context, seq_len, *rest, rep=1):
        B, L = x.shape[0], x.shape[1]
        Ll = L // world
        rows = x[:, rank * Ll:(rank + 1) * Ll]
        y = torch.stack([rows[b] * float(t[b]) + context[b].sum() for b in range(B)]).contiguous()
        if world > 1:
            sizes = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
            dist.all_gather(sizes, torch.tensor([B]))                      # lockstep: every rank computes the same sample count
            assert all(int(s) == B for s in sizes)
            y = sp.all_gather_tokens(y).clone()
        return torch.cat([y] * rep)
    return fwd


def _calls(model):
    torch.manual_seed(0)
    x = torch.randn(3, 16, 4)
    t = torch.tensor([900., 800., 700.])
    ctx = [torch.randn(5, 4), torch.randn(7, 4), torch.randn(3, 4)]
    outs = []
    model.enable_cfg_skip(0.5, 4)
    for B in (2, 3):
        for step in range(4):
            model.current_steps = step
            outs.append(model.forward(x[:B], t[:B], ctx[:B], 16).clone())
    model.disable_cfg_skip()
    return outs


def _worker(rank, world, port, q_out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from videocof_amd import WanTransformer3DModel
        from videocof_amd import dist as vdist
        vdist.set_multi_gpus_devices(ulysses_degree=world)
        m = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64)
        m._forward = _stand_in(vdist.get_sp_group(), rank, world)
        outs = _calls(m)
        q_out.put((rank, [o.numpy() for o in outs]))
    finally:
        dist.destroy_process_group()


def test_skipped_step_under_two_ranks_equals_the_single_process():
    from videocof_amd import WanTransformer3DModel
    single = WanTransformer3DModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64)
    single._forward = _stand_in(None, 0, 1)
    want = _calls(single)
    # steps 0, 1 full; steps 2, 3 on x[bs // 2:], returned twice (an odd batch of 3 computes 2 and returns 4)
    assert [o.shape[0] for o in want] == [2, 2, 2, 2, 3, 3, 4, 4]
    assert torch.equal(want[2][0], want[2][1]) and torch.equal(want[2][0], want[0][1]) and not torch.equal(want[0][0], want[0][1])
    assert torch.equal(want[6][:2], want[6][2:]) and torch.equal(want[6][:2], want[4][1:])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(2)), key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, got in res:
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert torch.equal(torch.from_numpy(a), b), rank
