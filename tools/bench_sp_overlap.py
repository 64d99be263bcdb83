#!/usr/bin/env python3
"""What the Ulysses exchanges cost when they really run beside the projections -- on ONE GPU, in emulation.

One rank of P = 2, 4, 8 of the headline workload (14B dims, the 81-frame CoF shape of bench.py's "14b-cof"), `--layers` layers of it,
under `videocof_amd.dist.EmulatedRank`.  Arms, alternated in one process on one warm model (never compared with a number of another run):

    serial            every exchange an inline copy on the compute stream (today's `bench.py --emulate-sp`)
    c<N>/r0           concurrent: every exchange a `wan_sp_channel_copy` of N channels x 512 threads on a side stream, waited for by event
    c<N>/r<N>         the same with N CUs reserved: the persistent GEMM / cross-attention grids leave N CUs free (sp_reserve_cus)

Per arm, HIP events only, medians over `--rounds` rounds:
    ms/step           one forward of the rank (clean pass: no events inside it; the scheduler update is not part of it)
    V / q proj        the V^T and the q projection GEMMs of a layer (instrumented pass).  In the concurrent arms the k copy is in flight
                      under the V projection and the V^T copy under the q projection; in the serial arm nothing is
    exposed           per layer: time of the compute stream inside each exchange call + its wait (serial: the copy itself; concurrent:
                      what the projections did not cover), by exchange: k, v, q (both head groups), o (both), and the all-gather per step

WHAT THIS IS NOT: bytes between devices.  One GPU copies to itself through HBM -- no xGMI, no peer latency, no RCCL protocol; that a
collective looks like "N workgroups of 512 threads" is an assumption (include/wan_hip.h).  It asserts nothing about speed.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class TimedRank:
    """Delegates to an EmulatedRank and brackets every exchange call and every wait with HIP events on the compute stream."""

    def __init__(self, inner, names, torch):
        self.inner, self.names, self.torch = inner, names, torch
        self.rank, self.world_size, self.group, self._host_staged = inner.rank, inner.world_size, None, False
        self.spans, self.last = [], None          # (tag, start event, end event); tag of the exchange issued last

    def _span(self, tag, fn):
        a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        self.spans.append((tag, a, b))
        return r

    def _tag(self, recv):
        p = recv.data_ptr()
        for name, lo, hi in self.names:
            if lo <= p < hi:
                return name
        return "other"

    def exchange(self, recv, send, async_op=False):
        tag = self._tag(recv)
        self.last = tag
        wait = self._span(tag, lambda: self.inner.exchange(recv, send, async_op=async_op))
        if wait is None:
            return None
        return lambda: self._span(tag, wait)

    def all_reduce_max(self, t):
        return self.inner.all_reduce_max(t)

    def all_gather_tokens(self, y):
        return self._span("all_gather", lambda: self.inner.all_gather_tokens(y))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--degrees", default="2,4,8", help="Ulysses degrees P to emulate one rank of")
    ap.add_argument("--layers", type=int, default=4, help="DiT layers to run (of 40); per-layer figures do not depend on it")
    ap.add_argument("--rounds", type=int, default=5, help="rounds over all arms (medians over rounds)")
    ap.add_argument("--steps", type=int, default=2, help="clean forwards timed per arm and round")
    ap.add_argument("--channels", default="8,16,32")
    ap.add_argument("--threads", type=int, default=512)
    ap.add_argument("--workload", default="14b-cof")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sp_overlap needs a GPU: its numbers are HIP event times")
    import bench
    from videocof_amd import WanTransformer3DModel, ops
    from videocof_amd import dist as vdist
    from videocof_amd.weights import random_dit_state_dict

    dev = torch.device("cuda", 0)
    wl = dict(bench.WORKLOADS[args.workload])
    layers = min(args.layers, wl["num_layers"])
    model = WanTransformer3DModel(dim=wl["dim"], ffn_dim=wl["ffn_dim"], num_heads=wl["num_heads"], num_layers=layers)
    model.load_state_dict(random_dit_state_dict(dev, seed=0, dim=wl["dim"], ffn_dim=wl["ffn_dim"], num_layers=layers), device=dev)
    Fs, G, Ft = wl["fs"], wl["g"], wl["ft"]
    g = torch.Generator(device=dev).manual_seed(0)
    lat = torch.randn(1, 16, Fs + G + Ft, wl["h"], wl["w"], device=dev, generator=g).bfloat16()
    ctx = [torch.randn(37, 4096, device=dev, generator=g).bfloat16()]
    L = (Fs + G + Ft) * (wl["h"] // 2) * (wl["w"] // 2)
    t = torch.tensor([500], device=dev)
    kw = dict(frame_split_indices=[Fs], ground_frame_indices=[(Fs, Fs + G)]) if Fs else {}

    def forward():
        return model(lat, t, ctx, L, **kw)

    chans = [int(c) for c in args.channels.split(",")]
    arms = [("serial", None, 0)] + [(f"c{c}/r{r}", c, r) for c in chans for r in (0, c)]
    print(f"# bench_sp_overlap: {args.workload} dims {wl['dim']}/{wl['ffn_dim']}/{wl['num_heads']} heads, L = {L} tokens, {layers} of {wl['num_layers']} layers, "
          f"{args.rounds} rounds x {args.steps} forwards per arm, threads per channel {args.threads}")
    print(f"# device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs; ONE GPU copying to itself: no xGMI, no peer")
    print("# all times are HIP event times in ms, medians over rounds; ms/step covers the layers run, the other columns are per layer "
          "(all-gather: per step)")

    real_gemm = ops.gemm
    for P in [int(p) for p in args.degrees.split(",")]:
        def enter(arm):
            _, c, r = arm
            sp = vdist.init_sequence_parallel(backend="emulated", rank=0, world_size=P, reserve_cus=r, concurrent=c is not None,
                                              channels=c or 16, threads=args.threads)
            model.enable_multi_gpus_inference()
            return sp

        for arm in arms:                              # warm every arm: workspaces, wire buffers, code objects, the side streams' first use
            enter(arm)
            forward()
        torch.cuda.synchronize()
        b = model._bufs[model._bufs_last]
        names = [(n, x.data_ptr(), x.data_ptr() + x.numel() * x.element_size())
                 for n, x in (("k", b.kw_r), ("v", b.vw_r), ("q", b.qw_r), ("o", b.ow_r))]
        step_ms = {a[0]: [] for a in arms}
        detail = {a[0]: {k: [] for k in ("V proj", "q proj", "k", "v", "q", "o", "all_gather")} for a in arms}
        for rnd in range(args.rounds):
            order = arms if rnd % 2 == 0 else arms[::-1]          # alternate the order too: drift hits every arm alike
            for arm in order:
                enter(arm)
                forward()                                         # one untimed forward after the switch
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    forward()
                e.record()
                e.synchronize()
                step_ms[arm[0]].append(a.elapsed_time(e) / args.steps)
                # instrumented pass: events around the exchanges, their waits and the two projections that run beside a copy
                timed = TimedRank(model._sp, names, torch)
                model._sp = timed
                gemm_spans = []

                def gemm(*ga, **gk):
                    tag = {"k": "V proj", "v": "q proj"}.get(timed.last)
                    epilogue = ga[3] if len(ga) > 3 else gk.get("epilogue")
                    if tag is None or (tag == "V proj") != (epilogue == ops.EPI_BF16_T):
                        return real_gemm(*ga, **gk)
                    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s0.record()
                    out = real_gemm(*ga, **gk)
                    s1.record()
                    gemm_spans.append((tag, s0, s1))
                    return out
                ops.gemm = gemm
                try:
                    forward()
                finally:
                    ops.gemm = real_gemm
                    model._sp = timed.inner
                torch.cuda.synchronize()
                acc = {k: 0.0 for k in detail[arm[0]]}
                for tag, s0, s1 in timed.spans + gemm_spans:
                    acc[tag] = acc.get(tag, 0.0) + s0.elapsed_time(s1)
                for k in detail[arm[0]]:
                    detail[arm[0]][k].append(acc[k] / (1 if k == "all_gather" else layers))
        med = statistics.median
        base = med(step_ms["serial"])
        print(f"\n## P = {P}: rank 0 of {P}, {wl['num_heads'] // P} local heads, {L // P} local tokens (+ padding)")
        print(f"{'arm':<10}{'ms/step':>10}{'min..max':>20}{'vs serial':>11} |{'V proj':>9}{'q proj':>9} |"
              f"{'exp k':>8}{'exp v':>8}{'exp q':>8}{'exp o':>8}{'sum/layer':>11}{'all-gather':>12}")
        for name, _, _ in arms:
            s, d = step_ms[name], {k: med(v) for k, v in detail[name].items()}
            exp = d["k"] + d["v"] + d["q"] + d["o"]
            print(f"{name:<10}{med(s):>10.3f}{min(s):>10.3f}..{max(s):<8.3f}{med(s) / base:>11.4f} |{d['V proj']:>9.3f}{d['q proj']:>9.3f} |"
                  f"{d['k']:>8.3f}{d['v']:>8.3f}{d['q']:>8.3f}{d['o']:>8.3f}{exp:>11.3f}{d['all_gather']:>12.3f}")
        per_layer = base / layers
        print(f"# serial arm: {per_layer:.3f} ms per layer (head and embedding included in the step)")
    vdist.destroy_sequence_parallel()
    assert ops.get_tuning("sp_reserve_cus") == 0


if __name__ == "__main__":
    main()
