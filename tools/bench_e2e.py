#!/usr/bin/env python3
"""End-to-end VideoCoF edit on one MI355X: prompt strings + source video in, edited video out.

    python tools/bench_e2e.py [--model 14b|1.3b] [--steps 4] [--frames 81] [--height 480] [--width 832] [--uint8]
    python tools/bench_e2e.py --io-only [--frames 81] [--height 480] [--width 832] [--reps 5]

Everything the reference's fast_infer.py runs per video, through this package's WanPipeline: umT5-XXL encode of
the prompt, WanVAE encode of the source clip, the CoF denoise loop (source | grounding | target latents,
guidance 1.0 as in fast_infer.py:163), WanVAE decode of the grounding and edit segments.  Random-init weights of
the real architectures, synthetic video, a toy whitespace tokenizer (the tokenizer is host-side and not timed
meaningfully).  Reported: wall seconds per stage (HIP events would hide host gaps; these are synchronised
wall-clock stages) and the total.

--uint8 feeds the pipeline the uint8 [T, H, W, 3] frames of a video reader (host memory) and asks for output_type="uint8";
without it the pipeline gets a bf16 device tensor and returns float32 planar frames.  Both print the pipeline's own
`vae_encode` / `vae_decode` stage seconds and `caller_to_uint8`: what the CALLER then still spends to reach uint8 [T, H, W, 3]
(the reference writer's rearrangement and `(x * 255).astype(np.uint8)` on the float path; zero on the uint8 path).

--io-only builds no model and times the two ends alone, old and new path alternating in one process:
  out: decoder output on the device (VAE dtype) -> uint8 [T, H, W, 3] in host memory.  old = decode_latents' float path (device
       arithmetic, float32 planes through page-locked memory) + the reference writer's host conversion; new = decode_latents(
       as_uint8=True) (wan_video_to_frames_u8 + one copy).
  in:  uint8 frames in host memory -> the VAE's input on the device.  old = the reference loader's host conversion to float32
       (fast_infer.py:88-90) + `.to(device, dtype)`; new = bytes to the device + wan_frames_u8_to_video.
  cmp: the compare clip (save_side_by_side, fast_infer.py:183-206) as uint8 [T, H, 2 W, 3] in host memory.  old = the float32 planes
       both paths above leave on the host (the loader's video, the pipeline's frames), _normalize_to_01 of each, the crop, the
       cat and the writer's host conversion; new = the source's bytes to the device + compare_frames (wan_video_range_flag +
       wan_frames_u8_compose) on the edit's device frames + one copy into page-locked memory.
and each kernel alone with HIP events (bytes read + written per second)."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = {"14b": dict(dim=5120, ffn_dim=13824, num_heads=40, num_layers=40),
        "1.3b": dict(dim=1536, ffn_dim=8960, num_heads=12, num_layers=30)}


class ToyTokenizer:
    def __init__(self, vocab):
        self.vocab = vocab

    def __call__(self, prompt, padding=None, max_length=512, truncation=True, add_special_tokens=True, return_tensors="pt"):
        ids = torch.zeros(len(prompt), max_length, dtype=torch.long)
        mask = torch.zeros(len(prompt), max_length, dtype=torch.long)
        for b, p in enumerate(prompt):
            toks = [2 + (sum(map(ord, w)) % (self.vocab - 2)) for w in p.split()][: max_length - 1] + [1]
            ids[b, :len(toks)] = torch.tensor(toks)
            mask[b, :len(toks)] = 1
        return SimpleNamespace(input_ids=ids, attention_mask=mask)


def writer_bytes(videos):
    """The bytes the reference's writer makes of the pipeline's float32 [1, 3, T, H, W] frames (videox_fun/utils/utils.py:59-68, one
    video per call): channels last, times 255 in float32, truncated -> uint8 [T, H, W, 3].  Done here on the whole clip at once, which
    is no slower than the reference's frame-by-frame loop."""
    import numpy as np
    v = torch.from_numpy(videos) if isinstance(videos, np.ndarray) else videos
    return (v[0].permute(1, 2, 3, 0) * 255).numpy().astype(np.uint8)


def io_only(args):
    import numpy as np
    from videocof_amd import WanPipeline, ops
    from videocof_amd.video_io import compare_frames, reference_compare_frames, reference_frames_to_video
    dev = torch.device("cuda:0")
    T, H, W = args.frames, args.height, args.width
    dtype = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    decoded = (torch.rand(1, 3, T, H, W, device=dev, generator=g) * 2.2 - 1.1).clamp(-1, 1).to(dtype)      # a decoder output
    frames_host = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8)                                    # a reader's frames
    # the pipeline's own decode_latents around a stand-in decoder that returns `decoded`
    pipe = WanPipeline(transformer=SimpleNamespace(device=dev), scheduler=SimpleNamespace(),
                       vae=SimpleNamespace(dtype=dtype, decode=lambda z: SimpleNamespace(sample=decoded)))
    z = torch.zeros(1, device=dev, dtype=dtype)

    def out_old():
        return writer_bytes(pipe.decode_latents(z))

    def out_new():
        return pipe.decode_latents(z, as_uint8=True)[0]

    def in_old():
        return reference_frames_to_video(frames_host[None]).to(device=dev, dtype=dtype)

    def in_new():
        return ops.frames_u8_to_video(frames_host[None].to(dev), dtype)

    src_planes = reference_frames_to_video(frames_host[None])                   # what the reference's loader leaves on the host
    edit_planes = torch.from_numpy(pipe.decode_latents(z)).clone()             # what its pipeline returns: float32 [1, 3, T, H, W]
    edit_dev = ops.video_to_frames_u8(decoded)                                  # what output_type="uint8" keeps on the device
    cmp_host = torch.empty(1, T, H, 2 * W, 3, dtype=torch.uint8, pin_memory=True)

    def cmp_old():
        return reference_compare_frames(src_planes, edit_planes)

    def cmp_new():
        return compare_frames(frames_host[None].to(dev), edit_dev, out=cmp_host)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    res = {k: [] for k in ("out_old", "out_new", "in_old", "in_new", "cmp_old", "cmp_new")}
    for fn in (out_old, out_new, in_old, in_new, cmp_old, cmp_new):
        fn()                                             # warm-up: allocator, page-locked buffers
    for _ in range(args.reps):                           # alternating old / new
        for name, fn in (("out_old", out_old), ("out_new", out_new), ("in_old", in_old), ("in_new", in_new),
                         ("cmp_old", cmp_old), ("cmp_new", cmp_new)):
            res[name].append(round(wall(fn)[0], 5))
    assert np.array_equal(out_old(), out_new()), "old and new output paths disagree"
    assert torch.equal(in_old(), in_new()), "old and new input paths disagree"
    assert torch.equal(cmp_old(), cmp_new()), "old and new compare clips disagree"

    def kernel_seconds(fn, iters=20):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters / 1e3

    n = T * H * W * 3
    fr_dev = frames_host[None].to(dev)
    clip = torch.empty(1, T, H, W, 3, device=dev, dtype=torch.uint8)
    vid = torch.empty(1, 3, T, H, W, device=dev, dtype=dtype)
    lib, P = ops._lib.load(), ops._p
    st = torch.cuda.current_stream().cuda_stream
    k_in = kernel_seconds(lambda: lib.wan_frames_u8_to_video(P(fr_dev), P(vid), 1, 1, T, H, W, st))
    k_out = kernel_seconds(lambda: lib.wan_video_to_frames_u8(P(decoded), 1, P(clip), 1, T, H, W, 0, T, T, 0, st))
    canvas = torch.empty(T, H, 2 * W, 3, device=dev, dtype=torch.uint8)
    flag = ops.video_range_flag(fr_dev)
    srcs = [dict(tensor=fr_dev[0], mode=ops.COMPOSE_LOADER_ROUNDTRIP, flag=flag, dst=(0, 0)),
            dict(tensor=edit_dev[0], mode=ops.COMPOSE_COPY, dst=(0, W))]
    k_cmp = kernel_seconds(lambda: ops.frames_u8_compose(canvas, srcs))
    k_flag = kernel_seconds(lambda: ops.video_range_flag(fr_dev))
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"what": f"frame I/O alone, {T}f@{H}x{W}, bf16 VAE dtype, {args.reps} alternating repetitions, wall seconds",
                      "seconds": res, "median": {k: med(v) for k, v in res.items()},
                      "old_path_spread": {k: round(max(res[k]) - min(res[k]), 5) for k in ("out_old", "in_old", "cmp_old")},
                      "kernel_seconds": {"wan_frames_u8_to_video": round(k_in, 7), "wan_video_to_frames_u8": round(k_out, 7),
                                         "wan_frames_u8_compose": round(k_cmp, 7), "wan_video_range_flag": round(k_flag, 7)},
                      "kernel_tbps": {"wan_frames_u8_to_video": round(n * 3 / k_in / 1e12, 3),
                                      "wan_video_to_frames_u8": round(n * 3 / k_out / 1e12, 3),
                                      "wan_frames_u8_compose": round(n * 4 / k_cmp / 1e12, 3),
                                      "wan_video_range_flag": round(n / k_flag / 1e12, 3)},
                      "bytes": {"uint8": n, "bf16": 2 * n, "float32": 4 * n}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="14b", choices=sorted(DIMS))
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=81)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--uint8", action="store_true", help="uint8 frames in (host), uint8 frames out")
    ap.add_argument("--io-only", action="store_true", help="time the frame I/O at both ends alone, old and new path alternating")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.io_only:
        return io_only(args)
    from videocof_amd import (AutoencoderKLWan, FlowUniPCMultistepScheduler, WanPipeline, WanT5EncoderModel,
                              WanTransformer3DModel)
    from videocof_amd.weights import random_dit_state_dict, random_t5_state_dict, random_vae_state_dict
    dev = torch.device("cuda:0")
    d = DIMS[args.model]
    dit = WanTransformer3DModel(**d)
    dit.load_state_dict(random_dit_state_dict(dev, seed=0, dim=d["dim"], ffn_dim=d["ffn_dim"], num_layers=d["num_layers"]), device=dev)
    vae = AutoencoderKLWan()
    vae.load_state_dict(random_vae_state_dict(dev), device=dev)
    tcfg = dict(vocab=256384, dim=4096, dim_attn=4096, dim_ffn=10240, num_heads=64, num_layers=24, num_buckets=32)
    t5 = WanT5EncoderModel(shared_pos=False, **tcfg)
    t5.load_state_dict(random_t5_state_dict(dev, **tcfg), device=dev)
    pipe = WanPipeline(tokenizer=ToyTokenizer(tcfg["vocab"]), text_encoder=t5, vae=vae, transformer=dit,
                       scheduler=FlowUniPCMultistepScheduler(shift=1))
    g = torch.Generator(device=dev).manual_seed(0)
    if args.uint8:
        video = torch.randint(0, 256, (args.frames, args.height, args.width, 3), dtype=torch.uint8)      # host frames, as read
    else:
        video = (torch.rand(1, 3, args.frames, args.height, args.width, device=dev, generator=g) * 2 - 1).bfloat16()
    prompt = "remove the red cup from the wooden table and keep everything else unchanged"
    kw = dict(video=video, prompt=prompt, height=args.height, width=args.width, source_frames=args.frames,
              reasoning_frames=4, num_inference_steps=args.steps, guidance_scale=1.0, shift=3, repeat_rope=True, cot=True,
              generator=g, output_type="uint8" if args.uint8 else "numpy", return_dict=True)

    stages = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        stages[name] = round(time.perf_counter() - t0, 4)
        return out

    pipe(**{**kw, "num_inference_steps": 1})            # warm-up: allocator, workspaces, LDS attributes
    # stage timings with the same calls the pipeline makes
    timed("text_encoder", lambda: pipe.encode_prompt(prompt, None, False, device=dev))
    from videocof_amd import frames_to_video
    timed("vae_encode", lambda: vae.encode(frames_to_video(video.to(dev)) if args.uint8 else video)[0].mode())
    pipe.stage_seconds = {}
    out = timed("pipeline_total", lambda: pipe(**kw))
    own = {k: round(v, 4) for k, v in pipe.stage_seconds.items()}
    pipe.stage_seconds = None
    t0 = time.perf_counter()
    frames_u8 = out.videos[0] if args.uint8 else writer_bytes(out.videos)
    caller = 0.0 if args.uint8 else round(time.perf_counter() - t0, 4)
    assert frames_u8.dtype.name == "uint8" and frames_u8.shape[1:] == (args.height, args.width, 3)
    lat = out.latents if getattr(out, "latents", None) is not None else None
    tl = (args.frames - 1) // 4 + 1
    z = torch.randn(1, 16, tl + 1, args.height // 8, args.width // 8, device=dev, generator=g).bfloat16()
    timed("vae_decode_ground_plus_edit", lambda: (vae.decode(z[:, :, :1]).sample, vae.decode(z[:, :, 1:]).sample))
    stages["dit_denoise_loop"] = round(stages["pipeline_total"] - stages["text_encoder"] - stages["vae_encode"]
                                       - stages["vae_decode_ground_plus_edit"], 4)
    print(json.dumps({"what": f"VideoCoF edit end to end, Wan2.1-{args.model} dims, {args.frames}f@{args.height}x{args.width}, "
                              f"{args.steps} steps, guidance 1.0, {'uint8 frames in and out' if args.uint8 else 'bf16 device video in, float32 frames out'}",
                      "seconds": stages, "pipeline_stage_seconds": own, "caller_to_uint8": caller,
                      "edit_video_shape": list(out.edit_videos.shape), "ground_video_shape": list(out.ground_videos.shape),
                      "note": "dit_denoise_loop = pipeline_total - the separately timed stages; pipeline uses cache_context "
                              "and skip_source_prediction (its defaults)"}))


if __name__ == "__main__":
    main()
