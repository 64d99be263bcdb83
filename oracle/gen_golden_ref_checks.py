#!/usr/bin/env python3
"""tests/golden/ref_*.npz + tests/golden/ref_surface.json: what the reference computes on the inputs of
tests/test_oracle_vs_reference.py, so that those checks run wherever the repository is -- without the reference tree.

The inputs are NOT stored: the tests regenerate them from the same seeded generators, in the same order, as below (every
draw of a torch.Generator / random.Random here is mirrored there).  Stored: the reference's outputs (fp32), the scheduler
timesteps / sigmas as the reference's tensors hold them, the tensors a reference LoRA merge CHANGED (the delta against the
deterministic base state dict, stored as its rank-r factors in fp64: a LoRA delta has the rank of the LoRA; the factors are checked
here to give back the reference's fp32 delta to rel-L2 < 1e-6 of the delta itself), the constructor configs (repr, read back with
ast.literal_eval), and the call signatures and method names of the seams the mirrors implement (names and default expressions read
with `ast`).  Several files, none of them large: see FILES.
Build container only (needs the reference tree; oracle/ref_import.py)."""
import ast
import itertools
import json
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_import import REFERENCE_ROOT, load_reference          # noqa: E402
from videocof_amd.weights import (deterministic_dit_state_dict, deterministic_t5_state_dict,   # noqa: E402
                                  deterministic_vae_state_dict)

GOLDEN = os.path.join(ROOT, "tests", "golden")
# output file -> key prefixes (several small files; the sweep's trajectory is split over SWEEP_PARTS files)
FILES = {"ref_dit.npz": ("dit_",), "ref_t5_vae.npz": ("t5_", "vae_"), "ref_host.npz": ("unipc_", "host_", "lora_case/"),
         "ref_sweep_0.npz": ("sweep_timesteps", "sweep_sigmas", "sweep_nsteps", "sweep_ok", "sweep_traj_0")}
SWEEP_PARTS = 3
FILES.update({f"ref_sweep_{i}.npz": FILES.get(f"ref_sweep_{i}.npz", ()) + (f"sweep_traj_{i}",) for i in range(1, SWEEP_PARTS)})
SURFACE = os.path.join(ROOT, "tests", "golden", "ref_surface.json")

# the seams of tests/test_oracle_vs_reference.py::test_call_signatures_are_the_references: (file under videox_fun/, class, function)
SEAMS = [
    ("models/wan_transformer3d.py", "WanTransformer3DModel", "forward"),
    ("models/wan_transformer3d.py", "WanTransformer3DModel", "__init__"),
    ("models/wan_transformer3d.py", "WanTransformer3DModel", "from_pretrained"),
    ("models/wan_transformer3d.py", "WanTransformer3DModel", "enable_teacache"),
    ("models/attention_utils.py", None, "attention"),
    ("models/attention_utils.py", None, "flash_attention"),
    ("utils/fm_solvers_unipc.py", "FlowUniPCMultistepScheduler", "__init__"),
    ("utils/fm_solvers_unipc.py", "FlowUniPCMultistepScheduler", "set_timesteps"),
    ("utils/fm_solvers_unipc.py", "FlowUniPCMultistepScheduler", "step"),
    ("pipeline/pipeline_wan.py", "WanPipeline", "__call__"),
    ("pipeline/pipeline_wan.py", "WanPipeline", "__init__"),
    ("pipeline/pipeline_wan.py", "WanPipeline", "prepare_latents"),
    ("pipeline/pipeline_wan.py", "WanPipeline", "prepare_video_latents"),
    ("pipeline/pipeline_wan.py", "WanPipeline", "prepare_video_latents_new"),
    ("pipeline/pipeline_wan.py", "WanPipeline", "prepare_cot_video_latents"),
    ("pipeline/pipeline_wan.py", "WanPipeline", "prepare_extra_step_kwargs"),
    ("pipeline/pipeline_wan.py", "WanPipeline", "decode_latents"),
    ("pipeline/pipeline_wan.py", "WanPipeline", "check_inputs"),
    ("pipeline/pipeline_wan.py", "WanPipeline", "encode_prompt"),
    ("pipeline/pipeline_wan.py", "WanPipeline", "_get_t5_prompt_embeds"),
    ("models/wan_transformer3d.py", "WanTransformer3DModel", "unpatchify"),
    ("models/wan_transformer3d.py", "WanTransformer3DModel", "share_cfg_skip"),
    ("models/wan_transformer3d.py", "WanTransformer3DModel", "share_teacache"),
    ("models/wan_transformer3d.py", "WanTransformer3DModel", "enable_cfg_skip"),
    ("models/wan_transformer3d.py", "WanTransformer3DModel", "enable_riflex"),
    ("models/cache_utils.py", "TeaCache", "__init__"),
    ("utils/fm_solvers_unipc.py", "FlowUniPCMultistepScheduler", "index_for_timestep"),
    ("utils/fm_solvers_unipc.py", "FlowUniPCMultistepScheduler", "add_noise"),
    ("utils/fm_solvers_unipc.py", "FlowUniPCMultistepScheduler", "scale_model_input"),
    ("utils/fm_solvers_unipc.py", "FlowUniPCMultistepScheduler", "set_begin_index"),
    ("models/wan_vae.py", "AutoencoderKLWan", "encode"),
    ("models/wan_vae.py", "AutoencoderKLWan", "decode"),
    ("models/wan_vae.py", "AutoencoderKLWan", "__init__"),
    ("models/wan_vae.py", "AutoencoderKLWan", "from_pretrained"),
    ("models/wan_text_encoder.py", "WanT5EncoderModel", "forward"),
    ("models/wan_text_encoder.py", "WanT5EncoderModel", "__init__"),
    ("models/wan_text_encoder.py", "WanT5EncoderModel", "from_pretrained"),
    ("utils/lora_utils.py", None, "merge_lora"),
    ("utils/lora_utils.py", None, "unmerge_lora"),
    ("dist/fuser.py", None, "set_multi_gpus_devices"),
]
# the classes of tests/test_oracle_vs_reference.py::test_public_methods_of_the_reference_classes_exist_on_the_mirrors
CLASSES = [("models/wan_transformer3d.py", "WanTransformer3DModel"), ("pipeline/pipeline_wan.py", "WanPipeline"),
           ("models/wan_vae.py", "AutoencoderKLWan"), ("models/wan_text_encoder.py", "WanT5EncoderModel"),
           ("utils/fm_solvers_unipc.py", "FlowUniPCMultistepScheduler"), ("models/cache_utils.py", "TeaCache")]

DIT_SMALL = dict(dim=256, ffn_dim=512, num_layers=2, in_dim=16, out_dim=16, text_dim=64, freq_dim=256)


def _parse(path):
    with open(os.path.join(REFERENCE_ROOT, "videox_fun", path)) as f:
        return ast.parse(f.read()).body


def ref_sig(path, cls, fn):
    body = _parse(path)
    if cls:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    a = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == fn).args
    names = [x.arg for x in a.posonlyargs + a.args]
    defaults = [None] * (len(names) - len(a.defaults)) + list(a.defaults)
    out = [(n, None if d is None else ast.unparse(d)) for n, d in zip(names, defaults)]
    out += [(x.arg, None if d is None else ast.unparse(d)) for x, d in zip(a.kwonlyargs, a.kw_defaults)]
    return [[n, d] for n, d in out if n != "cls"]


def ref_methods(path, cls):
    c = next(n for n in _parse(path) if isinstance(n, ast.ClassDef) and n.name == cls)
    return [n.name for n in c.body if isinstance(n, ast.FunctionDef)]


def small_ref_dit(ns):
    return ns.transformer.WanTransformer3DModel(model_type="t2v", dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64,
                                                in_dim=16, out_dim=16, freq_dim=256, cross_attn_norm=True, qk_norm=True)


def low_rank(delta, max_rank=8):
    """(U S, V^T) in fp64 with U S @ V^T = delta to rel-L2 < 1e-6 (the rank of the LoRA; the rest is fp32 rounding)."""
    d = delta.double()
    u, sv, vt = torch.linalg.svd(d, full_matrices=False)
    r = int((sv > 1e-5 * sv[0]).sum())
    assert 1 <= r <= max_rank, r
    us, v = u[:, :r] * sv[:r], vt[:r]
    err = float((us @ v - d).norm() / d.norm())
    assert err < 1e-6, err
    return us, v


def merged_deltas(ns, base, lora, multiplier):
    """The reference's merge_lora on its own model loaded with `base`: {key: merged - base} of every tensor it changed."""
    m = small_ref_dit(ns)
    m.load_state_dict(base, strict=True)
    ns.load_lora_utils().merge_lora(types.SimpleNamespace(transformer=m), None, multiplier, device="cpu", dtype=torch.float32,
                                    state_dict=dict(lora), transformer_only=True)
    want = m.state_dict()
    return {k: want[k] - base[k] for k in want if not torch.equal(want[k], base[k])}


@torch.no_grad()
def main():
    torch.set_num_threads(8)
    ns = load_reference()
    out, surf = {}, {}

    # ---- test_dit_forward_random_inputs
    cfgd = dict(dim=384, ffn_dim=640, num_layers=2, in_dim=16, out_dim=16, text_dim=96, freq_dim=256)
    sd = deterministic_dit_state_dict(**cfgd)
    m = ns.transformer.WanTransformer3DModel(model_type="t2v", dim=384, ffn_dim=640, num_heads=3, num_layers=2, text_dim=96,
                                             in_dim=16, out_dim=16, freq_dim=256, cross_attn_norm=True, qk_norm=True)
    m.load_state_dict(sd, strict=True)
    m.eval()
    g = torch.Generator().manual_seed(123)
    lat = torch.randn(2, 16, 8, 6, 10, generator=g)
    ctx = [torch.randn(17, 96, generator=g), torch.randn(3, 96, generator=g)]
    t = torch.tensor([612, 612])
    seq_len = 8 * 3 * 5
    out["dit_main"] = m(lat, t=t, context=ctx, seq_len=seq_len, frame_split_indices=[3, 3], ground_frame_indices=[(3, 5), (3, 5)])
    out["dit_pad"] = m(lat[:1], t=t[:1], context=ctx[:1], seq_len=seq_len + 8)
    rnd = random.Random(7)
    for case in range(14):
        F, Hl, Wl = rnd.randint(1, 9), 2 * rnd.randint(1, 7), 2 * rnd.randint(1, 9)
        B = rnd.choice([1, 1, 2])
        L = F * (Hl // 2) * (Wl // 2)
        rnd.choice([0, 0, 1, 5, 64])
        mode = ("t2v", "paired", "cof", "cof")[case % 4] if F >= 3 else "t2v"
        fsi = gfi = None
        if mode != "t2v":
            fs = rnd.randint(1, F - 2)
            fsi = [fs] * B
            if mode == "cof":
                gfi = [(fs, fs + rnd.randint(1, F - 1 - fs))] * B
        lat_c = torch.randn(B, 16, F, Hl, Wl, generator=g)
        ctx_c = [torch.randn(rnd.randint(1, 77), 96, generator=g) for _ in range(B)]
        t_c = torch.tensor([rnd.choice([999, 899, 749, 499, 37])] * B)
        out[f"dit_case{case}"] = m(lat_c, t=t_c, context=ctx_c, seq_len=L, frame_split_indices=fsi, ground_frame_indices=gfi)

    # ---- test_unipc_random_trajectory
    g = torch.Generator().manual_seed(7)
    for steps, shift in ((7, 3.0), (20, 5.0)):
        sch = ns.unipc.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, solver_order=2, prediction_type="flow_prediction")
        sch.set_timesteps(steps, device="cpu", shift=shift)
        out[f"unipc_{steps}_timesteps"] = sch.timesteps
        a = torch.randn(1, 16, 2, 4, 4, generator=g)
        traj = []
        for tt in sch.timesteps:
            v = torch.randn(1, 16, 2, 4, 4, generator=g)
            a = sch.step(v, tt, a, return_dict=False)[0]
            traj.append(a)
        out[f"unipc_{steps}_traj"] = torch.stack(traj)

    # ---- test_t5_random_tokens
    tcfg = dict(vocab=301, dim=192, dim_attn=192, dim_ffn=448, num_heads=3, num_layers=3, num_buckets=32)
    t5 = ns.load_text_encoder().WanT5EncoderModel(shared_pos=False, dropout=0.0, **tcfg).eval()
    t5.load_state_dict(deterministic_t5_state_dict(**tcfg), strict=True)
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 301, (2, 150), generator=g)
    mask = torch.ones(2, 150, dtype=torch.long)
    mask[1, 40:] = 0
    out["t5_out"] = t5(ids, mask)[0]

    # ---- test_vae_random_clip
    vae = ns.vae.AutoencoderKLWan()
    vae.load_state_dict(deterministic_vae_state_dict(), strict=True)
    vae.eval()
    g = torch.Generator().manual_seed(5)
    video = torch.rand(1, 3, 9, 16, 24, generator=g) * 2 - 1
    out["vae_mu0"] = vae.encode(video)[0].mode()
    z = torch.randn(1, 16, 2, 2, 3, generator=g)
    out["vae_dec0"] = vae.decode(z).sample
    for i, (T, H, W) in enumerate(((1, 16, 24), (2, 16, 16), (13, 24, 16), (9, 24, 40))):
        video = torch.rand(1, 3, T, H, W, generator=g) * 2 - 1
        mu = vae.encode(video)[0].mode()
        out[f"vae_mu{i + 1}"] = mu
        z = torch.randn(1, 16, mu.shape[2], H // 8, W // 8, generator=g)
        out[f"vae_dec{i + 1}"] = vae.decode(z).sample

    # ---- test_product_host_code_vs_reference
    g = torch.Generator().manual_seed(21)
    ref = ns.unipc.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, solver_order=2, prediction_type="flow_prediction")
    for steps, shift in ((9, 3.0), (25, 5.0)):
        ref.set_timesteps(steps, device="cpu", shift=shift)
        out[f"host_{steps}_timesteps"], out[f"host_{steps}_sigmas"] = ref.timesteps, ref.sigmas
        a = torch.randn(1, 16, 2, 4, 4, generator=g)
        traj = []
        for tt in ref.timesteps:
            v = torch.randn(1, 16, 2, 4, 4, generator=g)
            a = ref.step(v, tt, a, return_dict=False)[0]
            traj.append(a)
        out[f"host_{steps}_traj"] = torch.stack(traj)
    x0, nz = torch.randn(2, 16, 2, 4, 4, generator=g), torch.randn(2, 16, 2, 4, 4, generator=g)
    ref.set_timesteps(9, device="cpu", shift=3.0)
    tsel = ref.timesteps[[2, 5]]
    out["host_add_noise"] = ref.add_noise(x0, nz, tsel)
    surf["host_index_for_timestep"] = [ref.index_for_timestep(ref.timesteps[4]), ref.index_for_timestep(ref.timesteps[4], ref.timesteps[2:])]
    surf["host_len"] = len(ref)
    surf["host_scheduler_config"] = repr({k: v for k, v in vars(ref.config).items() if not k.startswith("_")})
    ref.set_begin_index(3)
    out["host_add_noise_begin3"] = ref.add_noise(x0, nz, tsel)
    surf["host_model_config"] = repr({k: (tuple(v) if isinstance(v, (list, tuple)) else v)
                                      for k, v in vars(small_ref_dit(ns).config).items() if not k.startswith("_")})
    lora = {}
    for name, (o, i) in {"blocks.1.self_attn.v": (256, 256), "blocks.0.ffn.2": (256, 512), "blocks.1.cross_attn.k": (256, 256)}.items():
        lora[f"diffusion_model.{name}.lora_down.weight"] = torch.randn(8, i, generator=g) * 0.1
        lora[f"diffusion_model.{name}.lora_up.weight"] = torch.randn(o, 8, generator=g) * 0.1
        lora[f"diffusion_model.{name}.alpha"] = torch.tensor(4.0)
    base = deterministic_dit_state_dict(**DIT_SMALL)
    deltas = merged_deltas(ns, base, lora, 0.6)
    surf["host_lora_changed"] = sorted(deltas)
    for k, v in deltas.items():
        out[f"host_lora/{k}/us"], out[f"host_lora/{k}/vt"] = low_rank(v)

    # ---- test_lora_key_conventions_take_part_exactly_as_in_the_reference
    from tests.test_oracle_vs_reference import lora_key_convention_cases
    surf["lora_cases_changed"] = {}
    for what, lora in lora_key_convention_cases(base).items():
        deltas = merged_deltas(ns, base, lora, 0.7)
        surf["lora_cases_changed"][what] = sorted(deltas)
        for k, v in deltas.items():
            out[f"lora_case/{what}/{k}/us"], out[f"lora_case/{what}/{k}/vt"] = low_rank(v)

    # ---- test_call_signatures_are_the_references, test_public_methods_of_the_reference_classes_exist_on_the_mirrors
    surf["signatures"] = [[path, cls, fn, ref_sig(path, cls, fn)] for path, cls, fn in SEAMS]
    surf["methods"] = [[path, cls, ref_methods(path, cls)] for path, cls in CLASSES]

    # ---- test_unipc_configuration_sweep: per configuration, the reference's timesteps / sigmas and its trajectory up to the first
    # step that raised or went non-finite (`ok` = the whole trajectory is finite)
    g = torch.Generator().manual_seed(0)
    ts, sg, tr, nsteps, oks = [], [], [], [], []
    for steps, shift, order, lof, dc, st in itertools.product([1, 2, 3, 4, 7, 20], [1.0, 3.0, 5.0], [1, 2, 3], [True, False], [[], [0], [1, 2]],
                                                              ["bh1", "bh2"]):
        kw = dict(num_train_timesteps=1000, shift=1, solver_order=order, lower_order_final=lof, disable_corrector=dc, solver_type=st)
        r = ns.unipc.FlowUniPCMultistepScheduler(prediction_type="flow_prediction", **kw)
        r.set_timesteps(steps, device="cpu", shift=shift)
        ts.append(r.timesteps)
        sg.append(r.sigmas)
        a = torch.randn(1, 4, 2, 3, 3, generator=g)
        ok, n = True, 0
        for tt in r.timesteps:
            v = torch.randn(1, 4, 2, 3, 3, generator=g)
            try:
                a = r.step(v, tt, a, return_dict=False)[0]
            except Exception:
                ok = False
            if not ok or not torch.isfinite(a).all():
                ok = False
                break
            tr.append(a)
            n += 1
        nsteps.append(n)
        oks.append(ok)
    out["sweep_timesteps"] = torch.cat(ts)
    out["sweep_sigmas"] = torch.cat(sg)
    tr = torch.stack(tr)
    for i, part in enumerate(torch.tensor_split(tr, SWEEP_PARTS)):
        out[f"sweep_traj_{i}"] = part
    out["sweep_nsteps"] = torch.tensor(nsteps)
    out["sweep_ok"] = torch.tensor(oks)
    print("sweep: %d configurations, %d with a finite trajectory" % (len(oks), sum(oks)))

    left = dict(out)
    for name, prefixes in FILES.items():
        part = {k: left.pop(k) for k in list(left) if k.startswith(prefixes)}
        path = os.path.join(GOLDEN, name)
        np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in part.items()})
        print(os.path.getsize(path) // 1024, "KiB", path)
    assert not left, sorted(left)
    with open(SURFACE, "w") as f:
        json.dump(surf, f, indent=1)
        f.write("\n")
    print(os.path.getsize(SURFACE) // 1024, "KiB", SURFACE)


if __name__ == "__main__":
    main()
