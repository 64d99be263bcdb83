"""VideoCoF denoising pipeline on the HIP-backed DiT.

Mirror of ``WanPipeline`` (``videox_fun/pipeline/pipeline_wan.py:125-138, 516-799``):
same constructor ``(tokenizer, text_encoder, vae, transformer, scheduler)``, same
``__call__`` argument names and ``WanPipelineOutput(videos, ground_videos,
edit_videos)``.  The denoise loop reproduces the reference's glue exactly:

    condition_count = (source_frames-1)//4 + 1                              (:630-631)
    G = 1 if reasoning_frames <= 1 else (reasoning_frames-1)//4 + 1          (:637)
    latents = cat([vae.encode(video).mode(), randn(Fs+G)], dim=2)            (:406-417)
    per step: v = transformer(x, t, ctx, seq_len, fsi=[cc]*B, gfi=[(cc,cc+G)]*B)
              CFG: v = v_uncond + s*(v_text - v_uncond), batch order [uncond, cond] (:700, 731-733)
              v[:, :, :cc] = 0                                              (:736)
              latents = scheduler.step(v, t, latents)[0]                    (:740)
    decode only the grounding and edit segments                             (:760-777)

Prompts: with a ``tokenizer`` (a HuggingFace tokenizer object, e.g. ``AutoTokenizer`` of
``google/umt5-xxl``) and a ``videocof_amd.WanT5EncoderModel`` the strings are encoded on the GPU as in
``_get_t5_prompt_embeds`` (:140-181); alternatively pass ``prompt_embeds`` /
``negative_prompt_embeds`` (lists of ``[len<=512, 4096]`` tensors), or a plain callable
``text_encoder(list[str]) -> list[Tensor]`` without a tokenizer.
"""
from __future__ import annotations

import math
from contextlib import contextmanager
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable, Optional, Union

import numpy as np
import torch

from .fm_solvers import FlowDPMSolverMultistepScheduler, get_sampling_sigmas, retrieve_timesteps
from .fm_solvers_unipc import FlowUniPCMultistepScheduler

__all__ = ["WanPipeline", "WanPipelineOutput"]


@dataclass
class WanPipelineOutput:
    videos: Optional[Union[torch.Tensor, np.ndarray]]
    ground_videos: Optional[Union[torch.Tensor, np.ndarray]] = None
    edit_videos: Optional[Union[torch.Tensor, np.ndarray]] = None
    latents: Optional[torch.Tensor] = None          # extension: final latents (output_type="latent")
    compare_videos: Optional[Union[torch.Tensor, np.ndarray]] = None   # extension: source | edit side by side (compare=True)
    edit_region: Optional[tuple] = None             # extension: (y, x, h, w) in pixels, what the loop ran on (edit_region=True); None when off
    edit_region_time: Optional[tuple] = None        # extension: (first pixel frame, pixel frame count) of it (edit_region_time_margin); None when off
    edit_region_vae: Optional[tuple] = None         # extension: (y, x, h, w) in pixels, the box the VAE ran on (edit_region_vae_halo); None when off
    edit_regions: Optional[tuple] = None            # extension: ((y, x, h, w), ...) in pixels, one per box the loop ran on (edit_region_split; edit_region then encloses them all); None when off or where the mask was not split
    edit_region_track: Optional[tuple] = None       # extension: ((h, w), ((y_f, x_f), ...)) in pixels, the box of every latent frame of the source segment (edit_region_follow; edit_region then encloses them all); None when off
    color_match: Optional[torch.Tensor] = None      # extension: int32 [B, T, 3, 2] on the device, the (gain, offset) in 1/4096 applied to every frame and channel of the edit segment (color_match=...); None when off


def _require_source(has_source: bool, why: str) -> None:
    if not has_source:
        raise ValueError(f"{why}; this call has none (no `video`, `source_latents` or `latents`)")


def _has_layout(frames: int, cc: int, G: int) -> bool:
    """The one statement of the CoF layout of `frames` latent frames; _LAYOUT.format(cc, G) describes it in a message."""
    return frames == 2 * cc + G


_LAYOUT = "[source | grounding | target] = [{0} | {1} | {0}]"


def _local_attention_args(local_attention, local_from, capture_graph) -> Optional[dict]:
    """The `local_attention` option as the arguments of ``enable_local_attention`` (None: the option is off)."""
    if local_attention is None:
        return None
    pair = isinstance(local_attention, (tuple, list)) and len(local_attention) == 2
    cfg = dict(local_attention) if isinstance(local_attention, dict) else dict(zip(("window_frames", "window_rows"), local_attention)) if pair else {}
    if set(cfg) - {"window_frames", "window_rows", "sink_frames", "dense_layers"} or not {"window_frames", "window_rows"} <= set(cfg):
        raise ValueError(f"local_attention={local_attention!r}: a (window_frames, window_rows) pair or a dict of the "
                         "enable_local_attention arguments")
    if isinstance(local_from, bool) or not isinstance(local_from, int) or local_from < 0:
        raise ValueError(f"local_attention_from_step={local_from!r}: a step index >= 0")
    if capture_graph == "loop":
        raise NotImplementedError("local_attention with capture_graph='loop': the recorded loop does not hold the key-tile "
                                  "plans (use capture_graph='step')")
    return cfg


class WanPipeline:
    def __init__(self, tokenizer=None, text_encoder=None, vae=None, transformer=None, scheduler=None):
        if transformer is None or scheduler is None:
            raise ValueError("WanPipeline needs at least a transformer and a scheduler")
        self.tokenizer, self.text_encoder, self.vae = tokenizer, text_encoder, vae
        self.transformer, self.scheduler = transformer, scheduler
        self._guidance_scale = 1.0
        self._num_timesteps = 0
        self._interrupt = False
        self._graphed = None
        self._graphed_loop = None
        self._cfg_skip_literal = False      # tests: take cfg_skip steps the reference's literal way (doubled batch, then guidance)
        self.release_workspaces_after_denoise = False     # see __call__: hand the DiT's activation buffers back before the VAE decode
        # Set to a dict to get synchronised wall seconds per stage of the next __call__ ("text_encoder", "vae_encode",
        # "denoise_loop", "vae_decode"): a measuring aid (bench.py's `e2e` object); None = no synchronisation anywhere.
        self.stage_seconds = None

    def _stage(self, name, t0=None):
        """Stage clock for ``stage_seconds``: call without t0 to start (returns the start time), with t0 to stop."""
        if self.stage_seconds is None:
            return None
        import time
        torch.cuda.synchronize()
        if t0 is None:
            return time.perf_counter()
        self.stage_seconds[name] = self.stage_seconds.get(name, 0.0) + time.perf_counter() - t0
        return None

    guidance_scale = property(lambda self: self._guidance_scale)
    num_timesteps = property(lambda self: self._num_timesteps)
    interrupt = property(lambda self: self._interrupt)

    # -------------------------------------------------------------- placement (fast_infer.py:347-362)
    def to(self, *args, device=None, **kwargs):
        """The models are packed on their HIP device by ``load_state_dict``; ``pipeline.to(device)`` only checks that
        the request matches (no parameters to move), so the reference's ``model_full_load`` branch works unchanged."""
        want = device if device is not None else next((a for a in args if isinstance(a, (str, torch.device))), None)
        if want is not None:
            want = torch.device(want)
            have = self.transformer.device
            if want.type != "cuda" or (want.index is not None and have is not None and have.index is not None
                                       and want.index != have.index):
                raise RuntimeError(f"WanPipeline.to({want}): the transformer was loaded on {have}; load it there instead")
        return self

    def enable_model_cpu_offload(self, *args, **kwargs):
        """No-op: 14B bf16 weights (28 GB) + umT5 (11 GB) + VAE stay resident in the 288 GB of HBM; there is nothing to
        offload (the reference's default ``sequential_cpu_offload`` exists for 24-80 GB cards)."""
        return None

    enable_sequential_cpu_offload = enable_model_cpu_offload

    # -------------------------------------------------------------- prompt handling (:140-256, :449-495) -- the reference's argument lists
    _callback_tensor_inputs = ["latents", "prompt_embeds", "negative_prompt_embeds"]              # :112-116

    def _get_t5_prompt_embeds(self, prompt=None, num_videos_per_prompt: int = 1, max_sequence_length: int = 512, device=None, dtype=None):
        """tokenizer(padding="max_length", max_length=512, truncation) -> text_encoder(ids, mask)[0], each
        sample trimmed to its own token count (pipeline_wan.py:140-181); ``num_videos_per_prompt`` repeats every sample in place."""
        device = device if device is not None else self.transformer.device
        prompt = [prompt] if isinstance(prompt, str) else list(prompt)
        enc = self.tokenizer(prompt, padding="max_length", max_length=max_sequence_length, truncation=True,
                             add_special_tokens=True, return_tensors="pt")
        ids = enc.input_ids if hasattr(enc, "input_ids") else enc["input_ids"]
        mask = enc.attention_mask if hasattr(enc, "attention_mask") else enc["attention_mask"]
        seq_lens = mask.gt(0).sum(dim=1).long().tolist()
        hidden = self.text_encoder(ids.to(device), attention_mask=mask.to(device))[0]
        if dtype is not None:
            hidden = hidden.to(dtype)
        out = [u[:v] for u, v in zip(hidden, seq_lens)]
        # (:176-179 repeats along the sequence axis and views as [B * n, seq, C]: sample b's n copies are consecutive)
        return [e for e in out for _ in range(int(num_videos_per_prompt))]

    def encode_prompt(self, prompt, negative_prompt=None, do_classifier_free_guidance: bool = True, num_videos_per_prompt: int = 1,
                      prompt_embeds=None, negative_prompt_embeds=None, max_sequence_length: int = 512, device=None, dtype=None):
        """:183-256.  Embeddings are LISTS of [len_i, 4096] tensors (what the transformer's ``context`` takes); a [len, 4096] or
        [B, len, 4096] tensor passed in is split into one.  Without a tokenizer the text encoder is called on the strings themselves."""
        device = device if device is not None else self.transformer.device

        def as_list(e):
            if torch.is_tensor(e):
                return [e] if e.dim() == 2 else list(e)
            return list(e)

        def enc(p):
            if self.text_encoder is None:
                raise ValueError("no text_encoder: provide `prompt_embeds`, or build the pipeline with a tokenizer "
                                 "and a WanT5EncoderModel")
            if self.tokenizer is not None:
                return self._get_t5_prompt_embeds(p, num_videos_per_prompt, max_sequence_length, device, dtype)
            return [e.to(device) for e in self.text_encoder(p) for _ in range(int(num_videos_per_prompt))]
        prompt = [prompt] if isinstance(prompt, str) else prompt
        if prompt_embeds is None:
            prompt_embeds = enc(prompt)
        prompt_embeds = as_list(prompt_embeds)
        batch_size = len(prompt) if prompt is not None else len(prompt_embeds)
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            negative_prompt = negative_prompt or ""
            negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
            if prompt is not None and type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                                f" {type(prompt)}.")
            if batch_size != len(negative_prompt):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`:"
                                 f" {prompt} has batch size {batch_size}. Please make sure that passed `negative_prompt` matches"
                                 " the batch size of `prompt`.")
            negative_prompt_embeds = enc(negative_prompt)
        if negative_prompt_embeds is not None:
            negative_prompt_embeds = as_list(negative_prompt_embeds)
            if do_classifier_free_guidance and len(negative_prompt_embeds) != len(prompt_embeds):
                raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same batch size")
        return prompt_embeds, negative_prompt_embeds

    def check_inputs(self, prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs, prompt_embeds=None,
                     negative_prompt_embeds=None):
        if height % 8 != 0 or width % 8 != 0:                                                   # :458-459
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_on_step_end_tensor_inputs is not None and not all(k in self._callback_tensor_inputs
                                                                       for k in callback_on_step_end_tensor_inputs):
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found "
                             f"{[k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError("Cannot forward both `prompt` and `prompt_embeds`.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        if prompt is not None and not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if prompt is not None and negative_prompt_embeds is not None:                           # :481-485
            raise ValueError("Cannot forward both `prompt` and `negative_prompt_embeds`.")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError("Cannot forward both `negative_prompt` and `negative_prompt_embeds`.")
        if torch.is_tensor(prompt_embeds) and torch.is_tensor(negative_prompt_embeds) and \
                prompt_embeds.shape != negative_prompt_embeds.shape:                            # :492-498
            raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                             f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds` {negative_prompt_embeds.shape}.")

    # -------------------------------------------------------------- latents (:258-419), with the reference's names and argument lists
    @staticmethod
    def _randn(shape, generator, device, dtype):
        """diffusers' randn_tensor for one generator: drawn on the generator's device, then moved."""
        return torch.randn(tuple(shape), generator=generator, device=generator.device if generator is not None else device,
                           dtype=dtype).to(device)

    def _encode_modes(self, video, device, dtype):
        if self.vae is None:
            raise ValueError("no VAE: provide `source_latents` (or full `latents`)")
        if isinstance(video, np.ndarray):
            video = torch.from_numpy(video)
        if video.dtype == torch.uint8:
            # frames as a video reader yields them, [B, T, H, W, 3] or [T, H, W, 3]: one byte per sample over the host link, then
            # wan_frames_u8_to_video = the reference loader's `x * (2.0 / 255.0) - 1.0` (fast_infer.py:88-90) and the cast to `dtype`
            from . import ops
            video = ops.frames_u8_to_video((video if video.dim() == 5 else video.unsqueeze(0)).to(device), dtype)
        else:
            video = video.to(device=device, dtype=dtype)
        return torch.cat([self.vae.encode(video[i:i + 1])[0].mode() for i in range(video.shape[0])])      # mode, no mean / std (:404-409)

    def prepare_latents(self, batch_size, num_channels_latents, num_frames, height, width, dtype, device, generator, latents=None):
        """:258-290 -- plain T2V noise [B, C, (num_frames - 1) / 4 + 1, H / 8, W / 8] (x ``scheduler.init_noise_sigma`` if it has one)."""
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        tr, sr = getattr(self.vae, "temporal_compression_ratio", 4), getattr(self.vae, "spatial_compression_ratio", 8)
        shape = (batch_size, num_channels_latents, (num_frames - 1) // tr + 1, height // sr, width // sr)
        latents = self._randn(shape, generator, device, dtype) if latents is None else latents.to(device)
        if hasattr(self.scheduler, "init_noise_sigma"):
            latents = latents * self.scheduler.init_noise_sigma
        return latents

    def prepare_video_latents(self, video, batch_size=1, num_channels_latents=16, height=480, width=832, dtype=torch.float32,
                              device=None, generator=None, condition_count=None, latents=None, timestep=None):
        """:292-341 -- the clip's latents with every frame from ``condition_count`` on replaced by noise."""
        if latents is not None:
            return latents.to(device=device, dtype=dtype)
        init = self._encode_modes(video, device, dtype)
        tr, sr = getattr(self.vae, "temporal_compression_ratio", 4), getattr(self.vae, "spatial_compression_ratio", 8)
        shape = (batch_size, num_channels_latents, (video.shape[2] - 1) // tr + 1, height // sr, width // sr)
        noise = self._randn(shape, generator, device, dtype)
        init[:, :, condition_count:] = noise[:, :, condition_count:]
        return init

    def prepare_video_latents_new(self, video, batch_size=1, num_channels_latents=16, height=480, width=832, dtype=torch.float32,
                                  device=None, generator=None, condition_count=None, latents=None, timestep=None, source_latents=None):
        """:343-378 -- [source latents | noise of the same shape] (the repeat / org layouts)."""
        return self.prepare_cot_video_latents(video, 0, batch_size, num_channels_latents, height, width, dtype, device, generator,
                                              condition_count, latents, timestep, source_latents)

    def prepare_cot_video_latents(self, video, reasoning_latent_count=1, batch_size=1, num_channels_latents=16, height=480, width=832,
                                  dtype=torch.float32, device=None, generator=None, condition_count=None, latents=None, timestep=None,
                                  source_latents=None):
        """:381-419 -- [source latents | noise over reasoning_latent_count + Fs frames].  The reference's argument list (its unused
        entries -- batch_size, num_channels_latents, height, width, condition_count, timestep -- are accepted and unused here too) plus
        ``source_latents``: the clip already encoded (no VAE in the pipeline, or the encode done elsewhere)."""
        if latents is not None:
            return latents.to(device=device, dtype=dtype)
        if source_latents is None:
            source_latents = self._encode_modes(video, device, dtype)
        org = source_latents.to(device=device, dtype=dtype)
        B, Cl, Fs, h, w = org.shape
        return torch.cat([org, self._randn((B, Cl, Fs + reasoning_latent_count, h, w), generator, device, dtype)], dim=2)

    def prepare_extra_step_kwargs(self, generator, eta):
        """:431-446 -- ``eta`` / ``generator`` only for schedulers whose ``step`` takes them (FlowUniPC takes ``generator``)."""
        import inspect
        names = set(inspect.signature(self.scheduler.step).parameters.keys())
        kw = {}
        if "eta" in names:
            kw["eta"] = eta
        if "generator" in names:
            kw["generator"] = generator
        return kw

    @property
    def attention_kwargs(self):
        return getattr(self, "_attention_kwargs", None)

    def _decode_frames_u8(self, latents, out, clip=None, dst_frame=0, keep=None, stitch=None, match=None) -> np.ndarray:
        """decode, then wan_video_to_frames_u8 into frames [dst_frame, dst_frame + T) of the device clip `clip` (uint8
        [B, T_clip, H, W, 3]; None = one of exactly T frames), then ONE asynchronous copy per sample of that frame range -- one
        contiguous run of bytes -- into `out`, a page-locked uint8 [B, T, H, W, 3] host tensor (or a frame slice of one).
        `keep`: a list that receives the device frames of the segment (the compare clip is composed from them).
        `match` (`color_match`): (the uint8 source frames, the edit mask or None, (pool_t, gain, min_pixels), a list) -- the segment's
        frames are matched to the source's colours in place on the device (video_io.color_match's kernels) before they are kept or
        copied, and the list receives the coefficient table.
        `stitch` (`edit_region_vae_halo`): (the device source frames, the box, the region's rectangle, the feather) -- the latents are
        the box's, and wan_video_box_stitch_u8 writes the whole frames instead: the source's bytes from frame 0 on, the decoder's inside
        the rectangle."""
        from . import ops
        frames = self.vae.decode(latents.to(self.vae.dtype)).sample
        if stitch is None:
            clip = ops.video_to_frames_u8(frames, out=clip, dst_frame=dst_frame)
        else:
            clip = ops.video_box_stitch_u8(frames, stitch[0], stitch[1], stitch[2], stitch[3], out=clip, dst_frame=dst_frame)
        seg = clip[:, dst_frame:dst_frame + frames.shape[2]]
        if match is not None:
            from . import video_io
            match[3].append(video_io._color_match_segment(seg, *match[:3]))
        if keep is not None:
            keep.append(seg)
        if out is None:
            out = torch.empty(seg.shape, dtype=torch.uint8, pin_memory=True)
        if tuple(out.shape) != tuple(seg.shape) or out.dtype != torch.uint8:
            raise ValueError(f"decode_latents: out {out.dtype} {tuple(out.shape)} for uint8 frames {tuple(seg.shape)}")
        for b in range(seg.shape[0]):
            out[b].copy_(seg[b], non_blocking=True)
        torch.cuda.current_stream(frames.device).synchronize()
        return out.numpy()

    def decode_latents(self, latents: torch.Tensor, out: Optional[torch.Tensor] = None, **switches) -> np.ndarray:
        """:423-428 -- decode, (x / 2 + 0.5).clamp(0, 1), float32 numpy.  The reference converts on the host
        (``frames.cpu().float().numpy()``: a pageable copy, a CPU cast and, in ``__call__``, a concatenate: ~0.1 s for 81 frames at
        480 x 832); here the cast runs on the device and the frames go ONCE, through page-locked memory, to where they stay:
        ``out`` = a pinned float32 host tensor [B, 3, T, H, W] (or a frame slice of one) that the result is a view of.
        ``as_uint8``: the frames a video writer takes instead, uint8 [B, T, H, W, 3] -- the bytes the reference's writer makes of
        the float frames (``(x * 255).numpy().astype(np.uint8)`` after ``b c t h w -> t h w c``, videox_fun/utils/utils.py:59-68),
        converted and transposed by wan_video_to_frames_u8 on the device; ``out`` is then a pinned uint8 host tensor of that shape.
        (``as_uint8=False`` is the one keyword in ``switches``: the named parameters stay the reference's plus ``out``, which
        tests/test_oracle_vs_reference.py pins.)"""
        as_uint8 = bool(switches.pop("as_uint8", False))
        if switches:
            raise TypeError(f"decode_latents() got an unexpected keyword argument {next(iter(switches))!r}")
        if as_uint8:
            return self._decode_frames_u8(latents, out)
        frames = self.vae.decode(latents.to(self.vae.dtype)).sample
        frames = (frames / 2 + 0.5).clamp(0, 1).float()        # the arithmetic in the VAE's dtype, as the reference does it; the cast on the device
        if not frames.is_cuda:
            return frames.numpy()
        if out is None:
            out = torch.empty(frames.shape, dtype=torch.float32, pin_memory=True)
        if tuple(out.shape) != tuple(frames.shape):
            raise ValueError(f"decode_latents: out {tuple(out.shape)} for frames {tuple(frames.shape)}")
        for b in range(frames.shape[0]):
            for c in range(frames.shape[1]):
                out[b, c].copy_(frames[b, c], non_blocking=True)       # (a frame slice of a longer clip is contiguous per channel)
        torch.cuda.current_stream(frames.device).synchronize()
        return out.numpy()

    # -------------------------------------------------------------- __call__ (:516-799): its stages, in the order it runs them
    def _parse_switches(self, switches, video, has_source, source_frames, height, width, output_type, capture_graph, has_latents=False):
        """The keywords of ``__call__`` that travel in `switches` (as `as_uint8` is decode_latents': the named parameters stay the
        reference's plus the extensions tests/test_oracle_vs_reference.py lists), and every check of them that needs no device."""
        o = SimpleNamespace(
            # `color_match=False`: True, or a dict of `pool_t`, `gain`, `min_pixels` (video_io.color_match's, with its defaults, which are
            # guesses): the edit segment's uint8 frames are brought back to the colours of the uint8 source frames on the device -- one
            # gain and offset per frame and RGB channel, estimated where `edit_mask` is 0 (everywhere without a mask), applied to the
            # whole frame -- before they are copied to the host and before the compare clip is composed; the table is returned in
            # `color_match` (device int32; with `video` and `edit_mask` on the device no synchronisation is added, from the host they are
            # uploaded once more first).  Needs uint8 frames as `video` and output_type="uint8".  Not with
            # `edit_region_vae_halo`.  Opt-in; no quality claim.
            color_match=switches.pop("color_match", False),
            color_args=None, color_source=None,          # set below: (pool_t, gain, min_pixels) checked (None: off); the uint8 source frames
            mask_args=None, compare_source=None,         # set below: (grow, grow_t, feather) checked; the uint8 source frames of compare=True
            # compare=True: also return the reference's compare clip (save_side_by_side, fast_infer.py:183-206, as its writer's bytes) in
            # `compare_videos`, composed on the device from the uint8 source frames and the edit segment (video_io.compare_frames)
            compare=bool(switches.pop("compare", False)),
            # `temporal_window=None, temporal_overlap=16, window_batch=None` (PIXEL frames; window_batch in windows): denoise a clip longer
            # than `temporal_window` as overlapping windows of that length, blended every step -- see `_windowed_form` below
            temporal_window=switches.pop("temporal_window", None), temporal_overlap=switches.pop("temporal_overlap", 16), window_batch=switches.pop("window_batch", None),
            # `spatial_window=None, spatial_overlap=(96, 128)` ((rows, columns) in PIXELS): denoise frames larger than `spatial_window` as
            # overlapping tiles of that size, blended every step; combines with `temporal_window`, `window_batch` then
            # counts tiles.  The default overlap is a guess: no real checkpoint has been run with it.  Opt-in and lossy; no quality claim.
            spatial_window=switches.pop("spatial_window", None), spatial_overlap=switches.pop("spatial_overlap", (96, 128)),
            # `local_attention=None, local_attention_from_step=0`: self-attention over a neighbourhood instead of every token (DESIGN.md
            # 13.3; WanTransformer3DModel.enable_local_attention).  A (window_frames, window_rows) pair or a dict of that method's
            # arguments; steps before `local_attention_from_step` run dense.  Opt-in and lossy; no quality claim.  The model's own
            # setting is restored when the call returns.
            local_attention=switches.pop("local_attention", None), local_from=switches.pop("local_attention_from_step", 0),
            # `edit_mask=None, edit_mask_grow=(1, 0), edit_mask_feather=1`: where the edit may happen.  uint8 [T, H, W] or
            # [B, T, H, W] with T = source_frames and H x W = height x width, host or device; 255 = edit freely, 0 = keep the source.  Every
            # step the target's prediction outside the mask is replaced by the one whose x0 is the source (wan_masked_prediction), so that
            # region ends on the source latents to rounding.  `edit_mask_grow` = (latent cells, latent frames) of margin, `edit_mask_feather`
            # = latent cells of soft edge (video_io.latent_edit_mask); the defaults are guesses.  Opt-in, changes outputs by design; no
            # quality claim.
            edit_mask=switches.pop("edit_mask", None), edit_mask_grow=switches.pop("edit_mask_grow", (1, 0)), edit_mask_feather=switches.pop("edit_mask_feather", 1),
            # `edit_region=False, edit_region_margin=(64, 64)` ((rows, columns) in PIXELS, multiples of 16): run the loop only on a rectangle
            # around the mask's non-zero latent weights (edit_region.region_plan): the loop state and the weights are
            # cropped once, the ordinary loop runs on the smaller clip -- one `spatial_window` tile where the margined box fits one, tiles
            # inside the region where it does not -- and the region is put back into the source latents once.  Needs `edit_mask`.  The
            # model sees the region only and positions start at its corner; `callback_on_step_end` sees the region-sized state, and the SDE
            # sampler's per-step noise is drawn region-shaped.  The default margin is a guess.  Opt-in and lossy; no quality claim.
            edit_region=bool(switches.pop("edit_region", False)), edit_region_margin=switches.pop("edit_region_margin", (64, 64)),
            region_margin=None,                          # set below: the margin in latent cells, checked
            # `edit_region_time_margin=None` (PIXEL frames, a multiple of 4): with `edit_region=True`, crop the time axis too -- the loop
            # runs on ONE contiguous range of latent frames around the frames the mask touches, with this much context on either side
            # (edit_region.region_time_plan), as the whole-clip form where the range fits one `temporal_window`, as windows inside the
            # range where it does not.  Positions start at the range's first frame; the source is still encoded whole and the decode is
            # whole-clip.  None: the time axis is not cropped.  There is no default margin: any value is a guess.  Opt-in and lossy, the
            # class of approximation of temporal context windows; no quality claim.
            edit_region_time_margin=switches.pop("edit_region_time_margin", None),
            region_time_margin=None,                     # set below: the margin in latent frames, checked (None: no time crop)
            # `edit_region_vae_halo=None, edit_region_stitch_feather=0` (PIXELS; the halo a multiple of 16): with `edit_region=True`, the
            # VAE encodes and decodes only the BOX -- the region's rectangle widened by the halo on every side, clamped to the frame
            # (edit_region.region_vae_box) -- and the returned frames are the source's own bytes outside the region's rectangle
            # (wan_frames_u8_box_to_video before the encoder, wan_video_box_stitch_u8 after the decoder).  Needs uint8 frames as `video`
            # and output_type="uint8"; `latents` in the output are then the box's.  The time axis is never cropped in the VAE.  The
            # feather is the width of a linear ramp on the inside of the rectangle's edges that are not the frame's border; 0 is the
            # literal stitch.  None: the VAE runs on whole frames.  The halo has no default: the VAE's receptive field is many 3 x 3
            # convolutions deep and its mid-block attention is global over the frame it sees, so no finite halo is exact and every
            # value is a guess.  Opt-in and lossy (a VAE that sees a crop is as lossy as a DiT that sees one); no quality claim.
            edit_region_vae_halo=switches.pop("edit_region_vae_halo", None), edit_region_stitch_feather=switches.pop("edit_region_stitch_feather", 0),
            vae_halo=None, stitch_feather=0,             # set below: the halo in latent cells (None: the VAE sees whole frames) and the feather, checked
            # `edit_region_follow=None` (PIXEL frames, a multiple of 4): with `edit_region=True`, the rectangle keeps ONE size and takes a
            # corner per latent frame, so a moving object's box stays the object's size, not its path's (edit_region.region_track_plan).
            # The value is the only smoothing: frame f's box covers the mask of the frames within this many pixel frames of it; 0 follows
            # every frame on its own, a value of the clip's length or more is `edit_region=True` alone.  Source frame f, target frame f
            # and the weights of frame f are cropped at the same corner (wan_region_crop_track / wan_region_restore_track), so the pin
            # to the source stays exact; the model sees a stabilised crop whose background slides.  Not with `edit_region_vae_halo`.
            # None: one rectangle for the clip.  There is no default: any value is a guess.  Opt-in and lossy; no quality claim.
            edit_region_follow=switches.pop("edit_region_follow", None),
            region_follow=None,                          # set below: the span in latent frames, checked (None: the box does not move)
            # `edit_region_split=None` (an int from 2 to 8): with `edit_region=True`, a mask of SEPARATE objects is split into at most this
            # many bands along ONE axis, columns or rows, every band gets a box of ONE common size (edit_region.region_split_plan, from the
            # spans wan_mask_spans brings to the host instead of the bounds), and the K' boxes run as K' x B samples of the ordinary loop
            # (wan_region_crop_split), so two small objects in opposite corners cost two small boxes, not their union.  In box A the cells
            # of object B are pinned to the source; every box is put back over the part of the frame its band owns
            # (wan_region_restore_split).  A box sees only itself.  A mask of one object, or one whose split does not pay, is
            # `edit_region=True` alone, bit for bit.  Not with `edit_region_follow` or `edit_region_vae_halo`.  None: one rectangle.
            # There is no default: any value is a guess.  Opt-in and lossy; no quality claim.
            edit_region_split=switches.pop("edit_region_split", None),
            region_split=None)                           # set below: the most boxes, checked (None: one rectangle)
        if switches:
            raise TypeError(f"__call__() got an unexpected keyword argument {next(iter(switches))!r}")
        if o.color_match is not False and o.color_match is not None and o.edit_region_vae_halo is not None:
            raise ValueError("color_match with edit_region_vae_halo: the pixels to estimate from there are the ring of the decoded box "
                             "around the region's rectangle, which the stitch discards; the two do not combine")
        if o.edit_mask is not None:
            from . import video_io
            _require_source(has_source, "edit_mask: outside the mask the clip is kept on its source")
            if not isinstance(o.edit_mask_grow, (tuple, list)) or len(o.edit_mask_grow) != 2:
                raise ValueError(f"edit_mask_grow={o.edit_mask_grow!r}: a (latent cells, latent frames) pair")
            o.mask_args = video_io._latent_mask_args("edit_mask", o.edit_mask_grow[0], o.edit_mask_grow[1], o.edit_mask_feather)
            want = f"uint8 [{source_frames}, {height}, {width}] or [B, {source_frames}, {height}, {width}]"
            try:
                o.edit_mask = video_io._as_mask(o.edit_mask, "edit_mask")
            except ValueError as e:
                raise ValueError(f"{e}; expected {want}") from None
            if tuple(o.edit_mask.shape[-3:]) != (source_frames, height, width):
                raise ValueError(f"edit_mask: expected {want} (source_frames, height, width of this call), got {tuple(o.edit_mask.shape)}")
            if capture_graph == "loop":
                raise NotImplementedError("edit_mask with capture_graph='loop': the recorded loop does not hold the mask's weights or "
                                          "the per-step sigma of the replacement (use capture_graph='step')")
        if o.edit_region:
            from .edit_region import region_margin_cells
            if o.edit_mask is None:
                raise ValueError("edit_region=True: the region is where `edit_mask` is, and this call has no edit_mask")
            o.region_margin = region_margin_cells(o.edit_region_margin)
        if o.edit_region_time_margin is not None:
            from .edit_region import region_time_margin_frames
            o.region_time_margin = region_time_margin_frames(o.edit_region_time_margin)
            if not o.edit_region:
                raise ValueError("edit_region_time_margin extends edit_region=True (the frame range is cropped with the rectangle), and "
                                 "this call does not set it")
        if o.edit_region_follow is not None:
            from .edit_region import region_follow_frames
            o.region_follow = region_follow_frames(o.edit_region_follow)
            if not o.edit_region:
                raise ValueError("edit_region_follow extends edit_region=True (the rectangle takes a corner per latent frame), and this "
                                 "call does not set it")
            if o.edit_region_vae_halo is not None:
                raise ValueError("edit_region_follow with edit_region_vae_halo: a pixel box that moves from frame to frame inside a "
                                 "causal VAE (whose every frame leans on the features of the frames before it, at the same pixels) is "
                                 "a different problem; the VAE box is one rectangle for the clip")
        if o.edit_region_split is not None:
            from .edit_region import region_split_count
            o.region_split = region_split_count(o.edit_region_split)
            if not o.edit_region:
                raise ValueError("edit_region_split extends edit_region=True (the rectangle becomes one box per object), and this call "
                                 "does not set it")
            if o.edit_region_follow is not None:
                raise ValueError("edit_region_split with edit_region_follow: the bands are cut from the union of the mask over all "
                                 "frames and a band's box has one corner for the clip; boxes that move would need a cut per frame")
            if o.edit_region_vae_halo is not None:
                raise ValueError("edit_region_split with edit_region_vae_halo: the VAE box is ONE rectangle around the region, and "
                                 "around boxes in opposite corners that is the whole frame again")
        from .edit_region import region_stitch_feather
        o.stitch_feather = region_stitch_feather(o.edit_region_stitch_feather)
        if o.edit_region_vae_halo is not None:
            from .edit_region import region_vae_halo_cells
            o.vae_halo = region_vae_halo_cells(o.edit_region_vae_halo)
            if not o.edit_region:
                raise ValueError("edit_region_vae_halo extends edit_region=True (the box is the region's rectangle and a halo), and this "
                                 "call does not set it")
            if output_type != "uint8":
                raise ValueError(f"edit_region_vae_halo returns the source's own bytes outside the region: it needs output_type='uint8', "
                                 f"not {output_type!r}")
            src = torch.from_numpy(video) if isinstance(video, np.ndarray) else video
            if has_latents or not torch.is_tensor(src) or src.dtype != torch.uint8 or src.dim() not in (4, 5) or src.shape[-1] != 3:
                raise ValueError("edit_region_vae_halo crops the source's pixels and stitches the result into them: it needs the uint8 "
                                 "source frames as `video` ([T, H, W, 3] or [B, T, H, W, 3]) and neither `latents` nor `source_latents`"
                                 + (", and this call gives latents" if has_latents else
                                    f", got {getattr(src, 'dtype', type(src))} {tuple(getattr(src, 'shape', ()))}"))
            if tuple(src.shape[-4:-1]) != (source_frames, height, width):
                raise ValueError(f"edit_region_vae_halo: `video` {tuple(src.shape)} is not [{source_frames}, {height}, {width}, 3] or [B, "
                                 f"{source_frames}, {height}, {width}, 3] (source_frames, height, width of this call)")
            if self.vae is None:
                raise ValueError("edit_region_vae_halo: the box is encoded and decoded by the VAE, and this pipeline has none")
        elif o.stitch_feather:
            raise ValueError(f"edit_region_stitch_feather={o.stitch_feather} softens the stitch of edit_region_vae_halo, and this call "
                             "does not set it")
        if o.compare:
            if output_type != "uint8":
                raise ValueError(f"compare=True composes the compare clip from uint8 frames on the device: it needs "
                                 f"output_type='uint8', not {output_type!r}")
            src = o.compare_source = torch.from_numpy(video) if isinstance(video, np.ndarray) else video
            if not torch.is_tensor(src) or src.dtype != torch.uint8 or src.dim() not in (4, 5) or src.shape[-1] != 3:
                raise ValueError("compare=True needs the uint8 source frames as `video` ([T, H, W, 3] or [B, T, H, W, 3]), got "
                                 f"{getattr(src, 'dtype', type(src))} {tuple(getattr(src, 'shape', ()))}")
        if o.color_match is not False and o.color_match is not None:
            from . import video_io
            if o.color_match is not True and not isinstance(o.color_match, dict):
                raise ValueError(f"color_match={o.color_match!r}: True, or a dict of pool_t, gain, min_pixels")
            args = {} if o.color_match is True else dict(o.color_match)
            o.color_args = video_io._color_args("color_match", args.pop("pool_t", 2), args.pop("gain", True), args.pop("min_pixels", 1024))
            if args:
                raise ValueError(f"color_match: unknown key {next(iter(args))!r} (pool_t, gain, min_pixels)")
            if output_type != "uint8":
                raise ValueError(f"color_match matches uint8 frames on the device: it needs output_type='uint8', not {output_type!r}")
            src = o.color_source = torch.from_numpy(video) if isinstance(video, np.ndarray) else video
            if not torch.is_tensor(src) or src.dtype != torch.uint8 or src.dim() not in (4, 5) or src.shape[-1] != 3:
                raise ValueError("color_match needs the uint8 source frames as `video` ([T, H, W, 3] or [B, T, H, W, 3]), got "
                                 f"{getattr(src, 'dtype', type(src))} {tuple(getattr(src, 'shape', ()))}")
            if tuple(src.shape[-4:-1]) != (source_frames, height, width):
                raise ValueError(f"color_match: `video` {tuple(src.shape)} is not [{source_frames}, {height}, {width}, 3] or [B, "
                                 f"{source_frames}, {height}, {width}, 3] (source_frames, height, width of this call)")
        return o

    def _set_timesteps(self, num_inference_steps, shift, device):
        if isinstance(self.scheduler, FlowUniPCMultistepScheduler):
            self.scheduler.set_timesteps(num_inference_steps, device=device, shift=shift)       # :613-615
            return self.scheduler.timesteps
        if isinstance(self.scheduler, FlowDPMSolverMultistepScheduler):
            return retrieve_timesteps(self.scheduler, device=device, sigmas=get_sampling_sigmas(num_inference_steps, shift))[0]   # :616-621
        raise NotImplementedError(f"{type(self.scheduler).__name__}: the schedulers built are FlowUniPCMultistepScheduler and "
                                  "FlowDPMSolverMultistepScheduler (fast_infer.py:328-337)")

    def _window_sizes(self, o, ratio, has_source):
        """The window options in latent cells: (temporal (n, overlap) or None, spatial ((th, tw), (oy, ox)) or None), checked."""
        window_latents = tile_cells = None
        if o.temporal_window is not None:
            from .windows import window_latent_frames
            window_latents = window_latent_frames(o.temporal_window, o.temporal_overlap, ratio)
        if o.spatial_window is not None:
            from .windows import spatial_window_cells
            tile_cells = spatial_window_cells(o.spatial_window, o.spatial_overlap, getattr(getattr(self.vae, "config", None),
                                              "spatial_compression_ratio", 8), self.transformer.config.patch_size[1])
        wb = o.window_batch
        for name, option in (("temporal_window", o.temporal_window), ("spatial_window", o.spatial_window)):
            if option is None:
                continue
            if wb is not None and (isinstance(wb, bool) or not isinstance(wb, int) or wb < 1):
                raise ValueError(f"window_batch={wb!r}: None (all windows in one forward) or a window count >= 1")
            _require_source(has_source, f"{name}={option}: the windows are cut from a source clip")
        return window_latents, tile_cells

    def _mask_weights(self, o, shape, device, cc, G, source_frames, height, width):
        """Edit inside a mask: the latent-cell weights uint8 [1 or B, Fs, hl, wl], made once (None without a mask).  `shape`: the
        latents' [B, C, F, hl, wl] -- or, before the encode (`edit_region_vae_halo`), what the call's sizes say it will be."""
        if o.mask_args is None:
            return None
        from . import video_io
        B, _, Ftot, hl, wl = shape
        lead = 1 if o.edit_mask.dim() == 3 else int(o.edit_mask.shape[0])
        cells = (height // video_io.LATENT_CELL, width // video_io.LATENT_CELL)
        if not _has_layout(Ftot, cc, G) or (hl, wl) != cells or lead not in (1, B):
            raise ValueError(f"edit_mask: a mask {tuple(o.edit_mask.shape)} for latents of {B} samples, {Ftot} frames of {hl} x {wl} "
                             f"cells; expected {_LAYOUT.format(cc, G)} frames of {cells[0]} x {cells[1]} cells and a mask for 1 or {B} samples")
        weights = video_io.latent_edit_mask((o.edit_mask if o.edit_mask.dim() == 4 else o.edit_mask.unsqueeze(0)).to(device),
                                            grow=o.mask_args[0], grow_t=o.mask_args[1], feather=o.mask_args[2])
        if weights.shape[1] != cc:
            raise ValueError(f"edit_mask: {source_frames} mask frames are {weights.shape[1]} latent frames; the source segment has {cc}")
        return weights

    def _plan_region(self, o, weights, hl, wl, tile_cells, cc, G):
        """The bounds of the non-zero weights (wan_mask_bounds), their copy to the host -- the ONE synchronisation of edit_region -- and
        the rules on it: (RegionPlan -- or, with `edit_region_follow`, the TrackPlan from the same host copy --, TimeRegion or None
        without `edit_region_time_margin`).  With `edit_region_split` the spans (wan_mask_spans) come to the host in place of the
        bounds, still ONE synchronisation, and the plan is a SplitPlan where splitting the mask pays, the RegionPlan where not."""
        from . import ops
        from .edit_region import region_plan, region_time_plan, region_track_plan
        if G > cc:
            raise ValueError(f"edit_region: {G} grounding frames for {cc} source frames; outside the region grounding frame g is "
                             "source frame g, so at most as many")
        rule = (hl, wl), o.region_margin, None if tile_cells is None else tile_cells[0], int(self.transformer.config.patch_size[1])
        if o.region_split is not None:
            # `edit_region_split`: the spans come to the host in place of the bounds (a frame's bounds are the min and max of its spans)
            from .edit_region import region_split_plan, spans_bounds
            spans = ops.mask_spans(weights).cpu()
            bounds = spans_bounds(spans, (hl, wl))
            plan = region_split_plan(spans, *rule, max_regions=o.region_split)
            return plan, None if o.region_time_margin is None else region_time_plan(bounds, cc, o.region_time_margin, G)
        bounds = ops.mask_bounds(weights).cpu()
        plan = region_plan(bounds, *rule) if o.region_follow is None else region_track_plan(bounds, *rule, span=o.region_follow)
        return plan, None if o.region_time_margin is None else region_time_plan(bounds, cc, o.region_time_margin, G)

    def _crop_to_region(self, o, latents, weights, tile_cells, cc, G):
        """Edit region, the first of its two stages: the bounds of the non-zero weights (wan_mask_bounds; their 16 bytes
        per latent frame come to the host -- the ONE synchronisation the option adds to a call), the region (edit_region.region_plan,
        with the tile of `spatial_window` if that is given), and the loop state and the weights cropped to it (wan_region_crop).
        With `edit_region_time_margin` the frame range (edit_region.region_time_plan) comes from the same host copy of the bounds, and
        state and weights are cropped in frames and cells at once (wan_region_crop_frames, still one launch each).
        With `edit_region_follow` the plan is a TrackPlan and both are cropped by ONE table of corners (wan_region_crop_track): the
        weights by the source frames' table, the state by the same table laid out as [source | grounding | target].
        With `edit_region_split` and a SplitPlan both are cropped into K' boxes at once (wan_region_crop_split), box-major: the state
        becomes [K' B, ...] and the weights, clipped to what each band owns, [K' B, ...] too.
        Returns (latents, weights, region, the source frames of the loop's clip): `region` is None with the option off -- nothing is
        launched then -- or (RegionPlan, the whole source block to restore into; None where nothing was cropped, the TimeRegion; None
        without a time crop)."""
        if not o.edit_region:
            return latents, weights, None, cc
        from . import ops
        hl, wl = int(latents.shape[3]), int(latents.shape[4])
        plan, span = self._plan_region(o, weights, hl, wl, tile_cells, cc, G)
        if hasattr(plan, "cuts"):
            # `edit_region_split`, and the mask was split: K' boxes of one size, box-major [K' B, ...] (one launch each); the weights
            # are clipped to what each band owns and given one row per sample of the state
            t0, n = (0, cc) if span is None else span
            runs = [(0, 2 * cc + G)] if span is None else [(t0, n)] + ([(cc, G)] if G else []) + [(cc + G + t0, n)]
            boxes = plan.origins, plan.cuts, plan.axis, (plan.h, plan.w)
            state = ops.region_crop_split(latents.contiguous(), runs, *boxes).flatten(0, 1)
            cropped = ops.region_crop_split(weights, [(t0, n)], *boxes, clip=True)
            if cropped.shape[1] != latents.shape[0]:
                cropped = cropped.expand(-1, latents.shape[0], -1, -1, -1)
            return state, cropped.reshape((-1,) + tuple(cropped.shape[2:])), (plan, latents[:, :, :cc], span), n
        if o.region_follow is not None:
            t0, n = (0, cc) if span is None else span
            if (plan.h, plan.w, n) == (hl, wl, cc):
                return latents, weights, (plan, None, span), cc
            table = np.concatenate([plan.origins, plan.origins[:G], plan.origins])
            runs = [(0, 2 * cc + G)] if span is None else [(t0, n)] + ([(cc, G)] if G else []) + [(cc + G + t0, n)]
            return (ops.region_crop_track(latents.contiguous(), runs, table, (plan.h, plan.w)),
                    ops.region_crop_track(weights, [(t0, n)], plan.origins, (plan.h, plan.w)), (plan, latents[:, :, :cc], span), n)
        if span is not None:
            if (plan.h, plan.w, span.n) == (hl, wl, cc):
                return latents, weights, (plan, None, span), cc
            t0, n = span
            runs = [(t0, n)] + ([(cc, G)] if G else []) + [(cc + G + t0, n)]
            return (ops.region_crop_frames(latents.contiguous(), runs, plan), ops.region_crop_frames(weights, [(t0, n)], plan),
                    (plan, latents[:, :, :cc], span), n)
        if (plan.h, plan.w) == (hl, wl):
            return latents, weights, (plan, None, None), cc
        return ops.region_crop(latents.contiguous(), plan), ops.region_crop(weights, plan), (plan, latents[:, :, :cc], None), cc

    @staticmethod
    def _restore_region(latents, region, box=None):
        """Edit region, the second stage: the loop's final state on the region put back into the source latents (wan_region_restore, or
        wan_region_restore_frames after a time crop, wan_region_restore_track where the box follows the mask, wan_region_restore_split
        where the mask was split into boxes) -- outside the region the grounding and target frames are the source's bits.
        `box` (`edit_region_vae_halo`): the source latents are the VAE box's, and the region's corner counts from the box's."""
        plan, source, span = region
        if source is None:
            return latents
        from . import ops
        if hasattr(plan, "cuts"):                        # `edit_region_split`: a SplitPlan (never with a VAE box)
            return ops.region_restore_split(source.to(latents.dtype), latents, plan.origins, plan.cuts, plan.axis,
                                            (0, source.shape[2]) if span is None else span)
        if hasattr(plan, "origins"):                     # `edit_region_follow`: a TrackPlan (never with a VAE box)
            return ops.region_restore_track(source.to(latents.dtype), latents, plan.origins,
                                            (0, source.shape[2]) if span is None else span)
        origin = (plan.y0, plan.x0) if box is None else (plan.y0 - box.y0, plan.x0 - box.x0)
        if span is not None:
            return ops.region_restore_frames(source.to(latents.dtype), latents, origin, span)
        return ops.region_restore(source.to(latents.dtype), latents, origin)

    def _encode_box_to_region(self, o, video, generator, dtype, device, tile_cells, cc, G, source_frames, height, width):
        """Edit region with `edit_region_vae_halo`: what prepare_*_latents, _mask_weights and _crop_to_region do, with
        the VAE on the box only.  The weights, the bounds and the region come first -- they need the mask and the call's sizes only --
        then the box (edit_region.region_vae_box).  The uint8 frames go to the device once and stay there (the stitch reads them);
        wan_frames_u8_box_to_video and the encoder give source latents of the box's size.  The noise is drawn with the ONE call
        prepare_cot_video_latents makes, for the whole frame, and cropped to the region: the call's random stream and the noise inside
        the region are those of the call without the option.  The loop state is [the box's source latents cropped to the region |
        the cropped noise]; the frame range of `edit_region_time_margin` is cropped at the latent level as ever (the VAE box is
        spatial only).  Returns (latents, weights, region, the source frames of the loop's clip, the box in cells, (the device
        frames, the box, the region's rectangle, the feather) for the stitch); `region` as _crop_to_region returns it, its source
        block the box's."""
        from . import ops
        from .edit_region import RegionPlan, region_vae_box
        frames = torch.from_numpy(video) if isinstance(video, np.ndarray) else video
        frames = (frames if frames.dim() == 5 else frames.unsqueeze(0)).to(device).contiguous()
        B, scr = int(frames.shape[0]), getattr(getattr(self.vae, "config", None), "spatial_compression_ratio", 8)
        hl, wl = height // scr, width // scr
        weights = self._mask_weights(o, (B, None, 2 * cc + G, hl, wl), device, cc, G, source_frames, height, width)
        plan, span = self._plan_region(o, weights, hl, wl, tile_cells, cc, G)
        box = region_vae_box(plan, (hl, wl), (o.vae_halo, o.vae_halo))
        inner = RegionPlan(plan.y0 - box.y0, plan.x0 - box.x0, plan.h, plan.w)           # the region inside the box
        t_stage = self._stage("vae_encode")
        planes = ops.frames_u8_box_to_video(frames, box.pixels(scr), dtype)
        source = torch.cat([self.vae.encode(planes[i:i + 1])[0].mode() for i in range(B)])       # as _encode_modes
        if source.shape[2] != cc:
            raise ValueError(f"edit_region_vae_halo: {source_frames} source frames are {source.shape[2]} latent frames; the source segment has {cc}")
        noise = self._randn((B, source.shape[1], cc + G, hl, wl), generator, device, dtype)
        self._stage("vae_encode", t_stage)
        stitch = (frames, box.pixels(scr), plan.pixels(scr), o.stitch_feather)
        t0, n = (0, cc) if span is None else span
        if (plan.h, plan.w, n) == (hl, wl, cc):                                              # nothing to crop: the box is the frame too
            return torch.cat([source, noise], dim=2), weights, (plan, None, span), cc, box, stitch
        if span is None:
            state = torch.cat([ops.region_crop(source, inner), ops.region_crop(noise, plan)], dim=2)
            return state, ops.region_crop(weights, plan), (plan, source, None), cc, box, stitch
        state = torch.cat([ops.region_crop_frames(source, [(t0, n)], inner),
                           ops.region_crop_frames(noise, ([(0, G)] if G else []) + [(G + t0, n)], plan)], dim=2)
        return state, ops.region_crop_frames(weights, [(t0, n)], plan), (plan, source, span), n, box, stitch

    def _plan_windows(self, o, sizes, shape, cc, G, capture_graph):
        """(plan, tiles) of a clip of latent `shape`: the temporal WindowPlan, or None where the clip fits one window (or the option
        is off); the TilePlan of the spatial windows, or None where every frame fits one tile (or the option is off)."""
        (window_latents, tile_cells), (_, _, Ftot, hl, wl) = sizes, shape
        plan = tiles = None
        for name, size in (("temporal_window", window_latents), ("spatial_window", tile_cells)):
            if size is not None and not _has_layout(Ftot, cc, G):
                raise ValueError(f"{name}={getattr(o, name)}: latents of {Ftot} frames are not {_LAYOUT.format(cc, G)}")
        if window_latents is not None:
            from .windows import window_plan
            plan = window_plan(cc, *window_latents)
            plan = plan if plan.K > 1 else None
        if tile_cells is not None:
            from .windows import TilePlan, window_plan
            (tile_h, tile_w), (over_h, over_w) = tile_cells
            plan_y, plan_x = window_plan(hl, tile_h, over_h), window_plan(wl, tile_w, over_w)
            if plan_y.K * plan_x.K > 1:
                # the t axis: the temporal windows, or one window of the whole clip without them
                tiles = TilePlan(plan if plan is not None else window_plan(cc, max(cc, 2), 0), plan_y, plan_x)
        if plan is not None or tiles is not None:
            option = "spatial_window" if tiles is not None else "temporal_window"
            if capture_graph == "loop":
                raise NotImplementedError(f"{option} with capture_graph='loop': the windowed loop is not recorded as one graph "
                                          "(use capture_graph='step')")
            if getattr(self.transformer, "teacache", None) is not None:
                raise NotImplementedError(f"{option} with TeaCache: it keeps one residual per call and counts calls, and a "
                                          "windowed step is several windows (and possibly several calls)")
        return plan, tiles

    @contextmanager
    def _transformer_settings(self, cache_context, skip_frames, mask_frames, local_cfg):
        """What a call sets on the transformer for the loop and puts back however the loop ends: `cache_context` (the prompt is fixed across
        steps; the context cache is cleared on both sides), `skip_source_frames`, `mask_source_frames`, the local-attention setting (if the
        call switches it), opt-in the workspaces.  Yields whether the loop must zero a prediction's source frames itself (:736)."""
        tr = self.transformer
        prev_cache, prev_skip = getattr(tr, "cache_context", False), getattr(tr, "skip_source_frames", 0)
        prev_mask, prev_local = getattr(tr, "mask_source_frames", None), getattr(tr, "local_attention", None)
        try:
            if hasattr(tr, "cache_context"):
                tr.cache_context = cache_context
            if hasattr(tr, "clear_context_cache"):
                tr.clear_context_cache()            # never reuse another call's text K/V
            if hasattr(tr, "skip_source_frames"):
                tr.skip_source_frames = skip_frames   # noise_pred[:, :, :condition_count] is zeroed (:736): the last block need not produce it
            if prev_mask is not None:
                tr.mask_source_frames = mask_frames
            yield prev_mask is None
        finally:
            if hasattr(tr, "cache_context"):
                tr.cache_context = prev_cache
            if hasattr(tr, "clear_context_cache"):
                tr.clear_context_cache()            # releases the hoisted K/V^T and the prompt embeddings
            if hasattr(tr, "skip_source_frames"):
                tr.skip_source_frames = prev_skip
            if prev_mask is not None:
                tr.mask_source_frames = prev_mask
            if local_cfg is not None:
                if prev_local is None:
                    tr.disable_local_attention()
                else:
                    tr.enable_local_attention(**prev_local)
            if self.release_workspaces_after_denoise and hasattr(tr, "release_workspaces"):
                # opt-in: 7 GB of activation buffers at 14B / 67k tokens handed back before the VAE decode (for hosts that share the
                # device); the sets a captured graph replays from stay.  Off by default: every call would re-allocate and zero-fill the
                # set, and a capture_graph='loop' capture call would allocate (and record the zero-fill of) its workspaces inside the graph.
                tr.release_workspaces(keep_pinned=True)

    def _guided_forward(self, forward, do_cfg, seq_len, fsi, gfi):
        """A call's `guided(build, n, neg, pos, t, windows)`: the prediction for `n` samples at timestep `t`, guidance applied -- the ONE
        place that decides about cfg_skip, calls the model and combines the halves.  `build(rep)` makes the model input, `rep` copies of
        the samples one after the other; `neg` / `pos` are the samples' prompts; `windows`: they are windows of a clip, not a clip each.
        A step the model's cfg_skip rule halves (enable_cfg_skip; cfg_optimization.py:5-38) returns the conditional prediction twice, and
        guidance on two equal halves is that prediction itself: such a step calls the model with the conditional samples and prompts only.
        `_cfg_skip_literal` keeps the reference's literal order (doubled batch through the model's rule, then guidance) reachable; both
        give the same latents (tests/test_gpu_cfg_skip.py)."""
        cfg_skip_now = getattr(self.transformer, "cfg_skip_now", None)
        can_suspend = hasattr(self.transformer, "_cfg_skip_suspended")
        def guided(build, n, neg, pos, t, windows):
            half = do_cfg and cfg_skip_now is not None and cfg_skip_now(2 * n)
            doubled = do_cfg and not (half and not self._cfg_skip_literal)
            x = self.scheduler.scale_model_input(build(2 if doubled else 1), t)                     # :700
            nb = x.shape[0]
            # The model's own rule is suspended for a halved step's single batch (it already IS the conditional half) and left alone for
            # its literal doubled one.  On any other step it halves ANY batch of two or more: a batch of windows is none of its business,
            # a batch of whole clips stays its own (what an unguided B >= 2 call gets from a model with cfg_skip on is the model's affair).
            suspend = ((not doubled) if half else windows) and can_suspend
            if suspend:
                self.transformer._cfg_skip_suspended = True
            try:
                noise_pred = forward(x=x, context=(neg + pos) if doubled else pos, t=t.expand(nb), seq_len=seq_len,    # :705, :721-728
                                     frame_split_indices=fsi and [fsi] * nb, ground_frame_indices=gfi and [gfi] * nb)  # :713, :716-718
            finally:
                if suspend:
                    self.transformer._cfg_skip_suspended = False
            if doubled:
                nu, nt = noise_pred.chunk(2)
                noise_pred = nu + self.guidance_scale * (nt - nu)                                   # :731-733
            return noise_pred
        return guided

    def _whole_clip_form(self, guided, cc, G, zero_source, boxes=False):
        """The loop's `predict` for a clip that is one model input (:700-736): `cat([latents] * 2)` or the latents themselves, one
        forward, guidance, the CoF mask.  `boxes` (`edit_region_split`): the samples are boxes of a clip, not a clip each -- windows, as
        far as the model's cfg_skip rule goes.  Returns (predict, the target's first frame in the loop state, the state -> latents cut)."""
        def predict(latents, neg, pos, i, t):
            noise_pred = guided(lambda rep: torch.cat([latents] * 2) if rep == 2 else latents, latents.shape[0], neg, pos, t, boxes)
            if zero_source:
                noise_pred[:, :, :cc] = 0                                                       # :736
            # else: already zero -- written by wan_unpatchify(zero_frames); CFG keeps it (0 + s * (0 - 0))
            return noise_pred
        return predict, cc + G, lambda latents: latents

    def _windowed_form(self, guided, latents, plan, tiles, window_batch, cc, G):
        """The loop's `predict` for a clip longer than the window (DESIGN.md "Temporal context windows").  The loop state is
        [source | ground_0 .. ground_{K-1} | target]: every temporal window owns a grounding block (all start as the same noise: the
        random stream of the call is unchanged), the target is shared.  A step gathers the K windows
        [source[a:a+n] | ground_k | target[a:a+n]] out of it (wan_window_gather, which also writes the doubled batch of a guided
        step), runs them as ONE forward of K * B samples (`window_batch` windows per forward if set), applies guidance per forward and
        blends the K predictions into one for the state (wan_window_blend: CoF mask, each window's grounding, the weighted target);
        the loop then steps the sampler ONCE on the whole state, and its callback receives the state in this windowed layout.  With spatial
        context windows the windows are the K = Kt * Ky * Kx tiles of `tiles`, cut and blended by wan_tile_gather /
        wan_tile_blend; the state has one grounding block per TEMPORAL window, shared by its spatial tiles.
        Returns (the state made of `latents`, predict, the target's first frame in it, the cut back to [source | ground_0 | target])."""
        from . import ops
        if tiles is None:
            K, Kt = plan.K, plan.K
            alpha = torch.from_numpy(plan.alpha).to(latents.device)
            gather = lambda s, k0, k1, rep: ops.window_gather(s, plan.starts, plan.window, G, k0, k1, rep=rep)
            blend = lambda p: ops.window_blend(p, alpha, plan.starts, plan.frames, G)
        else:
            K, Kt = tiles.K, tiles.Kt
            starts = (tiles.t.starts, tiles.y.starts, tiles.x.starts)
            tables = tuple(torch.from_numpy(axis.alpha).to(latents.device) for axis in (tiles.t, tiles.y, tiles.x))
            gather = lambda s, k0, k1, rep: ops.tile_gather(s, starts, tiles.shape, G, k0, k1, rep=rep)
            blend = lambda p: ops.tile_blend(p, tables, starts, tiles.extent, G)
        per_call = K if window_batch is None else min(int(window_batch), K)
        def predict(state, neg, pos, i, t):
            state = state.contiguous()
            nB = state.shape[0]
            preds = None
            for k0 in range(0, K, per_call):
                k1 = min(k0 + per_call, K)
                nk = k1 - k0
                noise_pred = guided(lambda rep: gather(state, k0, k1, rep), nk * nB, neg * nk, pos * nk, t, True)
                if nk == K:
                    preds = noise_pred
                else:
                    if preds is None:
                        preds = torch.empty((K * nB,) + tuple(noise_pred.shape[1:]), device=noise_pred.device, dtype=noise_pred.dtype)
                    preds[k0 * nB:k1 * nB].copy_(noise_pred)
            return blend(preds.contiguous())
        state = torch.cat([latents[:, :, :cc]] + [latents[:, :, cc:cc + G]] * Kt + [latents[:, :, cc + G:]], dim=2)
        return state, predict, cc + Kt * G, lambda state: torch.cat([state[:, :, :cc + G], state[:, :, cc + Kt * G:]], dim=2)

    def _denoise(self, latents, embeds, do_cfg, timesteps, predict, local, mask, step_kwargs, callback):
        """THE step loop (:694-750), eager or recorded into a hipGraph: `predict(latents, neg, pos, i, t)` is one of the two forms above.
        `local` = (enable_local_attention arguments, first local step) or None; `mask` = (weights, source frames, the target's first
        frame) or None; `callback` = (callback_on_step_end, the names it wants, {name: prompt embeddings}) or None."""
        neg, pos = (embeds[:len(embeds) // 2], embeds[len(embeds) // 2:]) if do_cfg else ([], embeds)    # [uncond | cond] under guidance (:605-608)
        for i, t in enumerate(timesteps):                                                       # :694
            self.transformer.current_steps = i
            if self._interrupt:
                continue
            if local is not None:        # dense before `local_attention_from_step`, local from there on
                if i >= local[1]:
                    self.transformer.enable_local_attention(**local[0])
                else:
                    self.transformer.disable_local_attention()
            noise_pred = predict(latents, neg, pos, i, t)
            if mask is not None:
                # Edit inside a mask: outside the mask the target's prediction becomes the one whose x0 is the source
                # block of the state, (x_t - s) / sigma_i -- in place on the step's prediction, after guidance (and after the window
                # blend).  The multistep history then holds the source there, the SDE variants keep their noise term, and the last step
                # (sigma_next = 0) lands the region on the source latents to rounding; inside the mask nothing changes.
                from . import ops
                dt = torch.promote_types(noise_pred.dtype, latents.dtype)      # (both samplers widen to it themselves: an exact cast)
                noise_pred = ops.masked_prediction_(noise_pred.to(dt).contiguous(), latents.to(dt), mask[0], mask[1], mask[2],
                                                    float(self.scheduler.sigmas[i]))
            latents = self.scheduler.step(noise_pred, t, latents, **step_kwargs, return_dict=False)[0]   # :740
            if callback is not None:
                # :742-750 -- the tensors named in callback_on_step_end_tensor_inputs; only `latents` coming back has an effect
                # (there as here: the embeddings of the loop were concatenated before it started, :605-608)
                callback_on_step_end, names, embeddings = callback
                out = callback_on_step_end(self, i, t, {k: {"latents": latents, **embeddings}[k] for k in (names or ())})
                if out:
                    latents = out.pop("latents", latents)
        return latents

    def _denoise_as_one_graph(self, key, loop, latents, embeds, timesteps, has_callback):
        """capture_graph='loop': `loop(latents, embeds)` as ONE hipGraph (videocof_amd.GraphedLoop): the first call of a signature runs
        eagerly, the second captures, later ones replay.  `key`: what of this call is baked into the recorded launches."""
        if has_callback:
            raise NotImplementedError("capture_graph='loop' replays all steps in one launch: no per-step callback")
        if not getattr(self.transformer, "cache_context", False):
            raise NotImplementedError("capture_graph='loop' needs cache_context (the text K/V are part of the graph)")
        cfg = self.scheduler.config
        if cfg.get("algorithm_type") == "sde-dpmsolver++":
            raise NotImplementedError("capture_graph='loop' with sde-dpmsolver++: the host generator's noise draws cannot be "
                                      "recorded into a graph (use capture_graph='step')")
        if self._graphed_loop is None or self._graphed_loop.model is not self.transformer:
            from .graph import GraphedLoop
            self._graphed_loop = GraphedLoop(self.transformer)
        self.scheduler.set_begin_index(0)       # no device round trip (index_for_timestep) inside a capture
        key = key + (int(cfg.solver_order), bool(cfg.lower_order_final), type(self.scheduler).__name__, cfg.get("algorithm_type"),
                     cfg.get("solver_type"), bool(cfg.get("euler_at_final", False)),
                     # which steps run on the conditional half only (enable_cfg_skip) is baked into the captured loop
                     getattr(self.transformer, "cfg_skip_ratio", None), getattr(self.transformer, "num_inference_steps", None),
                     bool(self._cfg_skip_literal))
        def loop_fn(lat, emb):
            self.scheduler._reset()
            self.scheduler.set_begin_index(0)
            return loop(lat, emb)
        return self._graphed_loop(key, latents, embeds, loop_fn, keep=(timesteps, self.scheduler.sigmas))

    def _decode_outputs(self, latents, output_type, cot, cc, G, compare_source, return_dict, stitch=None, match=None):
        """:757-790 -- decode only the grounding and edit segments: (videos, ground_videos, edit_videos, compare_videos).  `stitch`: see
        _decode_frames_u8 -- the frames have the source's size then, not the latents'.  `match`: see there; the edit segment only."""
        ground_video = edit_video = video_out = compare_out = None
        if output_type == "latent":
            return video_out, ground_video, edit_video, compare_out
        if output_type not in ("numpy", "uint8"):
            raise ValueError(f"output_type {output_type!r} not supported ('numpy', 'uint8' or 'latent')")
        if self.vae is None:
            raise ValueError(f"output_type={output_type!r} needs a VAE; use output_type='latent'")
        Ftot, u8 = latents.shape[2], output_type == "uint8"    # uint8 [B, T, H, W, 3] frames (wan_video_to_frames_u8), not float32 [B, 3, T, H, W]
        edit_dev = [] if compare_source is not None else None     # the edit segment's device frames, kept for the compare clip only
        if cot:
            g0, g1 = cc, cc + G
            # grounding | edit frames side by side in ONE page-locked clip (what the reference builds with np.concatenate, :786): each
            # segment is decoded straight into its frame slice, `ground_videos` / `edit_videos` are views of `videos`.  As bytes, the
            # kernel first writes both into their frames of ONE device clip; one contiguous run per segment and sample is copied from it
            tcr, scr = self.vae.config.temporal_compression_ratio, self.vae.config.spatial_compression_ratio
            nfr = lambda n: 1 + tcr * (n - 1) if n > 0 else 0
            ng = nfr(g1 - g0) if (g1 > g0 and g0 < Ftot) else 0
            ne = nfr(Ftot - g1) if g1 < Ftot else 0
            B, H, W = latents.shape[0], latents.shape[3] * scr, latents.shape[4] * scr
            if stitch is not None:
                H, W = int(stitch[0].shape[2]), int(stitch[0].shape[3])
            clip = dev_clip = None
            if ng + ne > 0 and (u8 or latents.is_cuda):
                shape, dtype = ((B, ng + ne, H, W, 3), torch.uint8) if u8 else ((B, 3, ng + ne, H, W), torch.float32)
                clip = torch.empty(shape, dtype=dtype, pin_memory=True)
                dev_clip = torch.empty(clip.shape, dtype=torch.uint8, device=latents.device) if u8 else None

            def segment(lat, a, b, keep=None, match=None):      # latent frames `lat` decoded into frames [a, b) of the clip
                if u8:
                    return self._decode_frames_u8(lat, clip[:, a:b], dev_clip, a, keep, stitch, match)
                return self.decode_latents(lat, None if clip is None else clip[:, :, a:b])
            if ng:
                ground_video = segment(latents[:, :, g0:g1], 0, ng)
            if ne:
                edit_video = segment(latents[:, :, g1:], ng, ng + ne, edit_dev, match)
            if clip is not None:
                video_out = clip.numpy()
            elif not u8:
                video_out = np.concatenate([v for v in (ground_video, edit_video) if v is not None], axis=2)
        elif cc < Ftot:
            video_out = edit_video = (self._decode_frames_u8(latents[:, :, cc:], None, keep=edit_dev, stitch=stitch, match=match)
                                      if edit_dev is not None or stitch is not None or match is not None else self.decode_latents(latents[:, :, cc:], as_uint8=u8))
        if edit_dev:
            from . import video_io
            src = (compare_source if compare_source.dim() == 5 else compare_source.unsqueeze(0)).to(edit_dev[0].device)
            T, H, W = (min(int(a), int(b)) for a, b in zip(src.shape[1:4], edit_dev[0].shape[1:4]))
            pinned = torch.empty((edit_dev[0].shape[0], T, H, 2 * W, 3), dtype=torch.uint8, pin_memory=True)
            compare_out = video_io.compare_frames(src, edit_dev[0], out=pinned).numpy()
        if not return_dict:
            video_out, ground_video, edit_video, compare_out = (torch.from_numpy(v) if isinstance(v, np.ndarray) else v
                                                                for v in (video_out, ground_video, edit_video, compare_out))
        return video_out, ground_video, edit_video, compare_out

    @torch.no_grad()
    def __call__(self, video: Optional[torch.Tensor] = None, prompt=None, negative_prompt=None,
                 height: int = 480, width: int = 720, num_frames: int = 49, source_frames: int = 33,
                 reasoning_frames: int = 4, num_inference_steps: int = 50, timesteps=None,
                 guidance_scale: float = 6.0, num_videos_per_prompt: int = 1, eta: float = 0.0,
                 generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds=None, negative_prompt_embeds=None, output_type: str = "numpy",
                 return_dict: bool = False, callback_on_step_end: Optional[Callable] = None,
                 attention_kwargs=None, callback_on_step_end_tensor_inputs=("latents",),
                 max_sequence_length: int = 512, comfyui_progressbar: bool = False,
                 shift: float = 5.0, repeat_rope: bool = True, cot: bool = False,
                 # extensions of this package (keyword-only in spirit; the names above are the reference's, :516-548)
                 source_latents: Optional[torch.Tensor] = None, device=None,
                 weight_dtype: torch.dtype = torch.bfloat16, cache_context: bool = True,
                 skip_source_prediction: bool = True, capture_graph=False, **switches):
        # -- the switches (see _parse_switches for what they are), checked before anything runs
        has_source = video is not None or source_latents is not None or latents is not None
        opt = self._parse_switches(switches, video, has_source, source_frames, height, width, output_type, capture_graph,
                                   has_latents=latents is not None or source_latents is not None)
        # `timesteps`: with either scheduler built here the reference never looks at it (pipeline_wan.py:613-621: UniPC takes
        # set_timesteps(num_inference_steps, device=, shift=), DPM++ the sigmas of get_sampling_sigmas); accepted and ignored here too.
        del timesteps
        self.check_inputs(prompt, height, width, negative_prompt, callback_on_step_end_tensor_inputs, prompt_embeds, negative_prompt_embeds)
        self._guidance_scale, self._interrupt = guidance_scale, False
        self._attention_kwargs = attention_kwargs                                               # :575 (stored, read by nothing, as there)
        device = torch.device(device) if device is not None else self.transformer.device
        do_cfg = guidance_scale > 1.0                                                           # :592
        # -- the prompt
        t_stage = self._stage("text_encoder")
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, negative_prompt, do_cfg, num_videos_per_prompt=1, prompt_embeds=prompt_embeds,       # (1: the reference overrides the
            negative_prompt_embeds=negative_prompt_embeds, max_sequence_length=max_sequence_length, device=device)   # argument, :561)
        self._stage("text_encoder", t_stage)
        in_prompt_embeds = (negative_prompt_embeds + prompt_embeds) if do_cfg else prompt_embeds   # :605-608
        # -- the timesteps
        timesteps = self._set_timesteps(num_inference_steps, shift, device)
        extra_step_kwargs = self.prepare_extra_step_kwargs(generator, eta)                       # :682
        self._num_timesteps = len(timesteps)
        # -- the latents [source | grounding | target]
        ratio = getattr(self.vae, "temporal_compression_ratio", 4)
        condition_count = 1 if source_frames == 1 else (source_frames - 1) // ratio + 1         # :630-631
        window_sizes = self._window_sizes(opt, ratio, has_source)
        ground_latent_count = 0
        if cot:
            ground_latent_count = 1 if reasoning_frames <= 1 else (reasoning_frames - 1) // ratio + 1   # :637
        vae_box = stitch = None
        if opt.vae_halo is not None:
            # `edit_region_vae_halo`: the mask, the region and the box first, then the encode of the box only
            latents, mask_weights, region, loop_cc, vae_box, stitch = self._encode_box_to_region(
                opt, video, generator, weight_dtype, device, window_sizes[1], condition_count, ground_latent_count, source_frames,
                height, width)
            if opt.compare:
                opt.compare_source = stitch[0]           # the source frames are on the device already
        else:
            t_stage = self._stage("vae_encode")
            if cot:
                latents = self.prepare_cot_video_latents(video, ground_latent_count, dtype=weight_dtype, device=device, generator=generator,
                                                         condition_count=condition_count, latents=latents, source_latents=source_latents)
            else:
                # repeat / org layouts: noise block has the source's frame count (:653-677 -> :343-378)
                latents = self.prepare_video_latents_new(video, dtype=weight_dtype, device=device, generator=generator,
                                                         condition_count=condition_count, latents=latents, source_latents=source_latents)
            self._stage("vae_encode", t_stage)
            # -- the mask and the windows; what one forward holds: the whole clip, or one window of `win_n` source frames and `win_hw` cells
            mask_weights = self._mask_weights(opt, latents.shape, latents.device, condition_count, ground_latent_count, source_frames,
                                              height, width)
            # `loop_cc`: the source frames of the clip the loop runs on -- condition_count, or the frame range's after a time crop
            latents, mask_weights, region, loop_cc = self._crop_to_region(opt, latents, mask_weights, window_sizes[1], condition_count,
                                                                          ground_latent_count)
        # `edit_region_split`: the K' boxes are K' x B samples, box-major, and every box takes its sample's prompts (the order in
        # which _windowed_form repeats them for its windows)
        boxes = len(region[0].origins) if region is not None and hasattr(region[0], "cuts") else 1
        if boxes > 1:
            in_prompt_embeds = (negative_prompt_embeds * boxes + prompt_embeds * boxes) if do_cfg else prompt_embeds * boxes
        plan, tiles = self._plan_windows(opt, window_sizes, latents.shape, loop_cc, ground_latent_count, capture_graph)
        windowed = plan is not None or tiles is not None
        win_n = loop_cc if not windowed else tiles.t.window if tiles is not None else plan.window
        win_hw = latents.shape[3] * latents.shape[4] if tiles is None else tiles.y.window * tiles.x.window
        win_frames = latents.shape[2] if not windowed else 2 * win_n + ground_latent_count
        seq_len = math.ceil(win_hw / math.prod(self.transformer.config.patch_size[1:]) * win_frames)     # :686-689
        self.transformer.num_inference_steps = num_inference_steps
        if capture_graph not in (False, True, "step", "loop"):
            raise ValueError(f"capture_graph={capture_graph!r}: False, True / 'step' (one hipGraph per forward) or 'loop' (the whole loop)")
        local_cfg = _local_attention_args(opt.local_attention, opt.local_from, capture_graph)
        # :713 is `if repeat_rope and video is not None`, and the reference cannot run without `video` at all (`video.to(...)` at :397 precedes
        # the `latents` short-cut), so on every call the reference accepts the condition is just `repeat_rope`.  Here `video` may be omitted
        # when `latents` (reference argument) or `source_latents` (extension) carry the encoded source: such calls are treated like the reference
        # treats the same call WITH its video; a call with none of the three has no source segment and keeps plain T2V positions.
        use_rope_map = repeat_rope and has_source
        # -- denoise
        t_stage = self._stage("denoise_loop")
        with self._transformer_settings(cache_context, win_n if skip_source_prediction else 0, win_n, local_cfg) as zero_source:
            forward = self.transformer
            if capture_graph in (True, "step"):
                # one hipGraph per call shape, kept across calls (videocof_amd/graph.py): step 0 of the first call runs
                # eagerly, step 1 is captured, every later step (and call) is a replay -- bit-identical latents
                if self._graphed is None or self._graphed.model is not self.transformer:
                    from .graph import GraphedForward
                    self._graphed = GraphedForward(self.transformer)
                forward = self._graphed
            guided = self._guided_forward(forward, do_cfg, seq_len, win_n if use_rope_map else None,
                             (win_n, win_n + ground_latent_count) if use_rope_map and cot else None)
            if windowed:
                latents, predict, target_frame0, cut = self._windowed_form(guided, latents, plan, tiles, opt.window_batch,
                                                                           loop_cc, ground_latent_count)
            else:
                predict, target_frame0, cut = self._whole_clip_form(guided, loop_cc, ground_latent_count, zero_source, boxes > 1)
            callback = None if callback_on_step_end is None else (callback_on_step_end, callback_on_step_end_tensor_inputs, {
                "prompt_embeds": prompt_embeds, "negative_prompt_embeds": negative_prompt_embeds})
            loop = lambda lat, embeds: cut(self._denoise(
                lat, embeds, do_cfg, timesteps, predict, None if local_cfg is None else (local_cfg, opt.local_from),
                None if mask_weights is None else (mask_weights, loop_cc, target_frame0), extra_step_kwargs, callback))
            if capture_graph == "loop":
                key = (int(num_inference_steps), float(shift), bool(do_cfg), float(guidance_scale) if do_cfg else 0.0,
                       int(condition_count), int(ground_latent_count), bool(cot), bool(use_rope_map), int(seq_len))
                latents = self._denoise_as_one_graph(key, loop, latents, in_prompt_embeds, timesteps, callback is not None)
            else:
                latents = loop(latents, in_prompt_embeds)
        if region is not None:
            latents = self._restore_region(latents, region, vae_box)
        self._stage("denoise_loop", t_stage)
        # -- decode (:757-790)
        t_stage = self._stage("vae_decode")
        match = None
        if opt.color_args is not None:
            # one upload of the source frames and the mask where they came from the host (compare=True then takes the same device frames)
            src = opt.color_source.to(latents.device)
            if opt.compare_source is not None and not opt.compare_source.is_cuda:
                opt.compare_source = src
            match = (src, None if opt.edit_mask is None else opt.edit_mask.to(latents.device), opt.color_args, [])
        videos, ground, edit, compared = self._decode_outputs(latents, output_type, cot, condition_count, ground_latent_count,
                                                              opt.compare_source, return_dict, stitch, match)
        self._stage("vae_decode", t_stage)
        tracked = region is not None and opt.region_follow is not None
        return WanPipelineOutput(videos=videos, ground_videos=ground, edit_videos=edit, latents=latents, compare_videos=compared,
                                 color_match=match[3][0] if match is not None and match[3] else None,
                                 edit_region=None if region is None else (region[0].enclosing() if tracked or boxes > 1 else region[0]).pixels(
                                     getattr(getattr(self.vae, "config", None), "spatial_compression_ratio", 8)),
                                 edit_regions=None if boxes == 1 else region[0].pixels(
                                     getattr(getattr(self.vae, "config", None), "spatial_compression_ratio", 8)),
                                 edit_region_track=None if not tracked else region[0].pixels(
                                     getattr(getattr(self.vae, "config", None), "spatial_compression_ratio", 8)),
                                 edit_region_time=None if region is None or region[2] is None else region[2].pixels(ratio),
                                 edit_region_vae=None if vae_box is None else vae_box.pixels(
                                     getattr(getattr(self.vae, "config", None), "spatial_compression_ratio", 8)))
