"""A recording stand-in for the DiT, shared by tests/test_pipeline_trace_host.py and tests/test_gpu_pipeline_trace.py: what
``WanPipeline.__call__`` hands to every forward, and which of the model's settings hold at that moment, as plain records that a test
compares with a list written out from the rules."""
from types import SimpleNamespace

import torch

from videocof_amd.wan_transformer3d import cfg_skip_active

POS_ROWS, NEG_ROWS = 5, 3              # prompts of different lengths: the context's row counts tell the two halves of a batch apart
LOCAL = {"window_frames": 2, "window_rows": 2}


def prompts(device="cpu"):
    """(prompt_embeds, negative_prompt_embeds) for one sample."""
    return [torch.ones(POS_ROWS, 8, device=device)], [torch.ones(NEG_ROWS, 8, device=device)]


def scale(rows: int) -> float:
    """The stub's prediction for a sample is ``x * scale(rows of its context)``: exact in bf16, different for the two prompts."""
    return rows / 4.0


class RecordingTransformer:
    """Every attribute the pipeline reads or sets on a transformer, and a forward that appends one record per call to ``calls``."""

    def __init__(self, device="cpu", fail_at=None):
        self.config = SimpleNamespace(patch_size=(1, 2, 2))
        self.device = torch.device(device)
        self.cache_context, self.skip_source_frames, self.mask_source_frames = False, 0, 0
        self.local_attention = None
        self.cfg_skip_ratio, self.current_steps, self.num_inference_steps = None, 0, None
        self._cfg_skip_suspended = False
        self.teacache = None
        self.fail_at = fail_at                     # the forward of this step raises
        self.calls, self.cache_clears, self.releases = [], 0, 0

    def clear_context_cache(self):
        self.cache_clears += 1

    def release_workspaces(self, keep_pinned=False):
        self.releases += 1

    def enable_local_attention(self, **kw):
        self.local_attention = dict(kw)

    def disable_local_attention(self):
        self.local_attention = None

    def cfg_skip_now(self, batch):
        return not self._cfg_skip_suspended and cfg_skip_active(batch, self.cfg_skip_ratio, self.current_steps, self.num_inference_steps)

    def settings(self):
        return dict(cache=self.cache_context, skip=self.skip_source_frames, mask=self.mask_source_frames,
                    local=None if self.local_attention is None else dict(self.local_attention), suspended=self._cfg_skip_suspended)

    def __call__(self, x, t, context, seq_len, frame_split_indices=None, ground_frame_indices=None):
        halved = self.cfg_skip_now(x.shape[0])
        self.calls.append(dict(step=self.current_steps, x=tuple(x.shape), ctx=[int(c.shape[0]) for c in context], t=t.tolist(),
                               seq_len=seq_len, fsi=frame_split_indices, gfi=ground_frame_indices, halved=halved, **self.settings()))
        if self.current_steps == self.fail_at:
            raise RuntimeError("the stub's forward fails at this step")
        s = torch.tensor([scale(c.shape[0]) for c in context], device=x.device, dtype=x.dtype).view(-1, 1, 1, 1, 1)
        out = x * s
        if halved:                                 # the model's own cfg_skip rule: the conditional half, twice
            out = torch.cat([out[x.shape[0] // 2:]] * 2)
        out[:, :, :self.mask_source_frames] = 0
        return out


def record(step, x, ctx, t, seq_len, n, G, *, suspended=False, halved=False, local=None, cache=True):
    """The record of one forward of ``x[0]`` samples over windows of ``n`` source frames and ``G`` grounding frames (G = 0: no CoF map)."""
    nb = x[0]
    return dict(step=step, x=tuple(x), ctx=list(ctx), t=[t] * nb, seq_len=seq_len, fsi=[n] * nb, gfi=[(n, n + G)] * nb if G else None,
                halved=halved, cache=cache, skip=n, mask=n, local=local, suspended=suspended)
