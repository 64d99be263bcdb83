"""-m gpu: the windowed denoise loop of ``WanPipeline.__call__`` seen from the transformer.  The recording stub of
tests/pipeline_trace.py stands in for the DiT on the device (the gather / blend / masked-prediction kernels and the sampler are the
real ones); every forward's record is compared with a list built here from the rules of DESIGN.md 13.1-13.4: which windows a forward
holds, in which batch order, with which prompts, and whether the model's own cfg_skip rule is suspended meanwhile.  A few seconds."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from videocof_amd import FlowUniPCMultistepScheduler, WanPipeline, ops
from videocof_amd.wan_transformer3d import cfg_skip_active

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pipeline_trace import NEG_ROWS, POS_ROWS, RecordingTransformer, prompts, record  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS, SHIFT, GUIDE, G = 4, 3.0, 3.0, 1
# name: (latent frames of the source, latent rows = columns, the options, windows K, temporal windows Kt, source frames of a window)
TEMPORAL = dict(temporal_window=13, temporal_overlap=8)                 # 7 frames / window 4 / overlap 2: starts (0, 2, 3)
SPATIAL = dict(spatial_window=(32, 32), spatial_overlap=(16, 16))       # 6 x 6 cells / tile 4 x 4 / overlap 2: starts (0, 2) per axis
PLANS = {"temporal": (7, 4, TEMPORAL, 3, 3, 4), "spatial": (3, 6, SPATIAL, 4, 1, 3), "both": (7, 6, {**TEMPORAL, **SPATIAL}, 12, 3, 4)}


def run(stub, plan, guidance=1.0, pipe=None, **kw):
    fs, hw, options = PLANS[plan][:3]
    pipe = pipe or WanPipeline(transformer=stub, scheduler=FlowUniPCMultistepScheduler(shift=1))
    g = torch.Generator().manual_seed(7)
    lat = torch.randn(1, 16, 2 * fs + G, hw, hw, generator=g)
    pos, neg = prompts(DEV)
    out = pipe(latents=lat, prompt_embeds=pos, negative_prompt_embeds=neg if guidance > 1 else None, guidance_scale=guidance,
               source_frames=4 * (fs - 1) + 1, height=8 * hw, width=8 * hw, reasoning_frames=4, num_inference_steps=STEPS, shift=SHIFT,
               cot=True, output_type="latent", **options, **kw)
    assert tuple(out.latents.shape) == (1, 16, 2 * fs + G, hw, hw)       # [source | ground_0 | target], as a whole-clip call returns
    return pipe, out.latents


def expected(pipe, plan, guided=False, window_batch=None, ratio=None, literal=False):
    """One forward per chunk of ``window_batch`` windows (all K in one without it), batch order [uncond windows | cond windows].  A step
    the cfg_skip rule halves runs the conditional windows only; the model's own rule, which would halve ANY batch of two or more,
    stays suspended -- except in the literal form on such a step, where the doubled batch goes through it."""
    K, n = PLANS[plan][3], PLANS[plan][5]
    x = (16, 2 * n + G, 4, 4)
    out = []
    for i, t in enumerate(pipe.scheduler.timesteps.tolist()):
        for k0 in range(0, K, window_batch or K):
            nk = min(k0 + (window_batch or K), K) - k0
            half = guided and cfg_skip_active(2 * nk, ratio, i, STEPS)
            doubled = guided and (literal or not half)
            ctx = [NEG_ROWS] * nk + [POS_ROWS] * nk if doubled else [POS_ROWS] * nk
            out.append(record(i, (len(ctx),) + x, ctx, t, math.ceil(4 * 4 / 4 * (2 * n + G)), n, G,
                              suspended=not (half and doubled), halved=half and doubled))
    return out


@pytest.mark.parametrize("plan,window_batch", [("temporal", None), ("temporal", 2), ("spatial", None), ("both", None), ("both", 5)])
@pytest.mark.parametrize("guidance", [1.0, GUIDE], ids=["unguided", "guided"])
def test_every_step_runs_the_windows_of_the_plan(plan, window_batch, guidance):
    stub = RecordingTransformer(DEV)
    pipe, got = run(stub, plan, guidance, window_batch=window_batch)
    assert stub.calls == expected(pipe, plan, guidance > 1, window_batch)
    assert stub.settings() == dict(cache=False, skip=0, mask=0, local=None, suspended=False)
    if window_batch is not None:          # the stub treats every sample on its own: how the windows are batched changes no bit
        assert torch.equal(got, run(RecordingTransformer(DEV), plan, guidance)[1])


@pytest.mark.parametrize("literal", [False, True], ids=["short", "literal"])
@pytest.mark.parametrize("plan,window_batch", [("temporal", None), ("temporal", 2), ("both", 5)])
def test_cfg_skip_over_windows(plan, window_batch, literal):
    """Ratio 0.5: steps 2 and 3 run the conditional windows only, or, in the literal form, the doubled batch through the model's rule."""
    stub = RecordingTransformer(DEV)
    stub.cfg_skip_ratio = 0.5
    pipe = WanPipeline(transformer=stub, scheduler=FlowUniPCMultistepScheduler(shift=1))
    pipe._cfg_skip_literal = literal
    run(stub, plan, GUIDE, pipe=pipe, window_batch=window_batch)
    want = expected(pipe, plan, True, window_batch, 0.5, literal)
    assert stub.calls == want and stub._cfg_skip_suspended is False
    assert [r["halved"] for r in want if r["step"] >= 2] == [literal] * (len(want) // 2)
    # without guidance nothing is a guidance pair: every batch of windows runs whole, the rule suspended
    plain = RecordingTransformer(DEV)
    plain.cfg_skip_ratio = 0.5
    pipe, _ = run(plain, plan, window_batch=window_batch)
    assert plain.calls == expected(pipe, plan, False, window_batch, 0.5)


def test_the_masked_step_receives_the_steps_sigma_and_the_target_of_the_windowed_state(monkeypatch):
    """An edit mask over windows: after the blend, the prediction for the state [source | ground_0 .. ground_2 | target] goes through
    wan_masked_prediction with sigma_i and the target's first frame in THAT layout, 7 + 3 * 1."""
    seen, real = [], ops.masked_prediction_

    def spy(pred, sample, weights, Fs, target_frame0, sigma):
        seen.append((tuple(pred.shape), tuple(sample.shape), tuple(weights.shape), Fs, target_frame0, sigma))
        return real(pred, sample, weights, Fs, target_frame0, sigma)
    monkeypatch.setattr(ops, "masked_prediction_", spy)
    mask = np.zeros((25, 32, 32), np.uint8)
    mask[:, 8:24, 8:24] = 255
    stub = RecordingTransformer(DEV)
    pipe, _ = run(stub, "temporal", GUIDE, edit_mask=mask)
    state = (1, 16, 7 + 3 * G + 7, 4, 4)
    assert seen == [(state, state, (1, 7, 4, 4), 7, 10, float(s)) for s in pipe.scheduler.sigmas[:STEPS]]
    assert stub.calls == expected(pipe, "temporal", True)


def test_the_step_graph_routes_the_same_forwards():
    """``capture_graph='step'`` sends every forward through ``pipe._graphed`` (a GraphedForward kept across calls while its ``model``
    is the pipeline's transformer).  A pass-through in its place sees the forwards of the eager call, the same settings at the time."""
    class Routed:
        def __init__(self, model):
            self.model, self.count = model, 0

        def __call__(self, **kw):
            self.count += 1
            return self.model(**kw)
    eager = RecordingTransformer(DEV)
    _, want = run(eager, "temporal", GUIDE, window_batch=2)
    stub = RecordingTransformer(DEV)
    pipe = WanPipeline(transformer=stub, scheduler=FlowUniPCMultistepScheduler(shift=1))
    pipe._graphed = routed = Routed(stub)
    _, got = run(stub, "temporal", GUIDE, pipe=pipe, window_batch=2, capture_graph="step")
    assert pipe._graphed is routed and routed.count == len(eager.calls) == 2 * STEPS
    assert stub.calls == eager.calls and torch.equal(got, want)
