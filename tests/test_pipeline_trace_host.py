"""The denoise loop of ``WanPipeline.__call__`` on the CPU, whole-clip path, seen from the transformer: a recording stub
(tests/pipeline_trace.py) notes what every forward receives and which of the model's settings hold at that moment.  The expected
records are written out here from the rules (pipeline_wan.py's module docstring; DESIGN.md "cfg_skip", 13.3), the expected latents
come from the same steps taken by hand on a second scheduler.  4 steps, B = 1, [3 source | 1 grounding | 3 target] frames of 4 x 4."""
import os
import sys

import pytest
import torch

from videocof_amd import FlowUniPCMultistepScheduler, WanPipeline

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pipeline_trace import LOCAL, NEG_ROWS, POS_ROWS, RecordingTransformer, prompts, record, scale  # noqa: E402

STEPS, SHIFT, GUIDE = 4, 3.0, 3.0
CC, G = 3, 1
SEQ = {True: 28, False: 24}            # ceil(4 * 4 / (2 * 2) * frames): 7 frames with the grounding frame, 6 without


def latents(cot=True):
    g = torch.Generator().manual_seed(5)
    return torch.randn(1, 16, 2 * CC + (G if cot else 0), 4, 4, generator=g)


def run(stub, guidance=1.0, cot=True, **kw):
    pipe = kw.pop("pipe", None) or WanPipeline(transformer=stub, scheduler=FlowUniPCMultistepScheduler(shift=1))
    pos, neg = prompts()
    out = pipe(latents=latents(cot), prompt_embeds=pos, negative_prompt_embeds=neg if guidance > 1 else None, guidance_scale=guidance,
               source_frames=9, reasoning_frames=4, num_inference_steps=STEPS, shift=SHIFT, cot=cot, output_type="latent",
               weight_dtype=torch.float32, device="cpu", **kw)
    return pipe, out.latents


def by_hand(guidance=1.0, cot=True, steps=STEPS, after=None):
    """The loop of :694-740 with the stub's arithmetic written out: v = x * scale(rows), guidance, the CoF mask, one sampler step."""
    sched = FlowUniPCMultistepScheduler(shift=1)
    sched.set_timesteps(STEPS, device="cpu", shift=SHIFT)
    x = latents(cot)
    for i, t in enumerate(sched.timesteps[:steps]):
        v = x * scale(POS_ROWS)
        if guidance > 1:
            nu = x * scale(NEG_ROWS)
            v = nu + guidance * (v - nu)
        v[:, :, :CC] = 0
        x = sched.step(v, t, x, return_dict=False)[0]
        if after is not None:
            x = after(i, x)
    return x, [float(t) for t in sched.timesteps]


def rec(i, ts, batch, ctx, cot=True, **kw):
    return record(i, (batch, 16, 2 * CC + (G if cot else 0), 4, 4), ctx, ts[i], SEQ[cot], CC, G if cot else 0, **kw)


@pytest.mark.parametrize("cot", [True, False], ids=["cot", "no-cot"])
@pytest.mark.parametrize("guidance", [1.0, GUIDE], ids=["unguided", "guided"])
def test_every_step_is_one_forward_of_the_whole_clip(guidance, cot):
    stub = RecordingTransformer()
    _, got = run(stub, guidance, cot)
    want, ts = by_hand(guidance, cot)
    batch, ctx = (2, [NEG_ROWS, POS_ROWS]) if guidance > 1 else (1, [POS_ROWS])          # batch order [uncond, cond] (:700)
    assert stub.calls == [rec(i, ts, batch, ctx, cot) for i in range(STEPS)]
    assert torch.equal(got, want)
    assert stub.settings() == dict(cache=False, skip=0, mask=0, local=None, suspended=False) and stub.cache_clears == 2


def test_a_cfg_skip_step_runs_the_conditional_half_only():
    """Ratio 0.5 of 4 steps: steps 2 and 3.  The short form calls the model with the positive prompts alone and the model's own rule
    suspended; guidance on two equal halves is the conditional prediction itself, so the latents are those of the literal form."""
    stub = RecordingTransformer()
    stub.cfg_skip_ratio = 0.5
    _, got = run(stub, GUIDE)
    ts = by_hand()[1]
    assert stub.calls == [rec(0, ts, 2, [NEG_ROWS, POS_ROWS]), rec(1, ts, 2, [NEG_ROWS, POS_ROWS]),
                          rec(2, ts, 1, [POS_ROWS], suspended=True), rec(3, ts, 1, [POS_ROWS], suspended=True)]
    assert stub._cfg_skip_suspended is False
    # the literal form: the doubled batch through the model's rule (not suspended: it halves the call itself), then guidance
    literal = RecordingTransformer()
    literal.cfg_skip_ratio = 0.5
    pipe = WanPipeline(transformer=literal, scheduler=FlowUniPCMultistepScheduler(shift=1))
    pipe._cfg_skip_literal = True
    _, want = run(literal, GUIDE, pipe=pipe)
    assert literal.calls == [rec(i, ts, 2, [NEG_ROWS, POS_ROWS], halved=i >= 2) for i in range(STEPS)]
    assert torch.equal(got, want)
    # and by hand: two guided steps, then two of the conditional prediction alone
    sched = FlowUniPCMultistepScheduler(shift=1)
    sched.set_timesteps(STEPS, device="cpu", shift=SHIFT)
    x = latents()
    for i, t in enumerate(sched.timesteps):
        v = x * scale(POS_ROWS)
        if i < 2:
            nu = x * scale(NEG_ROWS)
            v = nu + GUIDE * (v - nu)
        v[:, :, :CC] = 0
        x = sched.step(v, t, x, return_dict=False)[0]
    assert torch.equal(got, x)


def test_the_callback_sees_every_step_and_may_replace_the_latents():
    stub, seen = RecordingTransformer(), []

    def callback(pipe, i, t, tensors):
        seen.append((i, float(t), sorted(tensors), stub.current_steps))
        return {"latents": tensors["latents"] * 0.5} if i == 1 else {}
    _, got = run(stub, GUIDE, callback_on_step_end=callback, callback_on_step_end_tensor_inputs=("latents", "prompt_embeds"))
    want, ts = by_hand(GUIDE, after=lambda i, x: x * 0.5 if i == 1 else x)
    assert seen == [(i, ts[i], ["latents", "prompt_embeds"], i) for i in range(STEPS)]
    assert [c["step"] for c in stub.calls] == list(range(STEPS)) and torch.equal(got, want)


def test_an_interrupt_skips_the_remaining_forwards():
    stub = RecordingTransformer()

    def callback(pipe, i, t, tensors):
        pipe._interrupt = i == 1
        return {}
    pipe, got = run(stub, callback_on_step_end=callback)
    want, ts = by_hand(steps=2)
    assert stub.calls == [rec(i, ts, 1, [POS_ROWS]) for i in range(2)] and torch.equal(got, want)
    assert stub.current_steps == STEPS - 1 and pipe.interrupt         # the step counter still runs to the end (:694-697)
    run(stub, pipe=pipe)                                               # the next call starts with the interrupt cleared
    assert len(stub.calls) == 2 + STEPS


@pytest.mark.parametrize("own", [None, {"window_frames": 1, "window_rows": 1, "sink_frames": 1}], ids=["dense-model", "local-model"])
def test_local_attention_from_a_step_on(own):
    """Steps before ``local_attention_from_step`` run dense, whatever the model's own setting, which is back afterwards."""
    stub = RecordingTransformer()
    stub.local_attention = own
    run(stub, local_attention=(LOCAL["window_frames"], LOCAL["window_rows"]), local_attention_from_step=2)
    ts = by_hand()[1]
    assert stub.calls == [rec(i, ts, 1, [POS_ROWS], local=LOCAL if i >= 2 else None) for i in range(STEPS)]
    assert stub.local_attention == own


def test_a_failing_forward_leaves_the_models_settings_as_they_were():
    stub = RecordingTransformer(fail_at=1)
    stub.cache_context, stub.skip_source_frames, stub.mask_source_frames = False, 7, 5
    stub.local_attention = {"window_frames": 1, "window_rows": 1}
    stub.cfg_skip_ratio = 1.0                       # every step is a short one: the rule is suspended when the forward raises
    pipe = WanPipeline(transformer=stub, scheduler=FlowUniPCMultistepScheduler(shift=1))
    pipe.release_workspaces_after_denoise = True
    with pytest.raises(RuntimeError, match="fails at this step"):
        run(stub, GUIDE, pipe=pipe, local_attention=LOCAL, cache_context=True)
    assert [(c["step"], c["suspended"], c["cache"], c["skip"], c["mask"], c["local"]) for c in stub.calls] == \
        [(0, True, True, CC, CC, LOCAL), (1, True, True, CC, CC, LOCAL)]
    assert stub.settings() == dict(cache=False, skip=7, mask=5, local={"window_frames": 1, "window_rows": 1}, suspended=False)
    assert stub.cache_clears == 2 and stub.releases == 1
