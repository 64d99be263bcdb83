"""-m gpu: the change mask and the composite on the device (wan_change_mask, wan_plane_u8_resample, wan_frames_u8_composite behind
video_io.change_mask / composite_frames / keep_unedited) against ``reference_change_mask`` / ``reference_composite_frames``, the
numpy definitions that tests/test_keep_unedited_host.py checks.  EQUALITY everywhere: both sides are integer arithmetic.

The mask kernel's tile is 32 x 64 pixels with a border of up to 32, the composite moves 16 pixels per thread, so the shapes cover a
frame inside one tile, tiles with a remainder in both axes, windows larger than the frame, and a base at an odd address."""
import numpy as np
import pytest
import torch

from videocof_amd import (change_mask, composite_frames, fit_frames, keep_unedited, reference_change_mask, reference_composite_frames,
                          restore_frames)
from videocof_amd.video_io import fit_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLD = 10
PARAMS = [(0, 0, 0, 0), (2, 12, 1, 8), (7, 32, 4, 32)]            # (smooth, grow, grow_t, feather)


def clips(shape, seed=0):
    """A random source and an edit of it: noise of +-3 everywhere (below THRESHOLD), and per frame one repainted block and a few
    repainted single pixels at seeded places, so every step of the mask has edges inside the frame and at its borders."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (*shape, 3), generator=g, dtype=torch.uint8)
    edit = (src.long() + torch.randint(-3, 4, src.shape, generator=g)).clamp(0, 255)
    T, H, W = shape[-3:]
    flat_s, flat_e = src.view(-1, H, W, 3), edit.view(-1, H, W, 3)
    for n in range(flat_s.shape[0]):
        if n % 2 == 0 or T == 1:
            y, x = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
            flat_e[n, y:y + 4, x:x + 6] = 255 - flat_s[n, y:y + 4, x:x + 6].long()
            for _ in range(3):
                y, x = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
                flat_e[n, y, x] = 255 - flat_s[n, y, x].long()
    return src, edit.to(torch.uint8)


def check_mask(src, edit, params, dev_src=None, dev_edit=None):
    kw = dict(threshold=THRESHOLD, smooth=params[0], grow=params[1], grow_t=params[2], feather=params[3])
    want = reference_change_mask(src, edit, **kw)
    got = change_mask(src.to(DEV) if dev_src is None else dev_src, edit.to(DEV) if dev_edit is None else dev_edit, **kw)
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == tuple(want.shape)
    bad = int((got.cpu() != want).sum())
    print(f"change_mask {tuple(src.shape)} {params}: {bad} mismatches of {want.numel()}, alpha 0 / 255 / between = "
          f"{int((want == 0).sum())} / {int((want == 255).sum())} / {int(((want > 0) & (want < 255)).sum())}")
    assert bad == 0
    return want


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("shape", [(3, 19, 37), (4, 70, 200)])
def test_change_mask_equals_the_definition(shape, params):
    want = check_mask(*clips(shape, seed=shape[1]), params)
    if shape == (4, 70, 200):                                                        # all three kinds of alpha occur (19 x 37 is covered whole)
        assert 0 < int((want == 0).sum()) and 0 < int((want == 255).sum()) and (params[3] == 0 or 0 < int((want % 255 != 0).sum()))


def test_change_mask_windows_larger_than_the_frame():
    src, edit = clips((1, 5, 7), seed=2)
    check_mask(src, edit, (7, 8, 0, 8))
    check_mask(src, edit, (7, 8, 2, 8))                                              # T = 1 with grow_t = 2
    want = check_mask(src, edit, (0, 1, 4, 1))                                       # the same frame with windows that leave edges in it
    assert 0 < int((want == 0).sum()) and 0 < int((want % 255 != 0).sum())


@pytest.mark.parametrize("params", PARAMS)
def test_change_mask_of_a_misaligned_clip_and_a_batch(params):
    src, edit = clips((2, 3, 19, 37), seed=4)
    views = []
    for fr in (src, edit):
        flat = torch.zeros(fr.numel() + 1, dtype=torch.uint8, device=DEV)
        flat[1:] = fr.to(DEV).view(-1)
        views.append(flat[1:].view(fr.shape))
        assert views[-1].data_ptr() % 2 == 1
    want = check_mask(src, edit, params, *views)
    assert torch.equal(want[1], reference_change_mask(src[1], edit[1], threshold=THRESHOLD, smooth=params[0], grow=params[1],
                                                      grow_t=params[2], feather=params[3]))
    host = change_mask(src.numpy(), edit, threshold=THRESHOLD, smooth=params[0], grow=params[1], grow_t=params[2], feather=params[3])
    assert host.is_cuda and torch.equal(host.cpu(), want)                            # host input goes to the device as bytes


def test_same_size_composite_over_every_triple():
    """One 4096 x 4096 frame whose first channel runs through all 256^3 triples (alpha, edit, original); the other two channels are
    random.  The division by 255 is exact for every one of them."""
    n = torch.arange(4096 * 4096, dtype=torch.int32, device=DEV).view(1, 4096, 4096)
    g = torch.Generator(device=DEV).manual_seed(1)
    alpha = (n >> 16).to(torch.uint8)
    edit = torch.randint(0, 256, (1, 4096, 4096, 3), generator=g, dtype=torch.uint8, device=DEV)
    orig = torch.randint(0, 256, (1, 4096, 4096, 3), generator=g, dtype=torch.uint8, device=DEV)
    edit[..., 0] = ((n >> 8) & 255).to(torch.uint8)
    orig[..., 0] = (n & 255).to(torch.uint8)
    got = composite_frames(orig, edit, alpha)
    assert got.is_cuda and got.shape == orig.shape and got.dtype == torch.uint8
    want = reference_composite_frames(orig, edit, alpha)
    assert torch.equal(alpha.int() * 65536 + edit[..., 0].int() * 256 + orig[..., 0].int(), n)       # pixel n holds the triple number n
    bad = int((got.cpu() != want).sum())
    print(f"composite over all (a, e, o): {bad} mismatches of {want.numel()}")
    assert bad == 0


@pytest.fixture(scope="module", params=[((54, 100), (32, 48)), ((135, 240), (48, 80))], ids=["54x100", "135x240"])
def planned(request):
    orig, fit = request.param
    plan = fit_plan(*orig, *fit)
    g = torch.Generator().manual_seed(orig[1])
    o = torch.randint(0, 256, (2, *orig, 3), generator=g, dtype=torch.uint8)
    e = torch.randint(0, 256, (2, *fit, 3), generator=g, dtype=torch.uint8)
    a = torch.randint(0, 256, (2, *fit), generator=g, dtype=torch.uint8)
    return plan, o, e, a


@pytest.mark.parametrize("kind", ["random", "zero", "full"])
def test_composite_with_a_plan_equals_the_definition(planned, kind):
    plan, o, e, a = planned
    a = {"random": a, "zero": torch.zeros_like(a), "full": torch.full_like(a, 255)}[kind]
    want = reference_composite_frames(o, e, a, plan)
    got = composite_frames(o.to(DEV), e.to(DEV), a.to(DEV), plan)
    assert got.is_cuda and got.is_contiguous() and got.shape == o.shape
    bad = int((got.cpu() != want).sum())
    print(f"composite {tuple(o.shape)} <- {tuple(e.shape)} alpha {kind}: {bad} mismatches of {want.numel()}")
    assert bad == 0
    y, x, wh, ww = plan.source_window
    if kind == "zero":
        assert torch.equal(got.cpu(), o)
    if kind == "full":
        assert torch.equal(got[:, y:y + wh, x:x + ww], restore_frames(e.to(DEV), wh, ww))
    out = torch.empty(o.shape, dtype=torch.uint8, pin_memory=True)
    back = composite_frames(o[None], e[None].to(DEV), a[None], plan=plan, out=out[None])      # host original and alpha, a batch of one
    assert back.data_ptr() == out.data_ptr() and torch.equal(out, want)
    with pytest.raises(ValueError, match="out"):
        composite_frames(o.to(DEV), e.to(DEV), a.to(DEV), plan, out=torch.empty(2, 3, 3, 3, dtype=torch.uint8))


def test_keep_unedited_end_to_end():
    """A 2 x 135 x 240 clip through fit_frames, an "edit" that repaints a 10 x 14 block of the fitted frames: every byte of the result
    farther from the block (mapped into the original) than the mask can reach is the original's, and the block's centre is not."""
    g = torch.Generator().manual_seed(9)
    orig = torch.randint(0, 256, (2, 135, 240, 3), generator=g, dtype=torch.uint8)
    src, plan = fit_frames(orig.to(DEV), 48, 80)
    edit = src.clone()
    by, bx, bh, bw = 20, 30, 10, 14
    edit[:, by:by + bh, bx:bx + bw] = 255 - edit[:, by:by + bh, bx:bx + bw]
    kw = dict(threshold=THRESHOLD, smooth=1, grow=3, grow_t=1, feather=2)
    got = keep_unedited(orig, src, edit, plan, **kw)
    alpha = reference_change_mask(src.cpu(), edit.cpu(), **kw)
    assert torch.equal(got.cpu(), reference_composite_frames(orig, edit.cpu(), alpha, plan))
    # alpha can be non-zero within smooth + grow + feather = 6 fitted pixels of the block; one more for the filter's support, then
    # the fitted rectangle mapped into the original (scale = original / fitted inside the window) and rounded outwards
    y, x, wh, ww = plan.source_window
    reach = 7
    sy, sx = wh / 48, ww / 80
    y0, y1 = y + int(np.floor((by - reach) * sy)) - 1, y + int(np.ceil((by + bh + reach) * sy)) + 1
    x0, x1 = x + int(np.floor((bx - reach) * sx)) - 1, x + int(np.ceil((bx + bw + reach) * sx)) + 1
    far = torch.ones(135, 240, dtype=torch.bool)
    far[y0:y1, x0:x1] = False
    assert int(far.sum()) > 135 * 240 // 2
    assert torch.equal(got.cpu()[:, far], orig[:, far])
    cy, cx = y + int((by + bh / 2) * sy), x + int((bx + bw / 2) * sx)
    assert not torch.equal(got.cpu()[:, cy, cx], orig[:, cy, cx])
    out = torch.empty(orig.shape, dtype=torch.uint8, pin_memory=True)
    assert torch.equal(keep_unedited(orig, src, edit, plan, out=out, **kw), got.cpu())
