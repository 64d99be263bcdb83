"""Host side of the writer's grid and the compare clip (videocof_amd/video_io.py ``grid_frames`` / ``compare_frames``), no GPU.

The GPU tests (tests/test_gpu_frame_compose.py) compare ``wan_frames_u8_compose`` with ``reference_grid_frames`` /
``reference_compare_frames``, torch restatements of the reference's host code.  Here those restatements are pinned to the
reference itself: where its tree is present, ``_normalize_to_01`` (fast_infer.py:183-189), the body of ``save_side_by_side``
(fast_infer.py:194-204) and the writer's loop (videox_fun/utils/utils.py:60-67) are read from it and executed as they stand;
everywhere, they are compared with tests/golden/video_compose_ref.npz, recorded from those statements by
``record_video_compose_golden.py`` beside this file.  ``torchvision.utils.make_grid`` is taken from torchvision where it can be
imported; otherwise ``make_grid`` below stands in for it and the layout formula of its documentation (``xmaps = min(nrow, B)``,
cells of ``(H + 2, W + 2)``, a ``2``-pixel border of zeros) is the definition.  Equality throughout."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_video_io_host import (boundary_video, reference_lines, reference_present, run_reference_loader)  # noqa: E402
from videocof_amd import _lib, ops, video_io  # noqa: E402
from videocof_amd.video_io import grid_layout, reference_compare_frames, reference_grid_frames  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "video_compose_ref.npz")


def make_grid(tensor, nrow=8, padding=2, pad_value=0.0):
    """Stand-in for torchvision.utils.make_grid on a [B, 3, H, W] tensor, from its documented layout."""
    assert tensor.dim() == 4 and tensor.shape[1] == 3
    if tensor.shape[0] == 1:
        return tensor[0]
    nmaps = tensor.shape[0]
    xmaps = min(nrow, nmaps)
    ymaps = -(-nmaps // xmaps)
    height, width = tensor.shape[2] + padding, tensor.shape[3] + padding
    grid = tensor.new_full((3, height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid[:, y * height + padding:(y + 1) * height, x * width + padding:(x + 1) * width] = tensor[k]
            k += 1
    return grid


def torchvision_or_stand_in():
    try:
        import torchvision
        return torchvision
    except ImportError:
        return types.SimpleNamespace(utils=types.SimpleNamespace(make_grid=make_grid))


def run_reference_grid(videos_bcthw: torch.Tensor, rescale=False, n_rows=6) -> np.ndarray:
    """utils.py:60-67 on float32 [B, 3, T, H, W] -> uint8 [T, Hg, Wg, 3]: line 60, then the loop body 63-67 per frame."""
    from einops import rearrange
    ns = {"torch": torch, "np": np, "rearrange": rearrange, "torchvision": torchvision_or_stand_in(), "videos": videos_bcthw,
          "n_rows": n_rows, "rescale": rescale}
    exec(reference_lines("videox_fun/utils/utils.py", 60, 60), ns)
    body = reference_lines("videox_fun/utils/utils.py", 63, 67)
    outputs = []
    for x in ns["videos"]:
        ns["x"] = x
        exec(body, ns)
        outputs.append(ns["x"])
    return np.stack(outputs)


def reference_namespace():
    """``_normalize_to_01`` as the reference defines it (fast_infer.py:183-189)."""
    ns = {"torch": torch}
    exec(reference_lines("fast_infer.py", 183, 189), ns)
    return ns


def run_reference_compare(input_tensor: torch.Tensor, sample_tensor: torch.Tensor) -> np.ndarray:
    """fast_infer.py:194-204 on two float32 [1, 3, T, H, W] videos, then the writer: uint8 [T', H', 2 W', 3]."""
    ns = reference_namespace()
    ns.update(input_tensor=input_tensor, sample_tensor=sample_tensor)
    exec(reference_lines("fast_infer.py", 194, 204), ns)
    return run_reference_grid(ns["combined"])


def inputs():
    """The inputs of the pin, drawn from a fixed seed (the recorder stores them beside what the reference makes of them)."""
    g = torch.Generator().manual_seed(2025)
    src = torch.randint(0, 256, (5, 20, 30, 3), generator=g, dtype=torch.uint8)
    src.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)                       # every byte value
    edit_unit = torch.rand(1, 3, 3, 18, 27, generator=g)                            # what decode_latents returns: [0, 1]
    edit_unit.view(-1)[:4] = torch.tensor([0.0, 1.0, 254.0 / 255.0, 1.0 / 255.0])
    high = torch.randint(128, 256, (2, 6, 7, 3), generator=g, dtype=torch.uint8)    # no byte < 128: the loader's video is >= 0
    grid_unit = torch.rand(3, 3, 2, 6, 7, generator=g)
    grid_pm1 = torch.rand(7, 3, 2, 4, 5, generator=g) * 2 - 1
    inside = torch.rand(1, 3, 2, 6, 7, generator=g)
    below = inside.clone()
    below[0, 1, 1, 2, 3] = -1e-3
    above = inside.clone()
    above[0, 2, 0, 5, 6] = 1 + 1e-3
    nan = below.clone()
    nan[0, 0, 0, 0, 0] = float("nan")
    nan[0, 0, 0, 0, 1] = -1.0
    return dict(src=src, edit_unit=edit_unit, high=high, grid_unit=grid_unit, grid_pm1=grid_pm1, inside=inside, below=below,
                above=above, nan=nan)


def reference_outputs(x):
    """What the reference's statements make of ``inputs()`` (needs the reference tree)."""
    loader = lambda fr: run_reference_loader(fr.numpy())
    norm = reference_namespace()["_normalize_to_01"]
    out = dict(
        compare_u8=run_reference_compare(loader(x["src"]), x["edit_unit"]),
        compare_high=run_reference_compare(loader(x["high"]), x["inside"]),
        edit_bytes=run_reference_grid(x["edit_unit"]),
        grid_unit_2=run_reference_grid(x["grid_unit"], False, 2), grid_unit_6=run_reference_grid(x["grid_unit"], False, 6),
        grid_pm1_2=run_reference_grid(x["grid_pm1"], True, 2), grid_pm1_6=run_reference_grid(x["grid_pm1"], True, 6))
    for name in ("inside", "below", "above", "nan"):
        out["compare_" + name] = run_reference_compare(x[name], x["inside"])
        out["norm_" + name] = norm(x[name]).numpy()
    allb = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    out["byte_map"] = run_reference_compare(loader(allb), torch.zeros(1, 3, 1, 16, 16))[0, :, :16, 0].reshape(-1)
    out["bytes_moved"] = np.nonzero(out["byte_map"] != np.arange(256))[0].astype(np.int32)
    return out


def check_restatements(x, want):
    edit_u8 = torch.from_numpy(want["edit_bytes"])[None]                                   # uint8 [1, T, H, W, 3], the writer's bytes
    assert np.array_equal(reference_grid_frames(x["edit_unit"]).numpy(), want["edit_bytes"])
    for edit in (x["edit_unit"], edit_u8):                                                 # float edit, and its bytes placed as they are
        got = reference_compare_frames(x["src"][None], edit)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 3, 18, 54, 3)
        assert np.array_equal(got[0].numpy(), want["compare_u8"])
    assert np.array_equal(reference_compare_frames(x["high"][None], x["inside"])[0].numpy(), want["compare_high"])
    for name in ("inside", "below", "above", "nan"):
        got, ref = reference_compare_frames(x[name], x["inside"])[0].numpy().copy(), np.array(want["compare_" + name])
        if name == "nan":                                   # the byte a NaN becomes is the C cast's business, not the writer's
            got[0, 0, 0, 0] = ref[0, 0, 0, 0] = 0
        assert np.array_equal(got, ref), name
        assert np.array_equal(video_io._reference_normalize_to_01(x[name]).numpy(), want["norm_" + name], equal_nan=True), name
    for n_rows in (2, 6):
        assert np.array_equal(reference_grid_frames(x["grid_unit"], False, n_rows).numpy(), want[f"grid_unit_{n_rows}"])
        assert np.array_equal(reference_grid_frames(x["grid_pm1"], True, n_rows).numpy(), want[f"grid_pm1_{n_rows}"])


def test_restatements_equal_the_reference_statements():
    if not reference_present():
        pytest.skip("reference tree not present: see test_restatements_equal_the_recorded_fixture")
    x = inputs()
    check_restatements(x, reference_outputs(x))


def test_restatements_equal_the_recorded_fixture(golden):
    """The same pin for a checkout without the reference: the inputs are redrawn and must be the recorded ones."""
    g = golden("video_compose_ref")
    x = inputs()
    for name, t in x.items():
        assert np.array_equal(t.numpy(), g["in_" + name], equal_nan=True), name
    check_restatements(x, g)


def test_range_rule_with_a_nan_takes_no_rescale(golden):
    """float(video.min()) of a tensor with a NaN is NaN and `nan < 0.0`, `nan > 1.0` are both false: -1.0 beside a NaN is clamped
    to 0, not rescaled to 0 -- and 0.25 stays 0.25 instead of becoming 0.625."""
    v = torch.tensor([float("nan"), -1.0, 0.25]).view(1, 1, 3, 1, 1).expand(1, 3, 3, 1, 1).contiguous()
    got = video_io._reference_normalize_to_01(v)[0, 0, :, 0, 0]
    assert torch.isnan(got[0]) and got[1:].tolist() == [0.0, 0.25]
    g = golden("video_compose_ref")
    assert np.isnan(g["norm_nan"][0, 0, 0, 0, 0]) and g["norm_nan"][0, 0, 0, 0, 1] == 0.0
    assert g["norm_below"][0, 1, 1, 2, 3] == np.float32((np.float32(-1e-3) + np.float32(1.0)) / np.float32(2.0))
    assert np.array_equal(g["norm_inside"], g["in_inside"])


def test_loader_roundtrip_moves_bytes(golden):
    """The left half of the compare clip over all 256 byte values against the float32 chain written out in numpy: it is NOT the
    identity, which is what an implementation that concatenates the source's bytes would show."""
    u = np.arange(256, dtype=np.uint8)
    v = u.astype(np.float32) * np.float32(2.0 / 255.0) - np.float32(1.0)                      # fast_infer.py:88-90
    unit = np.clip((v + np.float32(1.0)) / np.float32(2.0), np.float32(0.0), np.float32(1.0))   # _normalize_to_01, min < 0
    chain = (unit * np.float32(255.0)).astype(np.uint8)                                       # utils.py:67
    assert unit.dtype == np.float32
    frames = torch.from_numpy(u).view(1, 1, 16, 16, 1).expand(1, 1, 16, 16, 3).contiguous()
    edit = torch.zeros(1, 1, 16, 16, 3, dtype=torch.uint8)
    got = reference_compare_frames(frames, edit)
    for c in range(3):
        assert np.array_equal(got[0, 0, :, :16, c].reshape(-1).numpy(), chain)
    assert int(got[0, 0, :, 16:].max()) == 0
    moved = np.nonzero(chain != u)[0]
    g = golden("video_compose_ref")
    assert np.array_equal(chain, g["byte_map"]) and np.array_equal(moved, g["bytes_moved"])
    assert len(moved) > 0 and np.all(chain[moved] == u[moved] - 1)                            # a truncation: one below, never above
    concatenated = torch.cat([frames, edit], dim=3)
    assert not torch.equal(concatenated, got)


@pytest.mark.parametrize("n_rows", [2, 6])
@pytest.mark.parametrize("B", [1, 2, 6, 7])
def test_grid_geometry(B, n_rows):
    T, H, W = 2, 3, 5
    videos = ((torch.arange(B * 3 * T * H * W, dtype=torch.float32) % 251 + 1) / 255.0).view(B, 3, T, H, W)     # no zero inside a sample
    hg, wg, cells = grid_layout(B, H, W, n_rows)
    got = reference_grid_frames(videos, n_rows=n_rows)
    if B == 1:
        assert (hg, wg, cells) == (H, W, [(0, 0)])
    else:
        xmaps = min(n_rows, B)
        ymaps = -(-B // xmaps)
        assert (hg, wg) == (ymaps * (H + 2) + 2, xmaps * (W + 2) + 2)
        assert cells == [(2 + (k // xmaps) * (H + 2), 2 + (k % xmaps) * (W + 2)) for k in range(B)]
    assert got.dtype == torch.uint8 and tuple(got.shape) == (T, hg, wg, 3)
    covered = torch.zeros(hg, wg, dtype=torch.bool)
    for k, (y, x) in enumerate(cells):
        want = (videos[k] * 255).permute(1, 2, 3, 0).to(torch.uint8)
        assert torch.equal(got[:, y:y + H, x:x + W], want), k
        assert not covered[y:y + H, x:x + W].any()
        covered[y:y + H, x:x + W] = True
    assert int(got[:, ~covered].max() if (~covered).any() else 0) == 0                        # border and unused cells
    assert int(got[:, covered].min()) > 0
    # the stand-in / torchvision's own make_grid, frame by frame
    mg = torchvision_or_stand_in().utils.make_grid
    for t in range(T):
        frame = (mg(videos[:, :, t], nrow=n_rows).permute(1, 2, 0) * 255).numpy().astype(np.uint8)
        assert np.array_equal(got[t].numpy(), frame)
    # uint8 frames are laid out as bytes
    u8 = (videos * 255).permute(0, 2, 3, 4, 1).to(torch.uint8).contiguous()
    assert torch.equal(reference_grid_frames(u8, n_rows=n_rows), got)


def test_boundary_video_is_shared_with_the_frame_io_tests():
    v = boundary_video()
    assert v.dtype == torch.bfloat16 and v.shape[:2] == (1, 3) and float(v.float().min()) == -1.5


def test_cpu_tensors_and_wrong_dtypes_raise():
    f32 = torch.zeros(2, 3, 2, 4, 4)
    u8 = torch.zeros(2, 2, 4, 4, 3, dtype=torch.uint8)
    for call in (lambda: video_io.grid_frames(f32), lambda: video_io.grid_frames(u8), lambda: video_io.compare_frames(u8, u8),
                 lambda: video_io.compare_frames(f32, f32), lambda: ops.video_range_flag(f32),
                 lambda: ops.frames_u8_compose(u8[0], [])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="expected float32 / bfloat16"):
        video_io.grid_frames(f32.half())
    with pytest.raises(ValueError, match="expected float32 / bfloat16"):
        video_io.compare_frames(u8, f32.double())
    with pytest.raises(ValueError, match="expected float32 / bfloat16"):
        video_io.grid_frames(torch.zeros(2, 4, 2, 4, 4))                                       # four channels
    with pytest.raises(ValueError, match="expected float32 / bfloat16"):
        video_io.compare_frames(u8[0], u8)                                                     # no batch axis
    with pytest.raises(ValueError, match="expected uint8, float32 or bfloat16"):
        ops.video_range_flag(f32.half())
    with pytest.raises(ValueError, match="grid_layout"):
        grid_layout(0, 4, 4)


class _NeverCalled:
    device = torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError(f"the pipeline touched .{name} before it checked `compare`")


def test_pipeline_compare_needs_uint8_frames_in_and_out():
    from videocof_amd import WanPipeline, WanPipelineOutput
    assert WanPipelineOutput(videos=None).compare_videos is None
    pipe = WanPipeline(transformer=_NeverCalled(), scheduler=_NeverCalled())
    frames = torch.zeros(9, 32, 48, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="needs the uint8 source frames"):
        pipe(video=torch.zeros(1, 3, 9, 32, 48), output_type="uint8", compare=True)
    with pytest.raises(ValueError, match="needs the uint8 source frames"):
        pipe(video=None, source_latents=torch.zeros(1, 16, 3, 4, 6), output_type="uint8", compare=True)
    for output_type in ("latent", "numpy"):
        with pytest.raises(ValueError, match="needs output_type='uint8'"):
            pipe(video=frames, output_type=output_type, compare=True)


def _src(**kw):
    d = dict(base=4096, extent=4 * 6 * 8 * 3, stride_c=1, stride_t=6 * 8 * 3, stride_y=8 * 3, stride_x=3, kind=_lib.COMPOSE_U8,
             mode=_lib.COMPOSE_COPY, t0=0, y0=0, x0=0, nt=4, h=6, w=8, dst_y=0, dst_x=0)
    d.update(kw)
    s = _lib.ComposeSrc()
    for k, v in d.items():
        setattr(s, k, v)
    return s


def test_the_library_validates_the_geometry_before_it_launches():
    """Windows that leave their tensor, rectangles that leave the canvas or overlap, modes that do not go with the kind: an error
    code before anything is enqueued (the pointers here are never dereferenced)."""
    lib = _lib.load()
    assert {"wan_frames_u8_compose", "wan_video_range_flag"} <= set(_lib.SIGNATURES) and _lib.ABI_VERSION == 11
    assert ctypes.sizeof(_lib.ComposeSrc) == 104 and _lib.ComposeSrc.kind.offset == 56 and _lib.ComposeSrc.dst_x.offset == 96

    def call(srcs, canvas=4096, T=4, H=6, W=16, pad=0):
        arr = (_lib.ComposeSrc * max(len(srcs), 1))(*srcs)
        return lib.wan_frames_u8_compose(arr, len(srcs), canvas, T, H, W, pad, None)

    INV, UNS = _lib.WAN_ERR_INVALID, _lib.WAN_ERR_UNSUPPORTED
    assert call([_src()], canvas=None) == INV
    assert call([_src(base=None)]) == INV
    assert call([_src(nt=5)]) == INV                                    # frames [0, 5) of 4
    assert call([_src(t0=1)]) == INV
    assert call([_src(y0=1)]) == INV and call([_src(x0=1)]) == INV
    assert call([_src(extent=4 * 6 * 8 * 3 - 1)]) == INV                # the last byte is outside
    assert call([_src(x0=-1, w=4)]) == INV and call([_src(w=0)]) == INV
    assert call([_src(dst_x=9)]) == INV and call([_src(dst_y=1)]) == INV and call([_src(dst_x=-1)]) == INV
    assert call([_src()], T=3) == INV                                   # more frames than the canvas has
    assert call([_src(), _src(dst_x=7)]) == INV                         # overlap
    with pytest.raises(ValueError, match="overlap"):
        _lib.check(call([_src(), _src(dst_x=7)]), "wan_frames_u8_compose")
    assert call([_src(mode=_lib.COMPOSE_WRITER)]) == INV and call([_src(kind=_lib.COMPOSE_F32)]) == INV
    assert call([_src(kind=3)]) == INV and call([_src(mode=4)]) == INV
    assert call([_src(kind=_lib.COMPOSE_F32, mode=_lib.COMPOSE_NORMALIZE, extent=1 << 20)]) == INV      # no flag
    assert call([_src(rescale_flag=4096)]) == INV                       # COPY takes none
    assert call([_src(stride_y=-24)]) == UNS
    assert call([_src()] * 17) == UNS
    with pytest.raises(RuntimeError, match="at most 16"):
        _lib.check(call([_src()] * 17), "wan_frames_u8_compose")
    assert call([_src()], T=70000) == UNS
    assert call([_src()], pad=256) == INV
    assert lib.wan_video_range_flag(None, 1, 16, None, None) == INV
    assert lib.wan_video_range_flag(4096, 3, 16, 4096, None) == INV
    assert lib.wan_video_range_flag(4096, 1, 0, 4096, None) == INV
