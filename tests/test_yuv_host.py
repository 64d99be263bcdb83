"""The YCbCr definition and the .y4m reader / writer, on the host.

The integer definition is checked over ALL 2^24 colours for both matrices and both ranges (the properties it was chosen for), against
Pillow where Pillow is installed, and through 4:2:0 on flat images.  ``read_y4m`` is given files assembled byte by byte from header
literals -- never made with the writer -- and ``write_y4m`` / ``load_y4m_frames`` run with the two device ops replaced by the numpy
references, so the layout, header, staging and frame-selection code is what is under test here; the kernels themselves are
tests/test_gpu_yuv.py."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from videocof_amd import _lib, ops, video_io
from videocof_amd.video_io import (chroma_shape, load_video_frames, read_y4m, reference_frames_to_yuv, reference_yuv_to_frames,
                                   select_frame_indices, write_y4m, y4m_frame_bytes, yuv_matrix, load_y4m_frames)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [("bt601", True), ("bt601", False), ("bt709", True), ("bt709", False)]


def all_colours(chunk):
    """Chunk ``chunk`` of 16 of the 2^24 colours as a [1, 1024, 1024, 3] frame."""
    v = np.arange(chunk << 20, (chunk + 1) << 20, dtype=np.uint32)
    rgb = np.stack([v >> 16, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8)
    return torch.from_numpy(rgb.reshape(1, 1024, 1024, 3))


# ------------------------------------------------------------------ the tables
def test_tables_follow_the_definition():
    for matrix, full in COMBOS:
        fwd, inv = yuv_matrix(matrix, full)
        assert fwd.dtype == inv.dtype == np.int64 and fwd.shape == inv.shape == (3, 3)
        ys = 255 if full else 219
        assert fwd.sum(axis=1).tolist() == [int(np.rint(ys / 255 * 65536)), 0, 0]
        assert inv[0, 1] == 0 and inv[2, 2] == 0 and inv[0, 0] == inv[1, 0] == inv[2, 0] == int(np.rint(255 / ys * 65536))
        assert int(np.abs(inv).max()) < 1 << 23 and int(np.abs(fwd).max()) < 1 << 23       # 24-bit multiplies on the device
        # every sum of the way in fits an int32 with room to spare
        assert int(np.abs(inv).sum(axis=1).max()) * 255 + (1 << 15) < 1 << 31
    kr, kb = 0.299, 0.114
    fwd, inv = yuv_matrix("bt601", True)
    assert fwd[0].tolist() == [19595, 38470, 7471] and fwd[1, 2] == fwd[2, 0] == 32768
    assert inv[0, 2] == int(np.rint(2 * (1 - kr) * 65536)) and inv[2, 1] == int(np.rint(2 * (1 - kb) * 65536))
    with pytest.raises(ValueError, match="matrix"):
        yuv_matrix("bt2020", True)


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_properties_over_all_colours(matrix, full):
    """Ranges, exact greys and the 4:4:4 round trip over all 2^24 colours."""
    # full range: within [0, 255] without the clamp -- the lowest chroma is 128 - 127.5 = 0.5, which rounds up to 1
    lo_y, hi_y, lo_c, hi_c = (0, 255, 1, 255) if full else (16, 235, 16, 240)
    worst, above_one, ymin, ymax, cmin, cmax = 0, 0, 255, 0, 255, 0
    for chunk in range(16):
        rgb = all_colours(chunk)
        y, cb, cr = reference_frames_to_yuv(rgb, chroma="444", matrix=matrix, full_range=full)
        ymin, ymax = min(ymin, int(y.min())), max(ymax, int(y.max()))
        cmin, cmax = min(cmin, int(cb.min()), int(cr.min())), max(cmax, int(cb.max()), int(cr.max()))
        back = reference_yuv_to_frames(y, cb, cr, chroma="444", matrix=matrix, full_range=full)
        err = (back.to(torch.int16) - rgb.to(torch.int16)).abs().amax(dim=-1)
        worst = max(worst, int(err.max()))
        above_one += int((err > 1).sum())
    print(f"{matrix} full={full}: Y [{ymin}, {ymax}] C [{cmin}, {cmax}] round trip max {worst}, > 1 level for {above_one / 2 ** 24:.4%}")
    assert (ymin, ymax, cmin, cmax) == (lo_y, hi_y, lo_c, hi_c)
    if full:
        assert worst <= 1
    else:
        assert worst <= 2 and above_one < 0.008 * 2 ** 24


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_every_grey_has_neutral_chroma(matrix, full):
    v = torch.arange(256, dtype=torch.uint8)
    y, cb, cr = reference_frames_to_yuv(v.view(1, 1, 256, 1).expand(1, 1, 256, 3), chroma="444", matrix=matrix, full_range=full)
    assert torch.all(cb == 128) and torch.all(cr == 128)
    assert int(y[0, 0, 0]) == (0 if full else 16) and int(y[0, 0, 255]) == (255 if full else 235)
    assert torch.all(y[0, 0, 1:].int() >= y[0, 0, :-1].int())


def test_bt601_full_range_is_pillows_ycbcr_within_one_level():
    Image = pytest.importorskip("PIL.Image")
    worst = 0
    for chunk in range(16):
        rgb = all_colours(chunk)
        y, cb, cr = reference_frames_to_yuv(rgb, chroma="444", matrix="bt601", full_range=True)
        pil = np.asarray(Image.fromarray(rgb[0].numpy(), "RGB").convert("YCbCr")).astype(np.int16)
        ours = torch.stack([y[0], cb[0], cr[0]], dim=-1).numpy().astype(np.int16)
        worst = max(worst, int(np.abs(ours - pil).max()))
    print(f"bt601 full range vs Pillow over 2^24 colours: max difference {worst}")
    assert worst <= 1                                                          # Pillow truncates where the definition rounds


@pytest.mark.parametrize("size", [(23, 37), (2, 2), (1, 5)])
def test_flat_image_through_420_and_back(size):
    """Averaging and interpolating equal values are exact: a flat image through 4:2:0 is its colour through 4:4:4, for both sitings."""
    h, w = size
    g = torch.Generator().manual_seed(h * 100 + w)
    colours = torch.cat([torch.randint(0, 256, (60, 3), generator=g, dtype=torch.uint8),
                         torch.tensor([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 0, 255]], dtype=torch.uint8)])
    flat = colours.view(-1, 1, 1, 3).expand(-1, h, w, 3).contiguous()
    for matrix, full in COMBOS:
        y, cb, cr = reference_frames_to_yuv(flat, chroma="420jpeg", matrix=matrix, full_range=full)
        assert tuple(cb.shape) == (len(colours), (h + 1) // 2, (w + 1) // 2)
        y4, cb4, cr4 = reference_frames_to_yuv(flat, chroma="444", matrix=matrix, full_range=full)
        want = reference_yuv_to_frames(y4, cb4, cr4, chroma="444", matrix=matrix, full_range=full)
        for siting in ("420jpeg", "420mpeg2"):
            back = reference_yuv_to_frames(y, cb, cr, chroma=siting, matrix=matrix, full_range=full)
            assert torch.equal(back, want)
            assert int((back.int() - flat.int()).abs().max()) <= (1 if full else 2)


def test_chroma_taps_of_the_definition():
    """The weights of the section, spelled out on a ramp: 4:2:0 centred and left co-sited, 4:2:2, odd widths, mono."""
    c = np.array([[[0, 16, 32]]], dtype=np.uint8)                               # one chroma row of 3 samples: a 1 x 5 and a 1 x 6 frame
    y = np.full((1, 1, 6), 128, np.uint8)
    _, inv = yuv_matrix("bt601", True)

    def cb_of(chroma, w):
        rgb = reference_yuv_to_frames(y[:, :, :w], c, np.full_like(c, 128), chroma=chroma, matrix="bt601", full_range=True).numpy().astype(np.int64)
        return rgb[0, 0, :, 2]                                                  # B = clamp(128 + (inv[2, 1] * (Cb - 128) + 2^15) >> 16)

    def blue(cb):
        return [int(np.clip(((128 << 16) + inv[2, 1] * (v - 128) + (1 << 15)) >> 16, 0, 255)) for v in cb]

    # vertical taps on a single chroma row are 1 + 3 of the same sample: horizontal only
    assert cb_of("420jpeg", 6).tolist() == blue([0, 4, 12, 20, 28, 32])         # (1, 3) / (3, 1) quarters, the borders clamped
    assert cb_of("420mpeg2", 6).tolist() == blue([0, 8, 16, 24, 32, 32])        # (4) / (2, 2)
    assert cb_of("422", 6).tolist() == blue([0, 8, 16, 24, 32, 32])
    assert cb_of("420jpeg", 5).tolist() == blue([0, 4, 12, 20, 28])
    assert cb_of("420", 5).tolist() == cb_of("420jpeg", 5).tolist()
    mono = reference_yuv_to_frames(y, chroma="mono", matrix="bt601", full_range=True)
    assert torch.all(mono == 128)
    assert chroma_shape(5, 7, "420jpeg") == (3, 4) and chroma_shape(5, 7, "422") == (5, 4) and chroma_shape(5, 7, "444") == (5, 7)
    assert chroma_shape(5, 7, "mono") == (0, 0) and y4m_frame_bytes(5, 7, "420") == 35 + 24
    # the way down: odd sizes repeat the last column and row
    rgb = torch.zeros(1, 3, 3, 3, dtype=torch.uint8)
    rgb[0, 2, 2, 2] = 255                                                        # one blue pixel in the corner
    _, cb, _ = reference_frames_to_yuv(rgb, chroma="420jpeg", matrix="bt601", full_range=True)
    px = reference_frames_to_yuv(rgb, chroma="444", matrix="bt601", full_range=True)[1]
    assert tuple(cb.shape) == (1, 2, 2) and int(cb[0, 1, 1]) == int(px[0, 2, 2]) and int(cb[0, 0, 0]) == 128


# ------------------------------------------------------------------ read_y4m on hand-assembled files
def planes(t, h, w, chroma, seed=0):
    rng = np.random.default_rng(seed)
    ch, cw = chroma_shape(h, w, chroma)
    y = rng.integers(0, 256, (t, h, w), dtype=np.uint8)
    if ch == 0:
        return y, None, None
    return y, rng.integers(0, 256, (t, ch, cw), dtype=np.uint8), rng.integers(0, 256, (t, ch, cw), dtype=np.uint8)


def assemble(header, ps, marker=b"FRAME\n"):
    out = [header]
    for t in range(ps[0].shape[0]):
        out.append(marker(t) if callable(marker) else marker)
        out += [p[t].tobytes() for p in ps if p is not None]
    return b"".join(out)


@pytest.mark.parametrize("tag,chroma", [(b" C420jpeg", "420jpeg"), (b" C420mpeg2", "420mpeg2"), (b" C420", "420jpeg"), (b"", "420jpeg"),
                                        (b" C422", "422"), (b" C444", "444"), (b" Cmono", "mono")])
def test_read_y4m_accepts_every_supported_tag(tmp_path, tag, chroma):
    ps = planes(3, 5, 7, chroma, seed=len(tag))                                 # odd sizes: chroma planes round up
    path = tmp_path / "clip.y4m"
    path.write_bytes(assemble(b"YUV4MPEG2 W7 H5 F30000:1001 Ip A1:1" + tag + b"\n", ps))
    clip = read_y4m(path)
    assert (clip.width, clip.height, clip.frames, clip.chroma) == (7, 5, 3, chroma)
    assert clip.fps == Fraction(30000, 1001) and clip.full_range is None and clip.aspect == "1:1"
    assert clip.frame_bytes == sum(p[0].size for p in ps if p is not None)
    assert isinstance(clip.data, np.memmap)
    for t in range(3):
        got = clip.planes(t)
        for g, p in zip(got, ps):
            assert (g is None and p is None) or (np.shares_memory(g, clip.data) and np.array_equal(g, p[t]))


def test_read_y4m_frame_lines_with_parameters_and_the_range_tag(tmp_path):
    ps = planes(4, 6, 10, "420jpeg", seed=3)
    path = tmp_path / "params.y4m"
    path.write_bytes(assemble(b"YUV4MPEG2 H6 W10 F25:1 I? XYSCSS=420JPEG XCOLORRANGE=FULL\n", ps,
                              marker=lambda t: b"FRAME\n" if t % 2 else b"FRAME Ip Xframe=%d\n" % t))
    clip = read_y4m(path)
    assert (clip.width, clip.height, clip.frames, clip.full_range, clip.fps) == (10, 6, 4, True, Fraction(25))
    assert len(set(np.diff(clip.offsets).tolist())) > 1                          # the markers differ in length: found by parsing
    for t in range(4):
        for g, p in zip(clip.planes(t), ps):
            assert np.array_equal(g, p[t])
    limited = tmp_path / "limited.y4m"
    limited.write_bytes(assemble(b"YUV4MPEG2 W10 H6 F25:1 XCOLORRANGE=LIMITED\n", ps))
    assert read_y4m(limited).full_range is False
    empty = tmp_path / "empty.y4m"
    empty.write_bytes(b"YUV4MPEG2 W10 H6 F25:1\n")
    assert read_y4m(empty).frames == 0


@pytest.mark.parametrize("header,message", [(b"YUV4MPEG2 W8 H4 F25:1 It C420jpeg\n", "interlaced"),
                                            (b"YUV4MPEG2 W8 H4 F25:1 Ib\n", "interlaced"),
                                            (b"YUV4MPEG2 W8 H4 F25:1 Im\n", "interlaced"),
                                            (b"YUV4MPEG2 W8 H4 F25:1 Ip C420p10\n", "more than 8 bits"),
                                            (b"YUV4MPEG2 W8 H4 F25:1 Ip C444p12\n", "more than 8 bits"),
                                            (b"YUV4MPEG2 W8 H4 F25:1 Ip Cmono16\n", "more than 8 bits"),
                                            (b"YUV4MPEG2 W8 H4 F25:1 Ip C411\n", "C411"),
                                            (b"YUV4MPEG2 W8 H4 F25:1 Ip C420paldv\n", "C420paldv"),
                                            (b"YUV4MPEG3 W8 H4 F25:1\n", "bad magic"),
                                            (b"RIFF\x00\x00\x00\x00AVI LIST\n", "bad magic"),
                                            (b"YUV4MPEG2 W8 F25:1\n", "W / H")])
def test_read_y4m_rejects(tmp_path, header, message):
    path = tmp_path / "bad.y4m"
    path.write_bytes(header + b"FRAME\n" + bytes(8 * 4 * 3))
    with pytest.raises(ValueError, match=message):
        read_y4m(path)


def test_read_y4m_rejects_a_truncated_last_frame(tmp_path):
    ps = planes(2, 4, 8, "420jpeg")
    whole = assemble(b"YUV4MPEG2 W8 H4 F25:1 Ip C420jpeg\n", ps)
    path = tmp_path / "cut.y4m"
    path.write_bytes(whole[:-5])
    with pytest.raises(ValueError, match="frame 1 is truncated"):
        read_y4m(path)
    path.write_bytes(whole + b"FRAM")
    with pytest.raises(ValueError, match="no FRAME line"):
        read_y4m(path)
    path.write_bytes(whole)
    assert read_y4m(path).frames == 2


# ------------------------------------------------------------------ the writer and the loader, device ops replaced by the references
def _which(table, index):
    for matrix, full in COMBOS:
        if yuv_matrix(matrix, full)[index].ravel().tolist() == list(table):
            return matrix, full
    raise AssertionError("coefficients of no known matrix")


@pytest.fixture
def host_ops(monkeypatch):
    """``ops.yuv_to_frames_u8`` / ``ops.frames_u8_to_yuv`` as the numpy references on host tensors; records what was asked for."""
    calls = []

    def to_frames(y, cb, cr, sub_x, sub_y, cosited, inverse, yo, out=None):
        matrix, full = _which(inverse, 1)
        chroma = "mono" if cb is None else {(True, True, False): "420jpeg", (True, True, True): "420mpeg2", (True, False, True): "422",
                                            (False, False, False): "444"}[(sub_x, sub_y, cosited)]
        calls.append(("in", chroma, matrix, full, tuple(y.shape)))
        return reference_yuv_to_frames(y, cb, cr, chroma=chroma, matrix=matrix, full_range=full)

    def to_yuv(frames, y, cb, cr, subsampled, forward, yo):
        matrix, full = _which(forward, 0)
        calls.append(("out", "420jpeg" if subsampled else "444", matrix, full, tuple(frames.shape)))
        for dst, src in zip((y, cb, cr), reference_frames_to_yuv(frames, chroma="420jpeg" if subsampled else "444", matrix=matrix,
                                                                 full_range=full)):
            dst.copy_(src)

    monkeypatch.setattr(ops, "yuv_to_frames_u8", to_frames)
    monkeypatch.setattr(ops, "frames_u8_to_yuv", to_yuv)
    monkeypatch.setattr(video_io, "_default_device", lambda: torch.device("cpu"))
    return calls


@pytest.mark.parametrize("chroma,size,full", [("420", (5, 7), False), ("420jpeg", (6, 8), True), ("444", (5, 7), False)])
def test_write_then_read_returns_the_planes(tmp_path, host_ops, chroma, size, full):
    h, w = size
    frames = torch.randint(0, 256, (3, h, w, 3), generator=torch.Generator().manual_seed(w), dtype=torch.uint8)
    path = tmp_path / "out.y4m"
    write_y4m(path, frames, fps=Fraction(24000, 1001), chroma=chroma, full_range=full)
    raw = path.read_bytes()
    name = "444" if chroma == "444" else "420jpeg"
    header = f"YUV4MPEG2 W{w} H{h} F24000:1001 Ip A1:1 C{name}" + (" XCOLORRANGE=FULL" if full else "") + "\n"
    assert raw.startswith(header.encode()) and raw[len(header):len(header) + 6] == b"FRAME\n"
    assert len(raw) == len(header) + 3 * (6 + y4m_frame_bytes(h, w, name))
    clip = read_y4m(path)
    assert (clip.width, clip.height, clip.frames, clip.chroma, clip.fps) == (w, h, 3, name, Fraction(24000, 1001))
    assert clip.full_range is (True if full else None)
    want = reference_frames_to_yuv(frames, chroma=name, matrix="bt601", full_range=full)
    for t in range(3):
        for g, p in zip(clip.planes(t), want):
            assert np.array_equal(g, p[t].numpy())
    assert host_ops == [("out", name, "bt601", full, (3, h, w, 3))]
    write_y4m(path, frames.numpy(), fps=16)                                      # a numpy clip, an integer rate
    assert read_y4m(path).fps == Fraction(16)
    with pytest.raises(ValueError, match="420jpeg or 444"):
        write_y4m(path, frames, chroma="422")
    with pytest.raises(ValueError, match="uint8"):
        write_y4m(path, frames.float())


def test_hd_clips_default_to_bt709(tmp_path, host_ops):
    frames = torch.zeros(1, 720, 16, 3, dtype=torch.uint8)
    write_y4m(tmp_path / "hd.y4m", frames)
    load_y4m_frames(tmp_path / "hd.y4m", 1)
    write_y4m(tmp_path / "sd.y4m", frames[:, :719])
    load_y4m_frames(tmp_path / "sd.y4m", 1, matrix="bt709", full_range=True)
    assert [(c[0], c[2], c[3]) for c in host_ops] == [("out", "bt709", False), ("in", "bt709", False), ("out", "bt601", False),
                                                     ("in", "bt709", True)]


@pytest.mark.parametrize("total,source_frames", [(40, 9), (100, 33), (7, 9), (9, 9), (1, 5)])
def test_load_y4m_frames_picks_what_load_video_frames_picks(tmp_path, host_ops, total, source_frames):
    """Frame t of the clip is grey level t, so the picked frames can be read off the result; a short clip repeats its last frame."""
    h, w = 4, 6
    y = np.arange(total, dtype=np.uint8)[:, None, None].repeat(h, 1).repeat(w, 2)
    c = np.full((total, 2, 3), 128, np.uint8)
    path = tmp_path / "ramp.y4m"
    path.write_bytes(assemble(b"YUV4MPEG2 W6 H4 F16:1 Ip C420jpeg XCOLORRANGE=FULL\n", (y, c, c)))
    for seed in (0, 1, 2):
        frames, hh, ww = load_y4m_frames(path, source_frames, generator=torch.Generator().manual_seed(seed))
        assert (hh, ww) == (h, w) and tuple(frames.shape) == (source_frames, h, w, 3) and frames.dtype == torch.uint8
        got = frames[:, 0, 0, 0].tolist()
        assert torch.equal(frames, frames[:, :1, :1, :1].expand_as(frames)) and torch.equal(frames[..., 0], frames[..., 2])
        rgb = torch.from_numpy(y)[..., None].expand(total, h, w, 3)
        ref, _, _ = load_video_frames(rgb, source_frames, generator=torch.Generator().manual_seed(seed))
        assert got == ref[:, 0, 0, 0].tolist() == select_frame_indices(total, source_frames, torch.Generator().manual_seed(seed))
        if total < source_frames:
            assert got[total - 1:] == [total - 1] * (source_frames - total + 1)
        # only the distinct frames were staged and converted
        assert host_ops[-1][4][0] == len(set(got))
    torch.manual_seed(5)
    a = load_y4m_frames(path, source_frames)[0]                                  # the global generator, as load_video_frames
    torch.manual_seed(5)
    b = load_video_frames(torch.from_numpy(y)[..., None].expand(total, h, w, 3), source_frames)[0]
    assert a[:, 0, 0, 0].tolist() == b[:, 0, 0, 0].tolist()


def test_load_y4m_frames_of_an_empty_clip(tmp_path, host_ops):
    path = tmp_path / "empty.y4m"
    path.write_bytes(b"YUV4MPEG2 W6 H4 F16:1\n")
    frames, h, w = load_y4m_frames(path, 5)
    assert (h, w) == (480, 832) and tuple(frames.shape) == (5, 480, 832, 3) and not frames.any()
    with pytest.raises(ValueError, match="source_frames"):
        load_y4m_frames(path, 0)


# ------------------------------------------------------------------ the C ABI
def test_abi_tables_hold_the_new_entries():
    new = {"wan_yuv_to_frames_u8", "wan_frames_u8_to_yuv"}
    header = open(os.path.join(ROOT, "include", "wan_hip.h")).read()
    declared = set(re.findall(r"\b(wan_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert new <= declared and new <= set(_lib.SIGNATURES) and all(hasattr(raw, s) for s in new)
    assert _lib.ABI_VERSION == 11 == _lib.load().wan_abi_version()
    assert ctypes.sizeof(_lib.YuvPlanes) == 3 * 8 + 7 * 8 + 4 * 4 and ctypes.sizeof(_lib.YuvCoef) == 40


def test_geometry_is_validated_before_anything_is_enqueued():
    """No GPU here: every call below has to return before it reaches a launch."""
    lib = _lib.load()
    INV, UNS = _lib.WAN_ERR_INVALID, _lib.WAN_ERR_UNSUPPORTED
    coef = _lib.YuvCoef((ctypes.c_int * 9)(*yuv_matrix("bt601", False)[1].ravel().tolist()), 16)

    def planes_of(h=4, w=8, **kw):
        p = _lib.YuvPlanes()
        p.y, p.cb, p.cr = 4096, 8192, 12288
        p.y_extent, p.cb_extent, p.cr_extent = 2 * h * w, h * w // 2, h * w // 2
        p.y_row, p.y_frame, p.c_row, p.c_frame = w, h * w, w // 2, h * w // 4
        p.c_step, p.sub_x, p.sub_y, p.cosited = 1, 1, 1, 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def into(p, t=2, h=4, w=8, c=coef, frames=65536):
        return lib.wan_yuv_to_frames_u8(ctypes.byref(p) if p is not None else None, ctypes.byref(c) if c is not None else None,
                                        frames, t, h, w, None)

    def outof(p, t=2, h=4, w=8):
        return lib.wan_frames_u8_to_yuv(65536, ctypes.byref(p), ctypes.byref(coef), t, h, w, None)

    assert into(None) == INV and into(planes_of(), c=None) == INV and into(planes_of(), frames=None) == INV
    assert into(planes_of(y=None)) == INV and into(planes_of(cr=None)) == INV
    assert into(planes_of(), t=0) == INV and into(planes_of(), t=65536) == UNS
    assert into(planes_of(y_extent=2 * 32 - 1)) == INV                           # the last luma row leaves the extent
    with pytest.raises(ValueError, match="Y plane: 2 frames of 4 rows"):
        _lib.check(into(planes_of(y_extent=63)), "wan_yuv_to_frames_u8")
    assert into(planes_of(cb_extent=15)) == INV and into(planes_of(cr_extent=15)) == INV
    assert into(planes_of(y_row=7)) == INV and into(planes_of(c_row=3)) == INV and into(planes_of(y_frame=-1)) == INV
    assert into(planes_of(c_step=3)) == INV and into(planes_of(sub_x=2)) == INV and into(planes_of(cosited=5)) == INV
    assert into(planes_of(c_step=2)) == INV                                      # 4 interleaved samples need 7 bytes per row
    assert into(planes_of(), w=9) == INV                                         # 9 columns: 5 chroma samples per row, the strides say 4
    bad = _lib.YuvCoef((ctypes.c_int * 9)(1 << 23, 0, 0, 0, 0, 0, 0, 0, 0), 16)
    assert into(planes_of(), c=bad) == INV
    assert outof(planes_of(cb=None, cr=None)) == INV                             # the way out needs chroma planes
    assert outof(planes_of(sub_y=0)) == UNS                                      # 4:2:2 is not written
    assert outof(planes_of(y_frame=31)) == INV                                   # frames would overwrite each other
    assert outof(planes_of(cb=4096 + 8)) == INV                                  # Cb inside the first luma frame
    with pytest.raises(ValueError, match="overlap"):
        _lib.check(outof(planes_of(cr=8192)), "wan_frames_u8_to_yuv")
