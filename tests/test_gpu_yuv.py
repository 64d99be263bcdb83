"""-m gpu: wan_yuv_to_frames_u8 / wan_frames_u8_to_yuv behind ``yuv_to_frames`` / ``frames_to_yuv`` / ``load_y4m_frames`` / ``write_y4m``
against the numpy definition (``reference_yuv_to_frames`` / ``reference_frames_to_yuv``, pinned on the host by tests/test_yuv_host.py).
EQUALITY everywhere: both sides are the same integer arithmetic on the same host-built tables; there is no rounding to differ in.

A thread moves 16 pixels of a row (of two rows on the way out to 4:2:0) and picks the width of every access from its address, so the
shapes cover: aligned rows (dwordx4 / dwordx2), rows that are no multiple of 16, 4 or 2 bytes (shifted dwords, bytes at both ends),
a last run shorter than 16 pixels, odd sizes (the chroma planes round up, the last column / row repeats), more than one workgroup in
each grid dimension, interleaved CbCr, plane bases at odd addresses, padded rows and the frames of a file with its FRAME lines."""
import numpy as np
import pytest
import torch

from videocof_amd import (fit_frames, frames_to_yuv, load_y4m_frames, ops, read_y4m, reference_fit_frames, reference_frames_to_yuv,
                          reference_yuv_to_frames, restore_frames, write_y4m, yuv_matrix, yuv_to_frames)
from videocof_amd.video_io import _resize_plan, chroma_shape, select_frame_indices, y4m_frame_bytes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5
COMBOS = [("bt601", True), ("bt601", False), ("bt709", True), ("bt709", False)]


def planes(t, h, w, chroma, seed=0):
    rng = np.random.default_rng(seed)
    ch, cw = chroma_shape(h, w, chroma)
    y = rng.integers(0, 256, (t, h, w), dtype=np.uint8)
    y.reshape(-1)[:min(256, y.size)] = np.arange(min(256, y.size), dtype=np.uint8)          # every byte value where it fits
    if ch == 0:
        return y, None, None
    return y, rng.integers(0, 256, (t, ch, cw), dtype=np.uint8), rng.integers(0, 256, (t, ch, cw), dtype=np.uint8)


def frames_of(t, h, w, seed=0):
    return torch.randint(0, 256, (t, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def embed(plane, offset, row_stride=None, frame_stride=None, step=1, tail=32):
    """``plane`` [T, rows, cols] in a canary-filled device buffer: -> (the strided view, the buffer, the buffer as it should stay)."""
    t, rows, cols = plane.shape
    row_stride = (cols - 1) * step + 1 if row_stride is None else row_stride
    frame_stride = rows * row_stride if frame_stride is None else frame_stride
    host = np.full(offset + t * frame_stride + tail, CANARY, np.uint8)
    np.lib.stride_tricks.as_strided(host[offset:], plane.shape, (frame_stride, row_stride, step))[...] = plane
    buf = torch.from_numpy(host).to(DEV)
    return torch.as_strided(buf, plane.shape, (frame_stride, row_stride, step), offset), buf, host


def check_in(ps, chroma, matrix="bt601", full=False, views=None, want=None):
    want = reference_yuv_to_frames(*ps, chroma=chroma, matrix=matrix, full_range=full) if want is None else want
    y, cb, cr = views if views is not None else [dev(p) for p in ps]
    got = yuv_to_frames(y, cb, cr, chroma=chroma, matrix=matrix, full_range=full)
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == tuple(want.shape)
    bad = int((got.cpu() != want).sum())
    print(f"yuv -> frames {chroma} {matrix} full={full} {tuple(want.shape)}: {bad} mismatches of {want.numel()}")
    assert bad == 0
    return got


def check_out(frames, chroma, matrix="bt601", full=False):
    want = reference_frames_to_yuv(frames, chroma=chroma, matrix=matrix, full_range=full)
    buf, got = frames_to_yuv(frames.to(DEV), chroma=chroma, matrix=matrix, full_range=full)
    t, h, w, _ = frames.shape
    assert buf.is_cuda and buf.dtype == torch.uint8 and tuple(buf.shape) == (t, y4m_frame_bytes(h, w, chroma))
    for name, g, p in zip("Y Cb Cr".split(), got, want):
        assert tuple(g.shape) == tuple(p.shape) and g.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        bad = int((g.cpu() != p).sum())
        print(f"frames -> yuv {chroma} {matrix} full={full} {tuple(frames.shape)} {name}: {bad} mismatches of {p.numel()}")
        assert bad == 0
    packed = torch.cat([p.reshape(t, -1) for p in want], dim=1)                  # the .y4m frame layout, nothing in between
    assert torch.equal(buf.cpu(), packed)
    return buf


# ------------------------------------------------------------------ the way in
def test_aligned_clip_both_ways():
    """64 x 48, T = 2: every row, plane and run is 16-byte aligned (dwordx4 for RGB and luma, dwordx2 for chroma)."""
    ps = planes(2, 48, 64, "420jpeg", seed=1)
    assert all(dev(p).data_ptr() % 16 == 0 for p in ps)
    for matrix, full in COMBOS:
        check_in(ps, "420jpeg", matrix, full)
    fr = frames_of(2, 48, 64, seed=2)
    for matrix, full in COMBOS:
        check_out(fr, "420jpeg", matrix, full)
    check_out(fr, "444")


@pytest.mark.parametrize("chroma", ["420jpeg", "420mpeg2", "420", "422", "444", "mono"])
def test_odd_size_every_layout(chroma):
    """37 x 23, T = 3: 37-byte luma rows, 19-byte chroma rows, 111-byte RGB rows; three runs per row, the last one of 5 pixels."""
    ps = planes(3, 23, 37, chroma, seed=3)
    got = check_in(ps, chroma, "bt601", False)
    check_in(ps, chroma, "bt709", True)
    if chroma == "420":
        assert torch.equal(got, check_in(ps, "420jpeg"))
    if chroma == "420mpeg2":                                                   # the siting is not ignored
        assert not torch.equal(got.cpu(), reference_yuv_to_frames(*ps, chroma="420jpeg"))


def test_854_wide_strip_and_several_workgroups():
    """854 x 4: 427-byte chroma rows, 2562-byte RGB rows, 54 runs per row = 4 workgroups across; then 40 rows = 3 workgroups down."""
    ps = planes(2, 4, 854, "420jpeg", seed=4)
    check_in(ps, "420jpeg")
    check_out(frames_of(2, 4, 854, seed=5), "420jpeg")
    ps = planes(1, 40, 270, "420mpeg2", seed=6)
    check_in(ps, "420mpeg2")
    check_out(frames_of(1, 40, 270, seed=7), "420jpeg")
    check_out(frames_of(1, 40, 270, seed=7), "444")


def test_nv12_interleaved_chroma():
    """32 x 16 NV12: one CbCr plane, the two chroma views are each other's odd bytes; NV21 swaps them."""
    y, cb, cr = planes(2, 16, 32, "420jpeg", seed=8)
    uv = torch.from_numpy(np.stack([cb, cr], axis=-1)).to(DEV)                  # [T, 8, 16, 2]
    assert uv[..., 0].stride() == (256, 32, 2)
    check_in((y, cb, cr), "420jpeg", views=(dev(y), uv[..., 0], uv[..., 1]))
    check_in((y, cr, cb), "420jpeg", views=(dev(y), uv[..., 1], uv[..., 0]))
    uv4 = torch.from_numpy(np.stack(planes(1, 5, 21, "444", seed=9)[1:], axis=-1)).to(DEV)
    y4 = planes(1, 5, 21, "444", seed=9)[0]
    check_in((y4, uv4[..., 0].cpu().numpy(), uv4[..., 1].cpu().numpy()), "444", views=(dev(y4), uv4[..., 0], uv4[..., 1]))
    # the way out into an interleaved plane, odd sizes, a canary around it
    fr = frames_of(2, 15, 29, seed=10)
    wy, wcb, wcr = reference_frames_to_yuv(fr, chroma="420jpeg")
    fwd, _ = yuv_matrix("bt601", False)
    yv, ybuf, yhost = embed(wy.numpy(), 3)
    inter = np.stack([wcb.numpy(), wcr.numpy()], axis=-1).reshape(2, 8, 30)      # what the plane should hold
    uvv, uvbuf, uvhost = embed(inter, 5, row_stride=37)
    cbv = torch.as_strided(uvbuf, (2, 8, 15), (8 * 37, 37, 2), 5)
    crv = torch.as_strided(uvbuf, (2, 8, 15), (8 * 37, 37, 2), 6)
    uvbuf.fill_(CANARY)
    ybuf.fill_(CANARY)
    ops.frames_u8_to_yuv(fr.to(DEV), yv, cbv, crv, True, fwd.ravel().tolist(), 16)
    assert np.array_equal(ybuf.cpu().numpy(), yhost) and np.array_equal(uvbuf.cpu().numpy(), uvhost)


@pytest.mark.parametrize("offset", [1, 3, 6])
def test_plane_bases_at_odd_addresses(offset):
    """Planes that start 1, 3 and 6 bytes into their buffers: no run is aligned to its own width."""
    ps = planes(2, 10, 50, "420jpeg", seed=offset)
    want = reference_yuv_to_frames(*ps, chroma="420jpeg")
    views = [embed(p, offset + i)[0] for i, p in enumerate(ps)]
    assert views[0].data_ptr() % 16 == offset
    check_in(ps, "420jpeg", views=views, want=want)
    views = [embed(p, offset)[0] for p in planes(2, 10, 50, "444", seed=offset)]
    check_in(planes(2, 10, 50, "444", seed=offset), "444", views=views)


def test_padded_rows_and_frames_do_not_change_the_result():
    """Row strides above the width and frame strides above a frame, canary bytes in the padding."""
    ps = planes(2, 12, 40, "420jpeg", seed=11)
    want = reference_yuv_to_frames(*ps, chroma="420jpeg")
    views = [embed(ps[0], 0, row_stride=64, frame_stride=12 * 64 + 48)[0], embed(ps[1], 0, row_stride=27, frame_stride=6 * 27 + 5)[0],
             embed(ps[2], 16, row_stride=32)[0]]
    with pytest.raises(ValueError, match="same for both planes"):
        yuv_to_frames(*views)
    views[2] = embed(ps[2], 2, row_stride=27, frame_stride=6 * 27 + 5)[0]
    check_in(ps, "420jpeg", views=views, want=want)


def file_bytes(header, ps):
    out = [header]
    for t in range(ps[0].shape[0]):
        out.append(b"FRAME\n")
        out += [p[t].tobytes() for p in ps if p is not None]
    return b"".join(out)


def test_the_bytes_of_a_file_uploaded_as_they_are():
    """The whole .y4m file on the device: the planes start where the header ends, 6 bytes of FRAME line between the frames."""
    h, w, t = 9, 21, 3
    ps = planes(t, h, w, "420jpeg", seed=12)
    header = b"YUV4MPEG2 W21 H9 F16:1 Ip A1:1 C420jpeg\n"
    raw = file_bytes(header, ps)
    buf = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    fb = y4m_frame_bytes(h, w, "420jpeg")
    pitch, first = 6 + fb, len(header) + 6
    y = torch.as_strided(buf, (t, h, w), (pitch, w, 1), first)
    cb = torch.as_strided(buf, (t, 5, 11), (pitch, 11, 1), first + h * w)
    cr = torch.as_strided(buf, (t, 5, 11), (pitch, 11, 1), first + h * w + 55)
    check_in(ps, "420jpeg", views=(y, cb, cr))


@pytest.mark.parametrize("value", [0, 255])
def test_constant_frames(value):
    for chroma in ("420jpeg", "444"):
        ch, cw = chroma_shape(18, 34, chroma)
        ps = (np.full((1, 18, 34), value, np.uint8), np.full((1, ch, cw), value, np.uint8), np.full((1, ch, cw), value, np.uint8))
        for matrix, full in COMBOS:
            check_in(ps, chroma, matrix, full)
            check_out(torch.full((1, 18, 34, 3), value, dtype=torch.uint8), chroma, matrix, full)


def test_out_of_gamut_samples_are_clamped():
    for ycc in ((255, 0, 255), (0, 255, 0)):
        ps = tuple(np.full((1, 6, 20), v, np.uint8) for v in ycc)
        for matrix, full in COMBOS:
            got = check_in(ps, "444", matrix, full)
            px = got[0, 0, 0].tolist()
            assert 0 in px or 255 in px, (ycc, matrix, full, px)
    # the limited-range ends on the way in: below 16 and above 235 clamp to black and white
    ps = (np.array([[[0, 8, 16, 235, 245, 255]]], np.uint8), np.full((1, 1, 6), 128, np.uint8), np.full((1, 1, 6), 128, np.uint8))
    got = check_in(ps, "444", "bt601", False)
    assert got[0, 0, :, 0].tolist() == [0, 0, 0, 255, 255, 255]


def all_triples(chunk, chunks):
    """Chunk ``chunk`` of ``chunks`` of the 2^24 byte triples as a [1, rows, 4096, 3] array, first component slowest."""
    n = (1 << 24) // chunks
    v = np.arange(chunk * n, (chunk + 1) * n, dtype=np.uint32)
    return np.stack([v >> 16, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(1, n // 4096, 4096, 3)


@pytest.mark.parametrize("chunk", range(4))
def test_every_colour_out_through_444(chunk):
    """All 2^24 RGB colours -> (Y, Cb, Cr), bt601 limited range, a quarter of them per case."""
    fr = torch.from_numpy(all_triples(chunk, 4))
    want = reference_frames_to_yuv(fr, chroma="444", matrix="bt601", full_range=False)
    _, got = frames_to_yuv(fr.to(DEV), chroma="444", matrix="bt601", full_range=False)
    for g, p in zip(got, want):
        assert torch.equal(g.cpu(), p)


@pytest.mark.parametrize("chunk", range(4))
def test_every_sample_triple_in_through_444(chunk):
    """All 2^24 (Y, Cb, Cr) triples -> RGB, bt601 limited range, a quarter of them per case: most of them are out of gamut."""
    ycc = all_triples(chunk, 4)
    ps = tuple(np.ascontiguousarray(ycc[..., c]) for c in range(3))
    want = reference_yuv_to_frames(*ps, chroma="444", matrix="bt601", full_range=False)
    got = yuv_to_frames(*[dev(p) for p in ps], chroma="444", matrix="bt601", full_range=False)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("matrix,full", [("bt601", True), ("bt709", True), ("bt709", False)])
def test_a_sample_of_colours_for_the_other_matrices(matrix, full):
    """2^18 colours / triples (every fourth level of each component, offset so that 0 and 255 occur) in both directions."""
    lv = np.concatenate([np.arange(0, 252, 4), [255]]).astype(np.uint8)[:64]
    lv[-1] = 255
    grid = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), axis=-1).reshape(1, 512, 512, 3)
    fr = torch.from_numpy(grid)
    want = reference_frames_to_yuv(fr, chroma="444", matrix=matrix, full_range=full)
    _, got = frames_to_yuv(fr.to(DEV), chroma="444", matrix=matrix, full_range=full)
    for g, p in zip(got, want):
        assert torch.equal(g.cpu(), p)
    ps = tuple(np.ascontiguousarray(grid[..., c]) for c in range(3))
    check_in(ps, "444", matrix, full)


# ------------------------------------------------------------------ the way out
@pytest.mark.parametrize("size", [(23, 37), (1, 5), (2, 2), (17, 16), (5, 33)])
def test_odd_sizes_out_with_canaries_around_every_plane(size):
    """Planes at odd addresses with padded rows inside canary-filled buffers: the planes equal the definition, every other byte of
    the buffers is untouched (a store wider than its run would show)."""
    h, w = size
    fr = frames_of(3, h, w, seed=h * 64 + w)
    for chroma in ("420jpeg", "444"):
        want = [p.numpy() for p in reference_frames_to_yuv(fr, chroma=chroma, matrix="bt709", full_range=True)]
        fwd, _ = yuv_matrix("bt709", True)
        cw = want[1].shape[2]
        for offset, pad in ((0, 0), (1, 0), (2, 3), (7, 5)):
            yv, ybuf, yhost = embed(want[0], offset, row_stride=w + pad)
            cbv, cbbuf, cbhost = embed(want[1], offset + 1, row_stride=cw + pad)
            crv, crbuf, crhost = embed(want[2], offset + 2, row_stride=cw + pad)
            for b in (ybuf, cbbuf, crbuf):
                b.fill_(CANARY)
            ops.frames_u8_to_yuv(fr.to(DEV), yv, cbv, crv, chroma == "420jpeg", fwd.ravel().tolist(), 0)
            for name, b, hst in (("Y", ybuf, yhost), ("Cb", cbbuf, cbhost), ("Cr", crbuf, crhost)):
                assert np.array_equal(b.cpu().numpy(), hst), (chroma, offset, pad, name)
    check_out(fr, "420jpeg")
    check_out(fr, "444", "bt709", True)


def test_the_frame_prefix_layout_of_the_writer():
    fr = frames_of(2, 9, 21, seed=13)
    want = reference_frames_to_yuv(fr, chroma="420jpeg")
    buf, (y, cb, cr) = frames_to_yuv(fr.to(DEV), chroma="420", frame_prefix=b"FRAME\n")
    assert tuple(buf.shape) == (2, 6 + y4m_frame_bytes(9, 21, "420"))
    raw = buf.cpu().numpy()
    assert all(bytes(raw[t, :6]) == b"FRAME\n" for t in range(2))
    assert np.array_equal(raw[:, 6:], torch.cat([p.reshape(2, -1) for p in want], dim=1).numpy())
    assert torch.equal(y.cpu(), want[0]) and torch.equal(cb.cpu(), want[1]) and torch.equal(cr.cpu(), want[2])


def test_the_out_path_and_the_argument_checks():
    ps = planes(2, 10, 22, "420jpeg", seed=14)
    want = reference_yuv_to_frames(*ps, chroma="420jpeg")
    out = torch.full((2, 10, 22, 3), CANARY, dtype=torch.uint8, device=DEV)
    y, cb, cr = [dev(p) for p in ps]
    back = yuv_to_frames(y, cb, cr, chroma="420jpeg", out=out)
    assert back is out and torch.equal(out.cpu(), want)
    with pytest.raises(ValueError, match="out"):
        yuv_to_frames(y, cb, cr, out=torch.empty(2, 10, 23, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yuv_to_frames(y.cpu(), cb.cpu(), cr.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        yuv_to_frames(y, cb.cpu(), cr.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames_to_yuv(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="chroma"):
        yuv_to_frames(y, cb, cr, chroma="mono")
    with pytest.raises(ValueError, match="chroma"):
        yuv_to_frames(y, chroma="420jpeg")
    with pytest.raises(ValueError, match="expected uint8"):
        yuv_to_frames(y, cb[:, :4], cr[:, :4])
    # a geometry that leaves the described extent (torch itself refuses to make such a view, so the description is edited): refused on
    # the host, nothing is enqueued and `out` keeps its bytes
    import ctypes
    from videocof_amd import _lib
    desc = ops._yuv_planes(y, cb, cr, True, True, False, "test")
    coef = ops._yuv_coef(yuv_matrix("bt601", False)[1].ravel().tolist(), 16)
    out.fill_(CANARY)
    for field, value in (("y_extent", 2 * 10 * 22 - 1), ("cr_extent", 2 * 5 * 11 - 1), ("y_row", 23), ("c_frame", 56)):
        keep = getattr(desc, field)
        setattr(desc, field, value)
        st = _lib.load().wan_yuv_to_frames_u8(ctypes.byref(desc), ctypes.byref(coef), out.data_ptr(), 2, 10, 22, None)
        setattr(desc, field, keep)
        with pytest.raises(ValueError, match="leave its"):
            _lib.check(st, "wan_yuv_to_frames_u8")
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())


# ------------------------------------------------------------------ file to file
def test_file_to_file_equals_the_chain_of_host_references(tmp_path):
    """A hand-assembled 70 x 40 clip: load_y4m_frames, fit_frames, restore_frames, write_y4m, read_y4m -- against read_y4m's planes
    through reference_yuv_to_frames, reference_fit_frames twice and reference_frames_to_yuv."""
    h, w, total, picked = 40, 70, 12, 5
    ps = planes(total, h, w, "420mpeg2", seed=15)
    src = tmp_path / "in.y4m"
    src.write_bytes(file_bytes(b"YUV4MPEG2 W70 H40 F24:1 Ip A1:1 C420mpeg2\n", ps))
    frames, hh, ww = load_y4m_frames(src, picked, generator=torch.Generator().manual_seed(3))
    assert (hh, ww) == (h, w) and frames.is_cuda and tuple(frames.shape) == (picked, h, w, 3)
    fitted, plan = fit_frames(frames, 32, 48)
    restored = restore_frames(fitted, h, w)
    dst = tmp_path / "out.y4m"
    write_y4m(dst, restored, fps=24)
    clip = read_y4m(dst)
    assert (clip.width, clip.height, clip.frames, clip.chroma, clip.full_range) == (w, h, picked, "420jpeg", None)

    idx = select_frame_indices(total, picked, torch.Generator().manual_seed(3))
    assert len(set(idx)) == picked
    host = reference_yuv_to_frames(*[p[idx] for p in ps], chroma="420mpeg2", matrix="bt601", full_range=False)
    assert torch.equal(frames.cpu(), host)
    host = reference_fit_frames(host, 32, 48)
    host = reference_fit_frames(host, h, w, plan=_resize_plan(32, 48, h, w))
    want = reference_frames_to_yuv(host, chroma="420jpeg", matrix="bt601", full_range=False)
    for t in range(picked):
        for g, p in zip(clip.planes(t), want):
            assert np.array_equal(g, p[t].numpy())
    # a short clip repeats its last frame on the device
    more, _, _ = load_y4m_frames(src, 15, generator=torch.Generator().manual_seed(3))
    assert tuple(more.shape) == (15, h, w, 3) and torch.equal(more[11], more[14]) and not torch.equal(more[10], more[11])
