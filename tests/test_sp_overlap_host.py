"""Host side of the concurrent-exchange emulation and of the CUs reserved for communication kernels: the C ABI entry, the tuning key
and the plans that follow it are host arithmetic / argument checks -- no GPU is needed (the CU count falls back to 256 without one)."""
import collections
import ctypes
import os
import re
import subprocess

import pytest

from videocof_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def reserve():
    """Sets tuning key sp_reserve_cus for one test; it is back at 0 afterwards whatever the test did."""
    lib = _lib.load()

    def set_(n):
        assert lib.wan_set_tuning(b"sp_reserve_cus", n) == _lib.WAN_OK
    yield set_
    lib.wan_set_tuning(b"sp_reserve_cus", 0)


def test_channel_copy_symbol_is_in_header_library_and_table():
    src = open(os.path.join(ROOT, "include", "wan_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bwan_sp_channel_copy\s*\(", src), "not declared in include/wan_hip.h"
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\sT wan_sp_channel_copy$", exported, flags=re.M), "not exported by libwan_hip.so"
    res, args = _lib.SIGNATURES["wan_sp_channel_copy"]
    assert res is ctypes.c_int and len(args) == 6
    assert hasattr(_lib.load(), "wan_sp_channel_copy")


def test_reserve_key_round_trips_and_defaults_to_zero(reserve):
    lib = _lib.load()
    assert lib.wan_get_tuning(b"sp_reserve_cus") == 0
    for n in (32, 8, 0):
        reserve(n)
        assert lib.wan_get_tuning(b"sp_reserve_cus") == n


def test_channel_copy_argument_errors():
    """Validated before anything is enqueued (the pointers are never dereferenced on the host)."""
    lib = _lib.load()
    buf = (ctypes.c_ubyte * 256)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 128
    f = lib.wan_sp_channel_copy
    for channels in (0, 33, -1):
        assert f(a, b, 64, channels, 256, None) == _lib.WAN_ERR_INVALID
        assert b"channels" in lib.wan_last_error()
    for threads in (128, 0, 1024, 384):
        assert f(a, b, 64, 16, threads, None) == _lib.WAN_ERR_INVALID
        assert b"threads" in lib.wan_last_error()
    assert f(None, b, 64, 16, 256, None) == _lib.WAN_ERR_INVALID and b"null" in lib.wan_last_error()
    assert f(a, None, 64, 16, 256, None) == _lib.WAN_ERR_INVALID and b"null" in lib.wan_last_error()
    assert f(a, b, -1, 16, 256, None) == _lib.WAN_ERR_INVALID
    assert f(a, a + 16, 64, 16, 256, None) == _lib.WAN_ERR_INVALID and b"overlapping" in lib.wan_last_error()
    with pytest.raises(ValueError, match="channels"):
        _lib.check(f(a, b, 64, 0, 256, None), "wan_sp_channel_copy")
    assert f(a, b, 0, 16, 256, None) == _lib.WAN_OK          # nothing to move: no launch


def test_emulated_rank_validates_the_concurrent_footprint():
    from videocof_amd import dist as vdist
    for bad in (dict(channels=0), dict(channels=33), dict(threads=128), dict(threads=384)):
        with pytest.raises(ValueError):
            vdist.EmulatedRank(0, 2, concurrent=True, **bad)
        with pytest.raises(ValueError):
            vdist.init_sequence_parallel(backend="emulated", rank=0, world_size=2, concurrent=True, **bad)
    sp = vdist.EmulatedRank(0, 2, concurrent=True, channels=32, threads=256, poison=True)
    assert (sp.concurrent, sp.channels, sp.threads, sp.poison) == (True, 32, 256, True)
    plain = vdist.EmulatedRank(0, 2)
    assert (plain.concurrent, plain.channels, plain.threads, plain.poison) == (False, 16, 512, False)
    # the concurrent mode runs a HIP kernel: host tensors are an error, not a quiet copy_
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.exchange(torch.zeros(8), torch.ones(8))


def test_init_sequence_parallel_sets_and_destroy_restores_the_reservation():
    from videocof_amd import dist as vdist
    lib = _lib.load()
    try:
        sp = vdist.init_sequence_parallel(backend="emulated", rank=0, world_size=4, reserve_cus=16, concurrent=True, channels=8, threads=256)
        assert lib.wan_get_tuning(b"sp_reserve_cus") == 16 and (sp.concurrent, sp.channels, sp.threads) == (True, 8, 256)
        vdist.init_sequence_parallel(backend="emulated", rank=0, world_size=4)          # a later init without it takes it back
        assert lib.wan_get_tuning(b"sp_reserve_cus") == 0
        vdist.init_sequence_parallel(backend="emulated", rank=0, world_size=4, reserve_cus=32)
        assert lib.wan_get_tuning(b"sp_reserve_cus") == 32
        with pytest.raises(ValueError, match="reserve_cus"):
            vdist.init_sequence_parallel(backend="emulated", rank=0, world_size=4, reserve_cus=-1)
    finally:
        vdist.destroy_sequence_parallel()
    assert lib.wan_get_tuning(b"sp_reserve_cus") == 0 and vdist.get_sp_group() is None


def _plan(lib, M, N, K):
    """(as tests/test_gemm_pk_plan.py queries it)"""
    G = lib.wan_gemm_pk_grid(M, N)
    out = (ctypes.c_int * 11)()
    segs = []
    for w in range(G):
        i = 0
        while lib.wan_gemm_pk_segment(M, N, K, w, i, out):
            segs.append((w, i) + tuple(out))
            i += 1
    return G, segs


@pytest.mark.parametrize("M,N,K", [(67080, 5120, 5120), (8392, 5120, 13824), (8392, 10240, 5120), (2304, 1536, 8960), (300, 300, 128)])
def test_persistent_gemm_plan_leaves_the_reserved_cus_free(reserve, M, N, K):
    """32 CUs reserved: 224 workers on a 256-CU count, and the plan over them is as sound as the one over 256 -- every (tile, K unit)
    exactly once, split tiles chained in K order, no shared slot; the workspace request follows the grid.  0: unchanged."""
    lib = _lib.load()
    G0, segs0 = _plan(lib, M, N, K)
    ws0 = int(lib.wan_gemm_workspace_bytes(M, N, K))
    reserve(32)
    G, segs = _plan(lib, M, N, K)
    assert G == G0 - 32 and G % 8 == 0
    if G0 == 256:
        assert G == 224
    nk, tiles_m, tiles_n = K // 64, (M + 255) // 256, (N + 255) // 256
    cover, slots, pieces = collections.Counter(), set(), collections.defaultdict(list)
    for (w, i, tm, tn, kb, ke, partial, slot, cnt, jlo, jhi, me, tau) in segs:
        assert 0 <= w < G and 0 <= tm < tiles_m and 0 <= tn < tiles_n and 0 <= kb < ke <= nk and kb % 2 == 0 and ke % 2 == 0
        for k in range(kb, ke, 2):
            cover[(tm, tn, k)] += 1
        assert bool(partial) == (not (kb == 0 and ke == nk))
        if partial:
            assert slot not in slots and slot // 2 == (w % 8) * (G // 8) + w // 8 and 0 <= cnt < 512
            slots.add(slot)
            pieces[(w % 8, cnt)].append((kb, ke, me, jlo, jhi))
    assert len(cover) == tiles_m * tiles_n * nk // 2 and set(cover.values()) == {1}
    for ps in pieces.values():
        ps.sort()
        assert ps[0][0] == 0 and ps[-1][1] == nk and all(a[1] == b[0] for a, b in zip(ps, ps[1:]))
        assert [p[2] for p in ps] == list(range(ps[0][3], ps[0][4] + 1))
    if lib.wan_gemm_ws_plan(M, N, K) == 3:                                      # (other shapes: no workspace, or the split-K form's)
        assert int(lib.wan_gemm_workspace_bytes(M, N, K)) == 4096 + G * 2 * 256 * 256 * 4
    assert lib.wan_set_tuning(b"gemm_pk_workers", 64) == _lib.WAN_OK           # an explicit grid still wins
    try:
        assert lib.wan_gemm_pk_grid(M, N) == 64
    finally:
        lib.wan_set_tuning(b"gemm_pk_workers", 0)
    reserve(0)
    assert _plan(lib, M, N, K) == (G0, segs0) and int(lib.wan_gemm_workspace_bytes(M, N, K)) == ws0


def test_reservation_is_clamped_to_a_grid_the_kernels_accept(reserve):
    lib = _lib.load()
    G0 = lib.wan_gemm_pk_grid(67080, 5120)
    reserve(G0 - 12)                      # 12 CUs left -> 8 workers (a multiple of 8)
    assert lib.wan_gemm_pk_grid(67080, 5120) == 8
    reserve(10000)                        # more than the chip has: the smallest grid, never zero or negative
    assert lib.wan_gemm_pk_grid(67080, 5120) == 8
    reserve(-5)                           # not a reservation
    assert lib.wan_gemm_pk_grid(67080, 5120) == G0
