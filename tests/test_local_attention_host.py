"""CPU: local self-attention plans (videocof_amd/local_attention.py) against the token-level brute force, the plan check values of
DESIGN.md 13.3, and the list validator of the C ABI (wan_attn_sparse_validate: host arithmetic, no GPU)."""
import numpy as np
import pytest

from videocof_amd import _lib, ops
from videocof_amd.local_attention import (K_TILE, Q_BLOCK, block_lift, local_attention_plan, plan_from_blocks, reference_local_mask)

# (grid, frame_split_indices, ground_frame_indices): [source n | grounding G | target n] frames, a grid without a source segment,
# and one whose token count (5 * 3 * 7 = 105) is no multiple of 64
GRIDS = [((7, 4, 6), [3], [(3, 4)]), ((11, 6, 20), [5], [(5, 6)]), ((5, 4, 6), None, None), ((5, 3, 7), [2], [(2, 3)])]
WINDOWS = [(0, 0), (1, 1), (1, 2), (2, 1)]


@pytest.mark.parametrize("grid,split,ground", GRIDS)
def test_plan_equals_the_block_lifting_of_the_token_rule(grid, split, ground):
    F, R, W = grid
    L = F * R * W
    for wf, wr in WINDOWS:
        for sink in (0, 1):
            mask = reference_local_mask(grid, split, ground, wf, wr, sink)
            want = plan_from_blocks(block_lift(mask), L, L)
            plan = local_attention_plan(grid, split, ground, wf, wr, sink)
            assert plan.n_qblocks == -(-L // Q_BLOCK) and plan.n_ktiles == -(-L // K_TILE)
            assert np.array_equal(plan.row_ptr, want.row_ptr) and np.array_equal(plan.tiles, want.tiles), (grid, wf, wr, sink)
            assert plan.row_ptr.dtype == np.int32 and plan.tiles.dtype == np.int32 and plan.row_ptr[0] == 0
            for i in range(plan.n_qblocks):
                row = plan.row(i)
                assert row.size > 0 and bool((np.diff(row) > 0).all()) and row[0] >= 0 and row[-1] < plan.n_ktiles
                own = np.arange(i * Q_BLOCK // K_TILE, (min((i + 1) * Q_BLOCK, L) - 1) // K_TILE + 1)
                assert np.isin(own, row).all(), (grid, wf, wr, i)            # a token attends itself: its own tiles are listed
            ops.attn_sparse_validate(plan.row_ptr, plan.tiles, plan.n_qblocks, plan.n_ktiles)


def test_the_token_rule_itself():
    """Spot checks of reference_local_mask at (7, 4, 6), n = 3, G = 1: tokens are (frame, y, x); frames 0-2 source, 3 grounding, 4-6 target."""
    grid = (7, 4, 6)
    tok = lambda f, y, x=0: (f * 4 + y) * 6 + x
    m = reference_local_mask(grid, [3], [(3, 4)], 0, 1, sink_frames=1)
    assert m[tok(1, 0), tok(1, 1, 5)] and not m[tok(1, 0), tok(1, 2)]              # rows: |dy| <= 1, columns free
    assert m[tok(1, 0), tok(5, 1)] and not m[tok(1, 0), tok(6, 0)]                 # source frame 1 <-> target frame 1 (f = 1 both)
    assert m[tok(2, 3), tok(3, 0)] and m[tok(3, 0), tok(2, 3)]                     # grounding: global both ways
    assert m[tok(2, 3), tok(0, 0)] and m[tok(2, 3), tok(4, 0)]                     # sinks: frame 0 of either segment, as KEYS
    assert not m[tok(0, 0), tok(2, 3)]                                             # ... a sink QUERY gets nothing extra
    m0 = reference_local_mask(grid, [3], [(3, 4)], 0, 1, sink_frames=0)
    assert not m0[tok(2, 3), tok(0, 0)]
    one = reference_local_mask((5, 4, 6), None, None, 1, 0)
    assert one[tok(3, 2), tok(4, 2)] and one[tok(3, 2), tok(0, 0)] and not one[tok(3, 2), tok(1, 2)]


def test_full_windows_list_every_tile():
    for grid, split, ground in GRIDS:
        n = grid[0] if split is None else split[0]
        plan = local_attention_plan(grid, split, ground, n, grid[1])
        assert plan.listed == plan.n_qblocks * plan.n_ktiles and plan.density == 1.0
    padded = local_attention_plan((7, 4, 6), [3], [(3, 4)], 3, 4, q_len=600)      # 168 tokens in 600 query rows: blocks 1, 2 hold none
    assert padded.n_qblocks == 3 and padded.row(0).size == 3 and list(padded.row(1)) == [0] and list(padded.row(2)) == [0]


@pytest.mark.parametrize("window,density,fewest,most", [((3, 10), 0.31738, 151, 1049), ((2, 8), 0.24071, 119, 1049),
                                                        ((4, 10), 0.37221, 173, 1049)])
def test_plan_check_values_at_the_headline_shape(window, density, fewest, most):
    """Grid (43, 30, 52), n = 21, G = 1, sink 1: 67 080 tokens, 263 query blocks, 1 049 key tiles."""
    plan = local_attention_plan((43, 30, 52), [21], [(21, 22)], *window)
    per_block = np.diff(plan.row_ptr)
    assert (plan.n_qblocks, plan.n_ktiles) == (263, 1049)
    assert round(plan.density, 5) == density and int(per_block.min()) == fewest and int(per_block.max()) == most


def test_plan_check_values_at_other_shapes():
    big = local_attention_plan((43, 45, 80), [21], [(21, 22)], 3, 12)
    assert (big.n_qblocks, big.n_ktiles, round(big.density, 5)) == (605, 2419, 0.25129)
    small = local_attention_plan((11, 6, 20), [5], [(5, 6)], 1, 2)
    assert (small.n_qblocks, small.n_ktiles, round(small.density, 5), int(np.diff(small.row_ptr).min())) == (6, 21, 0.88095, 14)


def test_bad_arguments():
    with pytest.raises(ValueError):
        local_attention_plan((7, 4, 6), [3], [(3, 4)], -1, 1)
    with pytest.raises(ValueError):
        local_attention_plan((7, 4, 6), [3], [(2, 4)], 1, 1)                        # grounding must follow the source segment
    with pytest.raises(ValueError):
        local_attention_plan((7, 4, 6), [3], [(3, 4)], 1, 1, q_len=100)
    with pytest.raises(NotImplementedError):
        local_attention_plan((7, 4, 6), [3, 2], None, 1, 1)


GOOD = (np.array([0, 2, 5], dtype=np.int32), np.array([0, 3, 1, 2, 4], dtype=np.int32), 2, 5)


def _bad(row_ptr=None, tiles=None):
    return (np.array(GOOD[0] if row_ptr is None else row_ptr, dtype=np.int32), np.array(GOOD[1] if tiles is None else tiles, dtype=np.int32), 2, 5)


@pytest.mark.parametrize("lists,message", [
    (_bad(tiles=[0, 3, 4, 2, 1]), "not ascending"),            # a descending row
    (_bad(tiles=[0, 3, 1, 1, 4]), "twice"),                    # a duplicated tile
    (_bad(tiles=[0, 5, 1, 2, 4]), "beyond the last"),          # a tile >= n_ktiles
    (_bad(tiles=[0, 3, -1, 2, 4]), "negative"),                # a negative tile
    (_bad(row_ptr=[0, 0, 5]), "lists no tile"),                # an empty row
    (_bad(row_ptr=[1, 2, 5]), r"row_ptr\[0\]"),                # row_ptr[0] != 0
    (_bad(row_ptr=[0, 3, 2]), "decreases"),
])
def test_the_validator_names_each_offence(lists, message):
    lib = _lib.load()
    rp, tl, nqb, nkt = lists
    assert lib.wan_attn_sparse_validate(rp.ctypes.data, tl.ctypes.data, nqb, nkt) == _lib.WAN_ERR_INVALID
    assert __import__("re").search(message, lib.wan_last_error().decode())
    with pytest.raises(ValueError, match=message):
        ops.attn_sparse_validate(rp, tl, nqb, nkt)


def test_the_validator_accepts_a_good_list_and_the_binding_guards_its_reads():
    lib = _lib.load()
    rp, tl, nqb, nkt = GOOD
    assert lib.wan_attn_sparse_validate(rp.ctypes.data, tl.ctypes.data, nqb, nkt) == _lib.WAN_OK
    ops.attn_sparse_validate(rp, tl, nqb, nkt)
    assert lib.wan_attn_sparse_validate(None, tl.ctypes.data, nqb, nkt) == _lib.WAN_ERR_INVALID
    with pytest.raises(ValueError, match="offsets into"):                           # row_ptr past the tiles: never handed to the library
        ops.attn_sparse_validate([0, 2, 9], tl, nqb, nkt)
    with pytest.raises(ValueError, match="offsets into"):
        ops.attn_sparse_validate([0, 5], tl, nqb, nkt)


def test_abi_is_additive():
    assert _lib.ABI_VERSION == 11 == _lib.load().wan_abi_version()
    for name in ("wan_attn_sparse_validate", "wan_attn_sparse_create", "wan_attn_sparse_destroy", "wan_attn_sparse_listed",
                 "wan_attention_fwd_sparse"):
        assert name in _lib.SIGNATURES
    assert _lib.ATTN_VARIANT_SPARSE == 64 and "listed key tiles" in _lib.attn_variant_name(1 | 64)
    # a null plan is refused before anything else is looked at; destroying / asking nothing is harmless
    assert _lib.load().wan_attention_fwd_sparse(1, 128, 0, 1, 128, 0, 1, 64, 0, 1, 128, 0, 1, 8, 8, None, 1, 128, 0.1, 0, None) == _lib.WAN_ERR_INVALID
    _lib.load().wan_attn_sparse_destroy(None)
    assert _lib.load().wan_attn_sparse_listed(None) == 0
