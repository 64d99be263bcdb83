"""The rule of the folded cross-attention branch -- wan_cross_fold_plan, host arithmetic of the library (include/wan_hip.h a9f) --
mirrored here line by line, and held against the shapes the launch traces of tests/golden/dit_block_paths_parent.json were
recorded at: none of them may fold under the default tuning, or those traces and output hashes would move.  No GPU."""
import itertools
import json
import os

import pytest

from videocof_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT_LEN = 512


def min_rows():
    """WAN_CROSS_FOLD_MIN_ROWS as the library was built with (cross_fold.hip): read from the source, not restated."""
    for line in open(os.path.join(ROOT, "videocof_amd", "csrc", "cross_fold.hip")):
        if line.startswith("#define WAN_CROSS_FOLD_MIN_ROWS"):
            return int(line.split()[2])
    raise AssertionError("WAN_CROSS_FOLD_MIN_ROWS not found")


def rule(rows, heads, text_len, kept, bf16, mode, threshold):
    """The mirror: fold when the weights are bf16, 1 <= kept, kept + 1 <= 64, kept < text_len (kept = text_len: not known),
    and -- unless mode 2 -- 64 H >= 1024, 64 H % 128 == 0 and rows >= the measured crossover."""
    if mode <= 0 or not bf16 or rows <= 0 or heads <= 0:
        return 0
    if kept < 1 or kept + 1 > 64 or kept >= text_len:
        return 0
    if mode >= 2:
        return 1
    k = heads * 64
    if k < 1024 or k % 128 != 0:
        return 0
    return 1 if rows >= threshold else 0


@pytest.fixture()
def lib():
    lib = _lib.load()
    assert lib.wan_get_tuning(b"cross_fold") == 1          # the default: by rule
    yield lib
    lib.wan_set_tuning(b"cross_fold", 1)


def test_rule_table(lib):
    thr = min_rows()
    assert thr > 2 * 448, "the recorded trace shapes (<= 2 x 448 rows) must stay below the crossover"
    rows = (1, 8, 420, 840, thr - 1, thr, thr + 1, 8192, 32760, 67080, 2 * 75600)
    heads = (1, 2, 8, 12, 15, 16, 17, 24, 40)
    kepts = (0, 1, 5, 37, 62, 63, 64, 100, 511, 512)
    for mode in (0, 1, 2):
        lib.wan_set_tuning(b"cross_fold", mode)
        for r, h, kept, bf16 in itertools.product(rows, heads, kepts, (0, 1)):
            got = lib.wan_cross_fold_plan(r, h, TEXT_LEN, kept, bf16)
            assert got == rule(r, h, TEXT_LEN, kept, bf16, mode, thr), (mode, r, h, kept, bf16)
    lib.wan_set_tuning(b"cross_fold", 1)
    # the headline shapes: 14B (40 heads) folds at the bench prompt, 1.3B (12 heads: 64 H = 768) does not
    assert lib.wan_cross_fold_plan(67080, 40, TEXT_LEN, 37, 1) == 1
    assert lib.wan_cross_fold_plan(32760, 12, TEXT_LEN, 37, 1) == 0
    assert lib.wan_cross_fold_plan(67080, 40, TEXT_LEN, 64, 1) == 0        # a 64-token prompt: 65 distinct keys
    assert lib.wan_cross_fold_plan(67080, 40, TEXT_LEN, TEXT_LEN, 1) == 0  # prompt length not known
    assert lib.wan_cross_fold_plan(67080, 40, TEXT_LEN, 37, 0) == 0        # e4m3 output projection ("cross")


def _cross_attention_shapes():
    """(config, rows, heads) of every cross-attention launch in the recorded traces (the per-op paths record ops.attention_fwd
    with the call site's workspace; the composites run the same shapes inside one C call)."""
    data = json.load(open(os.path.join(ROOT, "tests", "golden", "dit_block_paths_parent.json")))["configs"]
    found = []
    for name, cfg in data.items():
        for rec in cfg["trace"]:
            if rec[0] != "attention_fwd":
                continue
            ws = rec[2].get("workspace")
            if isinstance(ws, list) and ws[0] == "workspace" and ws[1].startswith("cross"):
                shape = rec[1][0][3]                       # q: ("T", storage, offset, shape, stride, dtype)
                found.append((name, shape[0] * shape[1], shape[2] // 128))
    return found


def test_recorded_trace_shapes_do_not_fold(lib):
    shapes = _cross_attention_shapes()
    assert len(shapes) >= 8
    for name, rows, heads in shapes:
        for kept in (5, 37):                               # the prompts of those forwards
            assert lib.wan_cross_fold_plan(rows, heads, TEXT_LEN, kept, 1) == 0, (name, rows, heads, kept)
    # ... and by the rule's own arithmetic for every model those tests build (<= 4 heads, <= 2 x 448 rows)
    for heads, rows, kept in itertools.product(range(1, 9), (420, 448, 840, 896), range(1, 64)):
        assert lib.wan_cross_fold_plan(rows, heads, TEXT_LEN, kept, 1) == 0


def test_workspace_bytes_and_argument_checks(lib):
    assert lib.wan_cross_fold_workspace_bytes(1, 5120) == 5120 * 2560 * 2          # the 26 MB of V'^T at 14B width
    assert lib.wan_cross_fold_workspace_bytes(2, 256) == 2 * 256 * 128 * 2
    assert lib.wan_cross_fold_workspace_bytes(1, 100) == 0
    # validation happens before any launch: no GPU needed
    assert lib.wan_cross_probs(None, 256, None, 256, 512 * 256, None, 128, 1, 8, 2, 37, 475, None) == _lib.WAN_ERR_INVALID
    assert lib.wan_cross_probs(16, 256, 16, 256, 512 * 256, 16, 128, 1, 8, 2, 64, 448, None) == _lib.WAN_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="kept"):
        _lib.check(_lib.WAN_ERR_UNSUPPORTED, "wan_cross_probs")
    assert lib.wan_cross_probs(16, 256, 16, 256, 512 * 256, 16, 100, 1, 8, 2, 37, 475, None) == _lib.WAN_ERR_INVALID      # ldp < 64 H
    assert lib.wan_cross_fold_values(16, 256, 16, 512, 256 * 512, 16, 128, 256 * 128, 1, 256, 2, 64, None) == _lib.WAN_ERR_UNSUPPORTED
    assert lib.wan_cross_fold_values(16, 256, 16, 512, 256 * 512, 16, 128, 256 * 128, 1, 300, 2, 37, None) == _lib.WAN_ERR_UNSUPPORTED
    assert lib.wan_cross_fold_values(8, 256, 16, 512, 256 * 512, 16, 128, 256 * 128, 1, 256, 2, 37, None) == _lib.WAN_ERR_INVALID   # alignment


def test_block_workspace_layout():
    """wan_block_workspace grew at its END (vfold, vfold_bytes, text_kept): a zero-initialised tail keeps the plain branch."""
    names = [f[0] for f in _lib.BlockWorkspace._fields_]
    assert names[-3:] == ["vfold", "vfold_bytes", "text_kept"] and names[-5:-3] == ["gemm_ws", "gemm_ws_bytes"]
    ws = _lib.BlockWorkspace()
    assert ws.vfold is None and ws.vfold_bytes == 0 and ws.text_kept == 0
    assert _lib.BlockWorkspace.vfold.offset == _lib.BlockWorkspace.gemm_ws_bytes.offset + 8
