"""-m gpu: the row kernels of the DiT block (LN-modulate, RMSNorm+RoPE, every output form, 1, 2 and 4 rows per workgroup) write, byte
for byte, what the commit before their one-row and R-rows bodies were merged wrote.

csrc/norm_kernels.hip has ONE body per operation, the rows per workgroup a template parameter, so
test_row_kernels_rows_per_workgroup_are_bitwise_the_one_row_kernels (test_gpu_kernels.py) compares instantiations of the same source.
The independent statement is this fixture: for seeded inputs, the sha256 of each output's bytes (the kernels have no atomics and are
bitwise reproducible), recorded on an MI355X from the PARENT commit's library -- which ran separately written one-row kernels for
row_group = 1, for dim > 6144 and for the fp8 form -- through this tree's unchanged `ops` API:
    WAN_HIP_LIB=<parent build>/libwan_hip.so python tests/test_gpu_row_kernels_parent.py --record
Recording asserts that the parent's bytes do not depend on row_group, so the fixture holds one hash per form.  Next to them it holds
the hash of the inputs: a mismatch there says the generator changed, not the kernels.

dim -> float4 per thread of LN-modulate / 16-byte chunks per thread of RMSNorm+RoPE: 256 -> 1 / 1, 1536 -> 2 / 1, 5120 -> 5 / 3,
7168 -> 7 (above 6: one row per workgroup whatever row_group says) / 4, 8192 -> 8 / 4.  27 rows = 3 samples of 9: a ragged last group
for 2 and 4 rows per workgroup, and sample boundaries inside a group.  No tolerance: equality.
"""
import hashlib
import json
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.append(ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "row_kernels_parent.json")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = (256, 1536, 5120, 7168, 8192)
ROWS_PER_BATCH, B, P, HEAD_DIM = 9, 3, 2, 128
ROW_GROUPS = (1, 2, 4)


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _inputs(dim):
    g = torch.Generator().manual_seed(1500 + dim)
    rows = ROWS_PER_BATCH * B
    ang = torch.rand(1024, HEAD_DIM // 2, generator=g) * (2 * math.pi)
    t = dict(x=torch.randn(rows, dim, generator=g), sc=torch.randn(B, dim, generator=g), sh=torch.randn(B, dim, generator=g),
             qk=torch.randn(rows, 2 * dim + 16, generator=g).to(torch.bfloat16),          # two column views, row stride 2 * dim + 16
             w0=torch.rand(dim, generator=g) + 0.5, w1=torch.rand(dim, generator=g) + 0.5, cos=ang.cos(), sin=ang.sin())
    return _sha(*(t[k] for k in sorted(t))), {k: v.to(DEV) for k, v in t.items()}


def run_forms(t, dim):
    """form -> sha256 of what the current row_group writes for inputs `t`."""
    from videocof_amd import ops
    from videocof_amd._lib import RopeParams
    rows, eps = ROWS_PER_BATCH * B, 1e-6
    rope = (t["cos"], t["sin"])
    rp = RopeParams(3, 3, 5, 2, 1, 2, 4, ROWS_PER_BATCH, 1024)      # CoF map of a (3, 3, 5) grid, tokens 4..12 of its 45
    # paired map, tokens 40..48: the last four rows of every sample are past the grid (they pass unrotated); positions clamped to 2 table rows
    rp_edge = RopeParams(3, 3, 5, 1, 1, 2, 40, ROWS_PER_BATCH, 2)
    q, k, w0, w1 = t["qk"][:, :dim], t["qk"][:, dim:2 * dim], t["w0"], t["w1"]
    res = {}
    res["ln"] = _sha(ops.ln_modulate(t["x"], t["sc"], t["sh"], True, ROWS_PER_BATCH, eps))
    res["ln_plain"] = _sha(ops.ln_modulate(t["x"], None, None, False, ROWS_PER_BATCH, eps))
    q8, s8 = ops.ln_modulate_fp8(t["x"], t["sc"], t["sh"], True, ROWS_PER_BATCH, eps)
    res["ln_fp8"] = _sha(q8.view(torch.uint8), s8)
    a = t["qk"].clone()
    ops.rmsnorm_rope_(a[:, :dim], w0, a[:, dim:2 * dim], w1, HEAD_DIM, eps, rope, rp, x0_scale=0.37)
    res["rms_in_place"] = _sha(a)                                    # the pad columns too: nothing outside the views is written
    a = t["qk"].clone()
    ops.rmsnorm_rope_(a[:, :dim], w0, a[:, dim:2 * dim], w1, HEAD_DIM, eps, rope, rp_edge)
    res["rms_in_place_past_grid"] = _sha(a)
    nr = q.clone()
    ops.rmsnorm_rope_(nr, w0, None, None, HEAD_DIM, eps)             # no rotation (the cross-attention q form)
    res["rms_no_rotation"] = _sha(nr)
    splits = [0] + ([(dim // P // 128 // 2) * 128] if dim // P >= 256 else [])
    for split in splits:
        wire0 = torch.zeros(rows * dim, device=DEV, dtype=torch.bfloat16)
        wire1 = torch.zeros_like(wire0)
        ops.rmsnorm_rope_sp(q, w0, k, w1, HEAD_DIM, eps, rope, rp, wire0, wire1, P, B, x0_scale=0.37, split=split)
        res["rms_wire_split" if split else "rms_wire"] = _sha(wire0, wire1)
    o0 = torch.zeros(rows, dim, device=DEV, dtype=ops.FP8)
    o1 = torch.zeros_like(o0)
    ops.rmsnorm_rope_fp8(q, w0, k, w1, HEAD_DIM, eps, rope, rp, o0, o1, x0_scale=4.0, x1_scale=2.0)
    res["rms_e4m3"] = _sha(o0.view(torch.uint8), o1.view(torch.uint8))
    torch.cuda.synchronize()
    return res


def run_dim(dim):
    """(sha256 of the inputs, {row_group: {form: sha256}})."""
    from videocof_amd import ops
    digest, t = _inputs(dim)
    keep = _sha(t["qk"])
    res = {}
    for R in ROW_GROUPS:
        ops.set_tuning("row_group", R)
        try:
            res[R] = run_forms(t, dim)
        finally:
            ops.set_tuning("row_group", 2)
    assert _sha(t["qk"]) == keep                                     # the wire and e4m3 forms leave their inputs alone
    return digest, res


@pytest.mark.parametrize("dim", DIMS)
def test_row_kernels_write_what_the_parent_wrote(dim):
    with open(GOLDEN) as f:
        want = json.load(f)["dims"][str(dim)]
    digest, got = run_dim(dim)
    assert digest == want["inputs"], "the seeded inputs differ from the recorded ones: the fixture does not apply"
    for R in ROW_GROUPS:
        assert set(got[R]) == set(want["forms"]), (dim, R)
        for form in sorted(want["forms"]):
            assert got[R][form] == want["forms"][form], f"dim {dim}, row_group {R}, {form}: not the parent's bytes"


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", nargs="?", const=GOLDEN, required=True, metavar="PATH")
    out = ap.parse_args().record
    from videocof_amd import _lib
    dims = {}
    for dim in DIMS:
        digest, got = run_dim(dim)
        for R in ROW_GROUPS[1:]:
            assert got[R] == got[ROW_GROUPS[0]], f"dim {dim}: row_group {R} and {ROW_GROUPS[0]} differ in this library"
        dims[str(dim)] = {"inputs": digest, "forms": got[ROW_GROUPS[0]]}
    with open(out, "w") as f:
        json.dump({"dims": dims}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"library {_lib.LIB_PATH}: {len(dims)} dims, {sum(len(d['forms']) for d in dims.values())} forms -> {out}")
