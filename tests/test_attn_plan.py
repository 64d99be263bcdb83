"""The attention front end answers what the commit before it answered: wan_attention_plan / wan_attention_workspace_bytes over the
shapes the project runs (x flags x workspace sizes x tuning keys), and status + message of calls the validator rejects.  Host
arithmetic and argument checks only -- every call here returns before any HIP call, so the pointers are made-up numbers.

tests/golden/attn_plan_parent.json was recorded from the library of the commit that still had the host code inside attn_fwd.hip:
    WAN_HIP_LIB=<that build>/libwan_hip.so python tests/test_attn_plan.py --record tests/golden/attn_plan_parent.json
(the two rejections that build reached only behind its LDS reservation -- softmax_scale, workspace alignment -- on a box with a GPU)."""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_plan_parent.json")
L = 67080
# (batch, Lq, Lk, heads, head_dim)
SHAPES = ([(1, L, L, h, 128) for h in (40, 5, 3, 2)] + [(1, 2304, 2304, 12, 128), (1, 32760, 32760, 12, 128), (2, 75600, 75600, 40, 128),
          (1, L, 512, 40, 128), (1, 13568, 13568, 5, 128)] + [(1, lq, 2304, 12, 128) for lq in (1, 255, 256, 257)] +
          [(1, 2304, lk, 12, 128) for lk in (1024, 1025)] + [(1, L, L, 5, 64)])
FLAGS = (0, 1, 1 | 2, 1 | 2 | 4)                 # WAN_ATTN_Q_PRESCALED, | WAN_ATTN_QK_FP8, | WAN_ATTN_PV_FP8
TUNE_KEYS = (b"attn_fast", b"attn_tail", b"attn_xcd_map", b"attn_ref")
TUNE_VALUES = tuple(itertools.product((0, 1, 2), (0, 1), (0, 1), (1, 2)))
TUNE_DEFAULT = (1, 1, 1, 1)


def flag_bytes(batch, lq, heads):
    return (16 + (lq + 255) // 256 * heads * batch * 4 + 255) // 256 * 256


def plan_rows(lib):
    rows = []
    try:
        for tune in TUNE_VALUES:
            for key, v in zip(TUNE_KEYS, tune):
                assert lib.wan_set_tuning(key, v) == 0
            for (b, lq, lk, h, d) in SHAPES:
                full = lib.wan_attention_workspace_bytes(b, lq, lk, h, d)
                fb = flag_bytes(b, lq, h)
                plans = [lib.wan_attention_plan(b, lq, lk, h, d, f, ws) for f in FLAGS for ws in (0, fb - 1, fb, full)]
                rows.append({"shape": [b, lq, lk, h, d], "tune": list(tune), "workspace_bytes": full, "plans": plans})
    finally:
        for key, v in zip(TUNE_KEYS, TUNE_DEFAULT):
            lib.wan_set_tuning(key, v)
    return rows


# ---- calls the validator rejects (and Lq = 0, the one valid call: WAN_OK before anything else is looked at)
def _args(entry, **over):
    a = dict(q=0x1000, ldq=128, q_bs=0, q_exp=0, k=0x2000, ldk=128, k_bs=0, k_exp=0, v8=0x5000, ldv8=64, v8_bs=0, vs8=0x6000,
             vt=0x3000, ldvt=64, vt_bs=0, out=0x4000, ldo=128, o_bs=0, batch=1, Lq=8, Lk=8, k_lens=0x7000, heads=1, dim=128,
             scale=0.125, flags=0, ws=None, ws_bytes=0)
    if entry == "wan_attention_fwd_f8":
        a.update(ws=0x8000, ws_bytes=1 << 20)
    assert set(over) <= set(a), over
    a.update(over)
    qkv = [a["q"], a["ldq"], a["q_bs"], a["k"], a["ldk"], a["k_bs"]]
    qkv8 = [a["q"], a["ldq"], a["q_bs"], a["q_exp"], a["k"], a["ldk"], a["k_bs"], a["k_exp"]]
    vto = [a["vt"], a["ldvt"], a["vt_bs"], a["out"], a["ldo"], a["o_bs"]]
    dims = [a["batch"], a["Lq"], a["Lk"], a["heads"], a["dim"]]
    tail = [a["ws"], a["ws_bytes"], None]
    return {"wan_attention_fwd": qkv + vto + dims + [a["scale"], a["flags"]] + tail,
            "wan_attention_fwd_varlen": qkv + vto + dims[:3] + [a["k_lens"]] + dims[3:] + [a["scale"], a["flags"]] + tail,
            "wan_attention_fwd_qk8": qkv8 + vto + dims + tail,
            "wan_attention_fwd_f8": qkv8 + [a["v8"], a["ldv8"], a["v8_bs"], a["vs8"]] + vto + dims + tail}[entry]


FWD, VARLEN, QK8, F8 = "wan_attention_fwd", "wan_attention_fwd_varlen", "wan_attention_fwd_qk8", "wan_attention_fwd_f8"
CALLS = [
    (FWD, dict(Lq=0)),                                                                   # valid: WAN_OK
    (FWD, dict(q=None)), (FWD, dict(out=None)), (VARLEN, dict(vt=None)), (QK8, dict(k=None)), (F8, dict(v8=None)), (F8, dict(vs8=None)),
    (VARLEN, dict(k_lens=None)), (VARLEN, dict(k_lens=0x7002)),
    (FWD, dict(flags=2)), (FWD, dict(flags=8)), (VARLEN, dict(flags=4)),
    (FWD, dict(dim=64)), (VARLEN, dict(dim=64)), (QK8, dict(dim=64)), (F8, dict(dim=64)),
    (FWD, dict(batch=0)), (FWD, dict(Lk=0)), (FWD, dict(heads=0)), (FWD, dict(Lq=-1)),
    (FWD, dict(heads=2)), (FWD, dict(ldk=132)), (FWD, dict(ldo=130)), (QK8, dict(ldq=136)), (QK8, dict(q=0x1008)), (QK8, dict(k_bs=8)),
    (FWD, dict(Lk=100, ldvt=64)), (FWD, dict(ldvt=68)), (F8, dict(Lk=65, ldvt=128, ldv8=64)), (F8, dict(ldv8=72)), (F8, dict(vs8=0x6002)),
    (QK8, dict(q_exp=101)), (QK8, dict(k_exp=-101)), (F8, dict(q_exp=-101)),
    (F8, dict(ws=None, ws_bytes=0)), (F8, dict(ws_bytes=255)),
    (FWD, dict(ws=0x8008, ws_bytes=1 << 20)), (VARLEN, dict(ws=0x8004, ws_bytes=1 << 20)), (QK8, dict(ws=0x8008, ws_bytes=1 << 20)),
    (F8, dict(ws=0x8008, ws_bytes=1 << 20)),
    (FWD, dict(scale=0.0)), (FWD, dict(scale=-0.125)), (FWD, dict(scale=float("inf"))), (VARLEN, dict(scale=0.0)),
]


def call_rows(lib, calls=CALLS):
    rows = []
    for entry, over in calls:
        status = getattr(lib, entry)(*_args(entry, **over))
        rows.append({"entry": entry, "override": {k: repr(v) for k, v in over.items()}, "status": status,
                     "error": lib.wan_last_error().decode() if status != 0 else ""})
    return rows


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_plan_and_workspace_answers_did_not_move():
    from videocof_amd import _lib
    want, got = _golden()["plans"], plan_rows(_lib.load())
    assert len(got) == len(want) == len(SHAPES) * len(TUNE_VALUES)
    for w, g in zip(want, got):
        assert g == w, (w, g)
    for key, v in zip(TUNE_KEYS, TUNE_DEFAULT):
        assert _lib.load().wan_get_tuning(key) == v


def test_rejected_calls_keep_status_and_message():
    """The pointers of CALLS are made-up numbers, and this test also runs where there is a GPU: it relies on every row being turned
    away (or, for Lq = 0, answered) before any launch.  The table is therefore walked one call at a time and stops at the first row
    that does not give the recorded answer, so that a validator that lets one row through is reported by that row."""
    from videocof_amd import _lib
    want = _golden()["calls"]
    assert len(want) == len(CALLS)
    assert want[0]["status"] == 0 and all(w["status"] != 0 for w in want[1:])
    for w, call in zip(want, CALLS):
        assert call_rows(_lib.load(), [call]) == [w], w


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from videocof_amd import _lib
    assert sys.argv[1] == "--record"
    with open(sys.argv[2], "w") as f:
        json.dump({"plans": plan_rows(_lib.load()), "calls": call_rows(_lib.load())}, f, separators=(",", ":"))
        f.write("\n")
