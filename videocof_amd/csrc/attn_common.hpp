// What attn_api.cpp (entry points, validator, plan) and attn_fwd.hip (kernels, their table, the launch function) share.  Internal.
#pragma once
#include "common.hpp"

// geometry the host arithmetic needs: a workgroup is 256 queries of one (batch, head), KV tiles are 64 keys, head_dim 128 only
constexpr int kWanAttnD = 128, kWanAttnQPerWG = 256, kWanAttnKV = 64;

// One attention call as the four C entry points receive it (wan_hip.h documents the operands).
struct WanAttnCall {
    const void* q; int64_t ldq, q_bs;          // bf16, or -- with `qk8` -- e4m3 whose strides count BYTES
    const void* k; int64_t ldk, k_bs;
    const void* vt; int64_t ldvt, vt_bs;
    void* out; int64_t ldo, o_bs;
    int batch, Lq, Lk, num_heads, head_dim;
    float softmax_scale; int flags;
    void* workspace; int64_t workspace_bytes;
    const int* k_lens;                         // _varlen: device array of batch key counts, or NULL
    bool qk8; int q_exp, k_exp;                // _qk8 / _f8: q and k are e4m3 with these scale exponents
    const void* v8; int64_t ldv8, v8_bs; const void* vs8;      // _f8: the MX e4m3 V^T and its scales, or NULL (bf16 P.V)
    const int* sp_row_ptr; const int* sp_tiles;                // _sparse: the plan's device lists (validated when it was created), or NULL
};

// Split-KV tail round (plan_tail in attn_api.cpp): the last `tq` query blocks of every (batch, head) leave the main launch
struct WanAttnTail { int tq = 0, nsplit = 1, tiles_per_split = 0, main_qb = 0, rows_tail = 0; int64_t ws_bytes = 0; };

// Every dispatch decision of one call (plan_attention in attn_api.cpp is the only place that takes them).
struct WanAttnPlan {
    WanAttnTail tail;
    int family = WAN_ATTN_VARIANT_W4_LAZY;      // the low bits of `variant`.  LAZY / LAZY_QK8: one launch; MAXFREE / F8: the checked attempt, then the fix-up on the same grid
    bool self = false;          // long KV stream (Lk > 1024): the attn_self instantiations; otherwise attn_cross
    bool ref2 = false;          // lazy reference in the packed-shift form (REF = 2) instead of the accumulator form (REF = 1)
    bool xcd = false;           // heads pinned to XCDs
    bool sparse = false;        // listed key tiles per query block (wan_attention_fwd_sparse): ONE launch of the lazy form, no scratch
    bool persist = false; int persist_grid = 0;     // cross-attention: `persist_grid` resident workgroups walk the `nwg` query blocks
    int64_t nwg = 0;            // workgroups (query blocks x heads x batch) of the main launch
    int64_t flag_bytes = 0;     // scratch layout: [flag_bytes: 16-byte header + one int per workgroup of the un-split grid][tail partials]
    bool scratch = false;       // the caller's workspace holds at least the flags
    int variant = 0;            // WAN_ATTN_VARIANT_* bits: what wan_attention_plan answers and "last_attn_variant" reports
};

inline int64_t wan_vt_mx_scale_bytes_per_head(int Lk) { return (int64_t)((Lk + kWanAttnKV - 1) / kWanAttnKV) * 256; }

// attn_fwd.hip, validated calls only.  A plan the table of instantiations does not hold is WAN_ERR_UNSUPPORTED.
wan_status_t wan_attn_launch(const WanAttnCall& c, const WanAttnPlan& plan, hipStream_t st);
// the synchronising `debug_checks` contract check: the V^T pad columns [Lk, roundup(Lk, 64)) must be finite
wan_status_t wan_attn_check_vt_padding(const WanAttnCall& c, hipStream_t st);
