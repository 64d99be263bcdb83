// Attention: the C entry points, their one validator and the host arithmetic that plans a call; wan_attn_launch (attn_fwd.hip)
// carries the plan out.
#include <algorithm>

#include "attn_common.hpp"

namespace {
constexpr int kD = kWanAttnD, kQPerWG = kWanAttnQPerWG, kKV = kWanAttnKV;

// Tail balancing.  Every workgroup of a launch costs the same (all stream the whole K/V of their head) and one fits per CU, so W
// workgroups take ceil(W / CUs) rounds and the last round may be nearly empty: the 5 heads of an 8-way Ulysses shard at L = 67 080 give
// 1315 = 5 x 256 + 35 workgroups -> 6 rounds for 5.14 rounds of work (measured 1007 vs 1165 TFLOP/s).  When the remainder is small, the
// last `tq` query blocks of every (batch, head) leave the main launch; a second launch covers them with the SPLIT form of the same kernel,
// each workgroup taking 1/nsplit of the keys (so that the tail fills the chip for 1/nsplit of a round), and a small kernel merges the
// partial (O, max, sum) triples.  Needs caller-provided workspace; without it the plain launch runs.
WanAttnTail plan_tail(int batch, int Lq, int Lk, int num_heads) {
    WanAttnTail p;
    const int ncu = wan_cu_count();
    const int nqb = (Lq + kQPerWG - 1) / kQPerWG, nkv = (Lk + kKV - 1) / kKV;
    p.main_qb = nqb;
    const int64_t hb = (int64_t)num_heads * batch, items = hb * nqb;
    if (wan_tune(WAN_TUNE_ATTN_TAIL) == 0 || Lk <= 1024 || items <= ncu || items % ncu == 0) return p;
    const int64_t rem = items % ncu;
    const int cand = (int)((rem + hb - 1) / hb);        // query blocks per (batch, head) moved to the tail launch
    if (cand >= nqb) return p;
    const int64_t tail_items = hb * cand, main_items = hb * (nqb - cand);
    int nsplit = (int)std::min<int64_t>(std::min<int64_t>(ncu / tail_items, nkv / 8), 16);
    if (nsplit < 2) return p;
    const int tps = (nkv + nsplit - 1) / nsplit;
    nsplit = (nkv + tps - 1) / tps;                     // no empty split
    const double before = (double)((items + ncu - 1) / ncu);
    const double after = (double)((main_items + ncu - 1) / ncu) + 1.0 / nsplit + 0.05;
    if (nsplit < 2 || after > before - 0.2) return p;
    p.tq = cand; p.nsplit = nsplit; p.tiles_per_split = tps; p.main_qb = nqb - cand;
    p.rows_tail = Lq - p.main_qb * kQPerWG;
    p.ws_bytes = (int64_t)batch * nsplit * num_heads * p.rows_tail * (kD + 2) * (int64_t)sizeof(float);
    return p;
}

// scratch layout: [16-byte header + one int per workgroup of the un-split grid, rounded up to 256 B][partials of the
// split tail round].  The header must be zero when the scratch is first used (it carries the sticky switch).
int64_t flag_bytes(int batch, int Lq, int num_heads) {
    const int64_t wgs = (int64_t)((Lq + kQPerWG - 1) / kQPerWG) * num_heads * batch;
    return (16 + wgs * (int64_t)sizeof(int) + 255) / 256 * 256;
}

// The dispatch decision, once per call: wan_attention_plan answers `variant` of it, wan_attn_launch carries all of it out.
// With scratch memory: (1) pre-scaled q first runs the max-free form, then the FIX launch of the lazy form on the flagged workgroups
// only; (2) the last partial round of a long launch is split over the keys (plan_tail).  Without scratch (or attn_fast = 0): ONE
// launch of the lazy form.  `ragged`: a k_lens call.  The attn_* tuning keys are developer A/B switches.
WanAttnPlan plan_attention(int batch, int Lq, int Lk, int num_heads, bool pre, bool qk8, bool pv8, bool ragged, int64_t workspace_bytes) {
    WanAttnPlan p;
    p.self = Lk > 1024;
    const int nqb_all = (Lq + kQPerWG - 1) / kQPerWG;
    // plain q always takes the packed-shift form (it applies softmax_scale exactly, in the same fma); pre-scaled q the
    // accumulator form unless the developer switch asks for the other; the fp8 QK^T kernels are accumulator-form kernels
    p.ref2 = !qk8 && (!pre || wan_tune(WAN_TUNE_ATTN_REF) == 2);
    p.flag_bytes = flag_bytes(batch, Lq, num_heads);
    p.scratch = workspace_bytes >= p.flag_bytes;
    bool fast = false;
    if (p.scratch) {
        // the attempt is worth its second launch (~5-15 us of workgroups that exit at once) only on long launches: self-attention
        // over >= 4 rounds of workgroups, or -- round 6 -- fewer rounds of LONG key streams (rounds x KV tiles >= 1024, i.e. >= ~1.5 ms of
        // launch at ~1.5 us per tile: the 2- and 3-head launches of an 8-way Ulysses rank at L = 67 080 are 2.05 / 3.08 rounds of 1 049
        // tiles and sat on the lazy form until `bench.py --emulate-sp 8` showed it); short launches (cross-attention's 8 KV tiles,
        // small grids) take the one-launch lazy form.  attn_fast = 2 forces the attempt whenever there is scratch (tests)
        const int fast_mode = wan_tune(WAN_TUNE_ATTN_FAST);
        const int64_t nwg_all = (int64_t)nqb_all * num_heads * batch, cus = wan_cu_count();
        const int64_t rounds = (nwg_all + cus - 1) / cus, kv_tiles = (Lk + kKV - 1) / kKV;
        const bool long_launch = p.self && (nwg_all >= 4 * cus || rounds * kv_tiles >= 1024);
        fast = pre && !qk8 && (fast_mode == 2 || (fast_mode == 1 && long_launch));
        // ragged batches: the split-KV tail round divides ONE key count, but every workgroup walks its own
        if (!ragged) p.tail = plan_tail(batch, Lq, Lk, num_heads);
        if (p.tail.tq > 0 && workspace_bytes - p.flag_bytes < p.tail.ws_bytes) p.tail = WanAttnTail();
    }
    p.nwg = (int64_t)(p.tail.tq > 0 ? p.tail.main_qb : nqb_all) * num_heads * batch;
    // heads pinned to XCDs: only worth it (and only balanced) when the (batch, head) pairs split evenly over the 8 XCDs
    p.xcd = wan_tune(WAN_TUNE_ATTN_XCD_MAP) != 0 && p.self && (num_heads * batch) % 8 == 0;
    // F8 (opt-in, lossy): checked max-free form with both products in fp8, flagged workgroups redone by the fp8-QK^T lazy kernel;
    // QK8 (opt-in, lossy): the lazy kernel with its S product on the fp8 pipe; else the max-free attempt (2 % faster) or the lazy kernel alone
    p.family = qk8 && pv8 && p.scratch ? WAN_ATTN_VARIANT_W4_F8 : qk8 ? WAN_ATTN_VARIANT_W4_LAZY_QK8
               : fast ? WAN_ATTN_VARIANT_W4_MAXFREE : WAN_ATTN_VARIANT_W4_LAZY;
    if (p.family == WAN_ATTN_VARIANT_W4_LAZY && !p.self) {
        // short KV streams (cross-attention: 8 tiles per query block): ONE resident workgroup per CU walks the blocks (PERSIST, see the
        // kernel); the grid stays a multiple of 8 so that w & 7 -- the XCD a head is pinned to -- is the same for every block of a workgroup
        // (wan_resident_cus: the CUs tuning key "sp_reserve_cus" leaves to communication kernels are not occupied)
        p.persist_grid = wan_resident_cus() & ~7;
        p.persist = wan_tune(WAN_TUNE_ATTN_PERSIST) != 0 && p.nwg > p.persist_grid && p.persist_grid >= 8;
    }
    p.variant = p.family;
    if (p.xcd) p.variant |= WAN_ATTN_VARIANT_XCD_PINNED;
    if (p.tail.tq > 0) p.variant |= WAN_ATTN_VARIANT_SPLIT_TAIL;
    return p;
}

// Every argument check of the four entry points, in the order callers have seen them fail; no HIP call is made before they pass.
// Lq == 0 is a valid empty call: what follows its place in the order is not asked of it.
wan_status_t validate(const WanAttnCall& c) {
    WAN_REQUIRE(c.q && c.k && c.vt && c.out, WAN_ERR_INVALID, "wan_attention_fwd: null tensor");
    WAN_REQUIRE((c.flags & ~WAN_ATTN_Q_PRESCALED) == 0, WAN_ERR_INVALID, "wan_attention_fwd: unknown flags 0x%x", c.flags);
    WAN_REQUIRE(c.head_dim == kD, WAN_ERR_UNSUPPORTED, "wan_attention_fwd: head_dim=%d (only 128 is built)", c.head_dim);
    WAN_REQUIRE(c.batch > 0 && c.Lq >= 0 && c.Lk > 0 && c.num_heads > 0, WAN_ERR_INVALID,
                "wan_attention_fwd: batch=%d Lq=%d Lk=%d heads=%d", c.batch, c.Lq, c.Lk, c.num_heads);
    const int64_t C = (int64_t)c.num_heads * kD;
    WAN_REQUIRE(c.ldq >= C && c.ldk >= C && c.ldo >= C && c.ldq % 8 == 0 && c.ldk % 8 == 0 && c.ldo % 4 == 0, WAN_ERR_INVALID,
                "wan_attention_fwd: row strides (%lld,%lld,%lld) too small/misaligned for %d heads",
                (long long)c.ldq, (long long)c.ldk, (long long)c.ldo, c.num_heads);
    if (c.qk8) {
        WAN_REQUIRE(c.ldq % 16 == 0 && c.ldk % 16 == 0 && ((uintptr_t)c.q & 15) == 0 && ((uintptr_t)c.k & 15) == 0 && c.q_bs % 16 == 0 &&
                        c.k_bs % 16 == 0, WAN_ERR_INVALID, "wan_attention_fwd_qk8: e4m3 rows must be 16-byte aligned");
        WAN_REQUIRE(c.q_exp >= -100 && c.q_exp <= 100 && c.k_exp >= -100 && c.k_exp <= 100, WAN_ERR_INVALID,
                    "wan_attention_fwd_qk8: scale exponents (%d, %d) out of range", c.q_exp, c.k_exp);
    }
    const int64_t lk_pad = ((int64_t)c.Lk + kKV - 1) / kKV * kKV;
    WAN_REQUIRE(c.ldvt >= lk_pad && c.ldvt % 8 == 0, WAN_ERR_INVALID,
                "wan_attention_fwd: ldvt=%lld must be >= roundup(Lk,64)=%lld and a multiple of 8", (long long)c.ldvt, (long long)lk_pad);
    if (c.v8) {
        WAN_REQUIRE(c.vs8 != nullptr && c.ldv8 >= lk_pad && c.ldv8 % 16 == 0 && c.v8_bs % 16 == 0 && ((uintptr_t)c.v8 & 15) == 0 &&
                        ((uintptr_t)c.vs8 & 3) == 0, WAN_ERR_INVALID,
                    "wan_attention_fwd_f8: v8 rows must be 16-byte aligned with ldv8=%lld >= roundup(Lk,64)=%lld, scales 4-byte aligned",
                    (long long)c.ldv8, (long long)lk_pad);
        WAN_REQUIRE(c.workspace != nullptr && c.workspace_bytes >= flag_bytes(c.batch, c.Lq, c.num_heads), WAN_ERR_INVALID,
                    "wan_attention_fwd_f8: needs the scratch of wan_attention_workspace_bytes (its softmax is the checked max-free form)");
    }
    if (c.Lq == 0) return WAN_OK;
    WAN_REQUIRE((c.flags & WAN_ATTN_Q_PRESCALED) != 0 || (c.softmax_scale > 0.f && c.softmax_scale < 1e30f), WAN_ERR_INVALID,
                "wan_attention_fwd: softmax_scale=%g must be positive and finite", (double)c.softmax_scale);
    WAN_REQUIRE(((uintptr_t)c.workspace & 15) == 0, WAN_ERR_INVALID, "wan_attention_fwd: workspace must be 16-byte aligned");
    return WAN_OK;
}

// Listed key tiles (wan_attention_fwd_sparse): ONE launch of the self-attention lazy form, whatever the shape -- no scratch, so no
// max-free attempt, and no split tail round (the workgroups of a sparse launch differ in length; plan_tail's arithmetic assumes they
// do not).  Heads are pinned to XCDs under the dense rule.
WanAttnPlan plan_sparse(int batch, int Lq, int num_heads, bool pre) {
    WanAttnPlan p;
    p.self = true;
    p.sparse = true;
    p.ref2 = !pre || wan_tune(WAN_TUNE_ATTN_REF) == 2;
    p.nwg = (int64_t)((Lq + kQPerWG - 1) / kQPerWG) * num_heads * batch;
    p.xcd = wan_tune(WAN_TUNE_ATTN_XCD_MAP) != 0 && (num_heads * batch) % 8 == 0;
    p.variant = p.family | WAN_ATTN_VARIANT_SPARSE | (p.xcd ? WAN_ATTN_VARIANT_XCD_PINNED : 0);
    return p;
}

// The list contract, in the order wan_hip.h states it.  Host arithmetic only: the kernel trusts every index it reads.
wan_status_t validate_lists(const int32_t* row_ptr, const int32_t* tiles, int n_qblocks, int n_ktiles) {
    WAN_REQUIRE(row_ptr && tiles, WAN_ERR_INVALID, "wan_attn_sparse: null list");
    WAN_REQUIRE(n_qblocks > 0 && n_ktiles > 0, WAN_ERR_INVALID, "wan_attn_sparse: n_qblocks=%d n_ktiles=%d", n_qblocks, n_ktiles);
    WAN_REQUIRE(row_ptr[0] == 0, WAN_ERR_INVALID, "wan_attn_sparse: row_ptr[0]=%d must be 0", row_ptr[0]);
    for (int b = 0; b < n_qblocks; ++b) {          // the offsets first: no tile is read through an offset that has not passed
        const int64_t lo = row_ptr[b], hi = row_ptr[b + 1];
        WAN_REQUIRE(hi >= lo, WAN_ERR_INVALID, "wan_attn_sparse: row_ptr decreases at query block %d (%lld -> %lld)", b, (long long)lo, (long long)hi);
        WAN_REQUIRE(hi > lo, WAN_ERR_INVALID, "wan_attn_sparse: query block %d lists no tile (an empty row)", b);
    }
    for (int b = 0; b < n_qblocks; ++b) {
        const int64_t lo = row_ptr[b], hi = row_ptr[b + 1];
        for (int64_t i = lo; i < hi; ++i) {
            WAN_REQUIRE(tiles[i] >= 0, WAN_ERR_INVALID, "wan_attn_sparse: query block %d lists the negative tile %d", b, tiles[i]);
            WAN_REQUIRE(tiles[i] < n_ktiles, WAN_ERR_INVALID, "wan_attn_sparse: query block %d lists tile %d beyond the last (n_ktiles=%d)", b, tiles[i], n_ktiles);
            if (i > lo) {
                WAN_REQUIRE(tiles[i] != tiles[i - 1], WAN_ERR_INVALID, "wan_attn_sparse: query block %d lists tile %d twice (a duplicate)", b, tiles[i]);
                WAN_REQUIRE(tiles[i] > tiles[i - 1], WAN_ERR_INVALID, "wan_attn_sparse: query block %d is not ascending (%d after %d)", b, tiles[i], tiles[i - 1]);
            }
        }
    }
    return WAN_OK;
}

wan_status_t attention_fwd(const WanAttnCall& c, void* stream) {
    const wan_status_t vs = validate(c);
    if (vs != WAN_OK || c.Lq == 0) return vs;
    if (wan_tune(WAN_TUNE_DEBUG_CHECKS) != 0 && c.k_lens == nullptr)         // synchronising contract check, developer builds / bring-up only
        if (const wan_status_t cs = wan_attn_check_vt_padding(c, (hipStream_t)stream); cs != WAN_OK) return cs;
    const WanAttnPlan plan = plan_attention(c.batch, c.Lq, c.Lk, c.num_heads, (c.flags & WAN_ATTN_Q_PRESCALED) != 0, c.qk8, c.v8 != nullptr,
                                            c.k_lens != nullptr, c.workspace != nullptr ? c.workspace_bytes : 0);
    WAN_REQUIRE(plan.nwg < (int64_t)1 << 31, WAN_ERR_UNSUPPORTED, "wan_attention_fwd: grid too large");
    return wan_attn_launch(c, plan, (hipStream_t)stream);
}
}  // namespace

extern "C" int wan_attention_plan(int batch, int Lq, int Lk, int num_heads, int head_dim, int flags, int64_t workspace_bytes) {
    if (batch <= 0 || Lq <= 0 || Lk <= 0 || num_heads <= 0 || head_dim != kD) return 0;
    return plan_attention(batch, Lq, Lk, num_heads, (flags & WAN_ATTN_Q_PRESCALED) != 0, (flags & WAN_ATTN_QK_FP8) != 0,
                          (flags & WAN_ATTN_PV_FP8) != 0, false, workspace_bytes).variant;
}

extern "C" int64_t wan_attention_workspace_bytes(int batch, int Lq, int Lk, int num_heads, int head_dim) {
    if (batch <= 0 || Lq <= 0 || Lk <= 0 || num_heads <= 0 || head_dim != kD) return 0;
    return flag_bytes(batch, Lq, num_heads) + plan_tail(batch, Lq, Lk, num_heads).ws_bytes;
}

extern "C" int64_t wan_vt_mx_scale_bytes(int batch, int num_heads, int Lk) {
    return batch > 0 && num_heads > 0 && Lk > 0 ? (int64_t)batch * num_heads * wan_vt_mx_scale_bytes_per_head(Lk) : 0;
}

extern "C" wan_status_t wan_attention_fwd(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk, int64_t k_bstride,
                                          const void* vt, int64_t ldvt, int64_t vt_bstride, void* out, int64_t ldo, int64_t o_bstride,
                                          int batch, int Lq, int Lk, int num_heads, int head_dim, float softmax_scale, int flags,
                                          void* workspace, int64_t workspace_bytes, void* stream) {
    const WanAttnCall c = {q, ldq, q_bstride, k, ldk, k_bstride, vt, ldvt, vt_bstride, out, ldo, o_bstride, batch, Lq, Lk, num_heads, head_dim,
                           softmax_scale, flags, workspace, workspace_bytes};
    return attention_fwd(c, stream);
}

extern "C" wan_status_t wan_attention_fwd_varlen(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk, int64_t k_bstride,
                                                 const void* vt, int64_t ldvt, int64_t vt_bstride, void* out, int64_t ldo, int64_t o_bstride,
                                                 int batch, int Lq, int Lk, const int32_t* k_lens, int num_heads, int head_dim,
                                                 float softmax_scale, int flags, void* workspace, int64_t workspace_bytes, void* stream) {
    WAN_REQUIRE(k_lens != nullptr && ((uintptr_t)k_lens & 3) == 0, WAN_ERR_INVALID, "wan_attention_fwd_varlen: k_lens must be a device array of batch int32");
    const WanAttnCall c = {q, ldq, q_bstride, k, ldk, k_bstride, vt, ldvt, vt_bstride, out, ldo, o_bstride, batch, Lq, Lk, num_heads, head_dim,
                           softmax_scale, flags, workspace, workspace_bytes, k_lens};
    return attention_fwd(c, stream);
}

extern "C" wan_status_t wan_attention_fwd_qk8(const void* q8, int64_t ldq8, int64_t q8_bstride, int q_exp,
                                              const void* k8, int64_t ldk8, int64_t k8_bstride, int k_exp,
                                              const void* vt, int64_t ldvt, int64_t vt_bstride, void* out, int64_t ldo, int64_t o_bstride,
                                              int batch, int Lq, int Lk, int num_heads, int head_dim, void* workspace, int64_t workspace_bytes, void* stream) {
    const WanAttnCall c = {q8, ldq8, q8_bstride, k8, ldk8, k8_bstride, vt, ldvt, vt_bstride, out, ldo, o_bstride, batch, Lq, Lk, num_heads, head_dim,
                           1.0f, WAN_ATTN_Q_PRESCALED, workspace, workspace_bytes, nullptr, true, q_exp, k_exp};
    return attention_fwd(c, stream);
}

extern "C" wan_status_t wan_attention_fwd_f8(const void* q8, int64_t ldq8, int64_t q8_bstride, int q_exp,
                                             const void* k8, int64_t ldk8, int64_t k8_bstride, int k_exp,
                                             const void* v8, int64_t ldv8, int64_t v8_bstride, const void* v8_scales,
                                             const void* vt, int64_t ldvt, int64_t vt_bstride, void* out, int64_t ldo, int64_t o_bstride,
                                             int batch, int Lq, int Lk, int num_heads, int head_dim, void* workspace, int64_t workspace_bytes, void* stream) {
    WAN_REQUIRE(v8 && v8_scales, WAN_ERR_INVALID, "wan_attention_fwd_f8: null tensor");
    const WanAttnCall c = {q8, ldq8, q8_bstride, k8, ldk8, k8_bstride, vt, ldvt, vt_bstride, out, ldo, o_bstride, batch, Lq, Lk, num_heads, head_dim,
                           1.0f, WAN_ATTN_Q_PRESCALED, workspace, workspace_bytes, nullptr, true, q_exp, k_exp, v8, ldv8, v8_bstride, v8_scales};
    return attention_fwd(c, stream);
}

// ---- listed key tiles per query block (local self-attention).  The plan is host-validated lists plus their one device copy.
struct wan_attn_sparse {
    int* d_lists = nullptr;     // row_ptr [n_qblocks + 1], then tiles [listed]
    int Lq = 0, Lk = 0, n_qblocks = 0, n_ktiles = 0;
    int64_t listed = 0;
};

extern "C" wan_status_t wan_attn_sparse_validate(const int32_t* row_ptr, const int32_t* tiles, int n_qblocks, int n_ktiles) {
    return validate_lists(row_ptr, tiles, n_qblocks, n_ktiles);
}

extern "C" wan_status_t wan_attn_sparse_create(const int32_t* row_ptr, const int32_t* tiles, int Lq, int Lk, wan_attn_sparse** out) {
    WAN_REQUIRE(out != nullptr, WAN_ERR_INVALID, "wan_attn_sparse_create: null out");
    *out = nullptr;
    WAN_REQUIRE(Lq > 0 && Lk > 0, WAN_ERR_INVALID, "wan_attn_sparse_create: Lq=%d Lk=%d", Lq, Lk);
    const int nqb = (Lq + kQPerWG - 1) / kQPerWG, nkt = (Lk + kKV - 1) / kKV;
    if (const wan_status_t vs = validate_lists(row_ptr, tiles, nqb, nkt); vs != WAN_OK) return vs;
    wan_attn_sparse* p = new wan_attn_sparse();
    p->Lq = Lq; p->Lk = Lk; p->n_qblocks = nqb; p->n_ktiles = nkt; p->listed = row_ptr[nqb];
    const size_t head = (size_t)(nqb + 1) * sizeof(int32_t), body = (size_t)p->listed * sizeof(int32_t);
    hipError_t e = hipMalloc((void**)&p->d_lists, head + body);
    if (e == hipSuccess) e = hipMemcpy(p->d_lists, row_ptr, head, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_lists + nqb + 1, tiles, body, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (p->d_lists) (void)hipFree(p->d_lists);
        delete p;
        wan_set_error("wan_attn_sparse_create: cannot upload the lists: %s", hipGetErrorString(e));
        return WAN_ERR_LAUNCH;
    }
    *out = p;
    return WAN_OK;
}

extern "C" void wan_attn_sparse_destroy(wan_attn_sparse* p) {
    if (p == nullptr) return;
    if (p->d_lists) (void)hipFree(p->d_lists);
    delete p;
}

extern "C" int64_t wan_attn_sparse_listed(const wan_attn_sparse* p) { return p ? p->listed : 0; }

extern "C" wan_status_t wan_attention_fwd_sparse(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk, int64_t k_bstride,
                                                 const void* vt, int64_t ldvt, int64_t vt_bstride, void* out, int64_t ldo, int64_t o_bstride,
                                                 int batch, int Lq, int Lk, const wan_attn_sparse* plan, int num_heads, int head_dim,
                                                 float softmax_scale, int flags, void* stream) {
    WAN_REQUIRE(plan != nullptr, WAN_ERR_INVALID, "wan_attention_fwd_sparse: null plan");
    WanAttnCall c = {q, ldq, q_bstride, k, ldk, k_bstride, vt, ldvt, vt_bstride, out, ldo, o_bstride, batch, Lq, Lk, num_heads, head_dim,
                     softmax_scale, flags, nullptr, 0};
    c.sp_row_ptr = plan->d_lists;
    c.sp_tiles = plan->d_lists + plan->n_qblocks + 1;
    if (const wan_status_t vs = validate(c); vs != WAN_OK) return vs;
    WAN_REQUIRE(Lq == plan->Lq && Lk == plan->Lk, WAN_ERR_INVALID, "wan_attention_fwd_sparse: Lq=%d Lk=%d, the plan was made for Lq=%d Lk=%d",
                Lq, Lk, plan->Lq, plan->Lk);
    const WanAttnPlan p = plan_sparse(batch, Lq, num_heads, (flags & WAN_ATTN_Q_PRESCALED) != 0);
    WAN_REQUIRE(p.nwg < (int64_t)1 << 31, WAN_ERR_UNSUPPORTED, "wan_attention_fwd_sparse: grid too large");
    return wan_attn_launch(c, p, (hipStream_t)stream);
}
