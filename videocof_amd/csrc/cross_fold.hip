// Cross-attention with the text values folded into the output projection ("the fold").
//
// The reference pads every prompt with zero rows to text_len BEFORE text_embedding and masks nothing (context_lens = None,
// videox_fun/models/wan_transformer3d.py:936), so every text row behind the longest prompt of a call is the same row in every layer.
// With `kept` rows scored one by one and ONE representative of the `pad_count` identical rows behind them (its score raised by
// log2(pad_count) in the exp2 domain, which is what pad_count equal terms of the softmax sum to), a head has kept + 1 <= 64
// distinct keys, and
//     att . W_co^T = sum_h (P_h V_h) W_co,h^T = sum_h P_h (V_h W_co,h^T) = P . V'
// so the output projection contracts over H * 64 probabilities instead of H * 128 channels.  Two kernels:
//     cross_probs_kernel  P  [rows, H * 64]   bf16  softmax over the distinct keys (columns > kept are exact zeros)
//     cross_fold_kernel   V'^T [C, H * 64]    bf16  V'^T[n, h * 64 + j] = sum_d W_co[n, h * 128 + d] V_h[j, d], nn.Linear layout
// Both are "a 64 x 128 per-head matrix (K_h or V_h) times 32-row blocks of a streamed matrix (q or W_co)": the small matrix is the
// A operand of v_mfma_f32_32x32x16_bf16 and stays in registers, the streamed rows are the B operand, read with 16-byte loads straight
// from global memory (every byte is used once: nothing to share through LDS), so that a lane ends up holding, for ITS streamed row,
// the 64 results of one head -- the softmax needs one exchange with lane ^ 32 and no LDS.  The rows of the small matrix are fed
// in a permuted order (perm_row) that makes a lane's 32 accumulators four runs of eight CONSECUTIVE columns: 16-byte stores.
// No scratch, no atomics; every access is predicated on its row.
#include "common.hpp"

#include <math.h>

namespace {

constexpr int CF_KEYS = 64;         // columns per head of P and of V'^T
constexpr int CF_D = 128;           // head_dim
constexpr int CF_PROB_NB = 8;       // 32-row query blocks per wave of cross_probs_kernel (K_h is fetched once per wave)
constexpr int CF_FOLD_NB = 2;       // 32-row blocks of W_co per wave of cross_fold_kernel (V_h is staged once per workgroup)
constexpr int CF_VS_LD = CF_D + 8;  // LDS row stride of the staged V_h in elements: 272 B, 16-byte aligned, rows 4 banks apart

// Row of the small matrix that row r (0..31) of MFMA tile t (0..1) carries.  Accumulator register 4 i + jj of a lane in half g
// (= lane >> 5) is tile row 8 i + 4 g + jj (C/D layout of the 32x32 MFMA), hence column 16 i + 8 g + 4 t + jj of the head:
// registers (t = 0, jj = 0..3), (t = 1, jj = 0..3) of one i are eight consecutive columns.
__device__ __forceinline__ int perm_row(int t, int r) { return 16 * (r >> 3) + 8 * ((r >> 2) & 1) + 4 * t + (r & 3); }

// The contraction index is permuted the same way in both operands: MFMA step s, lane half g, element e  <->  d = 64 g + 8 s + e,
// so that a lane reads 128 consecutive bytes of its row over the 8 steps.
__device__ __forceinline__ void mfma_head(const bf16x8 (&a)[2][8], const bf16x8 (&b)[8], f32x16 (&acc)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
#pragma unroll
        for (int s = 0; s < 8; ++s) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[t][s], b[s], acc[t], 0, 0, 0);
    }
}

__device__ __forceinline__ u32x4 pack8(const f32x16 (&acc)[2], int i) {
    u32x4 o;
    o[0] = pack_bf16x2(acc[0][4 * i + 0], acc[0][4 * i + 1]);
    o[1] = pack_bf16x2(acc[0][4 * i + 2], acc[0][4 * i + 3]);
    o[2] = pack_bf16x2(acc[1][4 * i + 0], acc[1][4 * i + 1]);
    o[3] = pack_bf16x2(acc[1][4 * i + 2], acc[1][4 * i + 3]);
    return o;
}

// grid (ceil(L / (32 * 4 * CF_PROB_NB)), H, B), 256 threads.  q [B * L][ldq] pre-scaled (softmax_scale * log2 e), k [B][>= kept + 1][ldk].
__global__ __launch_bounds__(256) void cross_probs_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k,
                                                          int64_t ldk, int64_t k_bstride, bf16_t* __restrict__ p, int64_t ldp, int L,
                                                          int kept, float log2_pad) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, g = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    bf16x8 ka[2][8];
    const bf16_t* kh = k + (int64_t)b * k_bstride + (int64_t)h * CF_D + g * 64;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int key = perm_row(t, r);
#pragma unroll
        for (int s = 0; s < 8; ++s) ka[t][s] = key <= kept ? *(const bf16x8*)(kh + (int64_t)key * ldk + s * 8) : zero8;
    }
    const int first = blockIdx.x * (4 * CF_PROB_NB);
    for (int it = 0; it < CF_PROB_NB; ++it) {
        const int row0 = (first + it * 4 + wave) * 32;
        if (row0 >= L) break;                                         // wave-uniform
        const int row = row0 + r;
        const int64_t grow = (int64_t)b * L + (row < L ? row : L - 1);  // rows past the end re-read the last row and store nothing
        const bf16_t* qr = q + grow * ldq + (int64_t)h * CF_D + g * 64;
        bf16x8 qb[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) qb[s] = *(const bf16x8*)(qr + s * 8);
        f32x16 acc[2];
        mfma_head(ka, qb, acc);
        // the lane's 32 scores: acc[t][4 i + jj] is key 16 i + 8 g + 4 t + jj; lane ^ 32 holds the other 32 of the same query row
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int key = 16 * i + 8 * g + 4 * t + jj;
                    float s = acc[t][4 * i + jj];
                    s = key == kept ? s + log2_pad : s;
                    s = key > kept ? -INFINITY : s;
                    acc[t][4 * i + jj] = s;
                    m = fmaxf(m, s);
                }
        m = fmaxf(m, __shfl_xor(m, 32, 64));                         // key 0 is always scored: m is finite
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float e = __builtin_amdgcn_exp2f(acc[t][i] - m);   // exp2(-inf) = 0: the guard columns are exact zeros
                acc[t][i] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] *= inv;
        if (row < L) {
            bf16_t* pr = p + grow * ldp + (int64_t)h * CF_KEYS + 8 * g;
#pragma unroll
            for (int i = 0; i < 4; ++i) *(u32x4*)(pr + 16 * i) = pack8(acc, i);
        }
    }
}

// grid (ceil(C / (32 * 4 * CF_FOLD_NB)), H, B), 256 threads.  w [C][ldw] = W_co, vt [B][C][ldvt] = V^T of the text tokens.
__global__ __launch_bounds__(256) void cross_fold_kernel(const bf16_t* __restrict__ w, int64_t ldw, const bf16_t* __restrict__ vt,
                                                         int64_t ldvt, int64_t vt_bstride, bf16_t* __restrict__ out, int64_t ldo,
                                                         int64_t out_bstride, int C, int kept) {
    __shared__ __attribute__((aligned(16))) bf16_t vs[CF_KEYS * CF_VS_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, g = lane >> 5;
    const int h = blockIdx.y, b = blockIdx.z;
    // V_h[j][d] = vt[h * 128 + d][j], j <= kept (zeros above): 16-byte loads along the keys, transposed through LDS
    const bf16_t* vh = vt + (int64_t)b * vt_bstride + (int64_t)h * CF_D * ldvt;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int idx = it * 256 + threadIdx.x, d = idx >> 3, c = idx & 7;
        bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (c * 8 <= kept) v = *(const bf16x8*)(vh + (int64_t)d * ldvt + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) vs[(c * 8 + e) * CF_VS_LD + d] = c * 8 + e <= kept ? v[e] : (bf16_t)0.f;
    }
    __syncthreads();
    bf16x8 va[2][8];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 8; ++s) va[t][s] = *(const bf16x8*)(vs + perm_row(t, r) * CF_VS_LD + g * 64 + s * 8);
    const int first = blockIdx.x * (4 * CF_FOLD_NB);
    for (int it = 0; it < CF_FOLD_NB; ++it) {
        const int n0 = (first + it * 4 + wave) * 32;
        if (n0 >= C) break;                                           // wave-uniform; C % 32 == 0 (C = H * 128)
        const int n = n0 + r;
        const bf16_t* wr = w + (int64_t)n * ldw + (int64_t)h * CF_D + g * 64;
        bf16x8 wb[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) wb[s] = *(const bf16x8*)(wr + s * 8);
        f32x16 acc[2];
        mfma_head(va, wb, acc);
        bf16_t* orow = out + (int64_t)b * out_bstride + (int64_t)n * ldo + (int64_t)h * CF_KEYS + 8 * g;
#pragma unroll
        for (int i = 0; i < 4; ++i) *(u32x4*)(orow + 16 * i) = pack8(acc, i);
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

std::atomic<int> g_last_cross_fold{0};

}  // namespace

int wan_last_cross_fold() { return g_last_cross_fold.load(std::memory_order_relaxed); }
void wan_note_cross_fold(int folded) { g_last_cross_fold.store(folded, std::memory_order_relaxed); }

// The rule (include/wan_hip.h).  Host arithmetic only.
//
// WAN_CROSS_FOLD_MIN_ROWS: where the fold starts to pay.  It removes rows * C * (C - 64 H) * 2 FLOP of the output projection and
// 7/8 of the 512-key attention, and adds cross_fold_kernel (a fixed cost per layer: W_co read once, V'^T written once) and one
// launch; below the crossover the fixed cost wins.
// measured at 14B width (40 heads, kept = 37; profiles/r07/cross_fold_crossover.log, HIP events, medians of 10): old pair -> new triple
// 0.0865 -> 0.0868 ms at 512 rows (break-even), 0.113 -> 0.104 at 1 024, 0.156 -> 0.128 at 2 048 (+18 %), 0.278 -> 0.202 at 4 096,
// 3.415 -> 1.783 at 67 080.  2 048: the first measured row count whose gain is several times the spread of such a measurement, and
// above every shape of the pinned launch traces (<= 896 rows, which 64 H >= 1024 keeps on the plain branch anyway).
#define WAN_CROSS_FOLD_MIN_ROWS 2048
extern "C" int wan_cross_fold_plan(int64_t rows, int num_heads, int text_len, int kept, int weights_bf16) {
    const int mode = wan_tune(WAN_TUNE_CROSS_FOLD);
    if (mode <= 0 || !weights_bf16 || rows <= 0 || num_heads <= 0) return 0;
    if (kept < 1 || kept + 1 > CF_KEYS || kept >= text_len) return 0;      // kept = text_len: "not known"; a 64-token prompt has 65 distinct keys
    if (mode >= 2) return 1;                                               // wherever the kernels are legal
    const int K = num_heads * CF_KEYS;
    if (K < 1024 || K % 128 != 0) return 0;                                 // the folded projection must still be a persistent-GEMM shape
    return rows >= WAN_CROSS_FOLD_MIN_ROWS ? 1 : 0;
}

extern "C" int64_t wan_cross_fold_workspace_bytes(int batch, int dim) {
    if (batch <= 0 || dim <= 0 || dim % CF_D != 0) return 0;
    return (int64_t)batch * dim * (dim / CF_D * CF_KEYS) * 2;
}

extern "C" wan_status_t wan_cross_probs(const void* q, int64_t ldq, const void* k, int64_t ldk, int64_t k_bstride, void* probs,
                                        int64_t ldp, int batch, int64_t rows_per_batch, int num_heads, int kept, int pad_count,
                                        void* stream) {
    WAN_REQUIRE(q && k && probs, WAN_ERR_INVALID, "wan_cross_probs: null tensor");
    WAN_REQUIRE(batch > 0 && rows_per_batch > 0 && num_heads > 0 && (int64_t)batch * rows_per_batch <= 0x7fffffff && batch <= 65535 &&
                    num_heads <= 65535,
                WAN_ERR_INVALID, "wan_cross_probs: batch=%d rows_per_batch=%lld heads=%d", batch, (long long)rows_per_batch, num_heads);
    WAN_REQUIRE(kept >= 0 && kept + 1 <= CF_KEYS && pad_count >= 1, WAN_ERR_UNSUPPORTED,
                "wan_cross_probs: kept=%d (kept + 1 distinct keys must be <= 64) pad_count=%d", kept, pad_count);
    WAN_REQUIRE(ldq >= (int64_t)num_heads * CF_D && ldk >= (int64_t)num_heads * CF_D && ldp >= (int64_t)num_heads * CF_KEYS &&
                    k_bstride >= (int64_t)(kept + 1) * ldk,
                WAN_ERR_INVALID, "wan_cross_probs: ldq=%lld ldk=%lld ldp=%lld k_bstride=%lld too small", (long long)ldq, (long long)ldk,
                (long long)ldp, (long long)k_bstride);
    WAN_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldp % 8 == 0 && k_bstride % 8 == 0 && aligned16(q) && aligned16(k) && aligned16(probs),
                WAN_ERR_INVALID, "wan_cross_probs: rows must be 16-byte aligned");
    const int L = (int)rows_per_batch;
    const int per_wg = 32 * 4 * CF_PROB_NB;
    dim3 grid((L + per_wg - 1) / per_wg, num_heads, batch);
    hipLaunchKernelGGL(cross_probs_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk,
                       k_bstride, (bf16_t*)probs, ldp, L, kept, log2f((float)pad_count));
    WAN_CHECK_LAUNCH("wan_cross_probs");
    return WAN_OK;
}

extern "C" wan_status_t wan_cross_fold_values(const void* w_co, int64_t ldw, const void* vt, int64_t ldvt, int64_t vt_bstride,
                                              void* vfold, int64_t ldo, int64_t vfold_bstride, int batch, int dim, int num_heads,
                                              int kept, void* stream) {
    WAN_REQUIRE(w_co && vt && vfold, WAN_ERR_INVALID, "wan_cross_fold_values: null tensor");
    WAN_REQUIRE(batch > 0 && batch <= 65535 && num_heads > 0 && num_heads <= 65535 && dim == num_heads * CF_D, WAN_ERR_UNSUPPORTED,
                "wan_cross_fold_values: batch=%d dim=%d heads=%d (head_dim must be 128)", batch, dim, num_heads);
    WAN_REQUIRE(kept >= 0 && kept + 1 <= CF_KEYS, WAN_ERR_UNSUPPORTED, "wan_cross_fold_values: kept=%d (kept + 1 must be <= 64)", kept);
    const int64_t K = (int64_t)num_heads * CF_KEYS;
    WAN_REQUIRE(ldw >= dim && ldvt >= (kept + 8) / 8 * 8 && ldo >= K && vt_bstride >= (int64_t)dim * ldvt && vfold_bstride >= (int64_t)dim * ldo,
                WAN_ERR_INVALID, "wan_cross_fold_values: ldw=%lld ldvt=%lld ldo=%lld vt_bstride=%lld vfold_bstride=%lld too small",
                (long long)ldw, (long long)ldvt, (long long)ldo, (long long)vt_bstride, (long long)vfold_bstride);
    WAN_REQUIRE(ldw % 8 == 0 && ldvt % 8 == 0 && ldo % 8 == 0 && vt_bstride % 8 == 0 && vfold_bstride % 8 == 0 && aligned16(w_co) &&
                    aligned16(vt) && aligned16(vfold),
                WAN_ERR_INVALID, "wan_cross_fold_values: rows must be 16-byte aligned");
    const int per_wg = 32 * 4 * CF_FOLD_NB;
    dim3 grid((dim + per_wg - 1) / per_wg, num_heads, batch);
    hipLaunchKernelGGL(cross_fold_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w_co, ldw, (const bf16_t*)vt, ldvt,
                       vt_bstride, (bf16_t*)vfold, ldo, vfold_bstride, dim, kept);
    WAN_CHECK_LAUNCH("wan_cross_fold_values");
    return WAN_OK;
}
