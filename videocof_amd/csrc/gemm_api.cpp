// nn.Linear: the C entry points of the GEMM family and the host arithmetic that picks a kernel for a shape.  The kernels and one
// launch function per family are in gemm_bf16.hip (128^2, split-K), gemm_bf16_256.hip (256^2: 8-wave phased, 4-wave, e4m3) and
// gemm_bf16_pk.hip (persistent stream-K); what they share is in gemm_common.hpp.
#include <algorithm>

#include "gemm_common.hpp"

// Small shapes on the 128^2 kernel (configs[0]: M = 2 304 tokens): when its output tiles do not fill the chip's 2 x CUs workgroup
// slots and K is deep enough, the K range of every tile is cut into `splits` pieces (2 .. 4) so that the launch is (close to) one
// full round of shorter workgroups -- ffn.2 at M = 2 304 (N = 1 536, K = 8 960) is 216 tiles of 140 serial K steps on 256 CUs, the
// same product as 432 workgroups of 70.  Needs the caller's workspace (wan_gemm_bf16_ws); 1 = no split.
static int64_t tiles128(int M, int N) { return (int64_t)((M + 127) / 128) * ((N + 127) / 128); }
static int wan_gemm_splitk(int M, int N, int K) {
    if (wan_tune(WAN_TUNE_GEMM_SPLITK) == 0) return 1;
    const int64_t tiles = tiles128(M, N);
    const int slots = 2 * wan_cu_count();
    const int nk = K / 64;
    if (const int f = wan_tune(WAN_TUNE_GEMM_SPLITK); f > 1) return (f <= 8 && nk >= 2 * f) ? f : 1;      // developer override
    if (tiles * 4 > (int64_t)slots * 3 || nk < 64) return 1;                // >= 3/4 of a round already, or nothing to cut
    // measured at M = 2 304 (profiles/r05/gemm_yardstick_small_splitk.log): K = 8 960 in two pieces 0.105 -> 0.087 ms; K = 1 536 in two pieces
    // 0.027 -> 0.033 ms -- the counter memset, the 64 KB round trip per piece and the second launch wave cost more than 12 K tiles
    int splits = (int)std::min<int64_t>(slots / tiles, 4);
    while (splits > 1 && nk / splits < 32) --splits;                       // at least 32 K tiles per piece
    return splits < 2 ? 1 : splits;
}
static int64_t splitk_counter_bytes(int M, int N) { return (tiles128(M, N) * 4 + 4095) / 4096 * 4096; }
static int64_t splitk_workspace_bytes(int M, int N, int splits) {
    return splitk_counter_bytes(M, N) + tiles128(M, N) * splits * (int64_t)(128 * 128 * 4);
}

// Which kernel family wan_gemm_bf16 dispatches a shape to (host arithmetic, no GPU needed).  Large shapes -> the 256^2 tile
// (one workgroup per CU: 8-wave phased kernel, or its 4-wave form for deep K), unless its tiles would leave more than half of
// the CUs idle (M ~ 1e3: the text encoder, the VAE's attention block): four times as many 128^2 tiles at two per CU fill the
// chip better.  gemm_variant = 1|2 is a developer A/B switch (wan_set_tuning), not a product option.
extern "C" int wan_gemm_plan(int M, int N, int K) {
    const int variant = wan_tune(WAN_TUNE_GEMM_VARIANT);
    const int64_t tiles256 = (int64_t)((M + 255) / 256) * ((N + 255) / 256);
    const bool big = M >= 1024 && N >= 256 && 2 * tiles256 > wan_cu_count();
    if (!(variant == 2 || (variant == 0 && big))) return WAN_GEMM_VARIANT_128;
    return wan_gemm256_uses_w4(K) ? WAN_GEMM_VARIANT_256_W4 : WAN_GEMM_VARIANT_256_W8;
}

// The persistent stream-K form (gemm_bf16_pk.hip) takes a product when the caller brought a workspace and a 256^2 kernel would
// have run it (gemm_pk = 1, default): every "big" shape with K % 128 == 0 and K >= 1024.  Round 4 stopped at K >= 4096 (where the
// 4-wave per-tile kernel ran); round 5 measured the K = 1536 Linears of the 1.3B model at M = 67 080 (profiles/r05/
// gemm_yardstick_1p3b_gate.log): persistent 0.567 / 0.335 / 0.386 / 0.282 / 1.551 ms against 0.638 / 0.342 / 0.443 / 0.325 / 1.654 for the
// 8-wave per-tile kernel (q|k, V^T, o + resid, cross q, ffn.0) -- at 24 K tiles per output tile the per-tile pipeline fill is
// >= 8 % of a tile, which a continuous K-tile stream does not pay.  Shallower K (the VAE attention block's K = 384) stays where it
// was: there the epilogue dominates and a second workgroup per CU hides it.
// gemm_pk = 2: whenever its shape rules allow (K % 128 == 0, at least one 256^2 tile each way); 0: never.
extern "C" int wan_gemm_ws_plan(int M, int N, int K) {
    const int pk = wan_tune(WAN_TUNE_GEMM_PK);
    const int base = wan_gemm_plan(M, N, K);
    // (shallow K only with at least four rounds of tiles: at M = 2 304 the K = 1536 ffn.0 of the 1.3B model is 315 tiles on 256 CUs --
    // mostly stream-K pieces, whose fix-up traffic costs more than the per-tile pipeline fill it saves: 0.095 vs 0.086 ms)
    const int64_t tiles256 = (int64_t)((M + 255) / 256) * ((N + 255) / 256);
    if (pk == 1 && base != WAN_GEMM_VARIANT_128 && K % 128 == 0 && (K >= 4096 || (K >= 1024 && tiles256 >= 4 * (int64_t)wan_cu_count())))
        return WAN_GEMM_VARIANT_256_PK;
    if (pk == 2 && K % 128 == 0 && M >= 256 && N >= 256) return WAN_GEMM_VARIANT_256_PK;
    return base;
}

// how many pieces wan_gemm_bf16_ws cuts the K range of this shape's tiles into (1: no split; host arithmetic)
extern "C" int wan_gemm_ws_splits(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0 || K % 64 != 0 || wan_gemm_ws_plan(M, N, K) != WAN_GEMM_VARIANT_128) return 1;
    return wan_gemm_splitk(M, N, K);
}

extern "C" int64_t wan_gemm_workspace_bytes(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    if (wan_gemm_ws_plan(M, N, K) == WAN_GEMM_VARIANT_256_PK) return wan_gemm_pk_workspace_bytes(M, N);
    const int splits = wan_gemm_ws_splits(M, N, K);
    return splits > 1 ? splitk_workspace_bytes(M, N, splits) : 0;
}

static wan_status_t gemm_bf16(WanGemmCall& c, hipStream_t s) {
    if (const wan_status_t st = wan_gemm_validate("wan_gemm_bf16", 2, c); st != WAN_OK) return st;
    if (c.M == 0) return WAN_OK;
    return wan_gemm_plan(c.M, c.N, c.K) != WAN_GEMM_VARIANT_128 ? wan_gemm_bf16_256(c, s) : wan_gemm_bf16_128(c, 1, 0, 0, 0, s);
}

extern "C" wan_status_t wan_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                                      void* out, int64_t ldo, int M, int N, int K, int epilogue,
                                      const float* gate, int64_t rows_per_batch, void* stream) {
    WanGemmCall c{A, lda, W, ldw, bias, out, ldo, M, N, K, epilogue, gate, rows_per_batch, nullptr, nullptr};
    return gemm_bf16(c, (hipStream_t)stream);
}

extern "C" wan_status_t wan_gemm_bf16_ws(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                                         void* out, int64_t ldo, int M, int N, int K, int epilogue,
                                         const float* gate, int64_t rows_per_batch, void* workspace, int64_t workspace_bytes,
                                         void* stream) {
    WanGemmCall c{A, lda, W, ldw, bias, out, ldo, M, N, K, epilogue, gate, rows_per_batch, nullptr, nullptr};
    hipStream_t s = (hipStream_t)stream;
    const int plan = workspace != nullptr && M > 0 && N > 0 && K > 0 ? wan_gemm_ws_plan(M, N, K) : -1;
    // small shapes: the 128^2 kernel with its K range cut into pieces when that fills the chip and the workspace can hold them
    // (an invalid call is answered in wan_gemm_bf16's name, as without a workspace)
    if (plan == WAN_GEMM_VARIANT_128) {
        const int splits = K % 64 == 0 ? wan_gemm_splitk(M, N, K) : 1;
        if (splits > 1 && workspace_bytes >= splitk_workspace_bytes(M, N, splits) && ((uintptr_t)workspace & 15) == 0) {
            if (const wan_status_t st = wan_gemm_validate("wan_gemm_bf16", 2, c); st != WAN_OK) return st;
            return wan_gemm_bf16_splitk(c, splits, workspace, splitk_counter_bytes(M, N), s);
        }
    }
    // (a gate whose samples are shorter than a wave's 128 rows: the persistent kernel's epilogue allows one sample seam per wave)
    if (plan != WAN_GEMM_VARIANT_256_PK || (gate != nullptr && rows_per_batch < 128)) return gemm_bf16(c, s);
    if (const wan_status_t st = wan_gemm_validate("wan_gemm_bf16_ws", 2, c); st != WAN_OK) return st;
    if (const wan_status_t st = wan_gemm_validate_ws("wan_gemm_bf16_ws", "wan_gemm_workspace_bytes", c, workspace, workspace_bytes,
                                                     wan_gemm_pk_workspace_bytes(M, N)); st != WAN_OK) return st;
    return wan_gemm_bf16_pk(c, workspace, s);
}

extern "C" wan_status_t wan_gemm_bf16_batched(const void* A, int64_t lda, int64_t strideA, const void* W, int64_t ldw,
                                              int64_t strideW, void* out, int64_t ldo, int64_t strideO,
                                              int M, int N, int K, int batch, int epilogue, void* stream) {
    WAN_REQUIRE(A && W && out, WAN_ERR_INVALID, "wan_gemm_bf16_batched: null tensor");
    WAN_REQUIRE(M >= 0 && N > 0 && K > 0 && batch >= 0 && batch <= 65535, WAN_ERR_INVALID,
                "wan_gemm_bf16_batched: M=%d N=%d K=%d batch=%d", M, N, K, batch);
    WAN_REQUIRE(K % 64 == 0 && N % 4 == 0, WAN_ERR_UNSUPPORTED, "wan_gemm_bf16_batched: K=%d %% 64 and N=%d %% 4 must be 0", K, N);
    WAN_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K && strideA % 8 == 0 && strideW % 8 == 0, WAN_ERR_INVALID,
                "wan_gemm_bf16_batched: lda=%lld ldw=%lld strideA=%lld strideW=%lld must be multiples of 8, ld >= K",
                (long long)lda, (long long)ldw, (long long)strideA, (long long)strideW);
    WAN_REQUIRE(ldo >= N && ldo % 4 == 0 && strideO % 4 == 0, WAN_ERR_INVALID,
                "wan_gemm_bf16_batched: ldo=%lld strideO=%lld", (long long)ldo, (long long)strideO);
    WAN_REQUIRE(epilogue == WAN_EPI_BF16 || epilogue == WAN_EPI_F32, WAN_ERR_UNSUPPORTED,
                "wan_gemm_bf16_batched: epilogue %d (only WAN_EPI_BF16 / WAN_EPI_F32)", epilogue);
    if (M == 0 || batch == 0) return WAN_OK;
    const WanGemmCall c{A, lda, W, ldw, nullptr, out, ldo, M, N, K, epilogue, nullptr, 1, nullptr, nullptr};
    return wan_gemm_bf16_128(c, batch, strideA, strideW, strideO, (hipStream_t)stream);
}

// The e4m3 Linear with a caller workspace: the persistent stream-K kernel's FP8 instantiation (gemm_bf16_pk.hip, "schedule P") where
// the bf16 product of the same TILE count would run persistent -- a K tile is 128 e4m3 elements, so the plan is asked about K / 2 --
// or where the bf16 product of the same SHAPE would and K >= 4096 (the 8-way Ulysses shard's M = 8 392: 660 tiles of 40 K tiles; measured
// 1.09-1.33x the per-tile kernel there, profiles/r06/gemm_fp8_sp8_shard.log); wan_gemm_fp8 (the 8-wave per-tile kernel) otherwise.
// Same contract as wan_gemm_bf16_ws: the workspace (wan_gemm_fp8_workspace_bytes(M, N, K) bytes) is not shared with another stream.
extern "C" int wan_gemm_fp8_ws_plan(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0 || K % 256 != 0) return WAN_GEMM_VARIANT_256_W8;
    if (wan_gemm_ws_plan(M, N, K / 2) == WAN_GEMM_VARIANT_256_PK) return WAN_GEMM_VARIANT_256_PK;
    return (K >= 4096 && wan_gemm_ws_plan(M, N, K) == WAN_GEMM_VARIANT_256_PK) ? WAN_GEMM_VARIANT_256_PK : WAN_GEMM_VARIANT_256_W8;
}

extern "C" int64_t wan_gemm_fp8_workspace_bytes(int M, int N, int K) {
    return wan_gemm_fp8_ws_plan(M, N, K) == WAN_GEMM_VARIANT_256_PK ? wan_gemm_pk_workspace_bytes(M, N) : 0;
}

static wan_status_t gemm_fp8(WanGemmCall& c, hipStream_t s) {
    if (const wan_status_t st = wan_gemm_validate("wan_gemm_fp8", 1, c); st != WAN_OK) return st;
    return c.M == 0 ? WAN_OK : wan_gemm_fp8_256(c, s);
}

extern "C" wan_status_t wan_gemm_fp8(const void* A_fp8, int64_t lda, const float* a_row_scale, const void* W_fp8, int64_t ldw,
                                     const float* w_row_scale, const float* bias, void* out, int64_t ldo, int M, int N, int K,
                                     int epilogue, const float* gate, int64_t rows_per_batch, void* stream) {
    WanGemmCall c{A_fp8, lda, W_fp8, ldw, bias, out, ldo, M, N, K, epilogue, gate, rows_per_batch, a_row_scale, w_row_scale};
    return gemm_fp8(c, (hipStream_t)stream);
}

extern "C" wan_status_t wan_gemm_fp8_ws(const void* A_fp8, int64_t lda, const float* a_row_scale, const void* W_fp8, int64_t ldw,
                                        const float* w_row_scale, const float* bias, void* out, int64_t ldo, int M, int N, int K,
                                        int epilogue, const float* gate, int64_t rows_per_batch, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
    WanGemmCall c{A_fp8, lda, W_fp8, ldw, bias, out, ldo, M, N, K, epilogue, gate, rows_per_batch, a_row_scale, w_row_scale};
    hipStream_t s = (hipStream_t)stream;
    if (workspace == nullptr || wan_gemm_fp8_ws_plan(M, N, K) != WAN_GEMM_VARIANT_256_PK || (gate != nullptr && rows_per_batch < 128))
        return gemm_fp8(c, s);
    if (const wan_status_t st = wan_gemm_validate("wan_gemm_fp8_ws", 1, c); st != WAN_OK) return st;
    if (const wan_status_t st = wan_gemm_validate_ws("wan_gemm_fp8_ws", "wan_gemm_fp8_workspace_bytes", c, workspace, workspace_bytes,
                                                     wan_gemm_pk_workspace_bytes(M, N)); st != WAN_OK) return st;
    return wan_gemm_fp8_pk(c, workspace, s);
}
