// What the GEMM family shares (internal): gemm_api.cpp holds the entry points and the plan arithmetic, gemm_bf16.hip (128^2 and its
// split-K form), gemm_bf16_256.hip (8-wave phased, 4-wave, e4m3) and gemm_bf16_pk.hip (persistent stream-K) hold the kernels and one
// launch function per family.
#pragma once
#include <type_traits>

#include "common.hpp"

// ---- host side ---------------------------------------------------------------------------------------------------------------
// One Linear call as the C entry points receive it.  wan_gemm_validate() checks it and leaves rows_per_batch >= 1 (what the
// kernels divide by); the launch functions below take validated calls only.
struct WanGemmCall {
    const void* A; int64_t lda;
    const void* W; int64_t ldw;
    const float* bias;
    void* out; int64_t ldo;
    int M, N, K, epilogue;
    const float* gate; int64_t rows_per_batch;
    const float* a_row_scale; const float* w_row_scale;      // e4m3 operands only (nullptr for bf16)
};

// `name`: the entry point the message speaks for; `elsize`: 2 (bf16: lda / ldw multiples of 8, K of 64) or 1 (e4m3: 16 and 128)
inline wan_status_t wan_gemm_validate(const char* name, int elsize, WanGemmCall& c) {
    const int ldmul = 16 / elsize, kmul = 128 / elsize;
    WAN_REQUIRE(c.A && c.W && c.out && (elsize == 2 || (c.a_row_scale && c.w_row_scale)), WAN_ERR_INVALID, "%s: null tensor", name);
    WAN_REQUIRE(c.M >= 0 && c.N > 0 && c.K > 0, WAN_ERR_INVALID, "%s: M=%d N=%d K=%d", name, c.M, c.N, c.K);
    WAN_REQUIRE(c.K % kmul == 0, WAN_ERR_UNSUPPORTED, "%s: K=%d must be a multiple of %d", name, c.K, kmul);
    WAN_REQUIRE(c.N % 4 == 0, WAN_ERR_UNSUPPORTED, "%s: N=%d must be a multiple of 4", name, c.N);
    WAN_REQUIRE(c.lda % ldmul == 0 && c.ldw % ldmul == 0 && c.lda >= c.K && c.ldw >= c.K, WAN_ERR_INVALID,
                "%s: lda=%lld ldw=%lld must be multiples of %d and >= K", name, (long long)c.lda, (long long)c.ldw, ldmul);
    if (c.epilogue == WAN_EPI_BF16_T)
        WAN_REQUIRE(c.ldo >= c.M && c.ldo % 4 == 0, WAN_ERR_INVALID, "%s: transposed ldo=%lld < M=%d or not a multiple of 4", name, (long long)c.ldo, c.M);
    else
        WAN_REQUIRE(c.ldo >= c.N && c.ldo % 4 == 0, WAN_ERR_INVALID, "%s: ldo=%lld < N=%d or not a multiple of 4", name, (long long)c.ldo, c.N);
    WAN_REQUIRE(c.gate == nullptr || (c.epilogue == WAN_EPI_RESID_F32 && c.rows_per_batch > 0), WAN_ERR_INVALID,
                "%s: gate needs WAN_EPI_RESID_F32 and rows_per_batch > 0", name);
    if (c.rows_per_batch < 1) c.rows_per_batch = 1;
    return WAN_OK;
}

// the caller's workspace of a `_ws` entry that is about to use it: `need` bytes (what `sizer`(M, N, K) answers), 16-byte aligned
inline wan_status_t wan_gemm_validate_ws(const char* name, const char* sizer, const WanGemmCall& c, const void* workspace,
                                         int64_t workspace_bytes, int64_t need) {
    WAN_REQUIRE(((uintptr_t)c.w_row_scale & 15) == 0, WAN_ERR_INVALID, "%s: w_row_scale must be 16-byte aligned", name);
    WAN_REQUIRE(workspace_bytes >= need, WAN_ERR_INVALID, "%s: workspace of %lld bytes, %s(%d, %d, %d) = %lld", name,
                (long long)workspace_bytes, sizer, c.M, c.N, c.K, (long long)need);
    WAN_REQUIRE(((uintptr_t)workspace & 15) == 0, WAN_ERR_INVALID, "%s: workspace must be 16-byte aligned", name);
    return WAN_OK;
}

// f(std::integral_constant<int, EPI>{}) for the run-time epilogue code
template <class F>
wan_status_t wan_gemm_epilogue(const char* name, int epilogue, F&& f) {
    switch (epilogue) {
        case WAN_EPI_BF16: return f(std::integral_constant<int, WAN_EPI_BF16>{});
        case WAN_EPI_GELU_BF16: return f(std::integral_constant<int, WAN_EPI_GELU_BF16>{});
        case WAN_EPI_F32: return f(std::integral_constant<int, WAN_EPI_F32>{});
        case WAN_EPI_RESID_F32: return f(std::integral_constant<int, WAN_EPI_RESID_F32>{});
        case WAN_EPI_BF16_T: return f(std::integral_constant<int, WAN_EPI_BF16_T>{});
        default: wan_set_error("%s: unknown epilogue %d", name, epilogue); return WAN_ERR_INVALID;
    }
}

// reserve the kernel's dynamic LDS (once per device), then launch it
template <auto Kernel, int LDS_BYTES, class Args>
wan_status_t wan_gemm_launch(const char* name, dim3 grid, int threads, hipStream_t s, const Args& g) {
    static std::atomic<uint64_t> attr_done{0};
    const wan_status_t st = wan_once_per_device(attr_done, +[]() -> wan_status_t {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) == hipSuccess
                   ? WAN_OK : WAN_ERR_LAUNCH;
    });
    if (st != WAN_OK) {
        wan_set_error("%s: cannot reserve %d B of LDS: %s", name, LDS_BYTES, hipGetErrorString(hipGetLastError()));
        return st;
    }
    hipLaunchKernelGGL(Kernel, grid, dim3((unsigned)threads), LDS_BYTES, s, g);
    WAN_CHECK_LAUNCH(name);
    return WAN_OK;
}

// internal entry points of the kernel files (validated calls); the plan helpers gemm_api.cpp asks
wan_status_t wan_gemm_bf16_128(const WanGemmCall& c, int batch, int64_t strideA, int64_t strideW, int64_t strideO, hipStream_t s);
wan_status_t wan_gemm_bf16_splitk(const WanGemmCall& c, int splits, void* workspace, int64_t counter_bytes, hipStream_t s);
wan_status_t wan_gemm_bf16_256(const WanGemmCall& c, hipStream_t s);
wan_status_t wan_gemm_fp8_256(const WanGemmCall& c, hipStream_t s);
wan_status_t wan_gemm_bf16_pk(const WanGemmCall& c, void* workspace, hipStream_t s);
wan_status_t wan_gemm_fp8_pk(const WanGemmCall& c, void* workspace, hipStream_t s);
bool wan_gemm256_uses_w4(int K);
int64_t wan_gemm_pk_workspace_bytes(int M, int N);
int wan_gemm_pk_workers(int M, int N);

// ---- device side -------------------------------------------------------------------------------------------------------------
// XCD slab remap (bijective): workgroup b runs on XCD b % 8 (observed, speed only), and XCD x owns the contiguous slab
// [wan_xcd_slab_start(nt, x), wan_xcd_slab_start(nt, x + 1)) of the nt-tile sequence, which it walks in workgroup order.
__host__ __device__ __forceinline__ int wan_xcd_slab_start(int nt, int xcd) {
    const int q = nt >> 3, r = nt & 7;
    return xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
}
// position t of the sequence -> tile: groups of `gm` M tiles x all N tiles, M fastest inside a group (the tiles in flight on an
// XCD share gm A panels and a run of W panels through its private L2)
__host__ __device__ __forceinline__ void wan_tile_of(int t, int gm_max, int tiles_m, int tiles_n, int& tm, int& tn) {
    const int per_group = gm_max * tiles_n;
    const int grp = t / per_group;
    const int first_m = grp * gm_max;
    const int gm = min(gm_max, tiles_m - first_m);
    const int in = t - grp * per_group;
    tm = first_m + in % gm;
    tn = in / gm;
}
// one workgroup per tile: the tile of block `bid`
__device__ __forceinline__ void wan_tile_coords(int bid, int gm, int tiles_m, int tiles_n, int& tm, int& tn) {
    wan_tile_of(wan_xcd_slab_start(tiles_m * tiles_n, bid & 7) + (bid >> 3), gm, tiles_m, tiles_n, tm, tn);
}
