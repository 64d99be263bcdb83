// nn.Linear on the gfx950 matrix cores:  acc[m,n] = sum_k A[m,k] * W[n,k]  (bf16 in, fp32 accumulate)
//
// Tile 128(M) x 128(N) x 64(K), 256 threads = 4 waves (2x2), each wave 64x64 as 4x4
// v_mfma_f32_16x16x32_bf16 tiles.  Both operands are K-contiguous ([rows][K]) so A and W tiles
// share one LDS image: row-major [128][64] bf16 (128-byte rows, eight 16-byte chunks).
//
// Staging is LDS-DMA (global_load_lds_dwordx4): one wave instruction lands 8 rows x 128 B lane-
// linearly, so the bank swizzle is applied to the per-lane SOURCE address and mirrored on the
// ds_read_b128 side (physical chunk = logical chunk ^ ((row >> 1) & 7), conflict-free for the
// 16-row MFMA fragment read).  Two LDS buffers: tile t+1 streams in while tile t is multiplied.
//
// MFMA operand order is chosen per epilogue so that every lane owns 4 CONSECUTIVE output elements
// in the output's contiguous dimension:
//   row-major epilogues:  D = mfma(Wfrag, Afrag) -> lane holds m = l&15, n = (l>>4)*4 + r
//   transposed epilogue:  D = mfma(Afrag, Wfrag) -> lane holds n = l&15, m = (l>>4)*4 + r
//
// Workgroup -> tile mapping is XCD-aware: block b runs on XCD b%8 (observed, speed only); each XCD
// walks a contiguous slab of the tile sequence ordered as 8(M) x all(N) groups so that the 64 tiles
// resident on an XCD share 8 A-panels and 8 W-panels through its private L2.
#include "gemm_common.hpp"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kThreads = 256;
constexpr int kTileBytes = BM * BK * 2;        // 16 KiB per operand tile
constexpr int kStageBytes = 2 * kTileBytes;    // A + W
constexpr int kLdsBytes = 2 * kStageBytes;     // double buffered: 64 KiB

struct GemmArgs {
    const bf16_t* A; int64_t lda;
    const bf16_t* W; int64_t ldw;
    const float* bias;
    void* out; int64_t ldo;
    const float* gate; int64_t rows_per_batch;
    int M, N, K;
    int tiles_m, tiles_n;
    int64_t sA, sW, sO;      // element strides between the problems of a batched launch (blockIdx.y)
    // split-K form (SPLITK instantiation, round 5): blockIdx.y = split index s of `splitk`; a workgroup multiplies K tiles
    // [s * nk / splitk, (s + 1) * nk / splitk) of its output tile, stores its fp32 accumulators to its slot of the caller's
    // workspace and takes a ticket on the tile's arrival counter; the LAST arriver adds the pieces IN SPLIT ORDER (its own from
    // registers) and runs the normal epilogue -- bitwise reproducible, nobody waits for anybody (as in gemm_bf16_pk.hip).
    int splitk;
    int* counters;           // workspace head: one arrival counter per output tile (zeroed by a memset node ahead of the launch)
    char* slots;             // behind the counters: [tile][split] slots of 128 x 128 fp32, register-major
};

__device__ __forceinline__ void tile_coords(const GemmArgs& g, int& tm, int& tn) {
    // bijective XCD remap (guide T1): XCD x gets tiles [start_x, start_x + cnt_x)
    const int nwg = g.tiles_m * g.tiles_n;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, loc = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    // grouped order: 8 M-tiles x all N-tiles per group, M fastest inside the group
    constexpr int GM = 8;
    const int per_group = GM * g.tiles_n;
    const int grp = t / per_group;
    const int first_m = grp * GM;
    const int gm = min(GM, g.tiles_m - first_m);
    const int in = t - grp * per_group;
    tm = first_m + in % gm;
    tn = in / gm;
}

template <int EPI, bool SPLITK = false>
__global__ __launch_bounds__(kThreads, 2) void gemm_bf16_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool kTransposed = (EPI == WAN_EPI_BF16_T);

    int tm, tn;
    tile_coords(g, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    if (!SPLITK && gridDim.y > 1) {         // wan_gemm_bf16_batched: problem blockIdx.y
        g.A += blockIdx.y * g.sA;
        g.W += blockIdx.y * g.sW;
        g.out = (char*)g.out + blockIdx.y * g.sO * ((EPI == WAN_EPI_F32 || EPI == WAN_EPI_RESID_F32) ? 4 : 2);
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1;

    // ---- staging addresses: wave `wid` DMA-copies pieces wid*4 .. wid*4+3 (8 rows each) of A and of W
    const int srow = lane >> 3;                 // row inside an 8-row piece
    const int spc = lane & 7;                   // physical 16-byte chunk
    const bf16_t* a_src[4];
    const bf16_t* w_src[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (wid * 4 + j) * 8 + srow;           // tile row 0..127
        const int c = spc ^ ((row >> 1) & 7);               // logical chunk this lane must fetch
        const int am = min(m0 + row, g.M - 1);
        const int wn = min(n0 + row, g.N - 1);
        a_src[j] = g.A + (int64_t)am * g.lda + c * 8;
        w_src[j] = g.W + (int64_t)wn * g.ldw + c * 8;
    }
    auto stage = [&](int buf, int kt) {
        char* base = smem + buf * kStageBytes;
        const int koff = kt * BK;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            glds16(a_src[j] + koff, base + (wid * 4 + j) * 1024);
            glds16(w_src[j] + koff, base + kTileBytes + (wid * 4 + j) * 1024);
        }
    };

    // ---- fragment read offsets (bytes inside a tile)
    const int frow = lane & 15;
    const int kg = lane >> 4;                   // k-group: 8 contiguous k per lane
    const int sw = (lane >> 1) & 7;             // == ((row >> 1) & 7) for every fragment row of this lane
    const int off_k0 = frow * 128 + ((kg ^ sw) << 4);            // logical chunk kg      (kk = 0)
    const int off_k1 = frow * 128 + (((kg + 4) ^ sw) << 4);      // logical chunk kg + 4  (kk = 1)
    const int a_base = wr * 64 * 128;
    const int w_base = kTileBytes + wc * 64 * 128;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk_all = g.K / BK;
    const int split = SPLITK ? (int)blockIdx.y : 0;
    const int kt0 = SPLITK ? (int)((int64_t)split * nk_all / g.splitk) : 0;
    const int nk = SPLITK ? (int)((int64_t)(split + 1) * nk_all / g.splitk) : nk_all;
    stage(0, kt0);
    __builtin_amdgcn_s_waitcnt(0);   // vmcnt(0): tile 0 landed
    __syncthreads();

    for (int kt = kt0; kt < nk; ++kt) {
        const int cur = (kt - kt0) & 1;
        if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
        const char* sb = smem + cur * kStageBytes;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int off = kk ? off_k1 : off_k0;
            bf16x8 af[4], wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                af[i] = *reinterpret_cast<const bf16x8*>(sb + a_base + i * 2048 + off);
                wf[i] = *reinterpret_cast<const bf16x8*>(sb + w_base + i * 2048 + off);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (kTransposed)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], wf[j], acc[i][j], 0, 0, 0);
                    else
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
                }
        }
        __builtin_amdgcn_s_waitcnt(0);   // next tile landed (vmcnt) + our ds_reads retired
        __syncthreads();
    }

    if constexpr (SPLITK) {
        // publish my piece with write-through (sc1) stores (no L2 write-back needed to make it visible: CDNA4 guide, "publish-large"),
        // drain them, take a ticket; only the last arriver of the tile goes on
        const int tile = tm * g.tiles_n + tn;
        char* const tile_slots = g.slots + (int64_t)tile * g.splitk * (BM * BN * 4);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(tile_slots + (int64_t)split * (BM * BN * 4)), 0, BM * BN * 4, 0x00020000);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[i][j]), rs, ((i * 4 + j) * kThreads + tid) * 16, 0, /*sc1*/ 16);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        volatile int* const lds_flag = reinterpret_cast<volatile int*>(smem);
        if (tid == 0) lds_flag[0] = __hip_atomic_fetch_add(g.counters + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(lds_flag[0]) != g.splitk - 1) return;
        if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __syncthreads();
        f32x4 sum[4][4];
        for (int sidx = 0; sidx < g.splitk; ++sidx) {            // in split order, whoever arrived last
            const f32x4* src = reinterpret_cast<const f32x4*>(tile_slots + (int64_t)sidx * (BM * BN * 4));
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 t = sidx == split ? acc[i][j] : src[(i * 4 + j) * kThreads + tid];
                    sum[i][j] = sidx == 0 ? t : sum[i][j] + t;
                }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = sum[i][j];
    }

    // ---- epilogue
    const int l15 = lane & 15, l4 = (lane >> 4) * 4;
    if constexpr (!kTransposed) {
        // The bias of a column group is loaded once; the fp32 read-modify-write epilogue reads the residual stream (and the gate
        // rows) of two row groups back to back and waits once (element by element the compiler emitted load / wait / store per
        // 4-element group).  Out-of-range rows / columns read a clamped (valid) address and are not stored.
        int nn[4];
        bool nok[4];
        float4 bj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wc * 64 + j * 16 + l4;      // N % 4 == 0 -> whole 4-group in or out
            nok[j] = n < g.N;
            nn[j] = nok[j] ? n : 0;
            bj[j] = g.bias ? *reinterpret_cast<const float4*>(g.bias + nn[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const int rpb = g.gate ? (int)g.rows_per_batch : 1;
#pragma unroll
        for (int ig = 0; ig < 4; ig += 2) {
            int mm[2];
            bool mok[2];
            float4 xr[2][4], gv[2][4];
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
                const int m = m0 + wr * 64 + (ig + ii) * 16 + l15;
                mok[ii] = m < g.M;
                mm[ii] = mok[ii] ? m : g.M - 1;
                if constexpr (EPI == WAN_EPI_RESID_F32) {
                    const int64_t brow = g.gate ? (int64_t)(mm[ii] / rpb) * g.N : 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        xr[ii][j] = *reinterpret_cast<const float4*>((const float*)g.out + (int64_t)mm[ii] * g.ldo + nn[j]);
                        gv[ii][j] = g.gate ? *reinterpret_cast<const float4*>(g.gate + brow + nn[j]) : make_float4(1.f, 1.f, 1.f, 1.f);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);          // all loads of the batch are issued before the first use waits
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f32x4 v = acc[ig + ii][j];
                    v[0] += bj[j].x; v[1] += bj[j].y; v[2] += bj[j].z; v[3] += bj[j].w;
                    if constexpr (EPI == WAN_EPI_GELU_BF16) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = gelu_tanh_f32(v[r]);
                    }
                    if (!(mok[ii] && nok[j])) continue;
                    const int64_t off = (int64_t)mm[ii] * g.ldo + nn[j];
                    if constexpr (EPI == WAN_EPI_BF16 || EPI == WAN_EPI_GELU_BF16) {
                        u32x2 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
                        *reinterpret_cast<u32x2*>((bf16_t*)g.out + off) = o;
                    } else if constexpr (EPI == WAN_EPI_F32) {
                        *reinterpret_cast<float4*>((float*)g.out + off) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {   // WAN_EPI_RESID_F32
                        const float4 x = xr[ii][j], gq = gv[ii][j];
                        *reinterpret_cast<float4*>((float*)g.out + off) =
                            make_float4(x.x + v[0] * gq.x, x.y + v[1] * gq.y, x.z + v[2] * gq.z, x.w + v[3] * gq.w);
                    }
                }
        }
    } else {
        // out[n, m..m+3]: lane holds n = l&15, m = (l>>4)*4 + r
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wc * 64 + j * 16 + l15;
            if (n >= g.N) continue;
            const float bv = g.bias ? g.bias[n] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + wr * 64 + i * 16 + l4;
                if (m >= g.M) continue;
                f32x4 v = acc[i][j];
                bf16_t* p = (bf16_t*)g.out + (int64_t)n * g.ldo + m;
                if (m + 3 < g.M) {
                    u32x2 o = {pack_bf16x2(v[0] + bv, v[1] + bv), pack_bf16x2(v[2] + bv, v[3] + bv)};
                    *reinterpret_cast<u32x2*>(p) = o;
                } else {
                    for (int r = 0; r < 4 && m + r < g.M; ++r) p[r] = (bf16_t)(v[r] + bv);
                }
            }
        }
    }
}

GemmArgs make_args(const WanGemmCall& c) {
    GemmArgs g;
    g.A = (const bf16_t*)c.A; g.lda = c.lda; g.W = (const bf16_t*)c.W; g.ldw = c.ldw; g.bias = c.bias;
    g.out = c.out; g.ldo = c.ldo; g.gate = c.gate; g.rows_per_batch = c.rows_per_batch;
    g.M = c.M; g.N = c.N; g.K = c.K;
    g.tiles_m = (c.M + BM - 1) / BM; g.tiles_n = (c.N + BN - 1) / BN;
    g.sA = g.sW = g.sO = 0;
    g.splitk = 1; g.counters = nullptr; g.slots = nullptr;
    return g;
}

}  // namespace

// one workgroup per 128^2 tile; `batch` problems (blockIdx.y) the strides apart
wan_status_t wan_gemm_bf16_128(const WanGemmCall& c, int batch, int64_t strideA, int64_t strideW, int64_t strideO, hipStream_t s) {
    GemmArgs g = make_args(c);
    g.sA = strideA; g.sW = strideW; g.sO = strideO;
    const dim3 grid((unsigned)(g.tiles_m * g.tiles_n), (unsigned)batch);
    return wan_gemm_epilogue("wan_gemm_bf16", c.epilogue, [&](auto epi) {
        return wan_gemm_launch<gemm_bf16_kernel<decltype(epi)::value>, kLdsBytes>("wan_gemm_bf16", grid, kThreads, s, g);
    });
}

// split-K form: `workspace` = one arrival counter per output tile (`counter_bytes`, cleared here), then [tile][split] fp32 slots
wan_status_t wan_gemm_bf16_splitk(const WanGemmCall& c, int splits, void* workspace, int64_t counter_bytes, hipStream_t s) {
    GemmArgs g = make_args(c);
    g.splitk = splits; g.counters = (int*)workspace; g.slots = (char*)workspace + counter_bytes;
    const dim3 grid((unsigned)(g.tiles_m * g.tiles_n), (unsigned)splits);
    return wan_gemm_epilogue("wan_gemm_bf16", c.epilogue, [&](auto epi) {
        if (hipMemsetAsync(g.counters, 0, (size_t)counter_bytes, s) != hipSuccess) {
            wan_set_error("wan_gemm_bf16_ws: cannot clear the arrival counters: %s", hipGetErrorString(hipGetLastError()));
            return WAN_ERR_LAUNCH;
        }
        return wan_gemm_launch<gemm_bf16_kernel<decltype(epi)::value, true>, kLdsBytes>("wan_gemm_bf16_ws (split-K)", grid, kThreads, s, g);
    });
}
