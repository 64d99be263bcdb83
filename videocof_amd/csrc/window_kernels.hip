// Temporal context windows ("Temporal context windows"): the two memory-bound passes a windowed denoise step adds.
//   state  [B, C, Fs + K*G + Fs, h, w] = [source | ground_0 .. ground_{K-1} | target]      (the loop's latents)
//   window [C, n + G + n, h, w]        = [source[a_k : a_k + n] | ground_k | target[a_k : a_k + n]]
// wan_window_gather copies windows [k0, k1) out of the state into the model's input batch [rep][k1 - k0][B]; wan_window_blend
// turns the K window predictions into the prediction for the state.  Both stream whole latent frames: one workgroup row per
// (window, sample, channel) resp. per output frame, 16-byte loads and stores when a frame is a multiple of 16 bytes and every
// base is aligned, element-wise otherwise.  All frame arithmetic is per workgroup (scalar); lanes only add their offset.
#include <algorithm>

#include "common.hpp"
#include "packets.hpp"

// The blend's products and sums are rounded separately (a torch float32 restatement then gives the same bits).  __fmul_rn /
// __fadd_rn do not guarantee that here: the headers define them as plain `x * y` / `x + y`, which contraction may fuse once
// they are inlined.  The pragma takes the permission away from every operation of this file instead.
#pragma clang fp contract(off)

namespace {

struct Starts { int a[WAN_WINDOW_MAX]; };
constexpr int UNROLL = 4;                            // grid-stride iterations a lane keeps in flight together

// U = the copy unit: u32x4 (16 bytes), or one element (unsigned int for fp32, unsigned short for bf16).  `fu` = units per frame.
template <typename U>
__global__ __launch_bounds__(256) void window_gather_kernel(U* __restrict__ out, const U* __restrict__ state, Starts st, int k0,
                                                            int B, int C, int K, int n, int G, int Fs, int64_t fu, int rep,
                                                            int64_t rep_stride) {
    const int row = blockIdx.x;                       // ((k - k0) * B + b) * C + c, < (k1 - k0) * B * C
    const int c = row % C, b = (row / C) % B, k = k0 + row / (C * B);
    const int a = st.a[k];                            // 0 <= a <= Fs - n (checked by the host)
    const U* srow = state + ((int64_t)b * C + c) * (2 * Fs + (int64_t)K * G) * fu;
    const U* s_src = srow + (int64_t)a * fu;
    const U* s_gro = srow + ((int64_t)Fs + (int64_t)k * G) * fu;
    const U* s_tgt = srow + ((int64_t)Fs + (int64_t)K * G + a) * fu;
    const int64_t nu = (int64_t)n * fu, gu = (int64_t)G * fu, row_u = 2 * nu + gu;
    U* orow = out + (int64_t)row * row_u;
    const int64_t stride = (int64_t)gridDim.y * 256;
    for (int64_t p0 = (int64_t)blockIdx.y * 256 + threadIdx.x; p0 < row_u; p0 += UNROLL * stride) {
        U v[UNROLL];                                  // UNROLL independent loads in flight per lane, then the stores
#pragma unroll
        for (int j = 0; j < UNROLL; ++j) {
            const int64_t p = p0 + j * stride;
            if (p < row_u) v[j] = p < nu ? s_src[p] : p < nu + gu ? s_gro[p - nu] : s_tgt[p - nu - gu];
        }
#pragma unroll
        for (int j = 0; j < UNROLL; ++j) {
            const int64_t p = p0 + j * stride;
            if (p < row_u)
                for (int r = 0; r < rep; ++r) orow[r * rep_stride + p] = v[j];
        }
    }
}

template <typename T> struct Raw;                    // one element as bits
template <> struct Raw<float> { typedef unsigned int type; };
template <> struct Raw<bf16_t> { typedef unsigned short type; };

// one output frame per blockIdx.x; `hw` = elements per frame
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void window_blend_kernel(T* __restrict__ out, const T* __restrict__ pred,
                                                           const float* __restrict__ alpha, Starts st, int B, int C, int K, int n,
                                                           int G, int Fs, int64_t hw) {
    constexpr int N = VEC ? Pk<T>::N : 1;
    const int Ftot = 2 * Fs + K * G;                  // B * C * Ftot < 2^31 (checked by the host)
    const int64_t Fw = 2 * (int64_t)n + G;
    const unsigned row = blockIdx.x;                  // (b * C + c) * Ftot + F
    const int F = (int)(row % (unsigned)Ftot);
    const unsigned bc = row / (unsigned)Ftot;
    const int b = (int)(bc / (unsigned)C), c = (int)(bc % (unsigned)C);
    T* o = out + (int64_t)row * hw;
    const int64_t units = hw / N, first = (int64_t)blockIdx.y * 256 + threadIdx.x, stride = (int64_t)gridDim.y * 256;
    // frame `wf` of window k's prediction, sample b, channel c
    auto frame = [&](int k, int wf) { return pred + ((((int64_t)k * B + b) * C + c) * Fw + wf) * hw; };
    if (F < Fs + K * G) {
        // source frames: the CoF mask; grounding frames: window k's own block, bits unchanged
        const T* src = F < Fs ? nullptr : frame((F - Fs) / G, n + (F - Fs) % G);
        for (int64_t u = first; u < units; u += stride) {
            if constexpr (VEC) {
                const u32x4 z = {0u, 0u, 0u, 0u};
                *(u32x4*)(o + u * N) = src ? *(const u32x4*)(src + u * N) : z;
            } else {
                typedef typename Raw<T>::type R;
                ((R*)o)[u] = src ? ((const R*)src)[u] : (R)0;
            }
        }
        return;
    }
    // target frame f: the windows that cover it are consecutive (equal lengths, ascending starts)
    const int f = F - Fs - K * G;
    int klo = 0;
    while (klo < K && st.a[klo] + n <= f) ++klo;
    int khi = klo;
    while (khi < K && st.a[khi] <= f) ++khi;          // klo < khi: the host checked that every frame is covered
    for (int64_t u0 = first; u0 < units; u0 += UNROLL * stride) {
        float acc[UNROLL][N];
        for (int k = klo; k < khi; ++k) {             // per window: its weight and frame once, then UNROLL independent loads per lane
            const float w = alpha[(int64_t)k * Fs + f];
            const T* p = frame(k, n + G + f - st.a[k]);
#pragma unroll
            for (int q = 0; q < UNROLL; ++q) {
                const int64_t u = u0 + q * stride;
                if (u >= units) continue;
                float x[N];
                if constexpr (VEC) load_pk(p + u * N, x); else x[0] = (float)p[u];
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const float term = w * x[j];      // rounded; never fused into the sum (see the pragma above)
                    acc[q][j] = k == klo ? term : acc[q][j] + term;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < UNROLL; ++q) {
            const int64_t u = u0 + q * stride;
            if (u >= units) continue;
            if constexpr (VEC) store_pk(o + u * N, acc[q]); else o[u] = (T)acc[q][0];
        }
    }
}

// starts ascending, every window inside [0, Fs), every frame of [0, Fs) covered
bool plan_ok(const int* starts, int K, int n, int Fs) {
    if (!starts || K < 1 || K > WAN_WINDOW_MAX || n < 1 || n > Fs || starts[0] != 0 || starts[K - 1] + n != Fs) return false;
    for (int k = 1; k < K; ++k)
        if (starts[k] <= starts[k - 1] || starts[k] > starts[k - 1] + n) return false;
    return true;
}

unsigned rows_y(int64_t units, int64_t rows) {        // workgroups along a row: <= ~2048 in all, the rest is a grid-stride loop
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((units + 255) / 256, 2048 / rows));
}

}  // namespace

extern "C" wan_status_t wan_window_gather(void* out, const void* state, int dtype, const int* starts, int K, int k0, int k1,
                                          int B, int C, int Fs, int n, int G, int64_t hw, int rep, int64_t rep_stride,
                                          void* stream) {
    WAN_REQUIRE(out && state, WAN_ERR_INVALID, "wan_window_gather: null tensor");
    WAN_REQUIRE(dtype == 0 || dtype == 1, WAN_ERR_INVALID, "wan_window_gather: dtype=%d (0 fp32, 1 bf16)", dtype);
    WAN_REQUIRE(B >= 1 && C >= 1 && G >= 0 && hw >= 1, WAN_ERR_INVALID, "wan_window_gather: B=%d C=%d G=%d hw=%lld", B, C, G,
                (long long)hw);
    WAN_REQUIRE(plan_ok(starts, K, n, Fs), WAN_ERR_INVALID,
                "wan_window_gather: K=%d (1..%d) windows of n=%d frames must ascend from 0, end at Fs=%d and leave no gap", K,
                WAN_WINDOW_MAX, n, Fs);
    WAN_REQUIRE(0 <= k0 && k0 < k1 && k1 <= K, WAN_ERR_INVALID, "wan_window_gather: window range [%d, %d) of %d", k0, k1, K);
    const int64_t rows = (int64_t)(k1 - k0) * B * C, row_len = (2 * (int64_t)n + G) * hw;
    WAN_REQUIRE(rows <= 0x7fffffff, WAN_ERR_INVALID, "wan_window_gather: %lld rows", (long long)rows);
    WAN_REQUIRE((rep == 1 || rep == 2) && (rep == 1 || rep_stride >= rows * row_len), WAN_ERR_INVALID,
                "wan_window_gather: rep=%d (1 or 2), rep_stride=%lld < %lld", rep, (long long)rep_stride, (long long)(rows * row_len));
    const int64_t es = dtype == 0 ? 4 : 2;
    const bool vec = (hw * es) % 16 == 0 && (rep == 1 || (rep_stride * es) % 16 == 0) && (((uintptr_t)out | (uintptr_t)state) & 15) == 0;
    Starts st{};
    std::copy(starts, starts + K, st.a);
    hipStream_t s = (hipStream_t)stream;
    if (vec) {
        const int64_t fu = hw * es / 16;
        hipLaunchKernelGGL(window_gather_kernel<u32x4>, dim3((unsigned)rows, rows_y((2 * (int64_t)n + G) * fu, rows)), dim3(256), 0, s,
                           (u32x4*)out, (const u32x4*)state, st, k0, B, C, K, n, G, Fs, fu, rep, rep_stride * es / 16);
    } else if (dtype == 0) {
        hipLaunchKernelGGL(window_gather_kernel<unsigned int>, dim3((unsigned)rows, rows_y(row_len, rows)), dim3(256), 0, s,
                           (unsigned int*)out, (const unsigned int*)state, st, k0, B, C, K, n, G, Fs, hw, rep, rep_stride);
    } else {
        hipLaunchKernelGGL(window_gather_kernel<unsigned short>, dim3((unsigned)rows, rows_y(row_len, rows)), dim3(256), 0, s,
                           (unsigned short*)out, (const unsigned short*)state, st, k0, B, C, K, n, G, Fs, hw, rep, rep_stride);
    }
    WAN_CHECK_LAUNCH("wan_window_gather");
    return WAN_OK;
}

extern "C" wan_status_t wan_window_blend(void* out, const void* pred, int dtype, const float* alpha, const int* starts, int K,
                                         int B, int C, int Fs, int n, int G, int64_t hw, void* stream) {
    WAN_REQUIRE(out && pred && alpha, WAN_ERR_INVALID, "wan_window_blend: null tensor");
    WAN_REQUIRE(dtype == 0 || dtype == 1, WAN_ERR_INVALID, "wan_window_blend: dtype=%d (0 fp32, 1 bf16)", dtype);
    WAN_REQUIRE(B >= 1 && C >= 1 && G >= 0 && hw >= 1, WAN_ERR_INVALID, "wan_window_blend: B=%d C=%d G=%d hw=%lld", B, C, G,
                (long long)hw);
    WAN_REQUIRE(plan_ok(starts, K, n, Fs), WAN_ERR_INVALID,
                "wan_window_blend: K=%d (1..%d) windows of n=%d frames must ascend from 0, end at Fs=%d and leave no gap", K,
                WAN_WINDOW_MAX, n, Fs);
    const int64_t rows = (int64_t)B * C * (2 * (int64_t)Fs + (int64_t)K * G);
    WAN_REQUIRE(rows <= 0x7fffffff, WAN_ERR_INVALID, "wan_window_blend: %lld output frames", (long long)rows);
    const int64_t es = dtype == 0 ? 4 : 2;
    const bool vec = (hw * es) % 16 == 0 && (((uintptr_t)out | (uintptr_t)pred) & 15) == 0;
    Starts st{};
    std::copy(starts, starts + K, st.a);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)rows, rows_y(vec ? hw * es / 16 : hw, rows));
#define WAN_BLEND(T, V)                                                                                                     \
    hipLaunchKernelGGL((window_blend_kernel<T, V>), grid, dim3(256), 0, s, (T*)out, (const T*)pred, alpha, st, B, C, K, n, G, \
                       Fs, hw)
    if (dtype == 0) { if (vec) WAN_BLEND(float, true); else WAN_BLEND(float, false); }
    else            { if (vec) WAN_BLEND(bf16_t, true); else WAN_BLEND(bf16_t, false); }
#undef WAN_BLEND
    WAN_CHECK_LAUNCH("wan_window_blend");
    return WAN_OK;
}
