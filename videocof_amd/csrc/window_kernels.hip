// Temporal context windows ("Temporal context windows"): the two memory-bound passes a windowed denoise step adds.
//   state  [B, C, Fs + K*G + Fs, h, w] = [source | ground_0 .. ground_{K-1} | target]      (the loop's latents)
//   window [C, n + G + n, h, w]        = [source[a_k : a_k + n] | ground_k | target[a_k : a_k + n]]
// wan_window_gather copies windows [k0, k1) out of the state into the model's input batch [rep][k1 - k0][B]; wan_window_blend
// turns the K window predictions into the prediction for the state.  Both stream whole latent frames: one workgroup row per
// (window, sample, channel) resp. per output frame, 16-byte loads and stores when a frame is a multiple of 16 bytes and every
// base is aligned, element-wise otherwise.  All frame arithmetic is per workgroup (scalar); lanes only add their offset.
// Spatial context windows are the same with tiles [n, th, tw] of the frames instead of whole frames:
// wan_tile_gather / wan_tile_blend, further down.
#include <algorithm>
#include <initializer_list>

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

// ---------------------------------------------------------------------------------------------- spatial context windows (13.2)
// Tiles instead of whole frames: a tile row is `tw` elements at pitch `W`.  The access unit is 16, 8 or 4 bytes or one element,
// the largest that divides everything a unit could straddle (tile_unit_bytes below), so all x arithmetic is in whole units.
// A workgroup is `rp` tile rows of `cw` lanes each (cw = min(units per row, 256), rp = 256 / cw; lanes beyond rp * cw idle): which
// frame, which tile and which rows of it are per workgroup (scalar); a lane adds its row and unit once.

template <int BYTES> struct RawOf;                    // BYTES of memory as one load / store
template <> struct RawOf<16> { typedef u32x4 type; };
template <> struct RawOf<8> { typedef u32x2 type; };
template <> struct RawOf<4> { typedef unsigned int type; };
template <> struct RawOf<2> { typedef unsigned short type; };

template <typename T, int N>
__device__ __forceinline__ void unpack(const typename RawOf<sizeof(T) * N>::type& r, float (&f)[N]) {
    if constexpr (sizeof(T) * N == 2) {
        f[0] = bf16lo_to_f32((unsigned int)r);
    } else {
        struct Words { unsigned int w[sizeof(T) * N / 4]; };
        const Words v = __builtin_bit_cast(Words, r);
#pragma unroll
        for (int i = 0; i < (int)(sizeof(T) * N / 4); ++i) {
            if constexpr (sizeof(T) == 4) f[i] = __uint_as_float(v.w[i]);
            else { f[2 * i] = bf16lo_to_f32(v.w[i]); f[2 * i + 1] = bf16hi_to_f32(v.w[i]); }
        }
    }
}

template <typename T, int N>
__device__ __forceinline__ typename RawOf<sizeof(T) * N>::type pack(const float (&f)[N]) {
    typedef typename RawOf<sizeof(T) * N>::type R;
    if constexpr (sizeof(T) * N == 2) {
        return (R)(pack_bf16x2(f[0], 0.f) & 0xffffu);
    } else {
        struct Words { unsigned int w[sizeof(T) * N / 4]; };
        Words v;
#pragma unroll
        for (int i = 0; i < (int)(sizeof(T) * N / 4); ++i) {
            if constexpr (sizeof(T) == 4) v.w[i] = __float_as_uint(f[i]);
            else v.w[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
        }
        return __builtin_bit_cast(R, v);
    }
}

// grid (row, window frame, row chunk); `pitch` = W, `ru` = tw, `hu` = H * W, all in units; `sx` holds the x starts in units
template <typename U>
__global__ __launch_bounds__(256) void tile_gather_kernel(U* __restrict__ out, const U* __restrict__ state, Starts st, Starts sy,
                                                          Starts sx, int k0, int B, int C, int Kt, int Ky, int Kx, int n, int th,
                                                          int G, int Fs, int64_t hu, int pitch, int ru, int cw, int rp, int rep,
                                                          int64_t rep_stride) {
    const int row = blockIdx.x;                       // ((k - k0) * B + b) * C + c, < (k1 - k0) * B * C
    const int c = row % C, b = (row / C) % B, k = k0 + row / (C * B);
    const int kx = k % Kx, ky = (k / Kx) % Ky, kt = k / (Kx * Ky);      // k < Kt * Ky * Kx (checked by the host)
    const int a = st.a[kt];                           // 0 <= a <= Fs - n, 0 <= y0 <= H - th, 0 <= x0 <= W - tw (checked by the host)
    const int wf = blockIdx.y;                        // frame of the window, < 2n + G; F = the state's frame it comes from
    const int F = wf < n ? a + wf : wf < n + G ? Fs + kt * G + (wf - n) : Fs + Kt * G + a + (wf - n - G);
    const U* src = state + (((int64_t)b * C + c) * (2 * Fs + (int64_t)Kt * G) + F) * hu + (int64_t)sy.a[ky] * pitch + sx.a[kx];
    U* dst = out + ((int64_t)row * (2 * n + G) + wf) * th * ru;
    const int lr = threadIdx.x / cw, lu = threadIdx.x % cw;
    if (lr >= rp) return;
    for (int r0 = blockIdx.z * UNROLL * rp; r0 < th; r0 += gridDim.z * UNROLL * rp)
        for (int u = lu; u < ru; u += cw) {           // one pass unless a tile row is longer than 256 units
            U v[UNROLL];                              // UNROLL independent loads in flight per lane, then the stores
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int r = r0 + j * rp + lr;
                if (r < th) v[j] = src[(int64_t)r * pitch + u];
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int r = r0 + j * rp + lr;
                if (r < th)
                    for (int q = 0; q < rep; ++q) dst[q * rep_stride + (int64_t)r * ru + u] = v[j];
            }
        }
}

// grid (output frame, row chunk); `wu` = W / N units per output row, `sx` holds the x starts in units
template <typename T, int N>
__global__ __launch_bounds__(256) void tile_blend_kernel(T* __restrict__ out, const T* __restrict__ pred,
                                                         const float* __restrict__ at_tab, const float* __restrict__ ay,
                                                         const float* __restrict__ ax, Starts st, Starts sy, Starts sx, int B, int C,
                                                         int Kt, int Ky, int Kx, int n, int th, int tw, int G, int Fs, int H, int W,
                                                         int wu, int cw, int rp) {
    typedef typename RawOf<sizeof(T) * N>::type R;
    const int Ftot = 2 * Fs + Kt * G;                 // B * C * Ftot * H < 2^31 (checked by the host)
    const int Fw = 2 * n + G;
    const unsigned row = blockIdx.x;                  // (b * C + c) * Ftot + F
    const int F = (int)(row % (unsigned)Ftot);
    const unsigned bc = row / (unsigned)Ftot;
    const int b = (int)(bc / (unsigned)C), c = (int)(bc % (unsigned)C);
    R* o = (R*)(out + (int64_t)row * H * W);
    const int lr = threadIdx.x / cw, lu = threadIdx.x % cw;
    if (lr >= rp) return;
    const int span = UNROLL * rp, first = blockIdx.y * span, stride = gridDim.y * span;
    if (F < Fs) {                                     // source frames: the CoF mask
        float z[N];
#pragma unroll
        for (int i = 0; i < N; ++i) z[i] = 0.f;
        for (int r0 = first; r0 < H; r0 += stride)
            for (int y = r0 + lr; y < min(r0 + span, H); y += rp)
                for (int u = lu; u < wu; u += cw) o[(int64_t)y * wu + u] = pack<T, N>(z);
        return;
    }
    // the temporal windows that cover this frame: its own one for a grounding frame; consecutive ones for a target frame (equal
    // lengths, ascending starts); klo < khi: the host checked that every position of every axis is covered
    const bool ground = F < Fs + Kt * G;
    const int f = ground ? 0 : F - Fs - Kt * G;
    int tlo, thi;
    if (ground) {
        tlo = (F - Fs) / G;
        thi = tlo + 1;
    } else {
        tlo = 0;
        while (tlo < Kt && st.a[tlo] + n <= f) ++tlo;
        thi = tlo;
        while (thi < Kt && st.a[thi] <= f) ++thi;
    }
    for (int r0 = first; r0 < H; r0 += stride) {
        // the y windows that cover any of the rows [r0, r0 + span) of this pass
        const int rend = min(r0 + span, H);
        int ylo = 0;
        while (ylo < Ky && sy.a[ylo] + th <= r0) ++ylo;
        int yhi = ylo;
        while (yhi < Ky && sy.a[yhi] < rend) ++yhi;
        for (int u = lu; u < wu; u += cw) {           // one pass unless an output row is longer than 256 units
            const int x = u * N;
            float acc[UNROLL][N];
            bool have[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                have[j] = false;
#pragma unroll
                for (int i = 0; i < N; ++i) acc[j][i] = 0.f;
            }
            for (int kt = tlo; kt < thi; ++kt) {
                const float wt = ground ? 1.0f : at_tab[(int64_t)kt * Fs + f];
                const int wf = ground ? n + (F - Fs) % G : n + G + f - st.a[kt];
                for (int ky = ylo; ky < yhi; ++ky) {
                    const int y0 = sy.a[ky];
                    float wty[UNROLL];                // round(at * ay) per row of the lane
                    bool in_y[UNROLL];
#pragma unroll
                    for (int j = 0; j < UNROLL; ++j) {
                        const int y = r0 + j * rp + lr;
                        in_y[j] = y < H && y >= y0 && y < y0 + th;
                        wty[j] = in_y[j] ? wt * ay[(int64_t)ky * H + y] : 0.f;
                    }
                    for (int kx = 0; kx < Kx; ++kx) {
                        const int x0 = sx.a[kx] * N;
                        if (x < x0 || x >= x0 + tw) continue;       // whole units: x0, tw and x are multiples of N
                        const T* p = pred + (((((int64_t)(kt * Ky + ky) * Kx + kx) * B + b) * C + c) * Fw + wf) * th * tw + (x - x0);
                        float wx[N];
                        if constexpr (sizeof(T) * N == 16) {
#pragma unroll
                            for (int i = 0; i < N; i += 4) {
                                const f32x4 v = *(const f32x4*)(ax + (int64_t)kx * W + x + i);
                                wx[i] = v[0]; wx[i + 1] = v[1]; wx[i + 2] = v[2]; wx[i + 3] = v[3];
                            }
                        } else {
#pragma unroll
                            for (int i = 0; i < N; ++i) wx[i] = ax[(int64_t)kx * W + x + i];
                        }
                        R raw[UNROLL];                // UNROLL independent loads in flight per lane, then the arithmetic
#pragma unroll
                        for (int j = 0; j < UNROLL; ++j)
                            if (in_y[j]) raw[j] = *(const R*)(p + (int64_t)(r0 + j * rp + lr - y0) * tw);
#pragma unroll
                        for (int j = 0; j < UNROLL; ++j) {
                            if (!in_y[j]) continue;
                            float v[N];
                            unpack<T, N>(raw[j], v);
#pragma unroll
                            for (int i = 0; i < N; ++i) {
                                const float w = wty[j] * wx[i];     // each product rounded; never fused (see the pragma above)
                                const float term = w * v[i];
                                acc[j][i] = have[j] ? acc[j][i] + term : term;
                            }
                            have[j] = true;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int y = r0 + j * rp + lr;
                if (y < H) o[(int64_t)y * wu + u] = pack<T, N>(acc[j]);
            }
        }
    }
}

// the largest of 16, 8, 4 bytes or one element that divides (in bytes) every length in `lens` (elements), every x start and
// every address: a power of two divides them all exactly when it divides their bitwise OR
int tile_unit_bytes(int64_t es, std::initializer_list<int64_t> lens, const int* xs, int Kx, uintptr_t addresses) {
    uint64_t m = (uint64_t)addresses;
    for (int64_t l : lens) m |= (uint64_t)(l * es);
    for (int k = 0; k < Kx; ++k) m |= (uint64_t)((int64_t)xs[k] * es);
    int ub = 16;
    while (ub > es && (m & (uint64_t)(ub - 1)) != 0) ub /= 2;
    return ub;
}

struct TileAxes { Starts t, y, x; };                 // x in units

// the kernel's copies of the starts; x_unit = elements per unit
TileAxes tile_axes(const int* ts, const int* ys, const int* xs, int Kt, int Ky, int Kx, int x_unit) {
    TileAxes ax{};
    std::copy(ts, ts + Kt, ax.t.a);
    std::copy(ys, ys + Ky, ax.y.a);
    for (int k = 0; k < Kx; ++k) ax.x.a[k] = xs[k] / x_unit;
    return ax;
}

unsigned chunks(int rows, int span, int64_t groups) { // workgroups along the rows of a frame: <= ~4096 in all, the rest is a loop
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + span - 1) / span, 4096 / groups));
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

namespace {

// what both tile entries ask of their arguments; nothing is enqueued before it holds
wan_status_t tile_args_ok(const char* who, int dtype, const int* ts, const int* ys, const int* xs, int Kt, int Ky, int Kx, int B,
                          int C, int Fs, int H, int W, int n, int th, int tw, int G) {
    WAN_REQUIRE(dtype == 0 || dtype == 1, WAN_ERR_INVALID, "%s: dtype=%d (0 fp32, 1 bf16)", who, dtype);
    WAN_REQUIRE(B >= 1 && C >= 1 && G >= 0, WAN_ERR_INVALID, "%s: B=%d C=%d G=%d", who, B, C, G);
    WAN_REQUIRE(plan_ok(ts, Kt, n, Fs), WAN_ERR_INVALID,
                "%s: Kt=%d (1..%d) windows of n=%d frames must ascend from 0, end at Fs=%d and leave no gap", who, Kt, WAN_WINDOW_MAX,
                n, Fs);
    WAN_REQUIRE(plan_ok(ys, Ky, th, H), WAN_ERR_INVALID,
                "%s: Ky=%d (1..%d) tiles of th=%d rows must ascend from 0, end at H=%d and leave no gap", who, Ky, WAN_WINDOW_MAX, th, H);
    WAN_REQUIRE(plan_ok(xs, Kx, tw, W), WAN_ERR_INVALID,
                "%s: Kx=%d (1..%d) tiles of tw=%d columns must ascend from 0, end at W=%d and leave no gap", who, Kx, WAN_WINDOW_MAX,
                tw, W);
    const int64_t Ftot = 2 * (int64_t)Fs + (int64_t)Kt * G, Fw = 2 * (int64_t)n + G;
    WAN_REQUIRE((int64_t)B * C * Ftot * H <= 0x7fffffff && Fw <= 65535 && (int64_t)th * tw <= 0x7fffffff, WAN_ERR_INVALID,
                "%s: %lld state rows, %lld frames per tile, %lld elements per tile frame", who, (long long)((int64_t)B * C * Ftot * H),
                (long long)Fw, (long long)((int64_t)th * tw));
    return WAN_OK;
}

}  // namespace

extern "C" wan_status_t wan_tile_gather(void* out, const void* state, int dtype, const int* t_starts, const int* y_starts,
                                        const int* x_starts, int Kt, int Ky, int Kx, int k0, int k1, int B, int C, int Fs, int H,
                                        int W, int n, int th, int tw, int G, int rep, int64_t rep_stride, void* stream) {
    WAN_REQUIRE(out && state, WAN_ERR_INVALID, "wan_tile_gather: null tensor");
    const wan_status_t ok = tile_args_ok("wan_tile_gather", dtype, t_starts, y_starts, x_starts, Kt, Ky, Kx, B, C, Fs, H, W, n, th, tw, G);
    if (ok != WAN_OK) return ok;
    const int K = Kt * Ky * Kx;                       // <= WAN_WINDOW_MAX^3
    WAN_REQUIRE(0 <= k0 && k0 < k1 && k1 <= K, WAN_ERR_INVALID, "wan_tile_gather: tile range [%d, %d) of %d", k0, k1, K);
    const int64_t Fw = 2 * (int64_t)n + G, rows = (int64_t)(k1 - k0) * B * C, row_len = Fw * th * tw;
    WAN_REQUIRE(rows * Fw * th <= 0x7fffffff, WAN_ERR_INVALID, "wan_tile_gather: %lld tile rows", (long long)(rows * Fw * th));
    WAN_REQUIRE((rep == 1 || rep == 2) && (rep == 1 || rep_stride >= rows * row_len), WAN_ERR_INVALID,
                "wan_tile_gather: rep=%d (1 or 2), rep_stride=%lld < %lld", rep, (long long)rep_stride, (long long)(rows * row_len));
    const int64_t es = dtype == 0 ? 4 : 2;
    const int ub = tile_unit_bytes(es, {tw, W, rep == 2 ? rep_stride : 0}, x_starts, Kx, (uintptr_t)out | (uintptr_t)state);
    const int N = (int)(ub / es), ru = tw / N, cw = std::min(ru, 256), rp = 256 / cw;
    const TileAxes ax = tile_axes(t_starts, y_starts, x_starts, Kt, Ky, Kx, N);
    const dim3 grid((unsigned)rows, (unsigned)Fw, chunks(th, UNROLL * rp, rows * Fw));
    hipStream_t s = (hipStream_t)stream;
#define WAN_GATHER(U)                                                                                                          \
    hipLaunchKernelGGL(tile_gather_kernel<U>, grid, dim3(256), 0, s, (U*)out, (const U*)state, ax.t, ax.y, ax.x, k0, B, C, Kt, Ky, \
                       Kx, n, th, G, Fs, (int64_t)H * W / N, W / N, ru, cw, rp, rep, rep_stride / N)
    if (ub == 16) WAN_GATHER(u32x4);
    else if (ub == 8) WAN_GATHER(u32x2);
    else if (ub == 4) WAN_GATHER(unsigned int);
    else WAN_GATHER(unsigned short);
#undef WAN_GATHER
    WAN_CHECK_LAUNCH("wan_tile_gather");
    return WAN_OK;
}

extern "C" wan_status_t wan_tile_blend(void* out, const void* pred, int dtype, const float* at_tab, const float* ay, const float* ax,
                                       const int* t_starts, const int* y_starts, const int* x_starts, int Kt, int Ky, int Kx, int B,
                                       int C, int Fs, int H, int W, int n, int th, int tw, int G, void* stream) {
    WAN_REQUIRE(out && pred && at_tab && ay && ax, WAN_ERR_INVALID, "wan_tile_blend: null tensor");
    const wan_status_t ok = tile_args_ok("wan_tile_blend", dtype, t_starts, y_starts, x_starts, Kt, Ky, Kx, B, C, Fs, H, W, n, th, tw, G);
    if (ok != WAN_OK) return ok;
    const int64_t Fw = 2 * (int64_t)n + G, frames = (int64_t)B * C * (2 * (int64_t)Fs + (int64_t)Kt * G);
    WAN_REQUIRE((int64_t)Kt * Ky * Kx * B * C * Fw * th <= 0x7fffffff, WAN_ERR_INVALID, "wan_tile_blend: %lld tile rows",
                (long long)((int64_t)Kt * Ky * Kx * B * C * Fw * th));
    const int64_t es = dtype == 0 ? 4 : 2;
    const int ub = tile_unit_bytes(es, {tw, W}, x_starts, Kx, (uintptr_t)out | (uintptr_t)pred | (uintptr_t)ax);
    const int N = (int)(ub / es), wu = W / N, cw = std::min(wu, 256), rp = 256 / cw;
    const TileAxes axes = tile_axes(t_starts, y_starts, x_starts, Kt, Ky, Kx, N);
    const dim3 grid((unsigned)frames, chunks(H, UNROLL * rp, frames));
    hipStream_t s = (hipStream_t)stream;
#define WAN_BLEND(T, N_)                                                                                                       \
    hipLaunchKernelGGL((tile_blend_kernel<T, N_>), grid, dim3(256), 0, s, (T*)out, (const T*)pred, at_tab, ay, ax, axes.t, axes.y, \
                       axes.x, B, C, Kt, Ky, Kx, n, th, tw, G, Fs, H, W, wu, cw, rp)
    if (dtype == 0) {
        if (N == 4) WAN_BLEND(float, 4); else if (N == 2) WAN_BLEND(float, 2); else WAN_BLEND(float, 1);
    } else {
        if (N == 8) WAN_BLEND(bf16_t, 8); else if (N == 4) WAN_BLEND(bf16_t, 4); else if (N == 2) WAN_BLEND(bf16_t, 2);
        else WAN_BLEND(bf16_t, 1);
    }
#undef WAN_BLEND
    WAN_CHECK_LAUNCH("wan_tile_blend");
    return WAN_OK;
}
