// Edit inside a mask: the two passes a masked denoise loop adds.
//   wan_latent_mask_u8     a pixel mask uint8 [B, T, H, W] as latent-cell weights uint8 [B, Fl, H/8, W/8], once per call: the maximum
//                          over a cell's pixels and frames, a grey-scale dilation, a box feather (three small integer kernels)
//   wan_masked_prediction  every step, in place on the prediction of the loop state [source | grounding | target]: outside the mask
//                          the target's prediction becomes the one whose x0 is the source, (x_t - s) / sigma
// The second streams the target block of every (sample, channel) row once: the widest of 16 / 8 / 4 bytes or one element that divides the
// block, the pitches and the bases.  All frame arithmetic is per workgroup (scalar); lanes only add their offset.
#include <algorithm>

#include "common.hpp"

// w * v, (1 - w) * r and their sum are rounded separately (a torch float32 restatement then gives the same bits); the pragma takes the
// permission to fuse them away from every operation of this file (see window_kernels.hip).
#pragma clang fp contract(off)

namespace {

constexpr int RATIO_S = 8, RATIO_T = 4;              // pixels per latent cell, pixel frames per latent frame (the first holds one)
constexpr int UNROLL = 4;                            // grid-stride iterations a lane keeps in flight together

// ------------------------------------------------------------------------------------------------------------- the latent mask
// one thread per latent cell (b, j, y, x): the maximum over its 8 x 8 pixels of its pixel frames.  `wide`: a cell row as one 8-byte load
// (W % 8 == 0 always; the base is 8-byte aligned), else byte by byte.
__global__ __launch_bounds__(256) void mask_pool_kernel(unsigned char* __restrict__ p, const unsigned char* __restrict__ alpha, int T,
                                                        int H, int W, int Fl, int h, int w, int64_t cells, bool wide) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const int x = (int)(i % w), y = (int)(i / w % h), j = (int)(i / ((int64_t)w * h) % Fl);
    const int64_t b = i / ((int64_t)w * h * Fl);
    const int t0 = j == 0 ? 0 : RATIO_T * j - (RATIO_T - 1), t1 = j == 0 ? 0 : min(RATIO_T * j, T - 1);      // inclusive, < T
    unsigned int m = 0;
    for (int t = t0; t <= t1; ++t) {
        const unsigned char* row = alpha + (((b * T + t) * H + (int64_t)y * RATIO_S) * W + (int64_t)x * RATIO_S);
#pragma unroll
        for (int r = 0; r < RATIO_S; ++r) {
            if (wide) {
                const u32x2 v = *(const u32x2*)(row + (int64_t)r * W);
                // bytewise maximum of the two words, then of the four bytes
                const unsigned int a = v[0], c = v[1];
#pragma unroll
                for (int k = 0; k < 4; ++k) m = max(m, max((a >> (8 * k)) & 255u, (c >> (8 * k)) & 255u));
            } else {
#pragma unroll
                for (int k = 0; k < RATIO_S; ++k) m = max(m, (unsigned int)row[(int64_t)r * W + k]);
            }
        }
    }
    p[i] = (unsigned char)m;
}

// grey-scale dilation: the maximum over the (2 grow + 1)^2 cells and 2 grow_t + 1 latent frames around a cell; nothing outside the frame,
// nothing outside the sample (the maximum is separable, so one pass over the box equals the definition's two)
__global__ __launch_bounds__(256) void mask_grow_kernel(unsigned char* __restrict__ g, const unsigned char* __restrict__ p, int Fl, int h,
                                                        int w, int grow, int grow_t, int64_t cells) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const int x = (int)(i % w), y = (int)(i / w % h), j = (int)(i / ((int64_t)w * h) % Fl);
    const int64_t b = i / ((int64_t)w * h * Fl);
    unsigned int m = 0;
    for (int jj = max(j - grow_t, 0); jj <= min(j + grow_t, Fl - 1); ++jj)
        for (int yy = max(y - grow, 0); yy <= min(y + grow, h - 1); ++yy) {
            const unsigned char* row = p + ((b * Fl + jj) * h + yy) * w;
            for (int xx = max(x - grow, 0); xx <= min(x + grow, w - 1); ++xx) m = max(m, (unsigned int)row[xx]);
        }
    g[i] = (unsigned char)m;
}

// the rounded mean over the (2 feather + 1)^2 cells around a cell, indices clamped: (2 S + m) / (2 m)
__global__ __launch_bounds__(256) void mask_feather_kernel(unsigned char* __restrict__ out, const unsigned char* __restrict__ g, int h,
                                                           int w, int feather, int64_t cells) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const int x = (int)(i % w), y = (int)(i / w % h);
    const unsigned char* frame = g + i / ((int64_t)w * h) * ((int64_t)w * h);
    unsigned int sum = 0;
    for (int dy = -feather; dy <= feather; ++dy) {
        const unsigned char* row = frame + (int64_t)min(max(y + dy, 0), h - 1) * w;
        for (int dx = -feather; dx <= feather; ++dx) sum += row[min(max(x + dx, 0), w - 1)];
    }
    const unsigned int m = (2 * feather + 1) * (2 * feather + 1);
    out[i] = (unsigned char)((2 * sum + m) / (2 * m));
}

// ------------------------------------------------------------------------------------------------------ the masked prediction
template <int BYTES> struct RawOf;                    // BYTES of memory as one load / store
template <> struct RawOf<16> { typedef u32x4 type; };
template <> struct RawOf<8> { typedef u32x2 type; };
template <> struct RawOf<4> { typedef unsigned int type; };
template <> struct RawOf<2> { typedef unsigned short type; };
template <> struct RawOf<1> { typedef unsigned char type; };

template <typename T> struct Bits;                   // one element as bits
template <> struct Bits<float> {
    typedef unsigned int type;
    static __device__ __forceinline__ float to_f32(unsigned int e) { return __uint_as_float(e); }
    static __device__ __forceinline__ unsigned int from_f32(float f) { return __float_as_uint(f); }
};
template <> struct Bits<bf16_t> {
    typedef unsigned short type;
    static __device__ __forceinline__ float to_f32(unsigned short e) { return bf16lo_to_f32((unsigned int)e); }
    static __device__ __forceinline__ unsigned short from_f32(float f) { return (unsigned short)(pack_bf16x2(f, 0.f) & 0xffffu); }   // RNE
};

// grid (row = b * C + c, chunk of the row's units).  `L` = Fs * hw elements of one row's target block, in units of N elements; `pitch` =
// F * hw and `t0` = target_frame0 * hw, in units too.  The weights of a unit are N bytes at unit * N of the sample's (or the one) mask.
template <typename T, int N>
__global__ __launch_bounds__(256) void masked_prediction_kernel(T* __restrict__ pred, const T* __restrict__ sample,
                                                                const unsigned char* __restrict__ weights, int C, int Bm, int64_t L,
                                                                int64_t pitch, int64_t t0, float sigma) {
    typedef typename RawOf<sizeof(T) * N>::type R;
    typedef typename RawOf<N>::type RW;
    typedef typename Bits<T>::type E;
    struct Elems { E e[N]; };
    struct Bytes { unsigned char a[N]; };
    const int64_t row = blockIdx.x;                   // < B * C (checked by the host)
    const int64_t b = row / C;
    R* v_row = (R*)pred + row * pitch + t0;
    const R* xt_row = (const R*)sample + row * pitch + t0;
    const R* s_row = (const R*)sample + row * pitch;
    const RW* w_row = (const RW*)weights + (Bm == 1 ? 0 : b) * L;
    const int64_t stride = (int64_t)gridDim.y * 256;
    for (int64_t u0 = (int64_t)blockIdx.y * 256 + threadIdx.x; u0 < L; u0 += UNROLL * stride) {
        RW wr[UNROLL];
        R vr[UNROLL], xr[UNROLL], sr[UNROLL];         // UNROLL independent loads in flight per lane, then the arithmetic
#pragma unroll
        for (int q = 0; q < UNROLL; ++q) {
            const int64_t u = u0 + q * stride;
            if (u < L) { wr[q] = w_row[u]; vr[q] = v_row[u]; xr[q] = xt_row[u]; sr[q] = s_row[u]; }
        }
#pragma unroll
        for (int q = 0; q < UNROLL; ++q) {
            const int64_t u = u0 + q * stride;
            if (u >= L) continue;
            const Bytes a = __builtin_bit_cast(Bytes, wr[q]);
            const Elems v = __builtin_bit_cast(Elems, vr[q]), xt = __builtin_bit_cast(Elems, xr[q]), s = __builtin_bit_cast(Elems, sr[q]);
            Elems o;
            bool keep = true;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const float w = (float)a.a[i] / 255.0f;                                   // every operation rounded on its own
                const float d = Bits<T>::to_f32(xt.e[i]) - Bits<T>::to_f32(s.e[i]);
                const float r = d / sigma;
                const float inside = w * Bits<T>::to_f32(v.e[i]);
                const float outside = (1.0f - w) * r;
                o.e[i] = a.a[i] == 255 ? v.e[i] : Bits<T>::from_f32(inside + outside);    // weight 255: the prediction's own bits
                keep = keep && a.a[i] == 255;
            }
            if (!keep) v_row[u] = __builtin_bit_cast(R, o);                               // a unit of 255s is not written at all
        }
    }
}

}  // namespace

extern "C" int64_t wan_latent_mask_workspace_bytes(int B, int T, int H, int W) {
    if (B < 1 || T < 1 || H < RATIO_S || W < RATIO_S) return 0;
    const int64_t Fl = 1 + (T - 1 + RATIO_T - 1) / RATIO_T;
    return 2 * (int64_t)B * Fl * (H / RATIO_S) * (W / RATIO_S);
}

extern "C" wan_status_t wan_latent_mask_u8(const void* alpha_u8, void* weights_u8, int B, int T, int H, int W, int ratio_s, int ratio_t,
                                           int grow, int grow_t, int feather, void* workspace, int64_t workspace_bytes, void* stream) {
    WAN_REQUIRE(alpha_u8 && weights_u8 && workspace, WAN_ERR_INVALID, "wan_latent_mask_u8: null tensor");
    WAN_REQUIRE(ratio_s == RATIO_S && ratio_t == RATIO_T, WAN_ERR_INVALID,
                "wan_latent_mask_u8: ratios %d (spatial) and %d (temporal); the kernels are built for %d and %d", ratio_s, ratio_t, RATIO_S,
                RATIO_T);
    WAN_REQUIRE(B >= 1 && T >= 1 && H >= 1 && W >= 1, WAN_ERR_INVALID, "wan_latent_mask_u8: B=%d T=%d H=%d W=%d", B, T, H, W);
    WAN_REQUIRE(H % RATIO_S == 0 && W % RATIO_S == 0, WAN_ERR_INVALID,
                "wan_latent_mask_u8: a frame of %d x %d pixels is no whole number of %d x %d latent cells", H, W, RATIO_S, RATIO_S);
    WAN_REQUIRE(0 <= grow && grow <= WAN_LATENT_MASK_MAX_GROW && 0 <= grow_t && grow_t <= WAN_LATENT_MASK_MAX_GROW_T && 0 <= feather &&
                    feather <= grow,
                WAN_ERR_INVALID, "wan_latent_mask_u8: grow=%d (0..%d) grow_t=%d (0..%d) feather=%d (0..grow)", grow,
                WAN_LATENT_MASK_MAX_GROW, grow_t, WAN_LATENT_MASK_MAX_GROW_T, feather);
    const int Fl = 1 + (T - 1 + RATIO_T - 1) / RATIO_T, h = H / RATIO_S, w = W / RATIO_S;
    const int64_t cells = (int64_t)B * Fl * h * w;
    WAN_REQUIRE((int64_t)B * T * H * W <= 0x7fffffff, WAN_ERR_INVALID, "wan_latent_mask_u8: %lld mask bytes (at most 2^31 - 1)",
                (long long)((int64_t)B * T * H * W));
    WAN_REQUIRE(workspace_bytes >= 2 * cells, WAN_ERR_INVALID, "wan_latent_mask_u8: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)(2 * cells));
    unsigned char* p = (unsigned char*)workspace;
    unsigned char* g = p + cells;
    const bool wide = ((uintptr_t)alpha_u8 & 7) == 0;                      // W % 8 == 0: every cell row then starts 8-byte aligned
    const dim3 grid((unsigned)((cells + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mask_pool_kernel, grid, dim3(256), 0, s, p, (const unsigned char*)alpha_u8, T, H, W, Fl, h, w, cells, wide);
    hipLaunchKernelGGL(mask_grow_kernel, grid, dim3(256), 0, s, g, p, Fl, h, w, grow, grow_t, cells);
    hipLaunchKernelGGL(mask_feather_kernel, grid, dim3(256), 0, s, (unsigned char*)weights_u8, g, h, w, feather, cells);
    WAN_CHECK_LAUNCH("wan_latent_mask_u8");
    return WAN_OK;
}

extern "C" wan_status_t wan_masked_prediction(void* pred, const void* sample, int dtype, const void* weights_u8, int B, int Bm, int C,
                                              int F, int Fs, int target_frame0, int64_t hw, float sigma, void* stream) {
    WAN_REQUIRE(pred && sample && weights_u8, WAN_ERR_INVALID, "wan_masked_prediction: null tensor");
    WAN_REQUIRE(dtype == 0 || dtype == 1, WAN_ERR_INVALID, "wan_masked_prediction: dtype=%d (0 fp32, 1 bf16)", dtype);
    WAN_REQUIRE(sigma > 0.0f && sigma <= 3.0e38f, WAN_ERR_INVALID, "wan_masked_prediction: sigma=%g (a finite value above 0)",
                (double)sigma);
    WAN_REQUIRE(B >= 1 && C >= 1 && hw >= 1 && (Bm == 1 || Bm == B), WAN_ERR_INVALID,
                "wan_masked_prediction: B=%d C=%d hw=%lld, weights for %d samples (1 or B)", B, C, (long long)hw, Bm);
    WAN_REQUIRE(Fs >= 1 && target_frame0 >= Fs && (int64_t)target_frame0 + Fs <= F, WAN_ERR_INVALID,
                "wan_masked_prediction: Fs=%d source frames and the target at [%d, %d + %d) do not fit %d frames", Fs, target_frame0,
                target_frame0, Fs, F);
    WAN_REQUIRE((int64_t)B * C <= 0x7fffffff && hw <= 0x7fffffff && (int64_t)F * hw <= 0x7fffffff, WAN_ERR_INVALID,
                "wan_masked_prediction: %lld rows of %lld elements (each at most 2^31 - 1)", (long long)((int64_t)B * C),
                (long long)((int64_t)F * hw));
    const int64_t es = dtype == 0 ? 4 : 2, L = (int64_t)Fs * hw, pitch = (int64_t)F * hw, t0 = (int64_t)target_frame0 * hw;
    // the largest of 16, 8, 4 bytes or one element that divides (in bytes) the block, the pitch, the target's offset and the tensors'
    // bases; a unit's N weights are N bytes at a multiple of N, so the mask's base must be a multiple of N as well
    uint64_t m = (uint64_t)(uintptr_t)pred | (uint64_t)(uintptr_t)sample | (uint64_t)(L * es) | (uint64_t)(pitch * es) | (uint64_t)(t0 * es);
    int ub = 16;
    while (ub > es && ((m & (uint64_t)(ub - 1)) != 0 || ((uintptr_t)weights_u8 & (uintptr_t)(ub / es - 1)) != 0)) ub /= 2;
    const int N = (int)(ub / es);
    const int64_t rows = (int64_t)B * C, units = L / N;
    const dim3 grid((unsigned)rows, (unsigned)std::max<int64_t>(1, std::min<int64_t>((units + 256 * UNROLL - 1) / (256 * UNROLL),
                                                                                     std::max<int64_t>(1, 4096 / rows))));
    hipStream_t s = (hipStream_t)stream;
#define WAN_MASKED(T, N_)                                                                                                     \
    hipLaunchKernelGGL((masked_prediction_kernel<T, N_>), grid, dim3(256), 0, s, (T*)pred, (const T*)sample,                  \
                       (const unsigned char*)weights_u8, C, Bm, units, pitch / N_, t0 / N_, sigma)
    if (dtype == 0) {
        if (N == 4) WAN_MASKED(float, 4); else if (N == 2) WAN_MASKED(float, 2); else WAN_MASKED(float, 1);
    } else {
        if (N == 8) WAN_MASKED(bf16_t, 8); else if (N == 4) WAN_MASKED(bf16_t, 4); else if (N == 2) WAN_MASKED(bf16_t, 2);
        else WAN_MASKED(bf16_t, 1);
    }
#undef WAN_MASKED
    WAN_CHECK_LAUNCH("wan_masked_prediction");
    return WAN_OK;
}
