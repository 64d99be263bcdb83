// uint8 video frames <-> the VAE's planar video, on both sides of an edit.
//   in : what a video reader yields, uint8 [B, T, H, W, 3]  ->  [B, 3, T, H, W] in the dtype AutoencoderKLWan.encode consumes
//   out: what AutoencoderKLWan.decode returns, [B, 3, T, H, W]  ->  uint8 [B, T, H, W, 3], what a video writer takes
// Pure streaming kernels.  A frame is one run of H*W pixels on both sides (3*H*W interleaved bytes, three planes of H*W elements),
// so the kernels index pixels of a frame, not rows.  Wide path: one thread per 16 pixels = 48 interleaved bytes = three 16-byte
// accesses; the 16 elements of each channel are two (bf16) or four (fp32) 16-byte accesses; whole pixels are regrouped in
// registers with compile-time byte positions.  It needs H*W % 16 == 0 and 16-byte aligned bases; everything else (odd byte rows,
// offset views) takes the element-wise kernels.
#include <algorithm>
#include <initializer_list>

#include "common.hpp"

namespace {

constexpr int PIX = 16;                     // pixels per thread on the wide path

// fast_infer.py:89-90: `.float()`, then `x * (2.0 / 255.0) - 1.0` = two float32 torch ops, each rounded on its own (the Python
// double 2.0 / 255.0 enters the float32 multiplication rounded to float32).  No contraction into one FMA.
__device__ __forceinline__ float byte_to_video(unsigned int u) {
#pragma clang fp contract(off)
    const float scaled = (float)u * (float)(2.0 / 255.0);
    return scaled - 1.0f;
}

// pipeline_wan.py:426-427 `(frames / 2 + 0.5).clamp(0, 1)` in the VAE's dtype (a bf16 tensor op computes in float32 and rounds its
// result to bf16: once after the division, once after the addition), `.float()`, then utils.py:67 `(x * 255)` in float32 and
// `.astype(np.uint8)` = truncation.
template <typename TIn> __device__ __forceinline__ float video_to_unit(float x);
template <> __device__ __forceinline__ float video_to_unit<bf16_t>(float x) {
#pragma clang fp contract(off)
    const float half = (float)(bf16_t)(x * 0.5f);
    return (float)(bf16_t)(half + 0.5f);
}
template <> __device__ __forceinline__ float video_to_unit<float>(float x) {
#pragma clang fp contract(off)
    const float half = x * 0.5f;
    return half + 0.5f;
}
template <typename TIn> __device__ __forceinline__ unsigned int video_to_byte(float x) {
    const float u = fminf(fmaxf(video_to_unit<TIn>(x), 0.f), 1.f);
    return (unsigned int)(u * 255.0f);                    // v_cvt_u32_f32 truncates
}

template <typename T> struct chunk16;                      // 16 planar elements as 16-byte words
template <> struct chunk16<bf16_t> { u32x4 q[2]; };
template <> struct chunk16<float> { f32x4 q[4]; };

__device__ __forceinline__ void unpack16(const chunk16<bf16_t>& c, float (&v)[PIX]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned int w = c.q[j >> 2][j & 3];
        v[2 * j] = bf16lo_to_f32(w);
        v[2 * j + 1] = bf16hi_to_f32(w);
    }
}
__device__ __forceinline__ void unpack16(const chunk16<float>& c, float (&v)[PIX]) {
#pragma unroll
    for (int j = 0; j < PIX; ++j) v[j] = c.q[j >> 2][j & 3];
}
__device__ __forceinline__ void pack16(const float (&v)[PIX], chunk16<bf16_t>& c) {
#pragma unroll
    for (int j = 0; j < 8; ++j) c.q[j >> 2][j & 3] = pack_bf16x2(v[2 * j], v[2 * j + 1]);      // round-to-nearest-even
}
__device__ __forceinline__ void pack16(const float (&v)[PIX], chunk16<float>& c) {
#pragma unroll
    for (int j = 0; j < PIX; ++j) c.q[j >> 2][j & 3] = v[j];
}

// ---- in: uint8 [BT, npix, 3] -> TOut [B, 3, T, npix]
template <typename TOut>
__global__ __launch_bounds__(256) void frames_to_video_wide_kernel(const uint8_t* __restrict__ frames, TOut* __restrict__ out,
                                                                   int T, int64_t npix) {
    const int64_t bt = blockIdx.y;                          // one frame per grid row (no 64-bit division per thread)
    const int64_t b = blockIdx.y / (unsigned)T, t = bt - b * T;
    for (int64_t p0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * PIX; p0 < npix; p0 += (int64_t)gridDim.x * blockDim.x * PIX) {
        const u32x4* src = reinterpret_cast<const u32x4*>(frames + (bt * npix + p0) * 3);
        const u32x4 s0 = src[0], s1 = src[1], s2 = src[2];
        unsigned int w[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) { w[j] = s0[j]; w[4 + j] = s1[j]; w[8 + j] = s2[j]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[PIX];
#pragma unroll
            for (int p = 0; p < PIX; ++p) {
                const int k = 3 * p + c;                    // byte of the 48
                v[p] = byte_to_video((w[k >> 2] >> ((k & 3) * 8)) & 0xffu);
            }
            chunk16<TOut> ch;
            pack16(v, ch);
            *reinterpret_cast<chunk16<TOut>*>(out + ((b * 3 + c) * T + t) * npix + p0) = ch;
        }
    }
}

template <typename TOut>
__global__ __launch_bounds__(256) void frames_to_video_kernel(const uint8_t* __restrict__ frames, TOut* __restrict__ out,
                                                              int T, int64_t npix) {
    // one thread per pixel: three byte reads, three plane writes (coalesced along the plane)
    const int64_t bt = blockIdx.y;
    const int64_t b = blockIdx.y / (unsigned)T, t = bt - b * T;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out[((b * 3 + c) * T + t) * npix + p] = (TOut)byte_to_video(frames[(bt * npix + p) * 3 + c]);
    }
}

// ---- out: TIn [B, 3, T, npix], frames [t0, t0 + nt) -> uint8 [B, T_out, npix, 3] from frame t_dst on
template <typename TIn>
__global__ __launch_bounds__(256) void video_to_frames_wide_kernel(const TIn* __restrict__ video, uint8_t* __restrict__ frames,
                                                                   int T, int64_t npix, int t0, int nt, int T_out, int t_dst) {
    const int64_t b = blockIdx.y / (unsigned)nt, t = blockIdx.y - b * nt;      // grid rows = B * nt frames
    for (int64_t p0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * PIX; p0 < npix; p0 += (int64_t)gridDim.x * blockDim.x * PIX) {
        unsigned int w[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) w[j] = 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const chunk16<TIn> ch = *reinterpret_cast<const chunk16<TIn>*>(video + ((b * 3 + c) * T + t0 + t) * npix + p0);
            float v[PIX];
            unpack16(ch, v);
#pragma unroll
            for (int p = 0; p < PIX; ++p) {
                const int k = 3 * p + c;
                w[k >> 2] |= video_to_byte<TIn>(v[p]) << ((k & 3) * 8);
            }
        }
        u32x4* dst = reinterpret_cast<u32x4*>(frames + ((b * T_out + t_dst + t) * npix + p0) * 3);
        dst[0] = u32x4{w[0], w[1], w[2], w[3]};
        dst[1] = u32x4{w[4], w[5], w[6], w[7]};
        dst[2] = u32x4{w[8], w[9], w[10], w[11]};
    }
}

template <typename TIn>
__global__ __launch_bounds__(256) void video_to_frames_kernel(const TIn* __restrict__ video, uint8_t* __restrict__ frames,
                                                              int T, int64_t npix, int t0, int nt, int T_out, int t_dst) {
    const int64_t b = blockIdx.y / (unsigned)nt, t = blockIdx.y - b * nt;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        uint8_t* dst = frames + ((b * T_out + t_dst + t) * npix + p) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            dst[c] = (uint8_t)video_to_byte<TIn>((float)video[((b * 3 + c) * T + t0 + t) * npix + p]);
    }
}

// ---- compose: n_src source clips -> rectangles of one uint8 [T_out, Hc, Wc, 3] canvas, the rest of it the pad byte
// A thread owns one 16-byte piece of a canvas row, cut at the 16-byte boundaries of the row's ADDRESS (as the resample kernel cuts
// its output): a piece that lies inside the row is one dwordx4 store whatever Wc * 3 and the base are, the one or two pieces that
// stick out of the row are stored byte by byte.  The destination rectangles do not overlap (checked on the host), so every source
// that touches the piece ORs its bytes into the piece's four words and what no source touches becomes the pad byte.  A piece that lies inside ONE
// interleaved uint8 source is read as the two aligned 16-byte words around its (arbitrarily aligned) source bytes and shifted into
// place; everything else -- planar float sources, pieces across a rectangle's edge, words that would reach outside the source
// tensor -- is read element by element.
struct compose_args {
    wan_compose_src src[WAN_COMPOSE_MAX_SRC];
    uint8_t* canvas;
    int n_src, Hc, Wc;
    unsigned int pad;        // the pad byte in all four bytes of a word
    int ppr;                 // pieces per row, an upper bound: (15 + Wc * 3 + 15) / 16
};

// fast_infer.py:188-189 `(video + 1.0) / 2.0` where the range rule asks for it, `.clamp(0.0, 1.0)`: tensor ops in the video's dtype
// (a bf16 op computes in float32 and rounds its result to bf16; halving is exact in both).
__device__ __forceinline__ float rescale_half(float x, bool rescale, bool bf) {
#pragma clang fp contract(off)
    if (rescale) {
        float a = x + 1.0f;
        if (bf) a = (float)(bf16_t)a;
        x = a * 0.5f;
        if (bf) x = (float)(bf16_t)x;
    }
    return x;
}
// utils.py:67 `(x * 255)` in float32, `.astype(np.uint8)` = truncation
__device__ __forceinline__ unsigned int unit_to_byte(float x) {
#pragma clang fp contract(off)
    return (unsigned int)(fminf(fmaxf(x, 0.f), 1.f) * 255.0f);
}
// the writer without a clamp in front (WAN_COMPOSE_WRITER): low byte of the truncated int32 outside [0, 256)
__device__ __forceinline__ unsigned int writer_byte(float x) {
#pragma clang fp contract(off)
    return (unsigned int)(int)(x * 255.0f) & 0xffu;
}
__device__ __forceinline__ unsigned int compose_u8(unsigned int u, int mode, bool rescale) {
    return mode == WAN_COMPOSE_COPY ? u : unit_to_byte(rescale_half(byte_to_video(u), rescale, false));
}
__device__ __forceinline__ unsigned int compose_float(float x, int mode, bool rescale, bool bf) {
    const float v = rescale_half(x, rescale, bf);
    return mode == WAN_COMPOSE_WRITER ? writer_byte(v) : unit_to_byte(v);
}

__device__ __forceinline__ bool compose_rescale(const wan_compose_src& s) {
    return s.rescale_flag ? *s.rescale_flag == 1 : s.rescale != 0;
}

// 16 bytes from the byte address `addr` (any alignment) out of the aligned words lo = [addr & ~15], hi = the next one
__device__ __forceinline__ void shift16(const u32x4 lo, const u32x4 hi, int sh, unsigned int (&w)[4]) {
    const unsigned int v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    const unsigned int sb = (unsigned int)sh & 3u;
    switch (sh >> 2) {
#define WAN_SHIFT16_CASE(o)                                                                              \
    case o:                                                                                              \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) w[i] = __builtin_amdgcn_alignbyte(v[i + o + 1], v[i + o], sb); \
        break;
        WAN_SHIFT16_CASE(0)
        WAN_SHIFT16_CASE(1)
        WAN_SHIFT16_CASE(2)
        default:
        WAN_SHIFT16_CASE(3)
#undef WAN_SHIFT16_CASE
    }
}

__global__ __launch_bounds__(256) void frames_compose_kernel(const compose_args a) {
    const int t = blockIdx.y;
    const int row_bytes = a.Wc * 3;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)a.Hc * a.ppr) return;
    const int y = (int)((unsigned int)idx / (unsigned int)a.ppr), q = (int)idx - y * a.ppr;
    uint8_t* row = a.canvas + ((int64_t)t * a.Hc + y) * row_bytes;
    const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15);
    const int b0 = 16 * q - mis;                                   // row byte at the piece's first byte (< 0 in front of the row)
    const int lo = max(b0, 0), hi = min(b0 + 16, row_bytes);       // the piece's bytes of this row: [lo, hi)
    if (lo >= hi) return;
    const int xa = lo / 3, xb = (hi - 1) / 3;                      // first and last pixel it touches
    const bool full = hi - lo == 16;
    unsigned int w[4] = {0u, 0u, 0u, 0u}, cov[4] = {0u, 0u, 0u, 0u};   // the piece's bytes; 0xff in every byte a source has written

    for (int k = 0; k < a.n_src; ++k) {
        const wan_compose_src& s = a.src[k];
        const int yy = y - s.dst_y;
        if (t >= s.nt || yy < 0 || yy >= s.h || xb < s.dst_x || xa >= s.dst_x + s.w) continue;
        const bool rescale = compose_rescale(s);
        // element offset of (frame t, row yy, column 0) of the crop window
        const int64_t off = (int64_t)(s.t0 + t) * s.stride_t + (int64_t)(s.y0 + yy) * s.stride_y + (int64_t)s.x0 * s.stride_x;
        if (s.kind == WAN_COMPOSE_U8) {
            const uint8_t* base = (const uint8_t*)s.base;
            bool done = false;
            if (full && xa >= s.dst_x && xb < s.dst_x + s.w && s.stride_x == 3 && s.stride_c == 1) {
                // source byte of row byte b: off + (b - 3 * dst_x); contiguous over the piece
                const int64_t so = off + (int64_t)b0 - 3 * (int64_t)s.dst_x;
                const int sh = (int)((reinterpret_cast<uintptr_t>(base) + (uintptr_t)so) & 15);
                const int64_t first = so - sh, end = first + (sh ? 32 : 16);
                if (first >= 0 && end <= s.extent) {
                    const u32x4* p = reinterpret_cast<const u32x4*>(base + first);
                    const u32x4 v0 = p[0];
                    const u32x4 v1 = sh ? p[1] : v0;
                    shift16(v0, v1, sh, w);
                    if (s.mode != WAN_COMPOSE_COPY) {
                        unsigned int r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                        for (int j = 0; j < 16; ++j)
                            r[j >> 2] |= compose_u8((w[j >> 2] >> ((j & 3) * 8)) & 0xffu, s.mode, rescale) << ((j & 3) * 8);
#pragma unroll
                        for (int i = 0; i < 4; ++i) w[i] = r[i];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) cov[i] = 0xffffffffu;
                    done = true;
                }
            }
            if (!done) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int b = b0 + j;
                    if (b < lo || b >= hi) continue;
                    const int x = (int)((unsigned int)b / 3u), c = b - 3 * x, xx = x - s.dst_x;
                    if (xx < 0 || xx >= s.w) continue;
                    const unsigned int u = base[off + (int64_t)xx * s.stride_x + (int64_t)c * s.stride_c];
                    w[j >> 2] |= compose_u8(u, s.mode, rescale) << ((j & 3) * 8);
                    cov[j >> 2] |= 0xffu << ((j & 3) * 8);
                }
            }
        } else {
            const bool bf = s.kind == WAN_COMPOSE_BF16;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int b = b0 + j;
                if (b < lo || b >= hi) continue;
                const int x = (int)((unsigned int)b / 3u), c = b - 3 * x, xx = x - s.dst_x;
                if (xx < 0 || xx >= s.w) continue;
                const int64_t e = off + (int64_t)xx * s.stride_x + (int64_t)c * s.stride_c;
                const float v = bf ? (float)((const bf16_t*)s.base)[e] : ((const float*)s.base)[e];
                w[j >> 2] |= compose_float(v, s.mode, rescale, bf) << ((j & 3) * 8);
                cov[j >> 2] |= 0xffu << ((j & 3) * 8);
            }
        }
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] |= a.pad & ~cov[i];
    uint8_t* d = row + b0;                                         // 16-byte aligned
    if (full) {
        *reinterpret_cast<u32x4*>(d) = u32x4{w[0], w[1], w[2], w[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (b0 + j >= lo && b0 + j < hi) d[j] = (uint8_t)(w[j >> 2] >> ((j & 3) * 8));
    }
}

// ---- the range rule of _normalize_to_01 (fast_infer.py:185-187) as a word in device memory
// bit 0: an element < 0 or > 1 was seen; bit 1: a NaN was seen.  Decided on the bits of the float32 value (the library is built
// with -fno-honor-nans, which lets the compiler fold float comparisons with a NaN).
__device__ __forceinline__ unsigned int range_bits(float x) {
    const unsigned int u = __float_as_uint(x), m = u & 0x7fffffffu;
    if (m > 0x7f800000u) return 2u;
    const bool neg = (u >> 31) != 0u && m != 0u;                   // -0.0 < 0.0 is false
    return (neg || (!(u >> 31) && m > 0x3f800000u)) ? 1u : 0u;
}
template <typename T> struct range_vec;
template <> struct range_vec<uint8_t> {
    static constexpr int N = 16;
    __device__ static unsigned int elem(const uint8_t* p) { return range_bits(byte_to_video(*p)); }
    __device__ static unsigned int vec(const u32x4 v) {
        unsigned int r = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) r |= range_bits(byte_to_video((v[j >> 2] >> ((j & 3) * 8)) & 0xffu));
        return r;
    }
};
template <> struct range_vec<float> {
    static constexpr int N = 4;
    __device__ static unsigned int elem(const float* p) { return range_bits(*p); }
    __device__ static unsigned int vec(const u32x4 v) {
        return range_bits(__uint_as_float(v[0])) | range_bits(__uint_as_float(v[1])) | range_bits(__uint_as_float(v[2])) |
               range_bits(__uint_as_float(v[3]));
    }
};
template <> struct range_vec<bf16_t> {
    static constexpr int N = 8;
    __device__ static unsigned int elem(const bf16_t* p) { return range_bits((float)*p); }
    __device__ static unsigned int vec(const u32x4 v) {
        unsigned int r = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) r |= range_bits(bf16lo_to_f32(v[j])) | range_bits(bf16hi_to_f32(v[j]));
        return r;
    }
};

// nvec 16-byte words from x (0 when x is not 16-byte aligned), then the elements [nvec * N, n) one by one
template <typename T>
__global__ __launch_bounds__(256) void range_flag_kernel(const T* __restrict__ x, int64_t n, int64_t nvec, int* __restrict__ flag) {
    using V = range_vec<T>;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    unsigned int bits = 0u;
    const u32x4* xv = reinterpret_cast<const u32x4*>(x);
    for (int64_t i = tid; i < nvec; i += step) bits |= V::vec(xv[i]);
    for (int64_t i = nvec * V::N + tid; i < n; i += step) bits |= V::elem(x + i);
    const unsigned int wave = (__any((int)(bits & 1u)) ? 1u : 0u) | (__any((int)(bits & 2u)) ? 2u : 0u);
    if ((threadIdx.x & (WAN_WAVE - 1)) == 0 && wave) atomicOr(flag, (int)wave);
}

template <typename T> void launch_range_flag(const void* x, int64_t n, int* flag, hipStream_t s) {
    const int64_t nvec = (uintptr_t)x % 16 == 0 ? n / range_vec<T>::N : 0;
    const int64_t items = std::max<int64_t>(nvec, n - nvec * range_vec<T>::N);
    const unsigned blocks = (unsigned)std::min<int64_t>((items + 255) / 256, 2048);
    hipLaunchKernelGGL(range_flag_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)x, n, nvec, flag);
}

// ---- the two conversions on a rectangle of the frame (`edit_region_vae_halo`): the VAE sees the box only
//   in : the box [by, by + bh) x [bx, bx + bw) of uint8 [B, T, H, W, 3]  ->  [B, 3, T, bh, bw], byte_to_video's arithmetic
//   out: [B, 3, T, bh, bw] and the uint8 source frames  ->  uint8 [B, T_out, H, W, 3]: the source's bytes, and inside the region's
//        rectangle (which lies inside the box) the decoder's bytes (video_to_byte) blended over them
// Streams of rows at a pitch, as the region kernels of edit_region.hip.  The access unit is N = 16, 8, 4, 2 or 1 PIXELS: the largest
// that divides W, the box's x origin and width and the byte tensors' base addresses, and leaves the planes' words aligned
// (box_unit_pixels below: the rule of tile_unit_bytes in window_kernels.hip, counted in pixels because an interleaved pixel is 3 bytes
// and 3 is odd -- N pixels are three aligned N-byte words exactly where N divides the pixel index and the base).  So all x arithmetic
// is in whole units and no unit straddles the box's edge.  A workgroup is `rp` rows of `cw` lanes each (cw = min(units per row, 256),
// rp = 256 / cw; lanes beyond rp * cw idle): which frame and where the box lies are per workgroup (scalar); a lane adds its row and unit.
template <int BYTES> struct RawOf;                        // BYTES of memory as one load / store
template <> struct RawOf<16> { typedef u32x4 type; };
template <> struct RawOf<8> { typedef u32x2 type; };
template <> struct RawOf<4> { typedef unsigned int type; };
template <> struct RawOf<2> { typedef unsigned short type; };
template <> struct RawOf<1> { typedef unsigned char type; };

template <int N> struct PixelUnit {                       // N interleaved pixels: three N-byte words
    typedef typename RawOf<N>::type word_t;
    struct Raw { word_t q[3]; };
    struct Bytes { unsigned char v[3 * N]; };
    __device__ static Bytes load(const uint8_t* p) {
        const word_t* w = reinterpret_cast<const word_t*>(p);
        const Raw r = {{w[0], w[1], w[2]}};
        return __builtin_bit_cast(Bytes, r);
    }
    __device__ static void store(uint8_t* p, const Bytes& b) {
        const Raw r = __builtin_bit_cast(Raw, b);
        word_t* w = reinterpret_cast<word_t*>(p);
        w[0] = r.q[0]; w[1] = r.q[1]; w[2] = r.q[2];
    }
};

template <typename T, int N> struct PlaneUnit {           // N planar elements: the widest words their bytes allow, 16 at the most
    static constexpr int BYTES = (int)sizeof(T) * N, WORD = BYTES < 16 ? BYTES : 16, WORDS = BYTES / WORD;
    typedef typename RawOf<WORD>::type word_t;
    struct Raw { word_t q[WORDS]; };
    struct Vals { T v[N]; };
    __device__ static Vals load(const T* p) {
        const word_t* w = reinterpret_cast<const word_t*>(p);
        Raw r;
#pragma unroll
        for (int i = 0; i < WORDS; ++i) r.q[i] = w[i];
        return __builtin_bit_cast(Vals, r);
    }
    __device__ static void store(T* p, const Vals& v) {
        const Raw r = __builtin_bit_cast(Raw, v);
        word_t* w = reinterpret_cast<word_t*>(p);
#pragma unroll
        for (int i = 0; i < WORDS; ++i) w[i] = r.q[i];
    }
};

// grid (b * T + t, row chunk); `bwu` = bw / N units per box row
template <typename TOut, int N>
__global__ __launch_bounds__(256) void frames_box_to_video_kernel(const uint8_t* __restrict__ frames, TOut* __restrict__ out, int T,
                                                                  int H, int W, int by, int bx, int bh, int bwu, int cw, int rp) {
    const unsigned bt = blockIdx.x;                       // < B * T (the grid)
    const unsigned b = bt / (unsigned)T, t = bt - b * (unsigned)T;
    const int lr = threadIdx.x / cw, lu = threadIdx.x % cw;
    if (lr >= rp) return;
    const uint8_t* src = frames + (((int64_t)bt * H + by) * W + bx) * 3;       // the box's first byte in this frame (inside it: the host)
    const int64_t plane = (int64_t)bh * bwu * N;
    TOut* dst = out + ((int64_t)b * 3 * T + t) * plane;   // channel c of this frame: + c * T * plane
    for (int y = blockIdx.y * rp + lr; y < bh; y += gridDim.y * rp)
        for (int u = lu; u < bwu; u += cw) {              // one pass unless a box row is longer than 256 units
            const typename PixelUnit<N>::Bytes px = PixelUnit<N>::load(src + ((int64_t)y * W + u * N) * 3);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                typename PlaneUnit<TOut, N>::Vals o;
#pragma unroll
                for (int j = 0; j < N; ++j) o.v[j] = (TOut)byte_to_video(px.v[3 * j + c]);
                PlaneUnit<TOut, N>::store(dst + c * T * plane + ((int64_t)y * bwu + u) * N, o);
            }
        }
}

struct stitch_args {
    const void* video;                                    // [B, 3, T, bh, bw]
    const uint8_t* source;                                // [Bs, Ts, H, W, 3]
    uint8_t* frames;                                      // [B, T_out, H, W, 3]
    int T, Ts, T_out, H, W, t0, nt, src_t0, t_dst;
    int one_source;                                       // Bs == 1: every sample stitches against sample 0
    int by, bx, bh, bw, ry, rx, rh, rw, feather;
    int top, bottom, left, right;                         // 1: that edge of the rectangle does not lie on the frame's border, so it ramps
    int wu, cw, rp;                                       // W / N units per frame row; the workgroup's shape
};

// grid (b * nt + t, row chunk).  Every byte of the frame is written once: the source's byte, or inside the rectangle
// (a * e + (255 - a) * o + 127) / 255 with e the decoder's byte and a the ramp's weight (255 where no ramp reaches).
template <typename TIn, int N>
__global__ __launch_bounds__(256) void video_box_stitch_kernel(const stitch_args a) {
    const unsigned row = blockIdx.x;                      // < B * nt (the grid)
    const unsigned b = row / (unsigned)a.nt, t = row - b * (unsigned)a.nt;
    const int lr = threadIdx.x / a.cw, lu = threadIdx.x % a.cw;
    if (lr >= a.rp) return;
    const int64_t frame_bytes = (int64_t)a.H * a.W * 3, plane = (int64_t)a.bh * a.bw;
    const uint8_t* src = a.source + ((int64_t)(a.one_source ? 0u : b) * a.Ts + a.src_t0 + t) * frame_bytes;
    uint8_t* dst = a.frames + ((int64_t)b * a.T_out + a.t_dst + t) * frame_bytes;
    const TIn* vid = (const TIn*)a.video + ((int64_t)b * 3 * a.T + a.t0 + t) * plane;      // channel c of this frame: + c * T * plane
    const int f = a.feather;
    for (int y = blockIdx.y * a.rp + lr; y < a.H; y += gridDim.y * a.rp) {
        const bool y_in = y >= a.ry && y < a.ry + a.rh;
        int dy = 0x7fffffff;                              // the distance to the rectangle's ramping rows; none: "infinity"
        if (a.top) dy = y - a.ry;
        if (a.bottom) dy = min(dy, a.ry + a.rh - 1 - y);
        for (int u = lu; u < a.wu; u += a.cw) {           // one pass unless a frame row is longer than 256 units
            const int x0 = u * N;
            const int64_t at = ((int64_t)y * a.W + x0) * 3;
            typename PixelUnit<N>::Bytes px = PixelUnit<N>::load(src + at);
            if (y_in && x0 + N > a.rx && x0 < a.rx + a.rw) {
                // the unit meets the rectangle, so it lies inside the box: bx, bw and x0 are whole units
                typename PlaneUnit<TIn, N>::Vals e[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) e[c] = PlaneUnit<TIn, N>::load(vid + c * a.T * plane + (int64_t)(y - a.by) * a.bw + (x0 - a.bx));
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const int x = x0 + j;
                    unsigned int w = 0u;                  // outside the rectangle: weight 0 gives the source's byte
                    if (x >= a.rx && x < a.rx + a.rw) {
                        int d = dy;
                        if (a.left) d = min(d, x - a.rx);
                        if (a.right) d = min(d, a.rx + a.rw - 1 - x);
                        w = (f == 0 || d >= f) ? 255u : 255u * (unsigned int)(d + 1) / (unsigned int)(f + 1);
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const unsigned int ev = video_to_byte<TIn>((float)e[c].v[j]), ov = px.v[3 * j + c];
                        px.v[3 * j + c] = (unsigned char)((w * ev + (255u - w) * ov + 127u) / 255u);
                    }
                }
            }
            PixelUnit<N>::store(dst + at, px);
        }
    }
}

// the largest of 16, 8, 4, 2 or 1 pixels that divides every length in `lens` (pixels) and the byte tensors' addresses, and whose
// planar elements (of `es` bytes, at `plane_address`) are aligned words of min(16, N * es) bytes
int box_unit_pixels(int64_t es, std::initializer_list<int64_t> lens, uintptr_t byte_addresses, uintptr_t plane_address) {
    uint64_t m = (uint64_t)byte_addresses;
    for (int64_t l : lens) m |= (uint64_t)l;
    int N = 16;
    while (N > 1 && ((m & (uint64_t)(N - 1)) != 0 || (plane_address & (uintptr_t)(std::min<int64_t>(16, N * es) - 1)) != 0)) N /= 2;
    return N;
}

// workgroups along the rows: <= ~4096 in all, at most what the grid's second axis holds; the rest is a grid-stride loop
unsigned box_row_chunks(int rows, int per_group, int64_t frames) {
    const int64_t need = ((int64_t)rows + per_group - 1) / per_group;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(need, 65535), 4096 / frames));
}

bool rect_inside(int H, int W, int y0, int x0, int h, int w) {
    return y0 >= 0 && x0 >= 0 && h >= 1 && w >= 1 && (int64_t)y0 + h <= H && (int64_t)x0 + w <= W;
}

#define WAN_BY_PIXELS(N, LAUNCH)                                         \
    do {                                                                 \
        if ((N) == 16) LAUNCH(16);                                       \
        else if ((N) == 8) LAUNCH(8);                                    \
        else if ((N) == 4) LAUNCH(4);                                    \
        else if ((N) == 2) LAUNCH(2);                                    \
        else LAUNCH(1);                                                  \
    } while (0)

// grid: x over the items (16-pixel chunks or pixels) of one frame, y = frames
dim3 grid_for(int64_t items_per_frame, int64_t frames) {
    return dim3((unsigned)std::min<int64_t>((items_per_frame + 255) / 256, 4096), (unsigned)frames);
}

}  // namespace

extern "C" wan_status_t wan_frames_u8_to_video(const void* frames_u8, void* out, int out_dtype, int B, int T, int H, int W,
                                               void* stream) {
    WAN_REQUIRE(frames_u8 && out, WAN_ERR_INVALID, "wan_frames_u8_to_video: null tensor");
    WAN_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0, WAN_ERR_INVALID, "wan_frames_u8_to_video: bad shape B=%d T=%d H=%d W=%d", B, T, H, W);
    WAN_REQUIRE(out_dtype == 0 || out_dtype == 1, WAN_ERR_INVALID, "wan_frames_u8_to_video: out_dtype=%d (0 fp32, 1 bf16)", out_dtype);
    const int64_t npix = (int64_t)H * W, BT = (int64_t)B * T;
    WAN_REQUIRE(BT <= 65535, WAN_ERR_INVALID, "wan_frames_u8_to_video: B * T = %lld frames (at most 65535 per call)", (long long)BT);
    const bool wide = npix % PIX == 0 && (uintptr_t)frames_u8 % 16 == 0 && (uintptr_t)out % 16 == 0;
    const dim3 blocks = grid_for(wide ? npix / PIX : npix, BT);
    hipStream_t s = (hipStream_t)stream;
    const uint8_t* src = (const uint8_t*)frames_u8;
    if (out_dtype == 0) {
        if (wide) hipLaunchKernelGGL(frames_to_video_wide_kernel<float>, blocks, dim3(256), 0, s, src, (float*)out, T, npix);
        else hipLaunchKernelGGL(frames_to_video_kernel<float>, blocks, dim3(256), 0, s, src, (float*)out, T, npix);
    } else {
        if (wide) hipLaunchKernelGGL(frames_to_video_wide_kernel<bf16_t>, blocks, dim3(256), 0, s, src, (bf16_t*)out, T, npix);
        else hipLaunchKernelGGL(frames_to_video_kernel<bf16_t>, blocks, dim3(256), 0, s, src, (bf16_t*)out, T, npix);
    }
    WAN_CHECK_LAUNCH("wan_frames_u8_to_video");
    return WAN_OK;
}

extern "C" wan_status_t wan_video_to_frames_u8(const void* video, int in_dtype, void* frames_u8, int B, int T, int H, int W,
                                               int t0, int nt, int T_out, int t_dst, void* stream) {
    WAN_REQUIRE(video && frames_u8, WAN_ERR_INVALID, "wan_video_to_frames_u8: null tensor");
    WAN_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0, WAN_ERR_INVALID, "wan_video_to_frames_u8: bad shape B=%d T=%d H=%d W=%d", B, T, H, W);
    WAN_REQUIRE(in_dtype == 0 || in_dtype == 1, WAN_ERR_INVALID, "wan_video_to_frames_u8: in_dtype=%d (0 fp32, 1 bf16)", in_dtype);
    WAN_REQUIRE(t0 >= 0 && nt >= 0 && nt <= T - t0, WAN_ERR_INVALID, "wan_video_to_frames_u8: frames [%d, %d + %d) of %d", t0, t0, nt, T);
    WAN_REQUIRE(t_dst >= 0 && T_out > 0 && nt <= T_out - t_dst, WAN_ERR_INVALID,
                "wan_video_to_frames_u8: %d frames at offset %d of a %d-frame clip", nt, t_dst, T_out);
    if (nt == 0) return WAN_OK;
    WAN_REQUIRE((int64_t)B * nt <= 65535, WAN_ERR_INVALID, "wan_video_to_frames_u8: B * nt = %lld frames (at most 65535 per call)",
                (long long)B * nt);
    const int64_t npix = (int64_t)H * W;
    const bool wide = npix % PIX == 0 && (uintptr_t)video % 16 == 0 && (uintptr_t)frames_u8 % 16 == 0;
    const dim3 blocks = grid_for(wide ? npix / PIX : npix, (int64_t)B * nt);
    hipStream_t s = (hipStream_t)stream;
    uint8_t* dst = (uint8_t*)frames_u8;
    if (in_dtype == 0) {
        if (wide) hipLaunchKernelGGL(video_to_frames_wide_kernel<float>, blocks, dim3(256), 0, s, (const float*)video, dst, T, npix, t0, nt, T_out, t_dst);
        else hipLaunchKernelGGL(video_to_frames_kernel<float>, blocks, dim3(256), 0, s, (const float*)video, dst, T, npix, t0, nt, T_out, t_dst);
    } else {
        if (wide) hipLaunchKernelGGL(video_to_frames_wide_kernel<bf16_t>, blocks, dim3(256), 0, s, (const bf16_t*)video, dst, T, npix, t0, nt, T_out, t_dst);
        else hipLaunchKernelGGL(video_to_frames_kernel<bf16_t>, blocks, dim3(256), 0, s, (const bf16_t*)video, dst, T, npix, t0, nt, T_out, t_dst);
    }
    WAN_CHECK_LAUNCH("wan_video_to_frames_u8");
    return WAN_OK;
}

extern "C" wan_status_t wan_video_range_flag(const void* x, int kind, int64_t n, int* flag, void* stream) {
    WAN_REQUIRE(x && flag, WAN_ERR_INVALID, "wan_video_range_flag: null tensor");
    WAN_REQUIRE(kind == WAN_COMPOSE_U8 || kind == WAN_COMPOSE_F32 || kind == WAN_COMPOSE_BF16, WAN_ERR_INVALID,
                "wan_video_range_flag: kind=%d (0 uint8, 1 fp32, 2 bf16)", kind);
    WAN_REQUIRE(n > 0, WAN_ERR_INVALID, "wan_video_range_flag: n=%lld elements", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    WAN_REQUIRE(e == hipSuccess, WAN_ERR_LAUNCH, "wan_video_range_flag: hipMemsetAsync: %s", hipGetErrorString(e));
    if (kind == WAN_COMPOSE_U8) launch_range_flag<uint8_t>(x, n, flag, s);
    else if (kind == WAN_COMPOSE_F32) launch_range_flag<float>(x, n, flag, s);
    else launch_range_flag<bf16_t>(x, n, flag, s);
    WAN_CHECK_LAUNCH("wan_video_range_flag");
    return WAN_OK;
}

extern "C" wan_status_t wan_frames_u8_compose(const wan_compose_src* srcs, int n_src, void* canvas_u8, int T_out, int Hc, int Wc,
                                              int pad, void* stream) {
    WAN_REQUIRE(srcs && canvas_u8, WAN_ERR_INVALID, "wan_frames_u8_compose: null argument");
    WAN_REQUIRE(n_src >= 0 && n_src <= WAN_COMPOSE_MAX_SRC, n_src < 0 ? WAN_ERR_INVALID : WAN_ERR_UNSUPPORTED,
                "wan_frames_u8_compose: n_src=%d sources (at most %d per canvas)", n_src, WAN_COMPOSE_MAX_SRC);
    WAN_REQUIRE(T_out > 0 && Hc > 0 && Wc > 0, WAN_ERR_INVALID, "wan_frames_u8_compose: bad canvas T=%d H=%d W=%d", T_out, Hc, Wc);
    compose_args a;
    a.canvas = (uint8_t*)canvas_u8;
    a.n_src = n_src; a.Hc = Hc; a.Wc = Wc;
    WAN_REQUIRE(pad >= 0 && pad <= 255, WAN_ERR_INVALID, "wan_frames_u8_compose: pad=%d is no byte", pad);
    a.pad = (unsigned int)pad * 0x01010101u;
    WAN_REQUIRE(T_out <= 65535 && Wc <= (1 << 28), WAN_ERR_UNSUPPORTED, "wan_frames_u8_compose: canvas T=%d W=%d too large", T_out, Wc);
    a.ppr = (15 + Wc * 3 + 15) / 16;
    const int64_t items = (int64_t)Hc * a.ppr;
    WAN_REQUIRE(items < (1ll << 31), WAN_ERR_UNSUPPORTED, "wan_frames_u8_compose: canvas frame %d x %d too large", Hc, Wc);
    for (int k = 0; k < n_src; ++k) {
        wan_compose_src s = srcs[k];
        WAN_REQUIRE(s.base && s.extent > 0, WAN_ERR_INVALID, "wan_frames_u8_compose: source %d: null or empty tensor", k);
        const bool u8 = s.kind == WAN_COMPOSE_U8, fl = s.kind == WAN_COMPOSE_F32 || s.kind == WAN_COMPOSE_BF16;
        WAN_REQUIRE(u8 || fl, WAN_ERR_INVALID, "wan_frames_u8_compose: source %d: kind=%d (0 uint8, 1 fp32, 2 bf16)", k, s.kind);
        WAN_REQUIRE(u8 ? (s.mode == WAN_COMPOSE_COPY || s.mode == WAN_COMPOSE_LOADER_ROUNDTRIP)
                       : (s.mode == WAN_COMPOSE_WRITER || s.mode == WAN_COMPOSE_NORMALIZE),
                    WAN_ERR_INVALID, "wan_frames_u8_compose: source %d: mode=%d does not go with kind=%d", k, s.mode, s.kind);
        WAN_REQUIRE(s.mode != WAN_COMPOSE_NORMALIZE || s.rescale_flag, WAN_ERR_INVALID,
                    "wan_frames_u8_compose: source %d: NORMALIZE needs the flag of wan_video_range_flag", k);
        WAN_REQUIRE((s.mode != WAN_COMPOSE_WRITER && s.mode != WAN_COMPOSE_COPY) || !s.rescale_flag, WAN_ERR_INVALID,
                    "wan_frames_u8_compose: source %d: mode=%d takes no rescale flag", k, s.mode);
        if (s.mode == WAN_COMPOSE_LOADER_ROUNDTRIP && !s.rescale_flag) s.rescale = 1;       // the loader's video always has a byte < 128
        WAN_REQUIRE(s.stride_c >= 0 && s.stride_t >= 0 && s.stride_y >= 0 && s.stride_x >= 0, WAN_ERR_UNSUPPORTED,
                    "wan_frames_u8_compose: source %d: negative stride", k);
        WAN_REQUIRE(s.t0 >= 0 && s.y0 >= 0 && s.x0 >= 0 && s.nt > 0 && s.h > 0 && s.w > 0, WAN_ERR_INVALID,
                    "wan_frames_u8_compose: source %d: window (t0=%d y0=%d x0=%d nt=%d h=%d w=%d)", k, s.t0, s.y0, s.x0, s.nt, s.h, s.w);
        const __int128 last = (__int128)2 * s.stride_c + ((__int128)s.t0 + s.nt - 1) * s.stride_t +
                              ((__int128)s.y0 + s.h - 1) * s.stride_y + ((__int128)s.x0 + s.w - 1) * s.stride_x;
        WAN_REQUIRE(last < (__int128)s.extent, WAN_ERR_INVALID,
                    "wan_frames_u8_compose: source %d: window (t0=%d y0=%d x0=%d nt=%d h=%d w=%d) reads outside its %lld elements", k,
                    s.t0, s.y0, s.x0, s.nt, s.h, s.w, (long long)s.extent);
        WAN_REQUIRE(s.nt <= T_out && s.dst_y >= 0 && s.dst_x >= 0 && (int64_t)s.dst_y + s.h <= Hc && (int64_t)s.dst_x + s.w <= Wc,
                    WAN_ERR_INVALID, "wan_frames_u8_compose: source %d: %d frames of %d x %d at (%d, %d) leave the %d x %d x %d canvas", k,
                    s.nt, s.h, s.w, s.dst_y, s.dst_x, T_out, Hc, Wc);
        for (int j = 0; j < k; ++j) {
            const wan_compose_src& o = a.src[j];
            WAN_REQUIRE(s.dst_y >= o.dst_y + o.h || o.dst_y >= s.dst_y + s.h || s.dst_x >= o.dst_x + o.w || o.dst_x >= s.dst_x + s.w,
                        WAN_ERR_INVALID, "wan_frames_u8_compose: sources %d and %d overlap on the canvas", j, k);
        }
        a.src[k] = s;
    }
    for (int k = n_src; k < WAN_COMPOSE_MAX_SRC; ++k) a.src[k] = wan_compose_src{};
    const dim3 grid((unsigned)((items + 255) / 256), (unsigned)T_out);
    hipLaunchKernelGGL(frames_compose_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    WAN_CHECK_LAUNCH("wan_frames_u8_compose");
    return WAN_OK;
}

extern "C" wan_status_t wan_frames_u8_box_to_video(const void* frames_u8, void* out, int out_dtype, int B, int T, int H, int W, int by,
                                                   int bx, int bh, int bw, void* stream) {
    WAN_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0, WAN_ERR_INVALID, "wan_frames_u8_box_to_video: bad shape B=%d T=%d H=%d W=%d", B, T, H, W);
    WAN_REQUIRE(out_dtype == 0 || out_dtype == 1, WAN_ERR_INVALID, "wan_frames_u8_box_to_video: out_dtype=%d (0 fp32, 1 bf16)", out_dtype);
    WAN_REQUIRE(rect_inside(H, W, by, bx, bh, bw), WAN_ERR_INVALID,
                "wan_frames_u8_box_to_video: the box [%d, %d + %d) x [%d, %d + %d) does not lie inside a frame of %d x %d", by, by, bh, bx,
                bx, bw, H, W);
    // (the box first: an empty box's output is an empty tensor, whose address is null)
    WAN_REQUIRE(frames_u8 && out, WAN_ERR_INVALID, "wan_frames_u8_box_to_video: null tensor");
    const int64_t frames = (int64_t)B * T;
    WAN_REQUIRE(frames <= 0x7fffffff && (int64_t)H * W * 3 <= 0x7fffffff, WAN_ERR_INVALID,
                "wan_frames_u8_box_to_video: %lld frames of %lld bytes (each at most 2^31 - 1)", (long long)frames, (long long)H * W * 3);
    const int64_t es = out_dtype == 0 ? 4 : 2;
    const int N = box_unit_pixels(es, {W, bx, bw}, (uintptr_t)frames_u8, (uintptr_t)out);
    const int bwu = bw / N, cw = std::min(bwu, 256), rp = 256 / cw;
    const dim3 grid((unsigned)frames, box_row_chunks(bh, rp, frames));
    hipStream_t s = (hipStream_t)stream;
#define WAN_BOX_IN(N_)                                                                                                          \
    do {                                                                                                                        \
        if (out_dtype == 0)                                                                                                     \
            hipLaunchKernelGGL((frames_box_to_video_kernel<float, N_>), grid, dim3(256), 0, s, (const uint8_t*)frames_u8,       \
                               (float*)out, T, H, W, by, bx, bh, bwu, cw, rp);                                                  \
        else                                                                                                                    \
            hipLaunchKernelGGL((frames_box_to_video_kernel<bf16_t, N_>), grid, dim3(256), 0, s, (const uint8_t*)frames_u8,      \
                               (bf16_t*)out, T, H, W, by, bx, bh, bwu, cw, rp);                                                 \
    } while (0)
    WAN_BY_PIXELS(N, WAN_BOX_IN);
#undef WAN_BOX_IN
    WAN_CHECK_LAUNCH("wan_frames_u8_box_to_video");
    return WAN_OK;
}

extern "C" wan_status_t wan_video_box_stitch_u8(const void* video, int in_dtype, const void* source_u8, void* frames_u8, int B, int Bs,
                                                int T, int Ts, int T_out, int H, int W, int by, int bx, int bh, int bw, int ry, int rx,
                                                int rh, int rw, int feather, int t0, int nt, int src_t0, int t_dst, void* stream) {
    const char* who = "wan_video_box_stitch_u8";
    WAN_REQUIRE(B > 0 && T > 0 && Ts > 0 && T_out > 0 && H > 0 && W > 0, WAN_ERR_INVALID,
                "%s: bad shape B=%d T=%d Ts=%d T_out=%d H=%d W=%d", who, B, T, Ts, T_out, H, W);
    WAN_REQUIRE(Bs == 1 || Bs == B, WAN_ERR_INVALID, "%s: Bs=%d source clips for B=%d samples (1 or B)", who, Bs, B);
    WAN_REQUIRE(in_dtype == 0 || in_dtype == 1, WAN_ERR_INVALID, "%s: in_dtype=%d (0 fp32, 1 bf16)", who, in_dtype);
    WAN_REQUIRE(rect_inside(H, W, by, bx, bh, bw), WAN_ERR_INVALID,
                "%s: the box [%d, %d + %d) x [%d, %d + %d) does not lie inside a frame of %d x %d", who, by, by, bh, bx, bx, bw, H, W);
    WAN_REQUIRE(rect_inside(bh, bw, ry - by, rx - bx, rh, rw), WAN_ERR_INVALID,
                "%s: the rectangle [%d, %d + %d) x [%d, %d + %d) does not lie inside the box [%d, %d + %d) x [%d, %d + %d)", who, ry, ry, rh,
                rx, rx, rw, by, by, bh, bx, bx, bw);
    WAN_REQUIRE(video && source_u8 && frames_u8, WAN_ERR_INVALID, "%s: null tensor", who);
    WAN_REQUIRE(feather >= 0, WAN_ERR_INVALID, "%s: feather=%d pixels (not negative)", who, feather);
    WAN_REQUIRE(t0 >= 0 && nt >= 0 && nt <= T - t0, WAN_ERR_INVALID, "%s: decoder frames [%d, %d + %d) of %d", who, t0, t0, nt, T);
    WAN_REQUIRE(src_t0 >= 0 && nt <= Ts - src_t0, WAN_ERR_INVALID, "%s: source frames [%d, %d + %d) of %d", who, src_t0, src_t0, nt, Ts);
    WAN_REQUIRE(t_dst >= 0 && nt <= T_out - t_dst, WAN_ERR_INVALID, "%s: %d frames at offset %d of a %d-frame clip", who, nt, t_dst, T_out);
    // (the ramp's 255 * (d + 1) stays below 2^32 with d < 2^24)
    WAN_REQUIRE((int64_t)B * nt <= 0x7fffffff && (int64_t)H * W * 3 <= 0x7fffffff && H <= (1 << 24) && W <= (1 << 24), WAN_ERR_INVALID,
                "%s: %lld frames of %d x %d pixels (frames and bytes a frame at most 2^31 - 1, a side at most 2^24)", who,
                (long long)B * nt, H, W);
    if (nt == 0) return WAN_OK;
    const int64_t es = in_dtype == 0 ? 4 : 2, frames = (int64_t)B * nt;
    const int N = box_unit_pixels(es, {W, bx, bw}, (uintptr_t)source_u8 | (uintptr_t)frames_u8, (uintptr_t)video);
    stitch_args a;
    a.video = video; a.source = (const uint8_t*)source_u8; a.frames = (uint8_t*)frames_u8;
    a.T = T; a.Ts = Ts; a.T_out = T_out; a.H = H; a.W = W; a.t0 = t0; a.nt = nt; a.src_t0 = src_t0; a.t_dst = t_dst;
    a.one_source = Bs == 1;
    a.by = by; a.bx = bx; a.bh = bh; a.bw = bw; a.ry = ry; a.rx = rx; a.rh = rh; a.rw = rw; a.feather = feather;
    a.top = ry > 0; a.bottom = ry + rh < H; a.left = rx > 0; a.right = rx + rw < W;
    a.wu = W / N; a.cw = std::min(a.wu, 256); a.rp = 256 / a.cw;
    const dim3 grid((unsigned)frames, box_row_chunks(H, a.rp, frames));
    hipStream_t s = (hipStream_t)stream;
#define WAN_BOX_OUT(N_)                                                                                          \
    do {                                                                                                         \
        if (in_dtype == 0) hipLaunchKernelGGL((video_box_stitch_kernel<float, N_>), grid, dim3(256), 0, s, a);   \
        else hipLaunchKernelGGL((video_box_stitch_kernel<bf16_t, N_>), grid, dim3(256), 0, s, a);                \
    } while (0)
    WAN_BY_PIXELS(N, WAN_BOX_OUT);
#undef WAN_BOX_OUT
    WAN_CHECK_LAUNCH(who);
    return WAN_OK;
}
