// uint8 video frames <-> the VAE's planar video, on both sides of an edit.
//   in : what a video reader yields, uint8 [B, T, H, W, 3]  ->  [B, 3, T, H, W] in the dtype AutoencoderKLWan.encode consumes
//   out: what AutoencoderKLWan.decode returns, [B, 3, T, H, W]  ->  uint8 [B, T, H, W, 3], what a video writer takes
// Pure streaming kernels.  A frame is one run of H*W pixels on both sides (3*H*W interleaved bytes, three planes of H*W elements),
// so the kernels index pixels of a frame, not rows.  Wide path: one thread per 16 pixels = 48 interleaved bytes = three 16-byte
// accesses; the 16 elements of each channel are two (bf16) or four (fp32) 16-byte accesses; whole pixels are regrouped in
// registers with compile-time byte positions.  It needs H*W % 16 == 0 and 16-byte aligned bases; everything else (odd byte rows,
// offset views) takes the element-wise kernels.
#include <algorithm>

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
