// Colour match: one gain and offset per frame and channel that bring the edit's colours back to the source's, estimated from the pixels
// the edit left alone (alpha == 0) and applied to the whole frame.  The definition is include/wan_hip.h (wan_color_stats, wan_color_coef,
// wan_frames_u8_affine); videocof_amd/video_io.py restates it in Python ints (reference_color_stats, reference_color_coefficients,
// reference_frames_affine) and the kernels equal that word for word.  Integers only: no floating point in this file.
//
//   color_sums_kernel    n and, per channel, the sums of ref, edit, ref^2 and edit^2 over the counted pixels of a frame.  As in
//                        frame_stats.hip the frame is a flat run of pixels and a thread owns 16 of them: 48 bytes of each clip and 16
//                        of alpha, each one run at an address of any alignment (byte_runs.hpp).  The bytes are never taken apart: a
//                        dword of a clip is ANDed with the dword of its pixels' "alpha is 0" bytes and with a channel's byte pattern,
//                        and v_dot4_u32_u8 adds its four bytes (against 0x01010101) and their squares (against itself)
//   color_reduce_kernel  stats[n] = the sum over the frame's workgroups' slots, words 13 .. 15 zero
//   color_coef_kernel    a thread per (frame, channel): the pooled sums, the variances in 128 bits, one 64-bit division, one integer
//                        square root, one more division for the offset
//   affine_kernel        out = clamp((g x + b + 2048) >> 12, 0, 255) on 48 bytes per thread: a run starts on channel 0 because 48 and
//                        a frame's bytes are multiples of 3, so the (g, b) of byte i of a run is that of channel i mod 3, known at
//                        compile time; v_mad_i32_i24, a shift and v_med3 per byte.  The other form, a 256-entry table per (frame,
//                        channel) in LDS, is tools/color_affine_lut.hip, measured by tools/bench_color_match.py
//
// No atomics: a workgroup writes what it summed ONCE, as plain stores into a slot of its own, and the reduce adds a frame's slots.
#include <algorithm>

#include "byte_runs.hpp"
#include "common.hpp"

namespace {

constexpr int WORDS = WAN_COLOR_STATS_WORDS, SUMS = 13;     // n, then (A, E, AA, EE) per channel
constexpr int MAX_GROUPS = 64, TARGET_WORKGROUPS = 2048;
constexpr int PIX = 16, TILE_PIX = 256 * PIX;

// workgroups per frame: enough to fill the device with few frames (8 per CU of 256), never more than the frame has tiles
int groups_of(int N, int H, int W) {
    const int64_t tiles = ((int64_t)H * W + TILE_PIX - 1) / TILE_PIX;
    return (int)std::min<int64_t>(std::min(std::max(TARGET_WORKGROUPS / N, 1), MAX_GROUPS), tiles);
}

struct sums_args {
    const uint8_t *ref, *edit, *alpha;       // [B, ref_T, H, W, 3], [B, T, H, W, 3], [B, ref_T, H, W] or null
    long long* slots;                        // [N, G, WORDS]
    int64_t ref_bytes, edit_bytes, alpha_bytes;
    int64_t P;                               // H * W
    int T, ref_T;
};

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the byte pattern of channel c in dword w of three (12 bytes = 4 pixels)
__device__ __forceinline__ constexpr unsigned int channel_mask(int w, int c) {
    unsigned int m = 0u;
    for (int b = 0; b < 4; ++b)
        if ((4 * w + b) % 3 == c) m |= 0xffu << (8 * b);
    return m;
}

__global__ __launch_bounds__(256) void color_sums_kernel(const sums_args a) {
    __shared__ long long red[4][SUMS];
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.y, P = a.P;
    const int64_t rn = a.ref_T == 1 ? n / a.T : n;                  // the ref frame (and alpha frame) paired with frame n
    unsigned int cnt = 0u, s1[2][3] = {};                           // n; A, E: below 2^32 for a frame below 2 GiB
    unsigned long long s2[2][3] = {};                               // AA, EE
    const int64_t tiles = (P + TILE_PIX - 1) / TILE_PIX;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t p0 = tile * TILE_PIX + (int64_t)tid * PIX;
        if (p0 >= P) continue;
        const int valid = (int)min((int64_t)PIX, P - p0);          // behind the frame's end: the next frame's bytes, not counted
        unsigned int wr[12], we[12], al[4] = {0u, 0u, 0u, 0u};
        load_bytes<12>(a.ref, a.ref_bytes, (rn * P + p0) * 3, wr);
        load_bytes<12>(a.edit, a.edit_bytes, (n * P + p0) * 3, we);
        if (a.alpha) load_bytes<4>(a.alpha, a.alpha_bytes, rn * P + p0, al);
        if (valid < PIX) {
#pragma unroll
            for (int j = 0; j < PIX; ++j)
                if (j >= valid) al[j >> 2] |= 0xffu << ((j & 3) * 8);
        }
        unsigned int q[2][3] = {};                                  // this tile's sums of squares: 16 * 255^2 each at the most
#pragma unroll
        for (int g = 0; g < 4; ++g) {                               // 4 pixels: one dword of alpha, three of each clip
            const unsigned int v = al[g];
            const unsigned int z = ((((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u) ^ 0x80808080u;     // 0x80 in the bytes that are 0
            const unsigned int k = z | (z - (z >> 7));                                                        // 0xff there
            cnt += (unsigned int)__builtin_popcount(z);
            const unsigned int km[3] = {__builtin_amdgcn_perm(k, k, 0x01000000u), __builtin_amdgcn_perm(k, k, 0x02020101u),
                                        __builtin_amdgcn_perm(k, k, 0x03030302u)};      // pixel bytes 0 0 0 1 | 1 1 2 2 | 2 3 3 3
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const unsigned int x[2] = {wr[3 * g + w] & km[w], we[3 * g + w] & km[w]};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const unsigned int y = x[s] & channel_mask(w, c);
                        s1[s][c] = __builtin_amdgcn_udot4(y, 0x01010101u, s1[s][c], false);
                        q[s][c] = __builtin_amdgcn_udot4(y, y, q[s][c], false);
                    }
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int c = 0; c < 3; ++c) s2[s][c] += q[s][c];
    }
    long long mine[SUMS];
    mine[0] = (long long)cnt;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mine[1 + 4 * c] = (long long)s1[0][c];
        mine[2 + 4 * c] = (long long)s1[1][c];
        mine[3 + 4 * c] = (long long)s2[0][c];
        mine[4 + 4 * c] = (long long)s2[1][c];
    }
#pragma unroll
    for (int k = 0; k < SUMS; ++k) {
        const long long v = wave_sum_i64(mine[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < WORDS)
        a.slots[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * WORDS + tid] =
            tid < SUMS ? red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid] : 0ll;
}

// a thread per word of stats: 16 frames per workgroup
__global__ __launch_bounds__(256) void color_reduce_kernel(const long long* slots, long long* stats, int N, int G) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * WORDS) return;
    const int64_t n = i / WORDS;
    const int w = (int)(i - n * WORDS);
    long long v = 0;
    if (w < SUMS)
        for (int g = 0; g < G; ++g) v += slots[(n * G + g) * WORDS + w];
    stats[i] = v;
}

// ---- the coefficients
typedef unsigned __int128 u128;

__device__ __forceinline__ int bit_length(u128 v) {
    const unsigned long long hi = (unsigned long long)(v >> 64), lo = (unsigned long long)v;
    return hi ? 128 - __builtin_clzll(hi) : lo ? 64 - __builtin_clzll(lo) : 0;
}

// floor(sqrt(v)): a bit of the root per turn, from the top
__device__ __forceinline__ unsigned long long isqrt64(unsigned long long v) {
    unsigned long long root = 0, bit = 1ull << 62;
    while (bit > v) bit >>= 2;
    while (bit) {
        if (v >= root + bit) {
            v -= root + bit;
            root = (root >> 1) + bit;
        } else {
            root >>= 1;
        }
        bit >>= 2;
    }
    return root;
}

__device__ __forceinline__ long long floor_div(long long a, long long d) {          // d > 0
    const long long q = a / d;
    return q - ((a % d) < 0 ? 1 : 0);
}

__global__ __launch_bounds__(64) void color_coef_kernel(const long long* stats, int* coef, int N, int T, int pool_t, int gain,
                                                        int min_pixels) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= N * 3) return;
    const int f = i / 3, c = i - 3 * f;
    const int t = f % T, f0 = f - t;                                // f0: the sample's first frame
    long long n = 0, A = 0, E = 0, AA = 0, EE = 0;
    for (int u = max(t - pool_t, 0); u <= min(t + pool_t, T - 1); ++u) {
        const long long* s = stats + (int64_t)(f0 + u) * WORDS;
        n += s[0]; A += s[1 + 4 * c]; E += s[2 + 4 * c]; AA += s[3 + 4 * c]; EE += s[4 + 4 * c];
    }
    constexpr long long ONE = WAN_COLOR_ONE;
    long long g = ONE, b = 0;
    if (n >= max(1, min_pixels)) {
        if (gain) {
            const u128 Vs = (u128)(unsigned long long)n * (unsigned long long)AA - (u128)(unsigned long long)A * (unsigned long long)A;
            const u128 Ve = (u128)(unsigned long long)n * (unsigned long long)EE - (u128)(unsigned long long)E * (unsigned long long)E;
            if (Ve != 0) {
                const int k = max(0, bit_length(Vs > Ve ? Vs : Ve) - 38);
                const unsigned long long vs = (unsigned long long)(Vs >> k), ve = (unsigned long long)(Ve >> k);      // below 2^38
                g = ve == 0 ? 2 * ONE : (long long)isqrt64((vs << 24) / ve);
                g = min(max(g, ONE / 2), 2 * ONE);
            }
        }
        b = floor_div(ONE * A - g * E + (n >> 1), n);
    }
    coef[2 * i] = (int)g;
    coef[2 * i + 1] = (int)b;
}

// ---- the transform
constexpr int RUN = 48, TILE_BYTES = 256 * RUN;

__global__ __launch_bounds__(256) void affine_kernel(const uint8_t* frames, const int* coef, uint8_t* out, int64_t frame_bytes,
                                                     int64_t total_bytes) {            // out may be frames: nothing is __restrict__
    const int64_t n = blockIdx.y;
    const int64_t o = ((int64_t)blockIdx.x * 256 + threadIdx.x) * RUN;
    if (o >= frame_bytes) return;
    const int* k = coef + n * 6;
    const int g[3] = {k[0], k[2], k[4]}, b[3] = {k[1] + WAN_COLOR_ONE / 2, k[3] + WAN_COLOR_ONE / 2, k[5] + WAN_COLOR_ONE / 2};
    unsigned int w[RUN / 4], r[RUN / 4];
    load_bytes<RUN / 4>(frames, total_bytes, n * frame_bytes + o, w);
#pragma unroll
    for (int q = 0; q < RUN / 4; ++q) {
        unsigned int v = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = (4 * q + j) % 3;
            // clamped BEFORE the shift, to [0, 256 * ONE): the same byte as clamp(y >> 12, 0, 255), the shift being monotone
            const int y = __mul24(g[c], (int)((w[q] >> (8 * j)) & 0xffu)) + b[c];
            v |= ((unsigned int)min(max(y, 0), 256 * WAN_COLOR_ONE - 1) >> 12) << (8 * j);
        }
        r[q] = v;
    }
    store_span<RUN / 4>(out + n * frame_bytes + o, r, (int)min((int64_t)RUN, frame_bytes - o));
}

}  // namespace

extern "C" int64_t wan_color_stats_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return ((int64_t)N * groups_of(N, H, W) * WORDS * 8 + 255) / 256 * 256;
}

extern "C" wan_status_t wan_color_stats(const void* ref_u8, const void* edit_u8, const void* alpha_u8, void* stats_i64, int B, int T,
                                        int ref_T, int H, int W, void* workspace, int64_t workspace_bytes, void* stream) {
    WAN_REQUIRE(ref_u8 && edit_u8 && stats_i64, WAN_ERR_INVALID, "wan_color_stats: null tensor");
    WAN_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0, WAN_ERR_INVALID, "wan_color_stats: bad shape B=%d T=%d H=%d W=%d", B, T, H, W);
    WAN_REQUIRE(ref_T == T || ref_T == 1, WAN_ERR_INVALID, "wan_color_stats: ref_T=%d (T=%d, or 1 frame per sample)", ref_T, T);
    WAN_REQUIRE((int64_t)B * T <= 65535 && (int64_t)H * W * 3 < (1ll << 31), WAN_ERR_UNSUPPORTED,
                "wan_color_stats: %d x %d frames of %d x %d (at most 65535 frames per call, a frame below 2 GiB)", B, T, H, W);
    const int N = B * T;
    WAN_REQUIRE(workspace && workspace_bytes >= wan_color_stats_workspace_bytes(N, H, W), WAN_ERR_INVALID,
                "wan_color_stats: workspace of %lld bytes, needs %lld", (long long)(workspace ? workspace_bytes : 0),
                (long long)wan_color_stats_workspace_bytes(N, H, W));
    const int G = groups_of(N, H, W);
    sums_args a;
    a.ref = (const uint8_t*)ref_u8; a.edit = (const uint8_t*)edit_u8; a.alpha = (const uint8_t*)alpha_u8;
    a.slots = (long long*)workspace;
    a.P = (int64_t)H * W;
    a.alpha_bytes = (int64_t)B * ref_T * a.P;
    a.ref_bytes = a.alpha_bytes * 3;
    a.edit_bytes = (int64_t)N * a.P * 3;
    a.T = T; a.ref_T = ref_T;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(color_sums_kernel, dim3((unsigned)G, (unsigned)N), dim3(256), 0, s, a);
    WAN_CHECK_LAUNCH("wan_color_stats (sums)");
    hipLaunchKernelGGL(color_reduce_kernel, dim3((unsigned)((N * WORDS + 255) / 256)), dim3(256), 0, s, (const long long*)workspace,
                       (long long*)stats_i64, N, G);
    WAN_CHECK_LAUNCH("wan_color_stats (reduce)");
    return WAN_OK;
}

extern "C" wan_status_t wan_color_coef(const void* stats_i64, void* coef_i32, int B, int T, int pool_t, int gain, int min_pixels,
                                       void* stream) {
    WAN_REQUIRE(stats_i64 && coef_i32, WAN_ERR_INVALID, "wan_color_coef: null tensor");
    WAN_REQUIRE(B > 0 && T > 0 && (int64_t)B * T <= (1 << 24), WAN_ERR_INVALID, "wan_color_coef: bad shape B=%d T=%d", B, T);
    WAN_REQUIRE(pool_t >= 0 && pool_t <= WAN_COLOR_MAX_POOL_T, WAN_ERR_INVALID, "wan_color_coef: pool_t=%d (0..%d)", pool_t,
                WAN_COLOR_MAX_POOL_T);
    WAN_REQUIRE(min_pixels >= 0, WAN_ERR_INVALID, "wan_color_coef: min_pixels=%d", min_pixels);
    const int N = B * T;
    hipLaunchKernelGGL(color_coef_kernel, dim3((unsigned)((N * 3 + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       (const long long*)stats_i64, (int*)coef_i32, N, T, pool_t, gain, min_pixels);
    WAN_CHECK_LAUNCH("wan_color_coef");
    return WAN_OK;
}

extern "C" wan_status_t wan_frames_u8_affine(const void* frames_u8, const void* coef_i32, void* out_u8, int N, int H, int W,
                                             void* stream) {
    WAN_REQUIRE(frames_u8 && coef_i32 && out_u8, WAN_ERR_INVALID, "wan_frames_u8_affine: null tensor");
    WAN_REQUIRE(N > 0 && H > 0 && W > 0, WAN_ERR_INVALID, "wan_frames_u8_affine: bad shape N=%d H=%d W=%d", N, H, W);
    WAN_REQUIRE(N <= 65535 && (int64_t)H * W * 3 < (1ll << 31), WAN_ERR_UNSUPPORTED,
                "wan_frames_u8_affine: N=%d frames of %d x %d (at most 65535 frames per call, a frame below 2 GiB)", N, H, W);
    const int64_t frame_bytes = (int64_t)H * W * 3;
    hipLaunchKernelGGL(affine_kernel, dim3((unsigned)((frame_bytes + TILE_BYTES - 1) / TILE_BYTES), (unsigned)N), dim3(256), 0,
                       (hipStream_t)stream, (const uint8_t*)frames_u8, (const int*)coef_i32, (uint8_t*)out_u8, frame_bytes,
                       (int64_t)N * frame_bytes);
    WAN_CHECK_LAUNCH("wan_frames_u8_affine");
    return WAN_OK;
}
