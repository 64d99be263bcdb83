// Clip statistics: how far is clip A from clip B, in exact integers per frame, split by a mask into "where alpha is 0" (region 0) and
// "where it is not" (region 1).  The definition is include/wan_hip.h (wan_clip_stats); videocof_amd/video_io.py restates it in numpy
// (reference_clip_stats) and the kernels equal that word for word.  Integer adds only, but for the one IEEE double division per SSIM
// window, whose rounded result is an integer again.
//
//   diff_hist_kernel     the histogram of |a - b| over the bytes of a frame.  The frame is a flat run of pixels: a thread owns 16 of
//                        them, 48 bytes of a and of b and 16 of alpha, each one run at an address of any alignment (byte_runs.hpp)
//   smooth_hist_kernel   d = max_c |a - b| summed over the (2 smooth + 1)^2 window with clamped indices, s = (2 S + n) / (2 n), the
//                        histogram of s: the tile, the border and the two passes of frame_keep.hip's box_sum_kernel<DIFF>
//   ssim_kernel          the x264 / ffmpeg 8-bit SSIM of each colour plane: sums per 4 x 4 block, windows of 2 x 2 blocks.  A thread
//                        owns one block (4 rows of 12 bytes of a and of b), a workgroup 8 x 32 blocks and the 7 x 31 windows inside them
//   reduce_kernel        the workgroups' partial words of a frame summed into stats, every word of it written
//
// Counting.  Two nearly identical clips put almost every value into the bins 0 .. 3, and an LDS atomic that 64 lanes aim at one
// address runs them one after the other.  So a thread counts the bins 0 .. 3 of both regions in registers (bin_counter: two words of
// four 8-bit fields, emptied into 32-bit counters before a field can overflow) and only the values from 4 up go to LDS atomics, on
// a histogram that the wave has to itself.  A workgroup walks over several tiles of its frame and writes what it counted ONCE, as
// plain stores into a slot of its own in the workspace; reduce_kernel adds a frame's slots.  No atomic touches global memory, no
// word is accumulated into across calls, and the result cannot depend on the order anything ran in.
#include <algorithm>

#include "byte_runs.hpp"
#include "common.hpp"

namespace {

constexpr int BINS = 256, HIST_WORDS = 2 * 2 * BINS;        // a slot: [diff | smooth][region][bin] uint32, then 4 int64 of SSIM
constexpr int SSIM_WORDS = 4;                               // [region][sum, windows]
constexpr int MAX_GROUPS = 64, TARGET_WORKGROUPS = 1536;

// workgroups per frame: enough of them to fill the device with few frames, few enough that the slots stay small beside the clips and
// that all are resident at once (6 per CU of 256: the kernels hold 60 .. 70 registers, 7 waves per SIMD) -- they do equal work, so a
// few left over for a second round would double the time
int groups_of(int N) { return std::min(std::max(TARGET_WORKGROUPS / N, 1), MAX_GROUPS); }

struct stats_args {
    const uint8_t *a, *b, *alpha;            // [N, H, W, 3] twice, [N, H, W] or null
    unsigned int* hist;                      // [N, G, HIST_WORDS]
    long long* ssim;                         // [N, G, SSIM_WORDS]
    int64_t frame_bytes, alpha_bytes;        // of the whole tensors
    int H, W, R;                             // R = smooth
};

// the bins 0 .. 3 of both regions in registers, everything else in the wave's LDS histogram [region][bin]
struct bin_counter {
    unsigned int pk[2] = {0u, 0u};
    unsigned int lo[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};

    __device__ __forceinline__ void add(unsigned int v, bool region, unsigned int* wave_hist) {
        if (v < 4u) {
            const unsigned int inc = 1u << (v * 8u);
            pk[0] += region ? 0u : inc;
            pk[1] += region ? inc : 0u;
        } else {
            atomicAdd(wave_hist + (region ? BINS : 0) + v, 1u);
        }
    }
    // after at most 255 add()s
    __device__ __forceinline__ void unpack() {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int k = 0; k < 4; ++k) lo[r][k] += (pk[r] >> (k * 8)) & 0xffu;
            pk[r] = 0u;
        }
    }
};

// wave_hist: [4 waves][2][BINS].  The registers join the waves' histograms, the four are added and the slot is written.
__device__ __forceinline__ void flush_hist(bin_counter& cnt, unsigned int* hist, unsigned int* slot) {
    const int tid = threadIdx.x;
    unsigned int* mine = hist + (tid >> 6) * 2 * BINS;
    cnt.unpack();
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (cnt.lo[r][k]) atomicAdd(mine + r * BINS + k, cnt.lo[r][k]);
    __syncthreads();
    for (int i = tid; i < 2 * BINS; i += 256) slot[i] = hist[i] + hist[2 * BINS + i] + hist[4 * BINS + i] + hist[6 * BINS + i];
}

// ---- the byte histogram
constexpr int PIX = 16, TILE_PIX = 256 * PIX;

__global__ __launch_bounds__(256) void diff_hist_kernel(const stats_args a) {
    __shared__ unsigned int hist[4 * 2 * BINS];
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.y, P = (int64_t)a.H * a.W;
    for (int i = tid; i < 4 * 2 * BINS; i += 256) hist[i] = 0u;
    __syncthreads();
    unsigned int* mine = hist + (tid >> 6) * 2 * BINS;
    bin_counter cnt;
    const int64_t tiles = (P + TILE_PIX - 1) / TILE_PIX;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t p0 = tile * TILE_PIX + (int64_t)tid * PIX;
        if (p0 >= P) continue;
        const int valid = (int)min((int64_t)PIX, P - p0);          // behind the frame's end: the next frame's bytes, not counted
        unsigned int wa[12], wb[12], al[4] = {0u, 0u, 0u, 0u};
        load_bytes<12>(a.a, a.frame_bytes, (n * P + p0) * 3, wa);
        load_bytes<12>(a.b, a.frame_bytes, (n * P + p0) * 3, wb);
        if (a.alpha) load_bytes<4>(a.alpha, a.alpha_bytes, n * P + p0, al);
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            if (j < valid) {
                const bool region = byte_of(al, j) != 0u;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int d = (int)byte_of(wa, 3 * j + c) - (int)byte_of(wb, 3 * j + c);
                    cnt.add((unsigned int)abs(d), region, mine);
                }
            }
        }
        cnt.unpack();                                              // 48 add()s
    }
    flush_hist(cnt, hist, a.hist + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * HIST_WORDS);
}

// ---- the smoothed histogram: box_sum_kernel<DIFF> of frame_keep.hip with the smaller border of WAN_MASK_MAX_SMOOTH, the value kept
// instead of compared with a threshold
constexpr int TR = 32, TC = 64;
constexpr int MAX_R = WAN_MASK_MAX_SMOOTH;
constexpr int LDS_ROWS = TR + 2 * MAX_R, LDS_COLS = TC + 2 * MAX_R;

__global__ __launch_bounds__(256) void smooth_hist_kernel(const stats_args a) {
    __shared__ unsigned int hist[4 * 2 * BINS];
    __shared__ uint8_t in[LDS_ROWS * LDS_COLS];
    __shared__ unsigned short hs[LDS_ROWS * TC];
    const int tid = threadIdx.x, R = a.R;
    const int64_t n = blockIdx.y;
    const int rows = TR + 2 * R, cols = TC + 2 * R;                 // <= LDS_ROWS, LDS_COLS: the host checks smooth <= MAX_R
    const unsigned int w = 2u * (unsigned int)R + 1u, area = w * w;
    // floor(u / d), d = 2 area <= 450, for u = 2 S + area < 2^17, as a multiply: m = ceil(2^32 / d), so m d = 2^32 + e with 0 <= e < d
    // and u m / 2^32 = u / d + (u / 2^32) (e / d).  The excess is below 2^-15 < 1 / d, too small to reach the next integer.
    // tests/test_gpu_clip_stats.py runs smooth 0, 1, 2 and 7 against the definition's division.
    const unsigned int magic = (unsigned int)(((1ull << 32) + 2u * area - 1u) / (2u * area));
    for (int i = tid; i < 4 * 2 * BINS; i += 256) hist[i] = 0u;
    unsigned int* mine = hist + (tid >> 6) * 2 * BINS;
    bin_counter cnt;
    const int tiles_x = (a.W + TC - 1) / TC, tiles = tiles_x * ((a.H + TR - 1) / TR);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int r0 = tile / tiles_x * TR, c0 = tile % tiles_x * TC;
        // the regions of this thread's VR pixels, asked for first: the loads are under way while the tile is summed
        constexpr int VR = TR / (256 / TC);
        const int c = tid & (TC - 1), rb = (tid / TC) * VR;
        unsigned int al[VR];
#pragma unroll
        for (int q = 0; q < VR; ++q)
            al[q] = (a.alpha && c0 + c < a.W && r0 + rb + q < a.H) ? a.alpha[(n * a.H + r0 + rb + q) * a.W + c0 + c] : 0u;
        __syncthreads();                                            // the tile before this one is done with in / hs; hist is zero
        // d of the tile and its border: 4 neighbouring pixels of a row per thread, 12 bytes of each clip as one run where no column
        // is clamped, else pixel by pixel
        const int runs = (cols + 3) / 4;
        for (int i = tid; i < rows * runs; i += 256) {
            const int r = i / runs, k = (i - r * runs) * 4;
            const int m = min(4, cols - k), x = c0 - R + k;
            const int64_t row = (n * a.H + min(max(r0 - R + r, 0), a.H - 1)) * a.W;
            uint8_t* dst = in + r * cols + k;
            if (x >= 0 && x + 3 < a.W) {
                unsigned int wa[3], wb[3];
                load_bytes<3>(a.a, a.frame_bytes, (row + x) * 3, wa);
                load_bytes<3>(a.b, a.frame_bytes, (row + x) * 3, wb);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int d = 0;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) d = max(d, abs((int)byte_of(wa, 3 * j + ch) - (int)byte_of(wb, 3 * j + ch)));
                    if (j < m) dst[j] = (uint8_t)d;
                }
            } else {
                for (int j = 0; j < m; ++j) {
                    const int64_t p = (row + min(max(x + j, 0), a.W - 1)) * 3;
                    int d = 0;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) d = max(d, abs((int)a.a[p + ch] - (int)a.b[p + ch]));
                    dst[j] = (uint8_t)d;
                }
            }
        }
        __syncthreads();
        // rows: a thread sums the windows of 4 neighbouring columns, each from the one before it
        for (int i = tid; i < rows * (TC / 4); i += 256) {
            const int r = i / (TC / 4), c = (i & (TC / 4 - 1)) * 4;
            const uint8_t* p = in + r * cols + c;
            unsigned int s = 0u;
            for (int j = 0; j <= 2 * R; ++j) s += p[j];             // <= 15 * 255
            unsigned short* h = hs + r * TC + c;
            h[0] = (unsigned short)s;
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                s += (unsigned int)p[2 * R + q] - (unsigned int)p[q - 1];
                h[q] = (unsigned short)s;
            }
        }
        __syncthreads();
        // columns: a thread owns VR rows of one column and slides its window down them
        if (c0 + c < a.W) {
            unsigned int s = 0u;
            for (int j = 0; j <= 2 * R; ++j) s += hs[(rb + j) * TC + c];
#pragma unroll
            for (int q = 0; q < VR; ++q) {
                if (r0 + rb + q >= a.H) break;
                if (q) s += (unsigned int)hs[(rb + q + 2 * R) * TC + c] - (unsigned int)hs[(rb + q - 1) * TC + c];
                cnt.add(__umulhi(2u * s + area, magic), al[q] != 0u, mine);             // (2 S + n) / (2 n) <= 255
            }
        }
        cnt.unpack();                                               // VR add()s
    }
    __syncthreads();
    flush_hist(cnt, hist, a.hist + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * HIST_WORDS + 2 * BINS);
}

// ---- SSIM
constexpr int SB_Y = 8, SB_X = 32;                                  // blocks of a workgroup; it owns the (SB_Y - 1) x (SB_X - 1) windows
constexpr int SSIM_C1 = 416, SSIM_C2 = 235963;                      // (.01 * 255)^2 * 64 + .5 and (.03 * 255)^2 * 64 * 63 + .5, truncated

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void ssim_kernel(const stats_args a) {
    __shared__ unsigned int blk[3][4][SB_Y * SB_X];                 // [plane][sum of a, of b, of a^2 + b^2, of a b][block]
    __shared__ unsigned int masked[SB_Y * SB_X];
    __shared__ long long red[4][SSIM_WORDS];
    const int tid = threadIdx.x, ty = tid / SB_X, tx = tid % SB_X;
    const int64_t n = blockIdx.y;
    const int h4 = a.H >> 2, w4 = a.W >> 2;
    const int tiles_x = w4 > 1 ? (w4 - 1 + SB_X - 2) / (SB_X - 1) : 0, tiles_y = h4 > 1 ? (h4 - 1 + SB_Y - 2) / (SB_Y - 1) : 0;
    const int tiles = tiles_x * tiles_y;
    long long acc[SSIM_WORDS] = {0, 0, 0, 0};
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int by = tile / tiles_x * (SB_Y - 1) + ty, bx = tile % tiles_x * (SB_X - 1) + tx;
        __syncthreads();                                            // the tile before this one is done with blk / masked
        if (by < h4 && bx < w4) {                                   // the block's 4 x 4 pixels lie inside the frame
            unsigned int s[3][4] = {};
            unsigned int any = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t p = (n * a.H + 4 * by + j) * a.W + 4 * bx;
                unsigned int wa[3], wb[3];
                load_bytes<3>(a.a, a.frame_bytes, p * 3, wa);
                load_bytes<3>(a.b, a.frame_bytes, p * 3, wb);
                if (a.alpha) {
                    unsigned int al[1];
                    load_bytes<1>(a.alpha, a.alpha_bytes, p, al);
                    any |= al[0];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const unsigned int x = byte_of(wa, 3 * i + c), y = byte_of(wb, 3 * i + c);
                        s[c][0] += x;
                        s[c][1] += y;
                        s[c][2] += __umul24(x, x) + __umul24(y, y);
                        s[c][3] += __umul24(x, y);
                    }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) blk[c][k][tid] = s[c][k];
            masked[tid] = any;
        }
        __syncthreads();
        if (ty < SB_Y - 1 && tx < SB_X - 1 && by + 1 < h4 && bx + 1 < w4) {
            const int i00 = tid, i01 = tid + 1, i10 = tid + SB_X, i11 = tid + SB_X + 1;
            const int region = (masked[i00] | masked[i01] | masked[i10] | masked[i11]) != 0u ? 1 : 0;
            long long q = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // <= 64 * 255 and <= 64 * 2 * 255^2: every product below stays under 2^31
                const int s1 = (int)(blk[c][0][i00] + blk[c][0][i01] + blk[c][0][i10] + blk[c][0][i11]);
                const int s2 = (int)(blk[c][1][i00] + blk[c][1][i01] + blk[c][1][i10] + blk[c][1][i11]);
                const int ss = (int)(blk[c][2][i00] + blk[c][2][i01] + blk[c][2][i10] + blk[c][2][i11]);
                const int s12 = (int)(blk[c][3][i00] + blk[c][3][i01] + blk[c][3][i10] + blk[c][3][i11]);
                const int vars = 64 * ss - s1 * s1 - s2 * s2, covar = 64 * s12 - s1 * s2;
                const double num = (double)(2 * s1 * s2 + SSIM_C1) * (double)(2 * covar + SSIM_C2);
                const double den = (double)(s1 * s1 + s2 * s2 + SSIM_C1) * (double)(vars + SSIM_C2);
                q += (long long)__builtin_rint(num / den * 1048576.0);
            }
            acc[2 * region] += q;
            acc[2 * region + 1] += 3;
        }
    }
#pragma unroll
    for (int k = 0; k < SSIM_WORDS; ++k) {
        const long long v = wave_sum_i64(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < SSIM_WORDS)
        a.ssim[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * SSIM_WORDS + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// ---- stats[n][region][word] = the sum over the frame's G slots.  A workgroup owns 64 words of a frame: four waves take every fourth slot
// each, so that no thread walks all G of them one load behind the other.
__global__ __launch_bounds__(256) void reduce_kernel(const unsigned int* hist, const long long* ssim, long long* stats, int G) {
    __shared__ long long part[4][64];
    const int64_t n = blockIdx.y;
    const int i = blockIdx.x * 64 + (threadIdx.x & 63), lane_g = threadIdx.x >> 6;
    long long v = 0;
    if (i < 2 * WAN_CLIP_STATS_WORDS) {
        const int r = i / WAN_CLIP_STATS_WORDS, k = i - r * WAN_CLIP_STATS_WORDS;
        if (k < 2 * BINS) {
            const unsigned int* p = hist + n * G * HIST_WORDS + (k / BINS) * 2 * BINS + r * BINS + (k & (BINS - 1));
            for (int g = lane_g; g < G; g += 4) v += p[(int64_t)g * HIST_WORDS];
        } else {
            const long long* p = ssim + n * G * SSIM_WORDS + 2 * r + (k - 2 * BINS);
            for (int g = lane_g; g < G; g += 4) v += p[g * SSIM_WORDS];
        }
    }
    part[lane_g][threadIdx.x & 63] = v;
    __syncthreads();
    if (lane_g == 0 && i < 2 * WAN_CLIP_STATS_WORDS)
        stats[n * 2 * WAN_CLIP_STATS_WORDS + i] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

}  // namespace

extern "C" int64_t wan_clip_stats_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    const int64_t slots = (int64_t)N * groups_of(N);
    return (slots * (HIST_WORDS * 4 + SSIM_WORDS * 8) + 255) / 256 * 256;
}

extern "C" wan_status_t wan_clip_stats(const void* a_u8, const void* b_u8, const void* alpha_u8, void* stats_i64, int N, int H, int W,
                                       int smooth, void* workspace, int64_t workspace_bytes, void* stream) {
    WAN_REQUIRE(a_u8 && b_u8 && stats_i64, WAN_ERR_INVALID, "wan_clip_stats: null tensor");
    WAN_REQUIRE(N > 0 && H > 0 && W > 0, WAN_ERR_INVALID, "wan_clip_stats: bad shape N=%d H=%d W=%d", N, H, W);
    WAN_REQUIRE(smooth >= 0 && smooth <= WAN_MASK_MAX_SMOOTH, WAN_ERR_INVALID, "wan_clip_stats: smooth=%d (0..%d)", smooth, WAN_MASK_MAX_SMOOTH);
    WAN_REQUIRE(N <= 65535 && (int64_t)H * W * 3 < (1ll << 31), WAN_ERR_UNSUPPORTED,
                "wan_clip_stats: N=%d frames of %d x %d (at most 65535 frames per call, a frame below 2 GiB)", N, H, W);
    WAN_REQUIRE(workspace && workspace_bytes >= wan_clip_stats_workspace_bytes(N, H, W), WAN_ERR_INVALID,
                "wan_clip_stats: workspace of %lld bytes, needs %lld", (long long)(workspace ? workspace_bytes : 0),
                (long long)wan_clip_stats_workspace_bytes(N, H, W));
    static_assert(WAN_CLIP_STATS_WORDS == 2 * BINS + 2, "a region's words: two histograms, the SSIM sum, its windows");
    const int G = groups_of(N);
    stats_args a;
    a.a = (const uint8_t*)a_u8; a.b = (const uint8_t*)b_u8; a.alpha = (const uint8_t*)alpha_u8;
    a.hist = (unsigned int*)workspace;
    a.ssim = (long long*)((uint8_t*)workspace + (int64_t)N * G * HIST_WORDS * 4);      // a multiple of 8 bytes behind an aligned base
    a.alpha_bytes = (int64_t)N * H * W;
    a.frame_bytes = a.alpha_bytes * 3;
    a.H = H; a.W = W; a.R = smooth;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)G, (unsigned)N);
    hipLaunchKernelGGL(diff_hist_kernel, grid, dim3(256), 0, s, a);
    WAN_CHECK_LAUNCH("wan_clip_stats (byte histogram)");
    hipLaunchKernelGGL(smooth_hist_kernel, grid, dim3(256), 0, s, a);
    WAN_CHECK_LAUNCH("wan_clip_stats (smoothed histogram)");
    hipLaunchKernelGGL(ssim_kernel, grid, dim3(256), 0, s, a);
    WAN_CHECK_LAUNCH("wan_clip_stats (SSIM)");
    hipLaunchKernelGGL(reduce_kernel, dim3((2 * WAN_CLIP_STATS_WORDS + 63) / 64, (unsigned)N), dim3(256), 0, s, a.hist, a.ssim,
                       (long long*)stats_i64, G);
    WAN_CHECK_LAUNCH("wan_clip_stats (reduce)");
    return WAN_OK;
}
