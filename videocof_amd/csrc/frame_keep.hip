// Keep what the edit left alone: the change mask of an edit against the frames the pipeline saw, and the composite of the edit over the
// original clip under that mask.  Integer arithmetic only, the definition of include/wan_hip.h (wan_change_mask, wan_plane_u8_resample,
// wan_frames_u8_composite); videocof_amd/video_io.py restates it in numpy (reference_change_mask, reference_composite_frames) and the
// kernels equal that byte for byte.  No floating point, no scratch.
//
//   box_sum_kernel<DIFF>     d = max_c |edit - source|, summed over the (2 smooth + 1)^2 window, indices clamped  -> b (0 / 1)
//   box_sum_kernel<GROW>     b ORed over the frames t - grow_t .. t + grow_t of the sample, summed over the (2 grow + 1)^2 window,
//                            nothing outside the frame                                                            -> g (0 / 1)
//   box_sum_kernel<FEATHER>  g summed over the (2 feather + 1)^2 window, indices clamped                          -> alpha
//   plane_rows_kernel, plane_columns_kernel   the two passes of the frame path's integer resample on one-channel planes (alpha to the
//                            source window's size)
//   composite_kernel         out = (a * e + (255 - a) * o + 127) / 255 inside the window, the original's bytes outside it
//
// The three steps of the mask are ONE kernel: a box sum in two passes of exact sums (a maximum of 0 / 1 values over a window is
// "their sum is not 0").  A workgroup owns TR x TC pixels of one frame; it loads them and a border of `radius` pixels into LDS as
// bytes (one pixel per thread and load, so a wave reads consecutive bytes and no alignment is assumed), sums rows into 16-bit
// words, then columns, each window from its neighbour's.  Every index is clamped or tested before the load, so nothing outside the
// planes is touched whatever the sizes; windows larger than the frame only repeat the border (clamped) or add nothing (GROW).
#include <algorithm>

#include "byte_runs.hpp"
#include "common.hpp"

namespace {

constexpr int TR = 32, TC = 64;             // pixels of a tile
constexpr int MAX_RADIUS = 32;              // WAN_MASK_MAX_GROW; smooth and feather are smaller
constexpr int LDS_ROWS = TR + 2 * MAX_RADIUS, LDS_COLS = TC + 2 * MAX_RADIUS;

enum { DIFF = 0, GROW = 1, FEATHER = 2 };

struct box_args {
    const uint8_t* src;      // DIFF: source frames [N, H, W, 3]; GROW / FEATHER: the plane [N, H, W]
    const uint8_t* edit;     // DIFF: edit frames
    uint8_t* dst;            // [N, H, W]
    int T, H, W;             // N = B * T frames; T is what GROW keeps its frames inside
    int radius, grow_t;
    unsigned int lim;        // DIFF: b = 2 S + n >= lim; FEATHER: alpha = (510 C + m) / lim
};

template <int MODE>
__device__ __forceinline__ unsigned int box_load(const box_args& a, int64_t n, int y, int x) {
    if constexpr (MODE == DIFF) {
        const int64_t p = ((n * a.H + min(max(y, 0), a.H - 1)) * a.W + min(max(x, 0), a.W - 1)) * 3;
        int d = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) d = max(d, abs((int)a.edit[p + c] - (int)a.src[p + c]));
        return (unsigned int)d;
    } else if constexpr (MODE == GROW) {
        if (y < 0 || y >= a.H || x < 0 || x >= a.W) return 0u;
        const int t = (int)(n % a.T);                               // frames of one sample only
        const int lo = max(t - a.grow_t, 0), hi = min(t + a.grow_t, a.T - 1);
        unsigned int v = 0u;
        for (int u = lo; u <= hi; ++u) v |= a.src[((n - t + u) * a.H + y) * a.W + x];
        return v;
    } else {
        return a.src[(n * a.H + min(max(y, 0), a.H - 1)) * a.W + min(max(x, 0), a.W - 1)];
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void box_sum_kernel(const box_args a) {
    __shared__ uint8_t in[LDS_ROWS * LDS_COLS];
    __shared__ unsigned short hs[LDS_ROWS * TC];
    const int tid = threadIdx.x, R = a.radius;
    const int c0 = blockIdx.x * TC, r0 = blockIdx.y * TR;
    const int64_t n = blockIdx.z;
    const int rows = TR + 2 * R, cols = TC + 2 * R;                 // <= LDS_ROWS, LDS_COLS: the host checks radius <= MAX_RADIUS

    for (int i = tid; i < rows * cols; i += 256) {
        const int r = i / cols, c = i - r * cols;
        in[i] = (uint8_t)box_load<MODE>(a, n, r0 - R + r, c0 - R + c);
    }
    __syncthreads();
    // rows: a thread sums the windows of 4 neighbouring columns, each from the one before it (one value leaves, one enters)
    for (int i = tid; i < rows * (TC / 4); i += 256) {
        const int r = i / (TC / 4), c = (i & (TC / 4 - 1)) * 4;
        const uint8_t* p = in + r * cols + c;
        unsigned int s = 0u;
        for (int j = 0; j <= 2 * R; ++j) s += p[j];                 // <= 65 * 255 < 2^16
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
    constexpr int VR = TR / (256 / TC);
    const int c = tid & (TC - 1), rb = (tid / TC) * VR;
    if (c0 + c >= a.W) return;
    unsigned int s = 0u;
    for (int j = 0; j <= 2 * R; ++j) s += hs[(rb + j) * TC + c];
    for (int q = 0; q < VR && r0 + rb + q < a.H; ++q) {
        if (q) s += (unsigned int)hs[(rb + q + 2 * R) * TC + c] - (unsigned int)hs[(rb + q - 1) * TC + c];
        unsigned int v;
        if constexpr (MODE == DIFF) {
            // (2 S + n) / (2 n) > threshold  <=>  2 S + n >= 2 n (threshold + 1): the definition's division, without dividing
            const unsigned int w = 2u * (unsigned int)R + 1u;
            v = 2u * s + w * w >= a.lim ? 1u : 0u;
        } else if constexpr (MODE == GROW) {
            v = s != 0u ? 1u : 0u;
        } else {
            const unsigned int w = 2u * (unsigned int)R + 1u;
            v = (510u * s + w * w) / a.lim;                         // an exact 32-bit division: 510 * 65^2 + 65^2 < 2^22
        }
        a.dst[(n * a.H + r0 + rb + q) * a.W + c0 + c] = (uint8_t)v;
    }
}

template <int MODE>
void launch_box(const box_args& a, int64_t N, hipStream_t s) {
    const dim3 grid((unsigned)((a.W + TC - 1) / TC), (unsigned)((a.H + TR - 1) / TR), (unsigned)N);
    hipLaunchKernelGGL(box_sum_kernel<MODE>, grid, dim3(256), 0, s, a);
}

// ---- the two passes of the resample on one-channel planes, the tables of wan_frames_u8_resample.  The tables are device memory:
// every window is clamped to the axis, so a malformed one gives wrong bytes, never a load outside src.
struct axis_args {
    const uint8_t* src;
    uint8_t* dst;
    const int* tab;          // int32 xmin[n_out] | n[n_out] | k[n_out][taps]
    int64_t rows;            // horizontal pass: N * H rows of W bytes
    int64_t src_bytes;
    int H, W, Ho, Wo, taps;
};

__device__ __forceinline__ void axis_window(const axis_args& a, int i, int n_in, int n_out, int& lo, int& n, const int*& k) {
    lo = min(max(a.tab[i], 0), n_in - 1);
    n = min(max(a.tab[n_out + i], 0), min(a.taps, n_in - lo));
    k = a.tab + 2 * (int64_t)n_out + (int64_t)i * a.taps;
}

// [rows, W] -> [rows, Wo]: one output byte per thread, a wave writes 64 consecutive bytes
__global__ __launch_bounds__(256) void plane_rows_kernel(const axis_args a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int64_t r = (int64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (r >= a.rows || i >= a.Wo) return;
    int lo, n;
    const int* k;
    axis_window(a, i, a.W, a.Wo, lo, n, k);
    const uint8_t* s = a.src + r * a.W + lo;
    unsigned int acc = 1u << 21;
    for (int j = 0; j < n; ++j) acc += __umul24(s[j], (unsigned int)k[j]);
    a.dst[r * a.Wo + i] = (uint8_t)min(acc >> 22, 255u);
}

// [N, H, Wo] -> [N, Ho, Wo]: 4 neighbouring bytes of one output row per thread, one run per tap (byte_runs.hpp)
__global__ __launch_bounds__(256) void plane_columns_kernel(const axis_args a) {
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4, i = blockIdx.y;
    const int64_t f = blockIdx.z;
    if (x >= a.Wo) return;
    int lo, n;
    const int* k;
    axis_window(a, i, a.H, a.Ho, lo, n, k);
    unsigned int acc[4] = {1u << 21, 1u << 21, 1u << 21, 1u << 21};
    for (int j = 0; j < n; ++j) {
        unsigned int w[1];
        load_bytes<1>(a.src, a.src_bytes, (f * a.H + lo + j) * a.Wo + x, w);       // behind the row's end: the next row's bytes, not stored
        const unsigned int kj = (unsigned int)k[j];
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[b] += __umul24(byte_of(w, b), kj);
    }
    unsigned int w[1] = {0u};
#pragma unroll
    for (int b = 0; b < 4; ++b) w[0] |= min(acc[b] >> 22, 255u) << (b * 8);
    store_span<1>(a.dst + (f * a.Ho + i) * a.Wo + x, w, min(4, a.Wo - x));
}

// ---- the composite.  A thread owns 16 pixels of one row of the output: 48 bytes of the original, and where the run meets the
// window 48 bytes of the edit and 16 of alpha, each one run at an address of any alignment (byte_runs.hpp).
constexpr int PIX = 16, BX = 16, BY = 16;

struct comp_args {
    const uint8_t *orig, *edit, *alpha;      // [N, Ho, Wo, 3], [N, wh, ww, 3], [N, wh, ww]
    uint8_t* out;                            // [N, Ho, Wo, 3]
    int64_t orig_bytes, edit_bytes, alpha_bytes;
    int Ho, Wo, wy, wx, wh, ww;
};

// floor(u / 255) for u < 2^16, as a 24-bit multiply and a shift: 0x8081 / 2^23 = (1 + 2^-15 + ...) / 255, and the excess
// u * (0x8081 / 2^23 - 1 / 255) < 65536 * 6e-8 < 1 / 255 never carries past the next multiple of 1 / 255.  u <= 255 * 255 + 127 here
// and u * 0x8081 < 2^32.  tests/test_gpu_keep_unedited.py runs all 256^3 triples (a, e, o).
__device__ __forceinline__ unsigned int div255(unsigned int u) { return __umul24(u, 0x8081u) >> 23; }

__global__ __launch_bounds__(BX * BY) void composite_kernel(const comp_args a) {
    const int k = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
    const int64_t n = blockIdx.z;
    const int x0 = k * PIX;
    if (y >= a.Ho || x0 >= a.Wo) return;
    const int64_t off = ((n * a.Ho + y) * a.Wo + x0) * 3;
    unsigned int w[12];
    load_bytes<12>(a.orig, a.orig_bytes, off, w);
    const int ey = y - a.wy, ex = x0 - a.wx;                        // the run in the window's coordinates
    if (ey >= 0 && ey < a.wh && ex + PIX > 0 && ex < a.ww) {
        unsigned int e[12], al[4];
        const int64_t eoff = (n * a.wh + ey) * a.ww + ex;           // may lie in front of the tensor or run past it: load_bytes reads
        load_bytes<12>(a.edit, a.edit_bytes, eoff * 3, e);          // nothing outside, and those pixels are outside the window
        load_bytes<4>(a.alpha, a.alpha_bytes, eoff, al);
        unsigned int r[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) r[i] = 0u;
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const unsigned int av = (ex + j >= 0 && ex + j < a.ww) ? byte_of(al, j) : 0u;      // alpha 0 gives the original's byte
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int b = 3 * j + c;
                const unsigned int u = __umul24(av, byte_of(e, b)) + __umul24(255u - av, byte_of(w, b)) + 127u;
                r[b >> 2] |= div255(u) << ((b & 3) * 8);
            }
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) w[i] = r[i];
    }
    store_span<12>(a.out + off, w, min(PIX, a.Wo - x0) * 3);
}

}  // namespace

extern "C" int64_t wan_change_mask_workspace_bytes(int B, int T, int H, int W) {
    if (B <= 0 || T <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * (((int64_t)B * T * H * W + 255) / 256 * 256);
}

extern "C" wan_status_t wan_change_mask(const void* source_u8, const void* edit_u8, void* alpha_u8, int B, int T, int H, int W,
                                        int threshold, int smooth, int grow, int grow_t, int feather, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
    WAN_REQUIRE(source_u8 && edit_u8 && alpha_u8 && workspace, WAN_ERR_INVALID, "wan_change_mask: null tensor");
    WAN_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0, WAN_ERR_INVALID, "wan_change_mask: bad shape B=%d T=%d H=%d W=%d", B, T, H, W);
    WAN_REQUIRE(threshold >= 0 && threshold <= 254 && smooth >= 0 && smooth <= WAN_MASK_MAX_SMOOTH && grow >= 0 && grow <= WAN_MASK_MAX_GROW &&
                    grow_t >= 0 && grow_t <= WAN_MASK_MAX_GROW_T && feather >= 0 && feather <= grow, WAN_ERR_INVALID,
                "wan_change_mask: threshold=%d (0..254) smooth=%d (0..%d) grow=%d (0..%d) grow_t=%d (0..%d) feather=%d (0..grow)", threshold,
                smooth, WAN_MASK_MAX_SMOOTH, grow, WAN_MASK_MAX_GROW, grow_t, WAN_MASK_MAX_GROW_T, feather);
    const int64_t N = (int64_t)B * T;
    WAN_REQUIRE(N <= 65535 && (H + TR - 1) / TR <= 65535 && (int64_t)H * W * 3 < (1ll << 31), WAN_ERR_UNSUPPORTED,
                "wan_change_mask: B * T = %lld frames of %d x %d (at most 65535 frames per call, a frame below 2 GiB)", (long long)N, H, W);
    WAN_REQUIRE(workspace_bytes >= wan_change_mask_workspace_bytes(B, T, H, W), WAN_ERR_INVALID,
                "wan_change_mask: workspace of %lld bytes, needs %lld", (long long)workspace_bytes,
                (long long)wan_change_mask_workspace_bytes(B, T, H, W));
    static_assert(WAN_MASK_MAX_GROW == MAX_RADIUS && WAN_MASK_MAX_SMOOTH <= MAX_RADIUS, "the LDS of box_sum_kernel is sized from MAX_RADIUS");
    uint8_t* b = (uint8_t*)workspace;
    uint8_t* g = b + wan_change_mask_workspace_bytes(B, T, H, W) / 2;
    hipStream_t s = (hipStream_t)stream;
    box_args a;
    a.T = T; a.H = H; a.W = W; a.grow_t = grow_t;
    a.src = (const uint8_t*)source_u8; a.edit = (const uint8_t*)edit_u8; a.dst = b;
    a.radius = smooth;
    a.lim = 2u * (unsigned)((2 * smooth + 1) * (2 * smooth + 1)) * (unsigned)(threshold + 1);
    launch_box<DIFF>(a, N, s);
    WAN_CHECK_LAUNCH("wan_change_mask (difference)");
    a.src = b; a.edit = nullptr; a.dst = g; a.radius = grow; a.lim = 0u;
    launch_box<GROW>(a, N, s);
    WAN_CHECK_LAUNCH("wan_change_mask (grow)");
    a.src = g; a.dst = (uint8_t*)alpha_u8; a.radius = feather;
    a.lim = 2u * (unsigned)((2 * feather + 1) * (2 * feather + 1));
    launch_box<FEATHER>(a, N, s);
    WAN_CHECK_LAUNCH("wan_change_mask (feather)");
    return WAN_OK;
}

extern "C" wan_status_t wan_plane_u8_resample(const void* src_u8, void* tmp_u8, void* dst_u8, int N, int H, int W, int Ho, int Wo,
                                              const void* xtab, int kx, const void* ytab, int ky, void* stream) {
    WAN_REQUIRE(src_u8 && tmp_u8 && dst_u8 && xtab && ytab, WAN_ERR_INVALID, "wan_plane_u8_resample: null tensor");
    WAN_REQUIRE(N > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, WAN_ERR_INVALID, "wan_plane_u8_resample: bad shape N=%d H=%d W=%d Ho=%d Wo=%d", N, H,
                W, Ho, Wo);
    WAN_REQUIRE(kx > 0 && ky > 0, WAN_ERR_INVALID, "wan_plane_u8_resample: tap counts kx=%d ky=%d", kx, ky);
    WAN_REQUIRE(kx <= WAN_RESAMPLE_MAX_TAPS && ky <= WAN_RESAMPLE_MAX_TAPS, WAN_ERR_UNSUPPORTED,
                "wan_plane_u8_resample: kx=%d ky=%d filter taps; built for at most %d", kx, ky, WAN_RESAMPLE_MAX_TAPS);
    const int64_t rows = (int64_t)N * H;
    const int64_t gy = std::min<int64_t>(rows, 32768), gz = (rows + gy - 1) / gy;
    WAN_REQUIRE(N <= 65535 && Ho <= 65535 && gz <= 65535, WAN_ERR_UNSUPPORTED, "wan_plane_u8_resample: N=%d planes of %d x %d -> %d x %d too large",
                N, H, W, Ho, Wo);
    hipStream_t s = (hipStream_t)stream;
    axis_args a;
    a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.rows = rows;
    a.src = (const uint8_t*)src_u8; a.dst = (uint8_t*)tmp_u8; a.tab = (const int*)xtab; a.taps = kx; a.src_bytes = rows * W;
    hipLaunchKernelGGL(plane_rows_kernel, dim3((unsigned)((Wo + 255) / 256), (unsigned)gy, (unsigned)gz), dim3(256), 0, s, a);
    WAN_CHECK_LAUNCH("wan_plane_u8_resample (horizontal)");
    a.src = (const uint8_t*)tmp_u8; a.dst = (uint8_t*)dst_u8; a.tab = (const int*)ytab; a.taps = ky; a.src_bytes = rows * Wo;
    hipLaunchKernelGGL(plane_columns_kernel, dim3((unsigned)((Wo + 1023) / 1024), (unsigned)Ho, (unsigned)N), dim3(256), 0, s, a);
    WAN_CHECK_LAUNCH("wan_plane_u8_resample (vertical)");
    return WAN_OK;
}

extern "C" wan_status_t wan_frames_u8_composite(const void* original_u8, const void* edit_u8, const void* alpha_u8, void* out_u8, int N,
                                                int Ho, int Wo, int wy, int wx, int wh, int ww, void* stream) {
    WAN_REQUIRE(original_u8 && edit_u8 && alpha_u8 && out_u8, WAN_ERR_INVALID, "wan_frames_u8_composite: null tensor");
    WAN_REQUIRE(N > 0 && Ho > 0 && Wo > 0, WAN_ERR_INVALID, "wan_frames_u8_composite: bad shape N=%d Ho=%d Wo=%d", N, Ho, Wo);
    WAN_REQUIRE(wy >= 0 && wx >= 0 && wh > 0 && ww > 0 && wy <= Ho - wh && wx <= Wo - ww, WAN_ERR_INVALID,
                "wan_frames_u8_composite: window (%d, %d, %d, %d) of a %d x %d frame", wy, wx, wh, ww, Ho, Wo);
    WAN_REQUIRE(N <= 65535 && (Ho + BY - 1) / BY <= 65535 && Wo <= (1 << 24), WAN_ERR_UNSUPPORTED,
                "wan_frames_u8_composite: N=%d frames of %d x %d (at most 65535 frames per call)", N, Ho, Wo);
    comp_args a;
    a.orig = (const uint8_t*)original_u8; a.edit = (const uint8_t*)edit_u8; a.alpha = (const uint8_t*)alpha_u8; a.out = (uint8_t*)out_u8;
    a.orig_bytes = (int64_t)N * Ho * Wo * 3;
    a.alpha_bytes = (int64_t)N * wh * ww;
    a.edit_bytes = a.alpha_bytes * 3;
    a.Ho = Ho; a.Wo = Wo; a.wy = wy; a.wx = wx; a.wh = wh; a.ww = ww;
    const int runs = (Wo + PIX - 1) / PIX;
    const dim3 grid((unsigned)((runs + BX - 1) / BX), (unsigned)((Ho + BY - 1) / BY), (unsigned)N), block(BX, BY);
    hipLaunchKernelGGL(composite_kernel, grid, block, 0, (hipStream_t)stream, a);
    WAN_CHECK_LAUNCH("wan_frames_u8_composite");
    return WAN_OK;
}
