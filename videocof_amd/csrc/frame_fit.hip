// Fit a uint8 clip to another size on the device: antialiased-triangle resample and crop of uint8 [B, T, H, W, 3] frames in one launch.
//   horizontal pass:  source rows -> an intermediate of the tile's source rows x the tile's output columns, rounded to uint8
//   vertical pass:    intermediate -> output rows, interleaved RGB
// Both passes are the integer arithmetic of include/wan_hip.h (wan_frames_u8_resample): (2^21 + sum_j src[xmin + j] * k[j]) >> 22,
// clipped to a byte, coefficients from the host's tables.  No floating point.
//
// A workgroup owns TR x TC output pixels of one frame.  The source rows it needs come in chunks: each chunk is staged in LDS with
// 16-byte loads, the horizontal pass reads it bytewise out of LDS and writes the intermediate, which never leaves LDS; the vertical
// pass reads 16 intermediate bytes per tap (ds_read_b128) and stores 16 output bytes (dwordx4).
//
// Alignment: a staged row starts at the 16-byte boundary at or below its first byte in global memory and the pass skips the
// 0..15 bytes in front, so EVERY row is read with 16-byte loads whatever W * 3 or the base pointer are (854 * 3 bytes per row is not
// even a multiple of 4); only a 16-byte piece that would reach outside the source tensor is read byte by byte.  An output piece is
// stored as one dwordx4 when its address is 16-byte aligned and it lies inside the row, byte by byte otherwise.
//
// Bounds: the tables are device memory, so the kernel trusts nothing in them.  Every window is clamped to the source, the staged
// columns and rows to the LDS the launch was given (sized from the tap counts, which bound the span of a tile of a valid table:
// span_bound below); a table that breaks the bound gives wrong bytes, never an access outside the buffers.
#include <algorithm>

#include "common.hpp"

namespace {

constexpr int TR = 16;                      // output rows of a tile
constexpr int TC = 64;                      // output columns of a tile (192 bytes = 12 pieces of 16)
constexpr int ROWB = TC * 3;                // bytes of an intermediate row
constexpr int PIECES = ROWB / 16;
constexpr int MAX_TAPS = WAN_RESAMPLE_MAX_TAPS;
constexpr int COEF_BITS = 22;
constexpr int STAGE_BUDGET = 16 * 1024;     // bytes of staged source rows per chunk (as many rows as fit, at least one)
constexpr int LDS_LIMIT = 64 * 1024;        // static + dynamic LDS of a launch without an opt-in

// Source positions a tile of `tile` consecutive outputs can span when the axis' largest tap count is k.  A window is
// [int(c - s + 0.5), int(c + s + 0.5)) around c = (i + 0.5) * scale with s = max(scale, 1), so taps >= 2 s - 1 somewhere and the
// span of a tile is <= (tile - 1) * scale + 2 s + 1 <= (tile - 1) * (k + 1) / 2 + k + 3 (tests/test_frame_fit_host.py sweeps it).
constexpr int span_bound(int tile, int k) { return (tile - 1) * ((k + 2) / 2) + k + 3; }

struct fit_args {
    const uint8_t* src;
    uint8_t* dst;
    const int* xtab;
    const int* ytab;
    int H, W, Ho, Wo, kx, ky;
    int seg_cols;            // staged source columns per row (span_bound(TC, kx), at most W)
    int stage_stride;        // bytes of a staged row: seg_cols * 3 + the 15 bytes in front, rounded up to 16, + 16
    int stage_rows;          // source rows per chunk
    int inter_rows;          // rows of the intermediate (span_bound(TR, ky), at most H)
    int64_t src_bytes;       // B * T * H * W * 3
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(256) void frames_resample_kernel(const fit_args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    // LDS: x coefficients int[kx][TC] | x window int[2][TC] | y coefficients int[TR][ky] | y window int[2][TR] | intermediate | stage
    int* xk = reinterpret_cast<int*>(lds);
    int* xw = xk + a.kx * TC;
    int* yk = xw + 2 * TC;
    int* yw = yk + TR * a.ky;
    uint8_t* inter = reinterpret_cast<uint8_t*>(yw + 2 * TR);
    inter += (16 - (reinterpret_cast<uintptr_t>(inter) & 15)) & 15;
    uint8_t* stage = inter + (size_t)a.inter_rows * ROWB;

    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * TC, r0 = blockIdx.y * TR;
    const int64_t bt = blockIdx.z;
    const int ncol = min(TC, a.Wo - c0), nrow = min(TR, a.Ho - r0);

    // ---- the tile's slice of the tables: int32 xmin[n_out], n[n_out], k[n_out][taps]
    for (int i = tid; i < TC; i += 256) {
        const bool in = i < ncol;
        xw[i] = in ? a.xtab[c0 + i] : 0;
        xw[TC + i] = in ? a.xtab[a.Wo + c0 + i] : 0;
    }
    for (int i = tid; i < a.kx * TC; i += 256) {
        const int c = i & (TC - 1), j = i / TC;
        xk[j * TC + c] = c < ncol ? a.xtab[2 * (int64_t)a.Wo + (int64_t)(c0 + c) * a.kx + j] : 0;
    }
    for (int i = tid; i < TR; i += 256) {
        const bool in = i < nrow;
        yw[i] = in ? a.ytab[r0 + i] : 0;
        yw[TR + i] = in ? a.ytab[a.Ho + r0 + i] : 0;
    }
    for (int i = tid; i < TR * a.ky; i += 256) {
        const int r = i / a.ky;
        yk[i] = r < nrow ? a.ytab[2 * (int64_t)a.Ho + (int64_t)r0 * a.ky + i] : 0;
    }
    __syncthreads();

    // source rectangle of the tile, clamped to the source and to what the LDS holds
    const int xs = clampi(xw[0], 0, a.W - 1);
    const int xe = clampi(xw[ncol - 1] + xw[TC + ncol - 1], xs + 1, min(a.W, xs + a.seg_cols));
    const int ys = clampi(yw[0], 0, a.H - 1);
    const int ye = clampi(yw[nrow - 1] + yw[TR + nrow - 1], ys + 1, min(a.H, ys + a.inter_rows));
    const int seg_bytes = (xe - xs) * 3;
    const int64_t row_bytes = (int64_t)a.W * 3;
    const int64_t frame_off = bt * a.H * row_bytes;                 // byte offset of the frame in src
    const uintptr_t src_lo = reinterpret_cast<uintptr_t>(a.src);

    // this thread's column of the horizontal pass
    const int hc = tid & (TC - 1);
    const int hx = clampi(xw[hc], xs, xe - 1);
    const int hn = clampi(xw[TC + hc], 0, min(a.kx, xe - hx));
    const int hoff = (hx - xs) * 3;

    for (int y0 = ys; y0 < ye; y0 += a.stage_rows) {
        const int rows = min(a.stage_rows, ye - y0);
        // ---- stage: half a wave per source row, 16 bytes per lane
        for (int r = tid >> 5; r < rows; r += 8) {
            const int64_t off = frame_off + (int64_t)(y0 + r) * row_bytes + (int64_t)xs * 3;      // first byte of the segment in src
            const int mis = (int)((src_lo + (uintptr_t)off) & 15);
            const int npiece = (mis + seg_bytes + 15) >> 4;
            uint8_t* srow = stage + (size_t)r * a.stage_stride;
            for (int q = tid & 31; q < npiece; q += 32) {
                const int64_t p = off - mis + 16 * (int64_t)q;                                   // may start before / end after src
                u32x4 v;
                if (p >= 0 && p + 16 <= a.src_bytes) {
                    v = *reinterpret_cast<const u32x4*>(a.src + p);
                } else {
                    unsigned int w[4] = {0u, 0u, 0u, 0u};
                    for (int b = 0; b < 16; ++b) {
                        const int64_t pb = p + b;
                        if (pb >= 0 && pb < a.src_bytes) w[b >> 2] |= (unsigned int)a.src[pb] << ((b & 3) * 8);
                    }
                    v = u32x4{w[0], w[1], w[2], w[3]};
                }
                *reinterpret_cast<u32x4*>(srow + 16 * q) = v;
            }
        }
        __syncthreads();
        // ---- horizontal pass: one output pixel of one source row per thread
        for (int r = tid >> 6; r < rows; r += 4) {
            const int64_t off = frame_off + (int64_t)(y0 + r) * row_bytes + (int64_t)xs * 3;
            const int mis = (int)((src_lo + (uintptr_t)off) & 15);
            const uint8_t* p = stage + (size_t)r * a.stage_stride + mis + hoff;
            unsigned int s0 = 1u << (COEF_BITS - 1), s1 = s0, s2 = s0;
            for (int j = 0; j < hn; ++j) {
                const unsigned int k = (unsigned int)xk[j * TC + hc];
                s0 += __umul24(p[3 * j], k);                      // a byte times a coefficient <= 2^22: v_mad_u32_u24
                s1 += __umul24(p[3 * j + 1], k);
                s2 += __umul24(p[3 * j + 2], k);
            }
            uint8_t* o = inter + (size_t)(y0 - ys + r) * ROWB + hc * 3;
            o[0] = (uint8_t)min(s0 >> COEF_BITS, 255u);
            o[1] = (uint8_t)min(s1 >> COEF_BITS, 255u);
            o[2] = (uint8_t)min(s2 >> COEF_BITS, 255u);
        }
        __syncthreads();
    }

    // ---- vertical pass: 16 bytes of one output row per thread
    if (tid < TR * PIECES) {
        const int r = tid / PIECES, q = tid - r * PIECES;
        const int valid = ncol * 3 - 16 * q;                         // bytes of this piece inside the row
        if (r < nrow && valid > 0) {
            const int vy = clampi(yw[r], ys, ye - 1);
            const int vn = clampi(yw[TR + r], 0, min(a.ky, ye - vy));
            const uint8_t* col = inter + (size_t)(vy - ys) * ROWB + 16 * q;
            unsigned int s[16];
#pragma unroll
            for (int b = 0; b < 16; ++b) s[b] = 1u << (COEF_BITS - 1);
            for (int j = 0; j < vn; ++j) {
                const unsigned int k = (unsigned int)yk[r * a.ky + j];
                const u32x4 v = *reinterpret_cast<const u32x4*>(col + (size_t)j * ROWB);
#pragma unroll
                for (int b = 0; b < 16; ++b) s[b] += __umul24((v[b >> 2] >> ((b & 3) * 8)) & 0xffu, k);
            }
            unsigned int w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int b = 0; b < 16; ++b) w[b >> 2] |= min(s[b] >> COEF_BITS, 255u) << ((b & 3) * 8);
            uint8_t* d = a.dst + ((bt * a.Ho + r0 + r) * a.Wo + c0) * 3 + 16 * q;
            if (valid >= 16 && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
                *reinterpret_cast<u32x4*>(d) = u32x4{w[0], w[1], w[2], w[3]};
            } else {
                const int nb = min(valid, 16);
                for (int b = 0; b < nb; ++b) d[b] = (uint8_t)(w[b >> 2] >> ((b & 3) * 8));
            }
        }
    }
}

}  // namespace

extern "C" int64_t wan_frames_resample_table_bytes(int n_out, int taps) {
    if (n_out <= 0 || taps <= 0) return 0;
    return (int64_t)n_out * (2 + (int64_t)taps) * 4;
}

extern "C" wan_status_t wan_frames_u8_resample(const void* src_u8, void* dst_u8, int B, int T, int H, int W, int Ho, int Wo,
                                               const void* xtab, int kx, const void* ytab, int ky, void* stream) {
    WAN_REQUIRE(src_u8 && dst_u8 && xtab && ytab, WAN_ERR_INVALID, "wan_frames_u8_resample: null tensor");
    WAN_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, WAN_ERR_INVALID,
                "wan_frames_u8_resample: bad shape B=%d T=%d H=%d W=%d Ho=%d Wo=%d", B, T, H, W, Ho, Wo);
    WAN_REQUIRE(kx > 0 && ky > 0, WAN_ERR_INVALID, "wan_frames_u8_resample: tap counts kx=%d ky=%d", kx, ky);
    WAN_REQUIRE(kx <= MAX_TAPS && ky <= MAX_TAPS, WAN_ERR_UNSUPPORTED,
                "wan_frames_u8_resample: kx=%d ky=%d filter taps; built for at most %d (a downscale of about %dx)", kx, ky, MAX_TAPS,
                MAX_TAPS / 2 - 1);
    const int64_t BT = (int64_t)B * T;
    WAN_REQUIRE(BT <= 65535, WAN_ERR_UNSUPPORTED, "wan_frames_u8_resample: B * T = %lld frames (at most 65535 per call)", (long long)BT);
    WAN_REQUIRE((int64_t)H * W * 3 < (1ll << 31) && (int64_t)Ho * Wo * 3 < (1ll << 31) && (Ho + TR - 1) / TR <= 65535, WAN_ERR_UNSUPPORTED,
                "wan_frames_u8_resample: frame %d x %d -> %d x %d too large", H, W, Ho, Wo);
    fit_args a;
    a.src = (const uint8_t*)src_u8;
    a.dst = (uint8_t*)dst_u8;
    a.xtab = (const int*)xtab;
    a.ytab = (const int*)ytab;
    a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.kx = kx; a.ky = ky;
    a.seg_cols = std::min(W, span_bound(TC, kx));
    a.stage_stride = (a.seg_cols * 3 + 15 + 15) / 16 * 16 + 16;
    a.inter_rows = std::min(H, span_bound(TR, ky));
    a.src_bytes = BT * H * W * 3;
    const int fixed = (kx * TC + 2 * TC + TR * ky + 2 * TR) * 4 + 16 + a.inter_rows * ROWB;
    a.stage_rows = std::min({a.inter_rows, STAGE_BUDGET / a.stage_stride, (LDS_LIMIT - fixed) / a.stage_stride});
    WAN_REQUIRE(a.stage_rows >= 1, WAN_ERR_UNSUPPORTED, "wan_frames_u8_resample: kx=%d ky=%d need more LDS than a workgroup has", kx, ky);
    const size_t lds = (size_t)fixed + (size_t)a.stage_rows * a.stage_stride;
    const dim3 grid((unsigned)((Wo + TC - 1) / TC), (unsigned)((Ho + TR - 1) / TR), (unsigned)BT);
    hipLaunchKernelGGL(frames_resample_kernel, grid, dim3(256), lds, (hipStream_t)stream, a);
    WAN_CHECK_LAUNCH("wan_frames_u8_resample");
    return WAN_OK;
}
