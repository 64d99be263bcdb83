// 8-bit YCbCr planes <-> interleaved uint8 RGB frames on the device: what a decoder yields and an encoder takes (planar 4:2:0 / 4:2:2 /
// 4:4:4 / mono, or NV12-style interleaved CbCr) on one side, the uint8 [T, H, W, 3] frames of the frame path on the other.
//   in : wan_yuv_to_frames_u8   chroma up (two taps per axis, weights in quarters, ONE rounding), the inverse matrix, clamp
//   out: wan_frames_u8_to_yuv   the forward matrix, clamp, chroma down ((a + b + c + d + 2) >> 2 with the last column / row replicated)
// The arithmetic is the integer definition of include/wan_hip.h: 16-bit fixed-point coefficients the host builds in float64
// (videocof_amd/video_io.py, yuv_matrix) and hands over by value; every product is a 24-bit multiply-add, every sum fits an int32.
// No floating point, no LDS, no scratch.
//
// A thread owns 16 pixels of one row ([16 k, 16 k + 16), so its chroma pairs start at an even column) -- of two rows on the way out
// when the chroma is subsampled, since a 2 x 2 block shares one chroma sample.  One grid dimension is the frame, one the row group,
// so no thread divides.  The 48 RGB bytes, the 16 luma bytes and the 8 (16) chroma bytes of a thread are each ONE run of bytes at
// an address of any alignment (an 854-wide clip has 2562-byte RGB rows and 427-byte chroma rows; the planes of a .y4m file uploaded
// as it is start wherever the header ends): load_bytes / store_span move a run as dwordx4 (dwordx2 for 8 bytes) when its address
// allows, else as aligned dwords shifted into place with v_alignbyte_b32 and the up to 3 bytes in front of / behind them one by
// one.  A run that is cut by the end of a row, and a load whose aligned words would leave the described extent, go byte by byte.
// Stores never touch a byte outside the run, so padding between rows, planes and frames keeps its contents.
#include <algorithm>

#include "byte_runs.hpp"
#include "common.hpp"

namespace {

constexpr int PIX = 16;                     // pixels per thread
constexpr int BX = 16, BY = 16;             // threads of a workgroup: 16 runs of a row x 16 rows (a wave = 4 rows x 768 RGB bytes)

struct yuv_args {
    uint8_t *y, *cb, *cr;                   // cb == nullptr: mono (reading only)
    uint8_t* frames;                        // uint8 [T, H, W, 3], contiguous
    int64_t y_extent, cb_extent, cr_extent; // bytes addressable from each plane's base
    int64_t frames_bytes;
    int64_t y_row, y_frame, c_row, c_frame; // strides in bytes
    int H, W, Ch, Cw;                       // chroma plane: Ch x Cw samples
    int sub_y, cosited;
    int k[9], yo;                           // the 3 x 3 matrix in 16-bit fixed point, the luma offset
};

// clamp(s >> 16, 0, 255) of a 16-bit fixed-point sum, written as a clamp of the sum and a logical shift.  NOT min(max(s >> 16, 0), 255):
// two of those packed side by side become one v_ashr_pk_u8_i32, whose result hipcc then ORs into the word as a whole dword although
// the instruction writes 16 bits and leaves the upper half of its destination as it was (seen on gfx950 with ROCm 7: the byte
// two places up came out ORed with the old register contents).  tests/test_gpu_yuv.py compares every byte.
__device__ __forceinline__ unsigned int fixed_to_byte(int s) { return (unsigned int)min(max(s, 0), 0xffffff) >> 16; }

// ---- in: one chroma row of a thread's 16 pixels
// SUBX: NS = 10 samples [8 k - 1, 8 k + 8]: the 8 of the thread's own pairs as one run, the two neighbours as single bytes at indices
// clamped to the plane.  Not subsampled: NS = 16 samples, one per pixel.  CSTEP = 2 picks every other byte of the run.
template <int SUBX, int CSTEP>
__device__ __forceinline__ void load_chroma_row(const uint8_t* base, int64_t extent, int64_t row_off, int k, int Cw, int (&c)[SUBX ? 10 : 16]) {
    if constexpr (SUBX) {
        unsigned int w[2 * CSTEP];
        load_bytes<2 * CSTEP>(base, extent, row_off + (int64_t)(8 * k) * CSTEP, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) c[1 + i] = (int)byte_of(w, i * CSTEP);
        c[0] = base[row_off + (int64_t)max(8 * k - 1, 0) * CSTEP];
        c[9] = base[row_off + (int64_t)min(8 * k + 8, Cw - 1) * CSTEP];
    } else {
        unsigned int w[4 * CSTEP];
        load_bytes<4 * CSTEP>(base, extent, row_off + (int64_t)(PIX * k) * CSTEP, w);
#pragma unroll
        for (int i = 0; i < PIX; ++i) c[i] = (int)byte_of(w, i * CSTEP);
    }
}

// one chroma plane at the thread's 16 pixels: (sum over the 2 x 2 taps of wy * wx * C + 8) >> 4
template <int SUBX, int CSTEP>
__device__ __forceinline__ void chroma_up(const yuv_args& a, const uint8_t* base, int64_t extent, int64_t t, int k, int r0, int r1,
                                          int wy0, int wy1, int (&out)[PIX]) {
    constexpr int NS = SUBX ? 10 : 16;
    int v[NS];
    load_chroma_row<SUBX, CSTEP>(base, extent, t * a.c_frame + (int64_t)r0 * a.c_row, k, a.Cw, v);
    if (a.sub_y) {
        int u[NS];
        load_chroma_row<SUBX, CSTEP>(base, extent, t * a.c_frame + (int64_t)r1 * a.c_row, k, a.Cw, u);
#pragma unroll
        for (int i = 0; i < NS; ++i) v[i] = wy0 * v[i] + wy1 * u[i];
    } else {
#pragma unroll
        for (int i = 0; i < NS; ++i) v[i] *= 4;
    }
    if constexpr (SUBX) {
        // samples of the run behind the plane's last column repeat it (the last pixel of an even row width reads column Cw)
#pragma unroll
        for (int i = 1; i < 8; ++i)
            if (8 * k + i > a.Cw - 1) v[1 + i] = v[i];
        // centred: even x = (c[x/2 - 1], 1), (c[x/2], 3), odd x = (c[x/2], 3), (c[x/2 + 1], 1); left co-sited: even (c[x/2], 4), odd (c[x/2], 2), (c[x/2 + 1], 2)
        const int ea = a.cosited ? 0 : 1, eb = 4 - ea, oa = a.cosited ? 2 : 3, ob = 4 - oa;
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const int h = j >> 1;
            out[j] = (j & 1) ? (oa * v[h + 1] + ob * v[h + 2] + 8) >> 4 : (ea * v[h] + eb * v[h + 1] + 8) >> 4;
        }
    } else {
#pragma unroll
        for (int j = 0; j < PIX; ++j) out[j] = (4 * v[j] + 8) >> 4;
    }
}

template <int SUBX, int CSTEP>
__global__ __launch_bounds__(BX * BY) void yuv_to_frames_kernel(const yuv_args a) {
    const int k = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y;
    const int64_t t = blockIdx.z;
    const int x0 = k * PIX;
    if (y >= a.H || x0 >= a.W) return;
    unsigned int yw[4];
    load_bytes<4>(a.y, a.y_extent, t * a.y_frame + (int64_t)y * a.y_row + x0, yw);
    int cb[PIX], cr[PIX];
    if (a.cb) {
        int r0 = y, r1 = y, wy0 = 4, wy1 = 0;
        if (a.sub_y) {                                              // the vertical axis is always centred
            const int h = y >> 1;
            if (y & 1) { r0 = h; r1 = min(h + 1, a.Ch - 1); wy0 = 3; wy1 = 1; }
            else { r0 = max(h - 1, 0); r1 = h; wy0 = 1; wy1 = 3; }
        }
        chroma_up<SUBX, CSTEP>(a, a.cb, a.cb_extent, t, k, r0, r1, wy0, wy1, cb);
        chroma_up<SUBX, CSTEP>(a, a.cr, a.cr_extent, t, k, r0, r1, wy0, wy1, cr);
    } else {
#pragma unroll
        for (int j = 0; j < PIX; ++j) cb[j] = cr[j] = 128;
    }
    unsigned int w[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) w[i] = 0u;
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const int yy = (int)byte_of(yw, j) - a.yo, u = cb[j] - 128, v = cr[j] - 128;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s = __mul24(a.k[3 * c], yy) + __mul24(a.k[3 * c + 1], u) + __mul24(a.k[3 * c + 2], v) + (1 << 15);
            const int b = 3 * j + c;
            w[b >> 2] |= fixed_to_byte(s) << ((b & 3) * 8);
        }
    }
    store_span<12>(a.frames + ((t * a.H + y) * a.W + x0) * 3, w, min(PIX, a.W - x0) * 3);
}

// ---- out: SUB = 1 writes 4:2:0 (a thread owns 16 pixels of the rows 2 r and 2 r + 1), SUB = 0 writes 4:4:4 (one row)
template <int SUB, int CSTEP>
__global__ __launch_bounds__(BX * BY) void frames_to_yuv_kernel(const yuv_args a) {
    const int k = blockIdx.x * BX + threadIdx.x, r = blockIdx.y * BY + threadIdx.y;
    const int64_t t = blockIdx.z;
    const int x0 = k * PIX;
    if (r >= a.Ch || x0 >= a.W) return;
    const int npix = min(PIX, a.W - x0);
    constexpr int NC = SUB ? PIX / 2 : PIX;                         // chroma samples of the thread per plane
    int sb[NC], sr[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) sb[i] = sr[i] = 0;
#pragma unroll
    for (int half = 0; half <= SUB; ++half) {
        const int row = SUB ? 2 * r + half : r;
        const int yrow = min(row, a.H - 1);                         // an odd height repeats its last row for the chroma
        unsigned int w[12];
        load_bytes<12>(a.frames, a.frames_bytes, ((t * a.H + yrow) * a.W + x0) * 3, w);
        unsigned int yw[4] = {0u, 0u, 0u, 0u};
        int cb[PIX], cr[PIX];
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const int R = (int)byte_of(w, 3 * j), G = (int)byte_of(w, 3 * j + 1), B = (int)byte_of(w, 3 * j + 2);
            const int yv = __mul24(a.k[0], R) + __mul24(a.k[1], G) + __mul24(a.k[2], B) + (a.yo << 16) + (1 << 15);
            const int bv = __mul24(a.k[3], R) + __mul24(a.k[4], G) + __mul24(a.k[5], B) + (128 << 16) + (1 << 15);
            const int rv = __mul24(a.k[6], R) + __mul24(a.k[7], G) + __mul24(a.k[8], B) + (128 << 16) + (1 << 15);
            yw[j >> 2] |= fixed_to_byte(yv) << ((j & 3) * 8);
            cb[j] = (int)fixed_to_byte(bv);
            cr[j] = (int)fixed_to_byte(rv);
        }
        if (row < a.H) store_span<4>(a.y + t * a.y_frame + (int64_t)row * a.y_row + x0, yw, npix);
        if constexpr (SUB) {
#pragma unroll
            for (int i = 0; i < NC; ++i) {                          // an odd width repeats its last column
                const bool pair = 2 * i + 1 < npix;
                sb[i] += cb[2 * i] + (pair ? cb[2 * i + 1] : cb[2 * i]);
                sr[i] += cr[2 * i] + (pair ? cr[2 * i + 1] : cr[2 * i]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NC; ++i) { sb[i] = cb[i]; sr[i] = cr[i]; }
        }
    }
    const int nc = SUB ? (npix + 1) >> 1 : npix;
    const int64_t coff = t * a.c_frame + (int64_t)r * a.c_row + (int64_t)(NC * k) * CSTEP;
    if constexpr (CSTEP == 1) {
        unsigned int wb[NC / 4], wr[NC / 4];
#pragma unroll
        for (int i = 0; i < NC / 4; ++i) wb[i] = wr[i] = 0u;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            wb[i >> 2] |= (unsigned int)(SUB ? (sb[i] + 2) >> 2 : sb[i]) << ((i & 3) * 8);
            wr[i >> 2] |= (unsigned int)(SUB ? (sr[i] + 2) >> 2 : sr[i]) << ((i & 3) * 8);
        }
        store_span<NC / 4>(a.cb + coff, wb, nc);
        store_span<NC / 4>(a.cr + coff, wr, nc);
    } else {
        // interleaved CbCr: the two planes are each other's odd bytes, so a plane is written one byte at a time
#pragma unroll
        for (int i = 0; i < NC; ++i)
            if (i < nc) {
                a.cb[coff + 2 * i] = (uint8_t)(SUB ? (sb[i] + 2) >> 2 : sb[i]);
                a.cr[coff + 2 * i] = (uint8_t)(SUB ? (sr[i] + 2) >> 2 : sr[i]);
            }
    }
}

// ---- host: the described geometry against the described extents, before anything is enqueued
struct span { uintptr_t lo, hi; };                                  // [lo, hi) of the bytes a plane touches

wan_status_t check_planes(const char* who, const wan_yuv_planes* p, const wan_yuv_coef* coef, const void* frames, int T, int H, int W,
                          bool writing, yuv_args& a) {
    WAN_REQUIRE(p && coef && frames, WAN_ERR_INVALID, "%s: null argument", who);
    WAN_REQUIRE(T > 0 && H > 0 && W > 0, WAN_ERR_INVALID, "%s: bad shape T=%d H=%d W=%d", who, T, H, W);
    WAN_REQUIRE(T <= 65535 && (H + BY - 1) / BY <= 65535 && W <= (1 << 24) && (int64_t)H * W * 3 < (1ll << 40), WAN_ERR_UNSUPPORTED,
                "%s: clip T=%d H=%d W=%d too large (at most 65535 frames per call)", who, T, H, W);
    WAN_REQUIRE(p->y, WAN_ERR_INVALID, "%s: null luma plane", who);
    WAN_REQUIRE((p->cb == nullptr) == (p->cr == nullptr), WAN_ERR_INVALID, "%s: one chroma plane without the other", who);
    const bool mono = p->cb == nullptr;
    WAN_REQUIRE(!(mono && writing), WAN_ERR_INVALID, "%s: writing needs both chroma planes", who);
    WAN_REQUIRE((p->sub_x == 0 || p->sub_x == 1) && (p->sub_y == 0 || p->sub_y == 1) && (p->cosited == 0 || p->cosited == 1) &&
                (p->c_step == 1 || p->c_step == 2), WAN_ERR_INVALID, "%s: sub_x=%d sub_y=%d cosited=%d (0 or 1), c_step=%d (1 or 2)", who,
                p->sub_x, p->sub_y, p->cosited, p->c_step);
    WAN_REQUIRE(!writing || p->sub_x == p->sub_y, WAN_ERR_UNSUPPORTED, "%s: writes 4:2:0 or 4:4:4, not sub_x=%d sub_y=%d", who, p->sub_x, p->sub_y);
    a.Cw = p->sub_x ? (W + 1) / 2 : W;
    a.Ch = p->sub_y ? (H + 1) / 2 : H;
    const struct { const char* name; const void* base; int64_t extent, row, frame; int rows, cols, step; } pl[3] = {
        {"Y", p->y, p->y_extent, p->y_row, p->y_frame, H, W, 1},
        {"Cb", p->cb, p->cb_extent, p->c_row, p->c_frame, a.Ch, a.Cw, p->c_step},
        {"Cr", p->cr, p->cr_extent, p->c_row, p->c_frame, a.Ch, a.Cw, p->c_step}};
    span sp[3] = {};
    for (int i = 0; i < (mono ? 1 : 3); ++i) {
        const int64_t row_bytes = (int64_t)(pl[i].cols - 1) * pl[i].step + 1;
        WAN_REQUIRE(pl[i].row >= row_bytes && pl[i].frame >= 0 && pl[i].extent > 0, WAN_ERR_INVALID,
                    "%s: %s plane: row stride %lld for %lld-byte rows, frame stride %lld, extent %lld", who, pl[i].name, (long long)pl[i].row,
                    (long long)row_bytes, (long long)pl[i].frame, (long long)pl[i].extent);
        const __int128 frame_bytes = (__int128)(pl[i].rows - 1) * pl[i].row + row_bytes;
        const __int128 last = (__int128)(T - 1) * pl[i].frame + frame_bytes;
        WAN_REQUIRE(last <= (__int128)pl[i].extent, WAN_ERR_INVALID,
                    "%s: %s plane: %d frames of %d rows (row stride %lld, frame stride %lld) leave its %lld bytes", who, pl[i].name, T,
                    pl[i].rows, (long long)pl[i].row, (long long)pl[i].frame, (long long)pl[i].extent);
        WAN_REQUIRE(!writing || T == 1 || (__int128)pl[i].frame >= frame_bytes, WAN_ERR_INVALID,
                    "%s: %s plane: frame stride %lld is less than a frame (%lld bytes): frames would overwrite each other", who,
                    pl[i].name, (long long)pl[i].frame, (long long)frame_bytes);
        sp[i].lo = (uintptr_t)pl[i].base;
        sp[i].hi = sp[i].lo + (uintptr_t)last;
    }
    if (writing) {
        // per frame the planes may interleave (the .y4m layout does), so only what cannot be right is refused: a chroma plane that
        // starts inside the first luma frame, planar Cb and Cr on the same bytes
        const uintptr_t y_end = sp[0].lo + (uintptr_t)((int64_t)(H - 1) * p->y_row + W);
        WAN_REQUIRE((sp[1].lo < sp[0].lo || sp[1].lo >= y_end) && (sp[2].lo < sp[0].lo || sp[2].lo >= y_end) && sp[1].lo != sp[2].lo,
                    WAN_ERR_INVALID, "%s: the output planes overlap", who);
        WAN_REQUIRE(p->c_step == 1 || sp[1].lo + 1 == sp[2].lo || sp[2].lo + 1 == sp[1].lo ||
                        sp[1].hi <= sp[2].lo || sp[2].hi <= sp[1].lo, WAN_ERR_INVALID,
                    "%s: c_step=2 planes are neither each other's odd bytes nor apart", who);
    }
    a.y = (uint8_t*)p->y; a.cb = (uint8_t*)p->cb; a.cr = (uint8_t*)p->cr;
    a.frames = (uint8_t*)frames;
    a.y_extent = p->y_extent; a.cb_extent = p->cb_extent; a.cr_extent = p->cr_extent;
    a.frames_bytes = (int64_t)T * H * W * 3;
    a.y_row = p->y_row; a.y_frame = p->y_frame; a.c_row = p->c_row; a.c_frame = p->c_frame;
    a.H = H; a.W = W; a.sub_y = p->sub_y; a.cosited = p->cosited;
    for (int i = 0; i < 9; ++i) {
        WAN_REQUIRE(coef->k[i] > -(1 << 23) && coef->k[i] < (1 << 23), WAN_ERR_INVALID, "%s: coefficient %d = %d is no 24-bit integer", who, i,
                    coef->k[i]);
        a.k[i] = coef->k[i];
    }
    WAN_REQUIRE(coef->yo >= 0 && coef->yo <= 255, WAN_ERR_INVALID, "%s: luma offset %d is no byte", who, coef->yo);
    a.yo = coef->yo;
    return WAN_OK;
}

dim3 grid_for(int rows, int W, int T) {
    const int runs = (W + PIX - 1) / PIX;
    return dim3((unsigned)((runs + BX - 1) / BX), (unsigned)((rows + BY - 1) / BY), (unsigned)T);
}

}  // namespace

extern "C" wan_status_t wan_yuv_to_frames_u8(const wan_yuv_planes* planes, const wan_yuv_coef* inverse, void* frames_u8, int T, int H,
                                             int W, void* stream) {
    yuv_args a;
    const wan_status_t st = check_planes("wan_yuv_to_frames_u8", planes, inverse, frames_u8, T, H, W, false, a);
    if (st != WAN_OK) return st;
    const dim3 grid = grid_for(H, W, T), block(BX, BY);
    hipStream_t s = (hipStream_t)stream;
    if (planes->sub_x) {
        if (planes->c_step == 1) hipLaunchKernelGGL((yuv_to_frames_kernel<1, 1>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((yuv_to_frames_kernel<1, 2>), grid, block, 0, s, a);
    } else {
        if (planes->c_step == 1) hipLaunchKernelGGL((yuv_to_frames_kernel<0, 1>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((yuv_to_frames_kernel<0, 2>), grid, block, 0, s, a);
    }
    WAN_CHECK_LAUNCH("wan_yuv_to_frames_u8");
    return WAN_OK;
}

extern "C" wan_status_t wan_frames_u8_to_yuv(const void* frames_u8, const wan_yuv_planes* planes, const wan_yuv_coef* forward, int T, int H,
                                             int W, void* stream) {
    yuv_args a;
    const wan_status_t st = check_planes("wan_frames_u8_to_yuv", planes, forward, frames_u8, T, H, W, true, a);
    if (st != WAN_OK) return st;
    const dim3 grid = grid_for(a.Ch, W, T), block(BX, BY);
    hipStream_t s = (hipStream_t)stream;
    if (planes->sub_x) {
        if (planes->c_step == 1) hipLaunchKernelGGL((frames_to_yuv_kernel<1, 1>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((frames_to_yuv_kernel<1, 2>), grid, block, 0, s, a);
    } else {
        if (planes->c_step == 1) hipLaunchKernelGGL((frames_to_yuv_kernel<0, 1>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((frames_to_yuv_kernel<0, 2>), grid, block, 0, s, a);
    }
    WAN_CHECK_LAUNCH("wan_frames_u8_to_yuv");
    return WAN_OK;
}
