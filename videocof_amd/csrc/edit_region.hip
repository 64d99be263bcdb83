// Edit region: run the denoise loop only where the edit mask is.  Three passes, each once per call:
//   wan_mask_bounds      latent-cell weights uint8 [Bm, Fs, h, w] -> per latent frame the inclusive bounds of the non-zero weights
//   wan_region_crop      the sub-box [y0, y0 + hr) x [x0, x0 + wr) of every frame of a contiguous [R, H, W] tensor -> [R, hr, wr]
//   wan_region_restore   the full-frame source block and the region-sized final state -> the full-frame state, in one launch
// and, where the call crops the time axis too (`edit_region_time_margin`: one contiguous range of latent frames, the approximation of
// the temporal context windows, whose first latent frame is not the clip's first either), the same two kernels with a range of frames:
//   wan_region_crop_frames      the sub-box of up to three runs of frames of a contiguous [R, F, H, W] tensor -> [R, Fo, hr, wr]
//   wan_region_restore_frames   the region holds the source frames [t0, t0 + n) only: target frames outside the range are the source
// and, where the box follows the mask from frame to frame (`edit_region_follow`: one size, a corner per latent frame), the frames forms
// with a table of corners in the kernel's arguments, which a workgroup indexes with its frame (a scalar load, like every other argument):
//   wan_region_crop_track       the box of input frame f lies at origins[f]
//   wan_region_restore_track    the box of source frame f (and of grounding and target frame f) lies at origins[f]
// All three are streams of rows at a pitch: the access unit is the widest of 16 / 8 / 4 bytes or one element that divides every length,
// pitch, x origin and base address (region_unit_bytes below: the rule of tile_unit_bytes in window_kernels.hip), so all x arithmetic is
// in whole units and no unit straddles the region's edge.  A workgroup is `rp` rows of `cw` lanes each (cw = min(units per row, 256),
// rp = 256 / cw; lanes beyond rp * cw idle): which frame, which rows and where the region lies are per workgroup (scalar); a lane adds
// its row and unit once.  Nothing is computed on an element: the copies move bits.
#include <algorithm>
#include <initializer_list>

#include "common.hpp"

namespace {

constexpr int UNROLL = 4;                            // rows a lane keeps in flight together

template <int BYTES> struct RawOf;                    // BYTES of memory as one load / store
template <> struct RawOf<16> { typedef u32x4 type; };
template <> struct RawOf<8> { typedef u32x2 type; };
template <> struct RawOf<4> { typedef unsigned int type; };
template <> struct RawOf<2> { typedef unsigned short type; };
template <> struct RawOf<1> { typedef unsigned char type; };

// ------------------------------------------------------------------------------------------------------------- the bounds
// grid (latent frame).  `wu` = w / N units per row.  Every lane keeps its own four extremes over the rows and units it reads, of every
// sample; the waves reduce them with shuffles, the workgroup through 16 words of LDS; lanes 0..3 write one word each.  No atomics, no
// init pass: an empty frame leaves the extremes at their start values (h, -1, w, -1).
template <int N>
__global__ __launch_bounds__(256) void mask_bounds_kernel(int* __restrict__ bounds, const unsigned char* __restrict__ weights, int Bm,
                                                          int Fs, int h, int w, int wu, int cw, int rp) {
    typedef typename RawOf<N>::type U;
    struct Bytes { unsigned char a[N]; };
    __shared__ int red[4][4];
    const int f = blockIdx.x;                         // < Fs
    const int lr = threadIdx.x / cw, lu = threadIdx.x % cw;
    int lo_y = h, hi_y = -1, lo_x = w, hi_x = -1;
    if (lr < rp) {
        for (int b = 0; b < Bm; ++b) {
            const U* frame = (const U*)(weights + ((int64_t)b * Fs + f) * h * w);      // Bm * Fs * h * w < 2^31 (checked by the host)
            for (int r0 = 0; r0 < h; r0 += UNROLL * rp)
                for (int u = lu; u < wu; u += cw) {   // one pass unless a row is longer than 256 units
                    U v[UNROLL];                      // UNROLL independent loads in flight per lane, then the comparisons
#pragma unroll
                    for (int j = 0; j < UNROLL; ++j) {
                        const int y = r0 + j * rp + lr;
                        if (y < h) v[j] = frame[(int64_t)y * wu + u];
                    }
#pragma unroll
                    for (int j = 0; j < UNROLL; ++j) {
                        const int y = r0 + j * rp + lr;
                        if (y >= h) continue;
                        const Bytes a = __builtin_bit_cast(Bytes, v[j]);
#pragma unroll
                        for (int i = 0; i < N; ++i)
                            if (a.a[i] != 0) {
                                const int x = u * N + i;
                                lo_y = min(lo_y, y); hi_y = max(hi_y, y); lo_x = min(lo_x, x); hi_x = max(hi_x, x);
                            }
                    }
                }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo_y = min(lo_y, __shfl_xor(lo_y, o, 64)); hi_y = max(hi_y, __shfl_xor(hi_y, o, 64));
        lo_x = min(lo_x, __shfl_xor(lo_x, o, 64)); hi_x = max(hi_x, __shfl_xor(hi_x, o, 64));
    }
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wid][0] = lo_y; red[wid][1] = hi_y; red[wid][2] = lo_x; red[wid][3] = hi_x; }
    __syncthreads();
    if (threadIdx.x < 4) {                            // word 0 and 2: a minimum; 1 and 3: a maximum
        const int t = threadIdx.x;
        int r = red[0][t];
#pragma unroll
        for (int k = 1; k < 4; ++k) r = (t & 1) ? max(r, red[k][t]) : min(r, red[k][t]);
        bounds[(int64_t)f * 4 + t] = r;
    }
}

// ------------------------------------------------------------------------------------------------------------- the crop
// up to three runs (start, count) of input frames, ascending; an unused run has count 0 and is never reached
struct FrameRuns { int start[3]; int count[3]; };

// grid (sample * Fo + output frame, row chunk); `F` input and `Fo` output frames per sample, `fu` = H * W, `pitch` = W, `ru` = wr,
// `org` = y0 * W + x0, all in units.  Which input frame stands behind an output frame is read off the runs, per workgroup.
template <typename U>
__global__ __launch_bounds__(256) void region_crop_kernel(U* __restrict__ out, const U* __restrict__ in, FrameRuns runs, unsigned Fo,
                                                          int F, int64_t fu, int pitch, int64_t org, int hr, int ru, int cw, int rp) {
    const unsigned row = blockIdx.x;                  // < R * Fo (the grid)
    int k = (int)(row % Fo);                          // < the sum of the counts
    const int64_t sample = row / Fo;
    int f = runs.start[0] + k;
    if (k >= runs.count[0]) {
        k -= runs.count[0];
        f = runs.start[1] + k;
        if (k >= runs.count[1]) f = runs.start[2] + k - runs.count[1];
    }
    const U* src = in + (sample * F + f) * fu + org;  // f < F, and the box lies inside the frame (checked by the host)
    U* dst = out + (int64_t)row * hr * ru;
    const int lr = threadIdx.x / cw, lu = threadIdx.x % cw;
    if (lr >= rp) return;
    for (int r0 = blockIdx.y * UNROLL * rp; r0 < hr; r0 += gridDim.y * UNROLL * rp)
        for (int u = lu; u < ru; u += cw) {           // one pass unless a region row is longer than 256 units
            U v[UNROLL];                              // UNROLL independent loads in flight per lane, then the stores
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int r = r0 + j * rp + lr;
                if (r < hr) v[j] = src[(int64_t)r * pitch + u];
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int r = r0 + j * rp + lr;
                if (r < hr) dst[(int64_t)r * ru + u] = v[j];
            }
        }
}

// ------------------------------------------------------------------------------------------------------------- the restore
// grid (output frame = (b * C + c) * (2 cc + G) + F, row chunk); `wu` = W, `x0u` = x0, `ru` = wr in units.  The region holds the frames
// [source t0 .. t0 + n | grounding | target t0 .. t0 + n].  Which source frame stands behind output frame F, and whether F takes the
// region at all (and from which of its frames), is per workgroup; a lane picks one of two addresses and loads once.
template <typename U>
__global__ __launch_bounds__(256) void region_restore_kernel(U* __restrict__ out, const U* __restrict__ source,
                                                             const U* __restrict__ region, int cc, int G, int t0, int n, int H, int wu,
                                                             int y0, int x0u, int hr, int ru, int cw, int rp) {
    const unsigned Ftot = (unsigned)(2 * cc + G);
    const unsigned row = blockIdx.x;                  // < B * C * Ftot (the grid)
    const int F = (int)(row % Ftot);
    const int64_t bc = row / Ftot;
    const int sf = F < cc ? F : F < cc + G ? F - cc : F - cc - G;       // < cc: G <= cc (checked by the host)
    // grounding frames, and target frames of the range, take the region inside its box: rf is their frame there (< 2 n + G), -1: none
    const int rf = F < cc ? -1 : F < cc + G ? n + (F - cc) : (sf >= t0 && sf < t0 + n) ? n + G + (sf - t0) : -1;
    const bool mixed = rf >= 0;
    const U* s = source + (bc * cc + sf) * H * wu;
    const U* r = region + (bc * (2 * n + G) + (mixed ? rf : 0)) * hr * ru;
    U* o = out + (int64_t)row * H * wu;
    const int lr = threadIdx.x / cw, lu = threadIdx.x % cw;
    if (lr >= rp) return;
    for (int r0 = blockIdx.y * UNROLL * rp; r0 < H; r0 += gridDim.y * UNROLL * rp)
        for (int u = lu; u < wu; u += cw) {           // one pass unless a row is longer than 256 units
            U v[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int y = r0 + j * rp + lr;
                if (y >= H) continue;
                const bool inside = mixed && y >= y0 && y < y0 + hr && u >= x0u && u < x0u + ru;
                const U* p = inside ? r + (int64_t)(y - y0) * ru + (u - x0u) : s + (int64_t)y * wu + u;
                v[j] = *p;
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int y = r0 + j * rp + lr;
                if (y < H) o[(int64_t)y * wu + u] = v[j];
            }
        }
}

// ------------------------------------------------------------------------------------------------------------- the box that follows
// the corners of up to WAN_REGION_TRACK_MAX_FRAMES frames, by value in the kernel's arguments: y0 in the high half, x0 in the low half
// (both < 2^16, checked by the host).  Indexed with the workgroup's frame only, so the read is one scalar load of the argument segment.
struct TrackTable { unsigned at[WAN_REGION_TRACK_MAX_FRAMES]; };

// region_crop_kernel with the box of input frame f at origins.at[f]; `xs` = log2 of the elements per unit (every x0 is whole units)
template <typename U>
__global__ __launch_bounds__(256) void region_crop_track_kernel(U* __restrict__ out, const U* __restrict__ in, FrameRuns runs,
                                                                TrackTable origins, unsigned Fo, int F, int64_t fu, int pitch, int xs,
                                                                int hr, int ru, int cw, int rp) {
    const unsigned row = blockIdx.x;                  // < R * Fo (the grid)
    int k = (int)(row % Fo);                          // < the sum of the counts
    const int64_t sample = row / Fo;
    int f = runs.start[0] + k;
    if (k >= runs.count[0]) {
        k -= runs.count[0];
        f = runs.start[1] + k;
        if (k >= runs.count[1]) f = runs.start[2] + k - runs.count[1];
    }
    const unsigned at = origins.at[f];                // f < F <= WAN_REGION_TRACK_MAX_FRAMES, and every box lies inside the frame (host)
    const int64_t org = (int64_t)(at >> 16) * pitch + ((at & 0xffffu) >> xs);
    const U* src = in + (sample * F + f) * fu + org;
    U* dst = out + (int64_t)row * hr * ru;
    const int lr = threadIdx.x / cw, lu = threadIdx.x % cw;
    if (lr >= rp) return;
    for (int r0 = blockIdx.y * UNROLL * rp; r0 < hr; r0 += gridDim.y * UNROLL * rp)
        for (int u = lu; u < ru; u += cw) {           // one pass unless a region row is longer than 256 units
            U v[UNROLL];                              // UNROLL independent loads in flight per lane, then the stores
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int r = r0 + j * rp + lr;
                if (r < hr) v[j] = src[(int64_t)r * pitch + u];
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int r = r0 + j * rp + lr;
                if (r < hr) dst[(int64_t)r * ru + u] = v[j];
            }
        }
}

// region_restore_kernel with the box of source frame sf at origins.at[sf]
template <typename U>
__global__ __launch_bounds__(256) void region_restore_track_kernel(U* __restrict__ out, const U* __restrict__ source,
                                                                   const U* __restrict__ region, TrackTable origins, int cc, int G,
                                                                   int t0, int n, int H, int wu, int xs, int hr, int ru, int cw,
                                                                   int rp) {
    const unsigned Ftot = (unsigned)(2 * cc + G);
    const unsigned row = blockIdx.x;                  // < B * C * Ftot (the grid)
    const int F = (int)(row % Ftot);
    const int64_t bc = row / Ftot;
    const int sf = F < cc ? F : F < cc + G ? F - cc : F - cc - G;       // < cc <= WAN_REGION_TRACK_MAX_FRAMES: G <= cc (checked by the host)
    const int rf = F < cc ? -1 : F < cc + G ? n + (F - cc) : (sf >= t0 && sf < t0 + n) ? n + G + (sf - t0) : -1;
    const bool mixed = rf >= 0;
    const unsigned at = origins.at[sf];
    const int y0 = (int)(at >> 16), x0u = (int)((at & 0xffffu) >> xs);
    const U* s = source + (bc * cc + sf) * H * wu;
    const U* r = region + (bc * (2 * n + G) + (mixed ? rf : 0)) * hr * ru;
    U* o = out + (int64_t)row * H * wu;
    const int lr = threadIdx.x / cw, lu = threadIdx.x % cw;
    if (lr >= rp) return;
    for (int r0 = blockIdx.y * UNROLL * rp; r0 < H; r0 += gridDim.y * UNROLL * rp)
        for (int u = lu; u < wu; u += cw) {           // one pass unless a row is longer than 256 units
            U v[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int y = r0 + j * rp + lr;
                if (y >= H) continue;
                const bool inside = mixed && y >= y0 && y < y0 + hr && u >= x0u && u < x0u + ru;
                const U* p = inside ? r + (int64_t)(y - y0) * ru + (u - x0u) : s + (int64_t)y * wu + u;
                v[j] = *p;
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int y = r0 + j * rp + lr;
                if (y < H) o[(int64_t)y * wu + u] = v[j];
            }
        }
}

// ------------------------------------------------------------------------------------------------------------- the spans
// grid (latent frame), four waves.  Two passes over the frame, `wu` = w / N units per row; a pair (lo, hi) of int16 is one 32-bit word
// (lo in the low half), and every word is written exactly once: no atomics, no init pass.
//   rows      a wave takes UNROLL rows at a time, its lanes the units of those rows of every sample; the 64 lanes reduce with shuffles and
//             lane 0 writes the rows' words
//   columns   the lanes are `rp` rows of `cw` units as in the bounds kernel; a lane keeps the extremes of the N columns of its unit over
//             the rows it reads; where rp > 1 (a row of at most 128 units: one pass) the rp partial results meet in LDS and the lanes of
//             the first row write; where rp == 1 every lane writes its own columns, pass by pass
inline __device__ unsigned span_word(int lo, int hi) { return ((unsigned)hi << 16) | ((unsigned)lo & 0xffffu); }

template <int N>
__global__ __launch_bounds__(256) void mask_spans_kernel(unsigned* __restrict__ spans, const unsigned char* __restrict__ weights, int Bm,
                                                         int Fs, int h, int w, int wu, int cw, int rp) {
    typedef typename RawOf<N>::type U;
    struct Bytes { unsigned char a[N]; };
    __shared__ short part_lo[256 * N], part_hi[256 * N];
    const int f = blockIdx.x;                         // < Fs
    const int64_t hw = (int64_t)h * w;                // Bm * Fs * h * w < 2^31 (checked by the host)
    unsigned* out = spans + (int64_t)f * (h + w);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int y0 = wid * UNROLL; y0 < h; y0 += 4 * UNROLL) {
        int lo[UNROLL], hi[UNROLL];
#pragma unroll
        for (int j = 0; j < UNROLL; ++j) { lo[j] = w; hi[j] = -1; }
        for (int b = 0; b < Bm; ++b) {
            const U* frame = (const U*)(weights + ((int64_t)b * Fs + f) * hw);
            for (int u = lane; u < wu; u += 64) {
                U v[UNROLL];
#pragma unroll
                for (int j = 0; j < UNROLL; ++j)
                    if (y0 + j < h) v[j] = frame[(int64_t)(y0 + j) * wu + u];
#pragma unroll
                for (int j = 0; j < UNROLL; ++j) {
                    if (y0 + j >= h) continue;
                    const Bytes a = __builtin_bit_cast(Bytes, v[j]);
#pragma unroll
                    for (int i = 0; i < N; ++i)
                        if (a.a[i] != 0) { lo[j] = min(lo[j], u * N + i); hi[j] = max(hi[j], u * N + i); }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < UNROLL; ++j) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo[j] = min(lo[j], __shfl_xor(lo[j], o, 64)); hi[j] = max(hi[j], __shfl_xor(hi[j], o, 64));
            }
            if (lane == 0 && y0 + j < h) out[y0 + j] = span_word(lo[j], hi[j]);
        }
    }
    const int lr = threadIdx.x / cw, lu = threadIdx.x % cw;
    for (int u0 = 0; u0 < wu; u0 += cw) {             // one pass unless a row is longer than 256 units (then rp == 1)
        const int u = u0 + lu;
        int lo[N], hi[N];
#pragma unroll
        for (int i = 0; i < N; ++i) { lo[i] = h; hi[i] = -1; }
        if (lr < rp && u < wu)
            for (int b = 0; b < Bm; ++b) {
                const U* frame = (const U*)(weights + ((int64_t)b * Fs + f) * hw);
                for (int r0 = 0; r0 < h; r0 += UNROLL * rp) {
                    U v[UNROLL];
#pragma unroll
                    for (int j = 0; j < UNROLL; ++j) {
                        const int y = r0 + j * rp + lr;
                        if (y < h) v[j] = frame[(int64_t)y * wu + u];
                    }
#pragma unroll
                    for (int j = 0; j < UNROLL; ++j) {
                        const int y = r0 + j * rp + lr;
                        if (y >= h) continue;
                        const Bytes a = __builtin_bit_cast(Bytes, v[j]);
#pragma unroll
                        for (int i = 0; i < N; ++i)
                            if (a.a[i] != 0) { lo[i] = min(lo[i], y); hi[i] = max(hi[i], y); }
                    }
                }
            }
        if (rp > 1) {                                 // uniform: cw == wu, this is the only pass
#pragma unroll
            for (int i = 0; i < N; ++i) { part_lo[threadIdx.x * N + i] = (short)lo[i]; part_hi[threadIdx.x * N + i] = (short)hi[i]; }
            __syncthreads();
            if (lr == 0)
                for (int k = 1; k < rp; ++k)
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        lo[i] = min(lo[i], (int)part_lo[(k * cw + lu) * N + i]); hi[i] = max(hi[i], (int)part_hi[(k * cw + lu) * N + i]);
                    }
        }
        if (lr == 0 && u < wu)
#pragma unroll
            for (int i = 0; i < N; ++i) out[h + u * N + i] = span_word(lo[i], hi[i]);
    }
}

// ------------------------------------------------------------------------------------------------------------- the split
// the boxes of up to WAN_REGION_SPLIT_MAX bands, by value in the kernel's arguments: the corner of box k and the interval [lo, hi) of
// the cut axis that band k owns (columns where `axis` is 1, rows where it is 0), all in elements.  The intervals tile the axis (host).
struct SplitTable { int y0[WAN_REGION_SPLIT_MAX], x0[WAN_REGION_SPLIT_MAX], lo[WAN_REGION_SPLIT_MAX], hi[WAN_REGION_SPLIT_MAX]; };

// region_crop_kernel for every box in one launch: grid ((box * R + sample) * Fo + output frame, row chunk); the workgroup indexes the
// table with its box (scalar).  `clip`: what lies outside the owned interval is written as zero, not read.
template <typename U>
__global__ __launch_bounds__(256) void region_crop_split_kernel(U* __restrict__ out, const U* __restrict__ in, FrameRuns runs,
                                                                SplitTable boxes, unsigned Fo, unsigned RFo, int F, int64_t fu,
                                                                int pitch, int xs, int axis, int clip, int hr, int ru, int cw, int rp) {
    const unsigned row = blockIdx.x;                  // < K * R * Fo (the grid)
    const unsigned box = row / RFo, rest = row % RFo; // box < K <= WAN_REGION_SPLIT_MAX
    int k = (int)(rest % Fo);
    const int64_t sample = rest / Fo;
    int f = runs.start[0] + k;
    if (k >= runs.count[0]) {
        k -= runs.count[0];
        f = runs.start[1] + k;
        if (k >= runs.count[1]) f = runs.start[2] + k - runs.count[1];
    }
    const int y0 = boxes.y0[box], x0u = boxes.x0[box] >> xs;         // every box lies inside the frame (checked by the host)
    int keep_y0 = 0, keep_y1 = hr, keep_u0 = 0, keep_u1 = ru;        // what of the box is kept, in its own rows and units
    if (clip) {
        if (axis) { keep_u0 = max(0, (boxes.lo[box] >> xs) - x0u); keep_u1 = min(ru, (boxes.hi[box] >> xs) - x0u); }
        else { keep_y0 = max(0, boxes.lo[box] - y0); keep_y1 = min(hr, boxes.hi[box] - y0); }
    }
    const U* src = in + (sample * F + f) * fu + (int64_t)y0 * pitch + x0u;
    U* dst = out + (int64_t)row * hr * ru;
    const int lr = threadIdx.x / cw, lu = threadIdx.x % cw;
    if (lr >= rp) return;
    for (int r0 = blockIdx.y * UNROLL * rp; r0 < hr; r0 += gridDim.y * UNROLL * rp)
        for (int u = lu; u < ru; u += cw) {           // one pass unless a region row is longer than 256 units
            U v[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int r = r0 + j * rp + lr;
                if (r >= hr) continue;
                if (r >= keep_y0 && r < keep_y1 && u >= keep_u0 && u < keep_u1) v[j] = src[(int64_t)r * pitch + u];
                else v[j] = U();
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int r = r0 + j * rp + lr;
                if (r < hr) dst[(int64_t)r * ru + u] = v[j];
            }
        }
}

// region_restore_kernel with K boxes: the band that owns a unit is found on the cut axis (the intervals tile it, so exactly one does),
// and the unit takes that band's box where it lies inside it.  The table is read with the loop's counter only (scalar); a lane selects.
// `BC` = B * C: the region is box-major, [K, B, C, n + G + n, hr, ru].
template <typename U>
__global__ __launch_bounds__(256) void region_restore_split_kernel(U* __restrict__ out, const U* __restrict__ source,
                                                                   const U* __restrict__ region, SplitTable boxes, int K, int axis,
                                                                   int64_t BC, int cc, int G, int t0, int n, int H, int wu, int xs,
                                                                   int hr, int ru, int cw, int rp) {
    const unsigned Ftot = (unsigned)(2 * cc + G);
    const unsigned row = blockIdx.x;                  // < B * C * Ftot (the grid)
    const int F = (int)(row % Ftot);
    const int64_t bc = row / Ftot;
    const int sf = F < cc ? F : F < cc + G ? F - cc : F - cc - G;       // < cc: G <= cc (checked by the host)
    const int rf = F < cc ? -1 : F < cc + G ? n + (F - cc) : (sf >= t0 && sf < t0 + n) ? n + G + (sf - t0) : -1;
    const bool mixed = rf >= 0;
    const int64_t ru_frame = (int64_t)hr * ru, frames = 2 * n + G;
    const U* s = source + (bc * cc + sf) * H * wu;
    U* o = out + (int64_t)row * H * wu;
    const int lr = threadIdx.x / cw, lu = threadIdx.x % cw;
    if (lr >= rp) return;
    for (int r0 = blockIdx.y * UNROLL * rp; r0 < H; r0 += gridDim.y * UNROLL * rp)
        for (int u = lu; u < wu; u += cw) {           // one pass unless a row is longer than 256 units
            U v[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int y = r0 + j * rp + lr;
                if (y >= H) continue;
                const U* p = s + (int64_t)y * wu + u;
                if (mixed)
                    for (int k = 0; k < K; ++k) {     // K <= WAN_REGION_SPLIT_MAX, uniform
                        const int at = axis ? u : y, lo = axis ? boxes.lo[k] >> xs : boxes.lo[k], hi = axis ? boxes.hi[k] >> xs : boxes.hi[k];
                        const int y0 = boxes.y0[k], x0u = boxes.x0[k] >> xs;
                        if (at >= lo && at < hi && y >= y0 && y < y0 + hr && u >= x0u && u < x0u + ru)
                            p = region + ((k * BC + bc) * frames + rf) * ru_frame + (int64_t)(y - y0) * ru + (u - x0u);
                    }
                v[j] = *p;
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int y = r0 + j * rp + lr;
                if (y < H) o[(int64_t)y * wu + u] = v[j];
            }
        }
}

// the largest of 16, 8, 4 bytes or one element that divides (in bytes) every length in `lens` (elements) and every address: a power of
// two divides them all exactly when it divides their bitwise OR
int region_unit_bytes(int64_t es, std::initializer_list<int64_t> lens, uintptr_t addresses) {
    uint64_t m = (uint64_t)addresses;
    for (int64_t l : lens) m |= (uint64_t)(l * es);
    int ub = 16;
    while (ub > es && (m & (uint64_t)(ub - 1)) != 0) ub /= 2;
    return ub;
}

// workgroups along the rows: <= ~4096 in all, at most what the grid's second axis holds; the rest is a grid-stride loop
unsigned row_chunks(int rows, int per_group, int64_t frames) {
    const int64_t need = ((int64_t)rows + per_group - 1) / per_group;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(need, 65535), 4096 / frames));
}

bool box_ok(int H, int W, int y0, int x0, int hr, int wr) {
    return H >= 1 && W >= 1 && y0 >= 0 && x0 >= 0 && hr >= 1 && wr >= 1 && (int64_t)y0 + hr <= H && (int64_t)x0 + wr <= W;
}

}  // namespace

extern "C" wan_status_t wan_mask_bounds(const void* weights_u8, void* bounds_i32, int Bm, int Fs, int h, int w, void* stream) {
    WAN_REQUIRE(weights_u8 && bounds_i32, WAN_ERR_INVALID, "wan_mask_bounds: null tensor");
    WAN_REQUIRE(Bm >= 1 && Fs >= 1 && h >= 1 && w >= 1, WAN_ERR_INVALID, "wan_mask_bounds: Bm=%d Fs=%d h=%d w=%d", Bm, Fs, h, w);
    WAN_REQUIRE((int64_t)Bm * Fs * h * w <= 0x7fffffff, WAN_ERR_INVALID, "wan_mask_bounds: %lld weights (at most 2^31 - 1)",
                (long long)((int64_t)Bm * Fs * h * w));
    WAN_REQUIRE(((uintptr_t)bounds_i32 & 3) == 0, WAN_ERR_INVALID, "wan_mask_bounds: bounds are int32 words; the address is not a multiple of 4");
    const int N = region_unit_bytes(1, {w}, (uintptr_t)weights_u8);
    const int wu = w / N, cw = std::min(wu, 256), rp = 256 / cw;
    hipStream_t s = (hipStream_t)stream;
#define WAN_BOUNDS(N_)                                                                                                        \
    hipLaunchKernelGGL(mask_bounds_kernel<N_>, dim3((unsigned)Fs), dim3(256), 0, s, (int*)bounds_i32,                          \
                       (const unsigned char*)weights_u8, Bm, Fs, h, w, wu, cw, rp)
    if (N == 16) WAN_BOUNDS(16); else if (N == 8) WAN_BOUNDS(8); else if (N == 4) WAN_BOUNDS(4); else if (N == 2) WAN_BOUNDS(2);
    else WAN_BOUNDS(1);
#undef WAN_BOUNDS
    WAN_CHECK_LAUNCH("wan_mask_bounds");
    return WAN_OK;
}

#define WAN_BY_UNIT(ub, LAUNCH)                                          \
    do {                                                                 \
        if ((ub) == 16) LAUNCH(u32x4);                                   \
        else if ((ub) == 8) LAUNCH(u32x2);                               \
        else if ((ub) == 4) LAUNCH(unsigned int);                        \
        else if ((ub) == 2) LAUNCH(unsigned short);                      \
        else LAUNCH(unsigned char);                                      \
    } while (0)

// the crop behind both of its entry points (`who` names the one called in the messages)
static wan_status_t crop_frames(const char* who, void* out, const void* in, int elem_bytes, int64_t R, int F, int H, int W,
                                const int* runs, int n_runs, int y0, int x0, int hr, int wr, void* stream) {
    // (the box and the runs first: an empty region's or an empty range's output is an empty tensor, whose address is null)
    WAN_REQUIRE(R >= 1 && F >= 1 && box_ok(H, W, y0, x0, hr, wr), WAN_ERR_INVALID,
                "%s: the region [%d, %d + %d) x [%d, %d + %d) does not lie inside %lld x %d frames of %d x %d", who, y0, y0, hr, x0, x0, wr,
                (long long)R, F, H, W);
    WAN_REQUIRE(runs && n_runs >= 1 && n_runs <= 3, WAN_ERR_INVALID, "%s: %d runs of frames at %p (1 to 3, not null)", who, n_runs,
                (const void*)runs);
    FrameRuns fr = {{0, 0, 0}, {0, 0, 0}};
    int64_t Fo = 0;
    for (int i = 0, end = 0; i < n_runs; ++i) {
        const int start = runs[2 * i], count = runs[2 * i + 1];
        WAN_REQUIRE(start >= end && count >= 1 && (int64_t)start + count <= F, WAN_ERR_INVALID,
                    "%s: run %d = frames [%d, %d + %d) of %d (ascending, not overlapping, at least one frame each, inside the clip)", who, i,
                    start, start, count, F);
        fr.start[i] = start; fr.count[i] = count;
        end = start + count;
        Fo += count;
    }
    WAN_REQUIRE(out && in, WAN_ERR_INVALID, "%s: null tensor", who);
    WAN_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, WAN_ERR_INVALID, "%s: elements of %d bytes (1, 2 or 4)", who,
                elem_bytes);
    WAN_REQUIRE(R <= 0x7fffffff && R * F <= 0x7fffffff && (int64_t)H * W <= 0x7fffffff, WAN_ERR_INVALID,
                "%s: %lld clips of %d frames of %lld elements (frames in all and elements a frame: each at most 2^31 - 1)", who,
                (long long)R, F, (long long)((int64_t)H * W));
    const int64_t es = elem_bytes, frames = R * Fo;
    const int ub = region_unit_bytes(es, {W, wr, x0}, (uintptr_t)out | (uintptr_t)in);
    const int N = (int)(ub / es), ru = wr / N, cw = std::min(ru, 256), rp = 256 / cw;
    const dim3 grid((unsigned)frames, row_chunks(hr, UNROLL * rp, frames));
    hipStream_t s = (hipStream_t)stream;
#define WAN_CROP(U)                                                                                                            \
    hipLaunchKernelGGL(region_crop_kernel<U>, grid, dim3(256), 0, s, (U*)out, (const U*)in, fr, (unsigned)Fo, F,               \
                       (int64_t)H * W / N, W / N, ((int64_t)y0 * W + x0) / N, hr, ru, cw, rp)
    WAN_BY_UNIT(ub, WAN_CROP);
#undef WAN_CROP
    WAN_CHECK_LAUNCH(who);
    return WAN_OK;
}

extern "C" wan_status_t wan_region_crop(void* out, const void* in, int elem_bytes, int64_t R, int H, int W, int y0, int x0, int hr,
                                        int wr, void* stream) {
    const int every[2] = {0, 1};                      // R clips of one frame each, every one kept
    return crop_frames("wan_region_crop", out, in, elem_bytes, R, 1, H, W, every, 1, y0, x0, hr, wr, stream);
}

extern "C" wan_status_t wan_region_crop_frames(void* out, const void* in, int elem_bytes, int64_t R, int F, int H, int W,
                                               const int* runs, int n_runs, int y0, int x0, int hr, int wr, void* stream) {
    return crop_frames("wan_region_crop_frames", out, in, elem_bytes, R, F, H, W, runs, n_runs, y0, x0, hr, wr, stream);
}

// the restore behind both of its entry points
static wan_status_t restore_frames(const char* who, void* out, const void* source, const void* region, int elem_bytes, int B, int C,
                                   int cc, int G, int H, int W, int t0, int n, int y0, int x0, int hr, int wr, void* stream) {
    WAN_REQUIRE(out && source && region, WAN_ERR_INVALID, "%s: null tensor", who);
    WAN_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, WAN_ERR_INVALID, "%s: elements of %d bytes (1, 2 or 4)", who,
                elem_bytes);
    WAN_REQUIRE(B >= 1 && C >= 1 && cc >= 1, WAN_ERR_INVALID, "%s: B=%d C=%d cc=%d", who, B, C, cc);
    WAN_REQUIRE(0 <= G && G <= cc, WAN_ERR_INVALID,
                "%s: G=%d grounding frames for cc=%d source frames (grounding frame g takes source frame g outside the region: "
                "0 <= G <= cc)", who, G, cc);
    WAN_REQUIRE(t0 >= 0 && n >= 1 && (int64_t)t0 + n <= cc, WAN_ERR_INVALID,
                "%s: the frames [%d, %d + %d) do not lie inside the %d source frames", who, t0, t0, n, cc);
    WAN_REQUIRE(box_ok(H, W, y0, x0, hr, wr), WAN_ERR_INVALID,
                "%s: the region [%d, %d + %d) x [%d, %d + %d) does not lie inside a frame of %d x %d", who, y0, y0, hr, x0, x0, wr, H, W);
    const int64_t frames = (int64_t)B * C * (2 * (int64_t)cc + G);
    WAN_REQUIRE(frames <= 0x7fffffff && (int64_t)H * W <= 0x7fffffff, WAN_ERR_INVALID,
                "%s: %lld frames of %lld elements (each at most 2^31 - 1)", who, (long long)frames, (long long)((int64_t)H * W));
    const int64_t es = elem_bytes;
    const int ub = region_unit_bytes(es, {W, wr, x0}, (uintptr_t)out | (uintptr_t)source | (uintptr_t)region);
    const int N = (int)(ub / es), wu = W / N, cw = std::min(wu, 256), rp = 256 / cw;
    const dim3 grid((unsigned)frames, row_chunks(H, UNROLL * rp, frames));
    hipStream_t s = (hipStream_t)stream;
#define WAN_RESTORE(U)                                                                                                         \
    hipLaunchKernelGGL(region_restore_kernel<U>, grid, dim3(256), 0, s, (U*)out, (const U*)source, (const U*)region, cc, G, t0, n, H, \
                       wu, y0, x0 / N, hr, wr / N, cw, rp)
    WAN_BY_UNIT(ub, WAN_RESTORE);
#undef WAN_RESTORE
    WAN_CHECK_LAUNCH(who);
    return WAN_OK;
}

extern "C" wan_status_t wan_region_restore(void* out, const void* source, const void* region, int elem_bytes, int B, int C, int cc,
                                           int G, int H, int W, int y0, int x0, int hr, int wr, void* stream) {
    return restore_frames("wan_region_restore", out, source, region, elem_bytes, B, C, cc, G, H, W, 0, cc, y0, x0, hr, wr, stream);
}

extern "C" wan_status_t wan_region_restore_frames(void* out, const void* source, const void* region, int elem_bytes, int B, int C,
                                                  int cc, int G, int H, int W, int t0, int n, int y0, int x0, int hr, int wr,
                                                  void* stream) {
    return restore_frames("wan_region_restore_frames", out, source, region, elem_bytes, B, C, cc, G, H, W, t0, n, y0, x0, hr, wr, stream);
}

// the table of corners, checked and packed: every one of the `frames` boxes of hr x wr lies inside the H x W frame.  `x_or` takes the
// bitwise OR of the x0 (the access unit must divide every one of them).
static wan_status_t pack_origins(const char* who, TrackTable* table, int64_t* x_or, const int* origins, int frames, int H, int W, int hr,
                                 int wr) {
    WAN_REQUIRE(origins, WAN_ERR_INVALID, "%s: null origins", who);
    WAN_REQUIRE(frames >= 1 && frames <= WAN_REGION_TRACK_MAX_FRAMES, WAN_ERR_INVALID,
                "%s: a table of %d frames (1 to %d: it travels in the kernel's arguments)", who, frames, WAN_REGION_TRACK_MAX_FRAMES);
    *x_or = 0;
    for (int f = 0; f < frames; ++f) {
        const int y0 = origins[2 * f], x0 = origins[2 * f + 1];
        WAN_REQUIRE(box_ok(H, W, y0, x0, hr, wr) && y0 <= 0xffff && x0 <= 0xffff, WAN_ERR_INVALID,
                    "%s: frame %d: the region [%d, %d + %d) x [%d, %d + %d) does not lie inside a frame of %d x %d (corners below 65536)",
                    who, f, y0, y0, hr, x0, x0, wr, H, W);
        table->at[f] = ((unsigned)y0 << 16) | (unsigned)x0;
        *x_or |= x0;
    }
    for (int f = frames; f < WAN_REGION_TRACK_MAX_FRAMES; ++f) table->at[f] = 0;
    return WAN_OK;
}

static int log2_of(int n) {                           // n = 1, 2, 4, 8 or 16
    int s = 0;
    while ((1 << s) < n) ++s;
    return s;
}

extern "C" wan_status_t wan_region_crop_track(void* out, const void* in, int elem_bytes, int64_t R, int F, int H, int W, const int* runs,
                                              int n_runs, const int* origins, int hr, int wr, void* stream) {
    const char* who = "wan_region_crop_track";
    // (the boxes and the runs first, as in crop_frames: an empty region's output is an empty tensor, whose address is null)
    WAN_REQUIRE(R >= 1 && F >= 1 && H >= 1 && W >= 1 && hr >= 1 && wr >= 1 && hr <= H && wr <= W, WAN_ERR_INVALID,
                "%s: a region of %d x %d in %lld x %d frames of %d x %d", who, hr, wr, (long long)R, F, H, W);
    TrackTable table;
    int64_t x_or = 0;
    const wan_status_t st = pack_origins(who, &table, &x_or, origins, F, H, W, hr, wr);
    if (st != WAN_OK) return st;
    WAN_REQUIRE(runs && n_runs >= 1 && n_runs <= 3, WAN_ERR_INVALID, "%s: %d runs of frames at %p (1 to 3, not null)", who, n_runs,
                (const void*)runs);
    FrameRuns fr = {{0, 0, 0}, {0, 0, 0}};
    int64_t Fo = 0;
    for (int i = 0, end = 0; i < n_runs; ++i) {
        const int start = runs[2 * i], count = runs[2 * i + 1];
        WAN_REQUIRE(start >= end && count >= 1 && (int64_t)start + count <= F, WAN_ERR_INVALID,
                    "%s: run %d = frames [%d, %d + %d) of %d (ascending, not overlapping, at least one frame each, inside the clip)", who, i,
                    start, start, count, F);
        fr.start[i] = start; fr.count[i] = count;
        end = start + count;
        Fo += count;
    }
    WAN_REQUIRE(out && in, WAN_ERR_INVALID, "%s: null tensor", who);
    WAN_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, WAN_ERR_INVALID, "%s: elements of %d bytes (1, 2 or 4)", who,
                elem_bytes);
    WAN_REQUIRE(R <= 0x7fffffff && R * F <= 0x7fffffff && (int64_t)H * W <= 0x7fffffff, WAN_ERR_INVALID,
                "%s: %lld clips of %d frames of %lld elements (frames in all and elements a frame: each at most 2^31 - 1)", who,
                (long long)R, F, (long long)((int64_t)H * W));
    const int64_t es = elem_bytes, frames = R * Fo;
    const int ub = region_unit_bytes(es, {W, wr, x_or}, (uintptr_t)out | (uintptr_t)in);
    const int N = (int)(ub / es), ru = wr / N, cw = std::min(ru, 256), rp = 256 / cw;
    const dim3 grid((unsigned)frames, row_chunks(hr, UNROLL * rp, frames));
    hipStream_t s = (hipStream_t)stream;
#define WAN_CROP_TRACK(U)                                                                                                      \
    hipLaunchKernelGGL(region_crop_track_kernel<U>, grid, dim3(256), 0, s, (U*)out, (const U*)in, fr, table, (unsigned)Fo, F,  \
                       (int64_t)H * W / N, W / N, log2_of(N), hr, ru, cw, rp)
    WAN_BY_UNIT(ub, WAN_CROP_TRACK);
#undef WAN_CROP_TRACK
    WAN_CHECK_LAUNCH(who);
    return WAN_OK;
}

extern "C" wan_status_t wan_region_restore_track(void* out, const void* source, const void* region, int elem_bytes, int B, int C, int cc,
                                                 int G, int H, int W, int t0, int n, const int* origins, int hr, int wr, void* stream) {
    const char* who = "wan_region_restore_track";
    WAN_REQUIRE(out && source && region, WAN_ERR_INVALID, "%s: null tensor", who);
    WAN_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, WAN_ERR_INVALID, "%s: elements of %d bytes (1, 2 or 4)", who,
                elem_bytes);
    WAN_REQUIRE(B >= 1 && C >= 1 && cc >= 1, WAN_ERR_INVALID, "%s: B=%d C=%d cc=%d", who, B, C, cc);
    WAN_REQUIRE(0 <= G && G <= cc, WAN_ERR_INVALID,
                "%s: G=%d grounding frames for cc=%d source frames (grounding frame g takes source frame g outside the region: "
                "0 <= G <= cc)", who, G, cc);
    WAN_REQUIRE(t0 >= 0 && n >= 1 && (int64_t)t0 + n <= cc, WAN_ERR_INVALID,
                "%s: the frames [%d, %d + %d) do not lie inside the %d source frames", who, t0, t0, n, cc);
    WAN_REQUIRE(H >= 1 && W >= 1 && hr >= 1 && wr >= 1 && hr <= H && wr <= W, WAN_ERR_INVALID,
                "%s: a region of %d x %d in a frame of %d x %d", who, hr, wr, H, W);
    TrackTable table;
    int64_t x_or = 0;
    const wan_status_t st = pack_origins(who, &table, &x_or, origins, cc, H, W, hr, wr);
    if (st != WAN_OK) return st;
    const int64_t frames = (int64_t)B * C * (2 * (int64_t)cc + G);
    WAN_REQUIRE(frames <= 0x7fffffff && (int64_t)H * W <= 0x7fffffff, WAN_ERR_INVALID,
                "%s: %lld frames of %lld elements (each at most 2^31 - 1)", who, (long long)frames, (long long)((int64_t)H * W));
    const int64_t es = elem_bytes;
    const int ub = region_unit_bytes(es, {W, wr, x_or}, (uintptr_t)out | (uintptr_t)source | (uintptr_t)region);
    const int N = (int)(ub / es), wu = W / N, cw = std::min(wu, 256), rp = 256 / cw;
    const dim3 grid((unsigned)frames, row_chunks(H, UNROLL * rp, frames));
    hipStream_t s = (hipStream_t)stream;
#define WAN_RESTORE_TRACK(U)                                                                                                   \
    hipLaunchKernelGGL(region_restore_track_kernel<U>, grid, dim3(256), 0, s, (U*)out, (const U*)source, (const U*)region, table, cc, \
                       G, t0, n, H, wu, log2_of(N), hr, wr / N, cw, rp)
    WAN_BY_UNIT(ub, WAN_RESTORE_TRACK);
#undef WAN_RESTORE_TRACK
    WAN_CHECK_LAUNCH(who);
    return WAN_OK;
}

extern "C" wan_status_t wan_mask_spans(const void* weights_u8, void* spans_i16, int Bm, int Fs, int h, int w, void* stream) {
    WAN_REQUIRE(weights_u8 && spans_i16, WAN_ERR_INVALID, "wan_mask_spans: null tensor");
    WAN_REQUIRE(Bm >= 1 && Fs >= 1 && h >= 1 && w >= 1, WAN_ERR_INVALID, "wan_mask_spans: Bm=%d Fs=%d h=%d w=%d", Bm, Fs, h, w);
    WAN_REQUIRE(h < 32768 && w < 32768, WAN_ERR_INVALID, "wan_mask_spans: a frame of %d x %d cells (each below 32768: the spans are int16)",
                h, w);
    WAN_REQUIRE((int64_t)Bm * Fs * h * w <= 0x7fffffff, WAN_ERR_INVALID, "wan_mask_spans: %lld weights (at most 2^31 - 1)",
                (long long)((int64_t)Bm * Fs * h * w));
    WAN_REQUIRE(((uintptr_t)spans_i16 & 3) == 0, WAN_ERR_INVALID,
                "wan_mask_spans: a pair of int16 is written as one word; the address is not a multiple of 4");
    const int N = region_unit_bytes(1, {w}, (uintptr_t)weights_u8);
    const int wu = w / N, cw = std::min(wu, 256), rp = 256 / cw;
    hipStream_t s = (hipStream_t)stream;
#define WAN_SPANS(N_)                                                                                                         \
    hipLaunchKernelGGL(mask_spans_kernel<N_>, dim3((unsigned)Fs), dim3(256), 0, s, (unsigned*)spans_i16,                       \
                       (const unsigned char*)weights_u8, Bm, Fs, h, w, wu, cw, rp)
    if (N == 16) WAN_SPANS(16); else if (N == 8) WAN_SPANS(8); else if (N == 4) WAN_SPANS(4); else if (N == 2) WAN_SPANS(2);
    else WAN_SPANS(1);
#undef WAN_SPANS
    WAN_CHECK_LAUNCH("wan_mask_spans");
    return WAN_OK;
}

// the boxes of a split, checked and laid out: 1 to WAN_REGION_SPLIT_MAX boxes of hr x wr inside the H x W frame; `cuts` ascend strictly
// from 0 to the cut axis' extent, so the owned intervals tile it.  `x_or` takes the bitwise OR of every x0 and, for a column cut, of
// every cut (the access unit must divide them all).
static wan_status_t pack_boxes(const char* who, SplitTable* table, int64_t* x_or, const int* origins, const int* cuts, int K, int axis,
                               int H, int W, int hr, int wr) {
    WAN_REQUIRE(origins && cuts, WAN_ERR_INVALID, "%s: null origins or cuts", who);
    WAN_REQUIRE(K >= 1 && K <= WAN_REGION_SPLIT_MAX, WAN_ERR_INVALID, "%s: %d boxes (1 to %d: their table travels in the kernel's arguments)",
                who, K, WAN_REGION_SPLIT_MAX);
    WAN_REQUIRE(axis == 0 || axis == 1, WAN_ERR_INVALID, "%s: axis=%d (1: the cuts are columns, 0: rows)", who, axis);
    const int extent = axis ? W : H;
    WAN_REQUIRE(cuts[0] == 0 && cuts[K] == extent, WAN_ERR_INVALID, "%s: the cuts run from %d to %d, not from 0 to %d", who, cuts[0], cuts[K],
                extent);
    *x_or = 0;
    for (int k = 0; k < WAN_REGION_SPLIT_MAX; ++k) table->y0[k] = table->x0[k] = table->lo[k] = table->hi[k] = 0;
    for (int k = 0; k < K; ++k) {
        const int y0 = origins[2 * k], x0 = origins[2 * k + 1];
        WAN_REQUIRE(box_ok(H, W, y0, x0, hr, wr), WAN_ERR_INVALID,
                    "%s: box %d: the region [%d, %d + %d) x [%d, %d + %d) does not lie inside a frame of %d x %d", who, k, y0, y0, hr, x0, x0,
                    wr, H, W);
        WAN_REQUIRE(cuts[k] < cuts[k + 1], WAN_ERR_INVALID, "%s: cut %d = %d does not lie above cut %d = %d (the cuts ascend)", who, k + 1,
                    cuts[k + 1], k, cuts[k]);
        table->y0[k] = y0; table->x0[k] = x0; table->lo[k] = cuts[k]; table->hi[k] = cuts[k + 1];
        *x_or |= x0;
        if (axis) *x_or |= cuts[k];
    }
    return WAN_OK;
}

extern "C" wan_status_t wan_region_crop_split(void* out, const void* in, int elem_bytes, int64_t R, int F, int H, int W, const int* runs,
                                              int n_runs, const int* origins, const int* cuts, int K, int axis, int clip, int hr, int wr,
                                              void* stream) {
    const char* who = "wan_region_crop_split";
    // (the boxes and the runs first, as in crop_frames: an empty region's output is an empty tensor, whose address is null)
    WAN_REQUIRE(R >= 1 && F >= 1 && H >= 1 && W >= 1 && hr >= 1 && wr >= 1 && hr <= H && wr <= W, WAN_ERR_INVALID,
                "%s: a region of %d x %d in %lld x %d frames of %d x %d", who, hr, wr, (long long)R, F, H, W);
    SplitTable table;
    int64_t x_or = 0;
    const wan_status_t st = pack_boxes(who, &table, &x_or, origins, cuts, K, axis, H, W, hr, wr);
    if (st != WAN_OK) return st;
    WAN_REQUIRE(runs && n_runs >= 1 && n_runs <= 3, WAN_ERR_INVALID, "%s: %d runs of frames at %p (1 to 3, not null)", who, n_runs,
                (const void*)runs);
    FrameRuns fr = {{0, 0, 0}, {0, 0, 0}};
    int64_t Fo = 0;
    for (int i = 0, end = 0; i < n_runs; ++i) {
        const int start = runs[2 * i], count = runs[2 * i + 1];
        WAN_REQUIRE(start >= end && count >= 1 && (int64_t)start + count <= F, WAN_ERR_INVALID,
                    "%s: run %d = frames [%d, %d + %d) of %d (ascending, not overlapping, at least one frame each, inside the clip)", who, i,
                    start, start, count, F);
        fr.start[i] = start; fr.count[i] = count;
        end = start + count;
        Fo += count;
    }
    WAN_REQUIRE(out && in, WAN_ERR_INVALID, "%s: null tensor", who);
    WAN_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, WAN_ERR_INVALID, "%s: elements of %d bytes (1, 2 or 4)", who,
                elem_bytes);
    WAN_REQUIRE(R <= 0x7fffffff && R * F <= 0x7fffffff && (int64_t)H * W <= 0x7fffffff && K * R * Fo <= 0x7fffffff, WAN_ERR_INVALID,
                "%s: %d boxes of %lld clips of %d frames of %lld elements (frames in all and elements a frame: each at most 2^31 - 1)", who, K,
                (long long)R, F, (long long)((int64_t)H * W));
    const int64_t es = elem_bytes, frames = K * R * Fo;
    // (only a clipped column cut zeroes part of a row, but one rule for both forms keeps the weights' and the state's units alike)
    const int ub = region_unit_bytes(es, {W, wr, x_or}, (uintptr_t)out | (uintptr_t)in);
    const int N = (int)(ub / es), ru = wr / N, cw = std::min(ru, 256), rp = 256 / cw;
    const dim3 grid((unsigned)frames, row_chunks(hr, UNROLL * rp, frames));
    hipStream_t s = (hipStream_t)stream;
#define WAN_CROP_SPLIT(U)                                                                                                      \
    hipLaunchKernelGGL(region_crop_split_kernel<U>, grid, dim3(256), 0, s, (U*)out, (const U*)in, fr, table, (unsigned)Fo,     \
                       (unsigned)(R * Fo), F, (int64_t)H * W / N, W / N, log2_of(N), axis, clip != 0, hr, ru, cw, rp)
    WAN_BY_UNIT(ub, WAN_CROP_SPLIT);
#undef WAN_CROP_SPLIT
    WAN_CHECK_LAUNCH(who);
    return WAN_OK;
}

extern "C" wan_status_t wan_region_restore_split(void* out, const void* source, const void* region, int elem_bytes, int B, int C, int cc,
                                                 int G, int H, int W, int t0, int n, const int* origins, const int* cuts, int K, int axis,
                                                 int hr, int wr, void* stream) {
    const char* who = "wan_region_restore_split";
    WAN_REQUIRE(out && source && region, WAN_ERR_INVALID, "%s: null tensor", who);
    WAN_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, WAN_ERR_INVALID, "%s: elements of %d bytes (1, 2 or 4)", who,
                elem_bytes);
    WAN_REQUIRE(B >= 1 && C >= 1 && cc >= 1, WAN_ERR_INVALID, "%s: B=%d C=%d cc=%d", who, B, C, cc);
    WAN_REQUIRE(0 <= G && G <= cc, WAN_ERR_INVALID,
                "%s: G=%d grounding frames for cc=%d source frames (grounding frame g takes source frame g outside the boxes: "
                "0 <= G <= cc)", who, G, cc);
    WAN_REQUIRE(t0 >= 0 && n >= 1 && (int64_t)t0 + n <= cc, WAN_ERR_INVALID,
                "%s: the frames [%d, %d + %d) do not lie inside the %d source frames", who, t0, t0, n, cc);
    WAN_REQUIRE(H >= 1 && W >= 1 && hr >= 1 && wr >= 1 && hr <= H && wr <= W, WAN_ERR_INVALID,
                "%s: a region of %d x %d in a frame of %d x %d", who, hr, wr, H, W);
    SplitTable table;
    int64_t x_or = 0;
    const wan_status_t st = pack_boxes(who, &table, &x_or, origins, cuts, K, axis, H, W, hr, wr);
    if (st != WAN_OK) return st;
    const int64_t frames = (int64_t)B * C * (2 * (int64_t)cc + G);
    WAN_REQUIRE(frames <= 0x7fffffff && (int64_t)H * W <= 0x7fffffff, WAN_ERR_INVALID,
                "%s: %lld frames of %lld elements (each at most 2^31 - 1)", who, (long long)frames, (long long)((int64_t)H * W));
    const int64_t es = elem_bytes;
    const int ub = region_unit_bytes(es, {W, wr, x_or}, (uintptr_t)out | (uintptr_t)source | (uintptr_t)region);
    const int N = (int)(ub / es), wu = W / N, cw = std::min(wu, 256), rp = 256 / cw;
    const dim3 grid((unsigned)frames, row_chunks(H, UNROLL * rp, frames));
    hipStream_t s = (hipStream_t)stream;
#define WAN_RESTORE_SPLIT(U)                                                                                                   \
    hipLaunchKernelGGL(region_restore_split_kernel<U>, grid, dim3(256), 0, s, (U*)out, (const U*)source, (const U*)region, table, K, \
                       axis, (int64_t)B * C, cc, G, t0, n, H, wu, log2_of(N), hr, wr / N, cw, rp)
    WAN_BY_UNIT(ub, WAN_RESTORE_SPLIT);
#undef WAN_RESTORE_SPLIT
    WAN_CHECK_LAUNCH(who);
    return WAN_OK;
}
