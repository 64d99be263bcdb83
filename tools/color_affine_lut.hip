// The form of wan_frames_u8_affine that was NOT kept: a 256-entry table per channel of the workgroup's frame, built in
// LDS by the workgroup (thread x computes entry x of the three tables), then one ds_read_u8 per byte instead of v_mad_i32_i24 + shift +
// v_med3.  Same tiling as affine_kernel of videocof_amd/csrc/frame_color.hip -- 48 bytes per thread, 12288 per workgroup -- so the two
// differ in the per-byte work only.  Not part of libwan_hip.so: tools/bench_color_match.py compiles this file, checks that it equals
// the product kernel byte for byte, and times it beside it.
#include <hip/hip_runtime.h>

#include "byte_runs.hpp"

namespace {

constexpr int RUN = 48, TILE_BYTES = 256 * RUN;

__global__ __launch_bounds__(256) void affine_lut_kernel(const uint8_t* frames, const int* coef, uint8_t* out, int64_t frame_bytes,
                                                         int64_t total_bytes) {
    __shared__ uint8_t table[3][256];
    const int64_t n = blockIdx.y;
    const int x = threadIdx.x;
    const int* k = coef + n * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) table[c][x] = (uint8_t)min(max((__mul24(k[2 * c], x) + k[2 * c + 1] + 2048) >> 12, 0), 255);
    __syncthreads();
    const int64_t o = ((int64_t)blockIdx.x * 256 + threadIdx.x) * RUN;
    if (o >= frame_bytes) return;
    unsigned int w[RUN / 4], r[RUN / 4];
    load_bytes<RUN / 4>(frames, total_bytes, n * frame_bytes + o, w);
#pragma unroll
    for (int q = 0; q < RUN / 4; ++q) {
        unsigned int v = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) v |= (unsigned int)table[(4 * q + j) % 3][(w[q] >> (8 * j)) & 0xffu] << (8 * j);
        r[q] = v;
    }
    store_span<RUN / 4>(out + n * frame_bytes + o, r, (int)min((int64_t)RUN, frame_bytes - o));
}

}  // namespace

extern "C" int color_affine_lut(const void* frames_u8, const void* coef_i32, void* out_u8, int N, int H, int W, void* stream) {
    if (!frames_u8 || !coef_i32 || !out_u8 || N <= 0 || N > 65535 || H <= 0 || W <= 0 || (int64_t)H * W * 3 >= (1ll << 31)) return 1;
    const int64_t frame_bytes = (int64_t)H * W * 3;
    hipLaunchKernelGGL(affine_lut_kernel, dim3((unsigned)((frame_bytes + TILE_BYTES - 1) / TILE_BYTES), (unsigned)N), dim3(256), 0,
                       (hipStream_t)stream, (const uint8_t*)frames_u8, (const int*)coef_i32, (uint8_t*)out_u8, frame_bytes,
                       (int64_t)N * frame_bytes);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
