// 16-byte packets of the streaming kernels (solver_step.hip, window_kernels.hip): 4 fp32 or 8 bf16 per lane, unpacked to fp32.
#pragma once
#include "common.hpp"

namespace {

template <typename T> struct Pk;                     // one 16-byte packet of T
template <> struct Pk<float> { static constexpr int N = 4; };
template <> struct Pk<bf16_t> { static constexpr int N = 8; };

__device__ __forceinline__ void load_pk(const float* p, float (&f)[4]) {
    const f32x4 v = *(const f32x4*)p;
    f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
}
__device__ __forceinline__ void load_pk(const bf16_t* p, float (&f)[8]) {
    const u32x4 w = *(const u32x4*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) { f[2 * k] = bf16lo_to_f32(w[k]); f[2 * k + 1] = bf16hi_to_f32(w[k]); }
}
// store f, and give back the values as stored (the bf16 rounding of x0 feeds the solver's update)
__device__ __forceinline__ void store_pk(float* p, float (&f)[4]) {
    const f32x4 v = {f[0], f[1], f[2], f[3]};
    *(f32x4*)p = v;
}
__device__ __forceinline__ void store_pk(bf16_t* p, float (&f)[8]) {
    u32x4 w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[k] = pack_bf16x2(f[2 * k], f[2 * k + 1]);
        f[2 * k] = bf16lo_to_f32(w[k]);
        f[2 * k + 1] = bf16hi_to_f32(w[k]);
    }
    *(u32x4*)p = w;
}

}  // namespace
