// The flow DPM-Solver++ step (videocof_amd/fm_solvers.py) in ONE pass over the latents: the x0 prediction of the model output,
// stored in the latent dtype (the scheduler's history entry), and the update from it, accumulated in fp32:
//     x0[i]   = a_s*sample[i] + a_v*v[i]
//     prev[i] = c_s*sample[i] + c_0*x0r[i] + c_1*m1[i] + c_2*m2[i] + c_n*noise[i]      (x0r = x0 as stored)
// The host folds the per-step scalar algebra into the seven coefficients (float64).  HBM-bound: 16-byte loads and stores
// (4 fp32 / 8 bf16 per lane), a grid-stride loop over the packets and an element loop for the tail (or for operands that are
// not 16-byte aligned).
#include <algorithm>

#include "common.hpp"
#include "packets.hpp"

namespace {

struct StepCoeffs { float a_s, a_v, c_s, c_0, c_1, c_2, c_n; };

template <typename T>
__global__ __launch_bounds__(256) void solver_step_kernel(T* __restrict__ x0_out, T* __restrict__ prev_out,
                                                          const T* __restrict__ sample, const T* __restrict__ v,
                                                          const T* __restrict__ m1, const T* __restrict__ m2,
                                                          const float* __restrict__ noise, StepCoeffs c, int64_t npk, int64_t n) {
    constexpr int N = Pk<T>::N;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t p = tid; p < npk; p += stride) {
        const int64_t base = p * N;                  // base + N <= npk * N <= n
        float s[N], x[N], acc[N];
        load_pk(sample + base, s);
        load_pk(v + base, x);
        // x0 rounded as wan_lincomb's code generation rounds its first two terms, fma(a_v, v, a_s * s): the same bits.  The
        // fmas are explicit: left to contraction, the vectoriser forms other roundings (two products and an add).
#pragma unroll
        for (int j = 0; j < N; ++j) x[j] = __builtin_fmaf(c.a_v, x[j], c.a_s * s[j]);
        store_pk(x0_out + base, x);             // x <- x0 as stored
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = __builtin_fmaf(c.c_0, x[j], c.c_s * s[j]);
        if (m1) {
            float t[N];
            load_pk(m1 + base, t);
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] = __builtin_fmaf(c.c_1, t[j], acc[j]);
        }
        if (m2) {
            float t[N];
            load_pk(m2 + base, t);
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] = __builtin_fmaf(c.c_2, t[j], acc[j]);
        }
        if (noise) {
#pragma unroll
            for (int q = 0; q < N / 4; ++q) {
                float t[4];
                load_pk(noise + base + 4 * q, t);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[4 * q + j] = __builtin_fmaf(c.c_n, t[j], acc[4 * q + j]);
            }
        }
        store_pk(prev_out + base, acc);
    }
    for (int64_t i = npk * N + tid; i < n; i += stride) {
        const float s = (float)sample[i];
        const T xs = (T)__builtin_fmaf(c.a_v, (float)v[i], c.a_s * s);
        x0_out[i] = xs;
        float acc = __builtin_fmaf(c.c_0, (float)xs, c.c_s * s);
        if (m1) acc = __builtin_fmaf(c.c_1, (float)m1[i], acc);
        if (m2) acc = __builtin_fmaf(c.c_2, (float)m2[i], acc);
        if (noise) acc = __builtin_fmaf(c.c_n, noise[i], acc);
        prev_out[i] = (T)acc;
    }
}

}  // namespace

extern "C" wan_status_t wan_solver_step(void* x0_out, void* prev_out, int dtype, const void* sample, const void* v,
                                        const void* m1, const void* m2, const float* noise, float a_s, float a_v, float c_s,
                                        float c_0, float c_1, float c_2, float c_n, int64_t n, void* stream) {
    WAN_REQUIRE(x0_out && prev_out && sample && v, WAN_ERR_INVALID, "wan_solver_step: null tensor");
    WAN_REQUIRE(dtype == 0 || dtype == 1, WAN_ERR_INVALID, "wan_solver_step: dtype=%d (0 fp32, 1 bf16)", dtype);
    WAN_REQUIRE(m1 || !m2, WAN_ERR_INVALID, "wan_solver_step: m2 without m1");
    WAN_REQUIRE(n >= 0, WAN_ERR_INVALID, "wan_solver_step: n=%lld", (long long)n);
    if (n == 0) return WAN_OK;
    const int vec = dtype == 0 ? Pk<float>::N : Pk<bf16_t>::N;
    bool aligned = true;
    for (const void* q : {(const void*)x0_out, (const void*)prev_out, sample, v, m1, m2, (const void*)noise})
        aligned = aligned && ((uintptr_t)q & 15) == 0;
    const int64_t npk = aligned ? n / vec : 0;
    const int64_t work = std::max<int64_t>(npk, n - npk * vec);
    const unsigned blocks = (unsigned)std::min<int64_t>((work + 255) / 256, 2048);
    const StepCoeffs c{a_s, a_v, c_s, c_0, c_1, c_2, c_n};
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0)
        hipLaunchKernelGGL(solver_step_kernel<float>, dim3(blocks), dim3(256), 0, s, (float*)x0_out, (float*)prev_out,
                           (const float*)sample, (const float*)v, (const float*)m1, (const float*)m2, noise, c, npk, n);
    else
        hipLaunchKernelGGL(solver_step_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, (bf16_t*)x0_out, (bf16_t*)prev_out,
                           (const bf16_t*)sample, (const bf16_t*)v, (const bf16_t*)m1, (const bf16_t*)m2, noise, c, npk, n);
    WAN_CHECK_LAUNCH("wan_solver_step");
    return WAN_OK;
}
