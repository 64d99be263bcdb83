// Runs of bytes at addresses of any alignment, for the kernels of the uint8 frame path (frame_yuv.hip, frame_keep.hip): a thread's
// bytes are ONE run, moved as dwordx4 (dwordx2 for 8 bytes) when its address allows, else as aligned dwords shifted into place with
// v_alignbyte_b32 and the up to 3 bytes in front of / behind them one by one.
#pragma once
#include "common.hpp"

__device__ __forceinline__ unsigned int byte_of(const unsigned int* w, int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }

// 4 * NW bytes from base + off (any alignment) into w.  Nothing outside [base, base + extent) is read.
template <int NW>
__device__ __forceinline__ void load_bytes(const uint8_t* base, int64_t extent, int64_t off, unsigned int (&w)[NW]) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(base) + (uintptr_t)off;
    const int a = (int)(addr & 3);
    if (off - a >= 0 && off - a + 4 * (NW + (a ? 1 : 0)) <= extent) {
        if constexpr (NW % 4 == 0) {
            if ((addr & 15) == 0) {
                const u32x4* p = reinterpret_cast<const u32x4*>(base + off);
#pragma unroll
                for (int q = 0; q < NW / 4; ++q) {
                    const u32x4 v = p[q];
#pragma unroll
                    for (int i = 0; i < 4; ++i) w[4 * q + i] = v[i];
                }
                return;
            }
        }
        if constexpr (NW == 2) {
            if ((addr & 7) == 0) {
                const u32x2 v = *reinterpret_cast<const u32x2*>(base + off);
                w[0] = v[0]; w[1] = v[1];
                return;
            }
        }
        const unsigned int* p = reinterpret_cast<const unsigned int*>(base + (off - a));      // 4-byte aligned
        if (a == 0) {
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = p[i];
        } else {
            unsigned int v[NW + 1];
#pragma unroll
            for (int i = 0; i <= NW; ++i) v[i] = p[i];
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = __builtin_amdgcn_alignbyte(v[i + 1], v[i], (unsigned int)a);
        }
    } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = 0u;
#pragma unroll
        for (int b = 0; b < 4 * NW; ++b) {
            const int64_t o = off + b;
            if (o >= 0 && o < extent) w[b >> 2] |= (unsigned int)base[o] << ((b & 3) * 8);
        }
    }
}

// the first n <= 4 * NW bytes of w to dst (any alignment); no other byte is written
template <int NW>
__device__ __forceinline__ void store_span(uint8_t* dst, const unsigned int (&w)[NW], int n) {
    if (n == 4 * NW) {
        const uintptr_t addr = reinterpret_cast<uintptr_t>(dst);
        if constexpr (NW % 4 == 0) {
            if ((addr & 15) == 0) {
#pragma unroll
                for (int q = 0; q < NW / 4; ++q)
                    reinterpret_cast<u32x4*>(dst)[q] = u32x4{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
                return;
            }
        }
        if constexpr (NW == 2) {
            if ((addr & 7) == 0) {
                *reinterpret_cast<u32x2*>(dst) = u32x2{w[0], w[1]};
                return;
            }
        }
        const int a = (int)(addr & 3);
        if (a == 0) {
#pragma unroll
            for (int i = 0; i < NW; ++i) reinterpret_cast<unsigned int*>(dst)[i] = w[i];
            return;
        }
        const int head = 4 - a;                                    // bytes up to the next aligned dword
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < head) dst[j] = (uint8_t)(w[0] >> (j * 8));
        unsigned int* p = reinterpret_cast<unsigned int*>(dst + head);
#pragma unroll
        for (int i = 0; i + 1 < NW; ++i) p[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], (unsigned int)head);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < a) dst[4 * NW - a + j] = (uint8_t)(w[NW - 1] >> ((head + j) * 8));
    } else {
#pragma unroll
        for (int b = 0; b < 4 * NW; ++b)
            if (b < n) dst[b] = (uint8_t)(w[b >> 2] >> ((b & 3) * 8));
    }
}
