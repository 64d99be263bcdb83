// A device-local copy with the launch footprint of a collective: what videocof_amd.dist.EmulatedRank(concurrent=True) puts on its
// side stream where a rank of a real Ulysses group would run an RCCL all-to-all (include/wan_hip.h, wan_sp_channel_copy).
//   grid  = `channels` workgroups (1..32) of `threads` lanes (256 or 512) -- nothing else: a launch never holds more than `channels`
//           CUs, however large the buffer is, and every workgroup is independent of the others (no LDS, no barrier, no atomic, no
//           flag it spins on), so the copy advances on a single free CU while resident kernels own the rest of the chip.
//   work  = workgroup c moves the c-th contiguous share of the buffer, 16 bytes per lane and access, four accesses in flight per lane.
// ASSUMPTION, not a measurement: that an RCCL all-to-all on this chip looks like "N channels = N workgroups of 256-512 threads"
// is taken from RCCL's public channel model; no RCCL kernel has been traced next to these kernels (the boxes have one GPU).
#include "common.hpp"

namespace {

constexpr int kMaxChannels = 32;

// V = u32x4: `n` 16-byte words behind a head of < 16 bytes (dst + head and src + head are both 16-byte aligned), then a tail of
// < 16 bytes.  V = unsigned char: dst and src are misaligned against each other, every byte is an element (head = tail = 0).
template <int THREADS, typename V>
__global__ __launch_bounds__(THREADS) void sp_channel_copy_kernel(unsigned char* __restrict__ dst, const unsigned char* __restrict__ src,
                                                                  int head, int64_t n, int tail) {
    const int64_t C = gridDim.x, c = blockIdx.x;
    const int64_t base = n / C, rem = n % C;                   // shares differ by at most one element: the first `rem` get base + 1
    const int64_t first = c * base + (c < rem ? c : rem), count = base + (c < rem ? 1 : 0);
    const V* __restrict__ s = reinterpret_cast<const V*>(src + head) + first;
    V* __restrict__ d = reinterpret_cast<V*>(dst + head) + first;
    int64_t i = threadIdx.x;
    for (; i + 3 * THREADS < count; i += 4 * THREADS) {         // four independent loads per lane before the first store
        const V a0 = s[i], a1 = s[i + THREADS], a2 = s[i + 2 * THREADS], a3 = s[i + 3 * THREADS];
        d[i] = a0; d[i + THREADS] = a1; d[i + 2 * THREADS] = a2; d[i + 3 * THREADS] = a3;
    }
    for (; i < count; i += THREADS) d[i] = s[i];
    if (c == 0 && (int)threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    if (c == C - 1 && (int)threadIdx.x < tail) {
        const int64_t at = head + n * (int64_t)sizeof(V) + threadIdx.x;
        dst[at] = src[at];
    }
}

template <int THREADS>
void launch_copy(unsigned char* dst, const unsigned char* src, int64_t bytes, int channels, hipStream_t s) {
    const uintptr_t da = (uintptr_t)dst, sa = (uintptr_t)src;
    if (((da ^ sa) & 15) == 0) {
        int head = (int)((16 - (da & 15)) & 15);
        if (head > bytes) head = (int)bytes;
        const int64_t n = (bytes - head) / 16;
        const int tail = (int)(bytes - head - n * 16);
        hipLaunchKernelGGL((sp_channel_copy_kernel<THREADS, u32x4>), dim3((unsigned)channels), dim3(THREADS), 0, s, dst, src, head, n, tail);
    } else {
        hipLaunchKernelGGL((sp_channel_copy_kernel<THREADS, unsigned char>), dim3((unsigned)channels), dim3(THREADS), 0, s, dst, src, 0, bytes, 0);
    }
}

}  // namespace

extern "C" wan_status_t wan_sp_channel_copy(void* dst, const void* src, int64_t bytes, int channels, int threads, void* stream) {
    WAN_REQUIRE(dst != nullptr && src != nullptr, WAN_ERR_INVALID, "wan_sp_channel_copy: null buffer");
    WAN_REQUIRE(bytes >= 0, WAN_ERR_INVALID, "wan_sp_channel_copy: %lld bytes", (long long)bytes);
    WAN_REQUIRE(channels >= 1 && channels <= kMaxChannels, WAN_ERR_INVALID, "wan_sp_channel_copy: %d channels (1..%d)", channels, kMaxChannels);
    WAN_REQUIRE(threads == 256 || threads == 512, WAN_ERR_INVALID, "wan_sp_channel_copy: %d threads per channel (256 or 512)", threads);
    const uintptr_t da = (uintptr_t)dst, sa = (uintptr_t)src;
    WAN_REQUIRE(da + (uintptr_t)bytes <= sa || sa + (uintptr_t)bytes <= da, WAN_ERR_INVALID,
                "wan_sp_channel_copy: in-place or overlapping buffers");
    if (bytes == 0) return WAN_OK;
    hipStream_t s = (hipStream_t)stream;
    if (threads == 256) launch_copy<256>((unsigned char*)dst, (const unsigned char*)src, bytes, channels, s);
    else launch_copy<512>((unsigned char*)dst, (const unsigned char*)src, bytes, channels, s);
    WAN_CHECK_LAUNCH("wan_sp_channel_copy");
    return WAN_OK;
}
