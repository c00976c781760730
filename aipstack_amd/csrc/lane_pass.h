// aipstack_amd -- what the passes that handle one element per lane share (the header-split
// fill's, the burst segmentation's and the Rx parse's passes, the split Tx fills' scatter):
// vector and global-pointer types, the 16-bit sum helpers, the wave-aligned grid-stride loop
// header, the whole-line store through LDS and the grid size. Below chksum_device.h, which
// includes it; no __device__ variable. Included by .hip translation units only; everything lives
// in an anonymous namespace.
#ifndef AIPSTACK_AMD_LANE_PASS_H
#define AIPSTACK_AMD_LANE_PASS_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"

namespace aipstack_amd {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kWave = 64;
constexpr int kBlock = 256;

// global_t<T, Align>: a T in global memory (address space 1) aligned to Align bytes (its own
// alignment by default). Accesses through a global_t pointer made from an address are
// global_load / global_store instructions, at any byte alignment (gfx9 under ROCm runs in
// unaligned-access mode: one instruction each). (A typedef in a struct: an alias template
// alone drops the alignment.)
template <class T, int Align>
struct Global {
    typedef __attribute__((address_space(1))) T type __attribute__((aligned(Align)));
};
template <class T, int Align = alignof(T)>
using global_t = typename Global<T, Align>::type;
static_assert(alignof(global_t<u32x4>) == 16 && alignof(global_t<const u32x4, 1>) == 1, "");

__device__ __forceinline__ uint32_t bswap16(uint32_t x) {
    return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu);
}

// x mod 0xFFFF with a nonzero multiple as 0xFFFF: zero only for x = 0.
__device__ __forceinline__ uint32_t fold16(uint32_t x) {
    x = (x & 0xFFFFu) + (x >> 16);
    return (x & 0xFFFFu) + (x >> 16);
}

// v, the same in every lane of the wave, in scalar registers.
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) |
           __builtin_amdgcn_readfirstlane((uint32_t)v);
}

// The header of a grid-stride loop in which every wave takes 64 consecutive elements per
// iteration: `for (uint64_t base = uniform64(ws.first); base < n; base += ws.step)`, the lane's
// element `base + ws.lane`. `first` is the same in every lane of a wave; through uniform64 the
// compiler knows it, and `base` stays in scalar registers.
struct WaveStride {
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t first = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~(uint32_t)(kWave - 1));
};

// The LDS of store_wave_lines for records of Q quads (16 * Q bytes): one tile per wave of the
// block (a kernel instantiated without the line path declares it with ON false: no LDS).
template <int Q, bool ON = true>
using LineTiles = u32x4[ON ? kBlock / kWave : 1][ON ? kWave : 1][Q];

// Stores the wave's records (`rec`: this lane's, Q quads) in whole lines: lane k's is record
// base + k of the 16-byte aligned array at `dst`, stored if bit k of the wave-uniform `live` is
// set. Record `lane` into the wave's tile, then store instruction r takes the quads of records
// (64 / Q) * r .. (64 / Q) * (r + 1) - 1 in memory order: 64 lanes x 16 bytes = 1 KiB
// contiguous. Every lane of the wave calls it.
template <int Q>
__device__ __forceinline__ void store_wave_lines(u32x4 (&tile)[kWave][Q], uint32_t lane,
                                                 uint64_t dst, uint64_t base, uint64_t live,
                                                 const uint32_t (&rec)[4 * Q]) {
#pragma unroll
    for (int q = 0; q < Q; ++q)
        tile[lane][q] = u32x4{rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]};
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (uint32_t r = 0; r < Q; ++r) {
        const uint32_t k = (kWave / Q) * r + lane / Q, q = lane % Q;
        const u32x4 v = tile[k][q];
        if ((live >> k) & 1ull)
            __builtin_nontemporal_store(
                v, reinterpret_cast<global_t<u32x4> *>(dst + (base + k) * (16u * Q) + q * 16u));
    }
    __builtin_amdgcn_wave_barrier();
}

// Blocks of kBlock lanes a pass over n elements launches on a device of `cus` compute units.
inline unsigned lane_pass_blocks(uint64_t n, int cus) {
    const uint64_t want = (n + kBlock - 1) / kBlock, most = tuning_aux_blocks(cus);
    return (unsigned)(want < most ? want : most);
}

// The same for the device `stream` belongs to; AIPSTACK_CHKSUM_EHIP if it cannot be asked.
inline int lane_pass_blocks(uint64_t n, hipStream_t stream, unsigned *blocks) {
    const int cus = device_cu_count(stream);
    if (cus <= 0) return AIPSTACK_CHKSUM_EHIP;
    *blocks = lane_pass_blocks(n, cus);
    return AIPSTACK_CHKSUM_OK;
}

}  // namespace
}  // namespace aipstack_amd

#endif
