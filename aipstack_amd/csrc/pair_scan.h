// aipstack_amd -- the scan between a counting pass and an emit pass that places a batch's
// selected frames in frame order (icmp_kernels.hip: responses and chunks; udprx_kernels.hip:
// deliveries and unreach requests): per tile of 256 frames a pair of 64-bit counts in the
// workspace, turned by ONE workgroup into the sums of the tiles in front, with the totals behind
// them. On top of lane_pass.h, for .hip translation units only, in an anonymous namespace.
#ifndef AIPSTACK_AMD_PAIR_SCAN_H
#define AIPSTACK_AMD_PAIR_SCAN_H

#include "lane_pass.h"

namespace aipstack_amd {
namespace {

constexpr int kScanWaves = kBlock / kWave;

// The inclusive running sum of v over the block's threads (v <= 256 each: below 2^32).
__device__ __forceinline__ uint32_t block_inclusive_sum(uint32_t v, uint32_t (&tot)[kScanWaves],
                                                        uint32_t lane, uint32_t wave) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, kWave);
        if (lane >= (uint32_t)d) v += u;
    }
    if (lane == kWave - 1) tot[wave] = v;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w)
        if ((uint32_t)w < wave) v += tot[w];
    __syncthreads();
    return v;
}

// One workgroup: ws[2t], ws[2t+1] become the sums of the tiles before t; the totals go to
// ws[2 * tiles], ws[2 * tiles + 1] and to counts[0..1]. (A tile's count is at most kBlock.)
__global__ __launch_bounds__(kBlock) void pair_scan_kernel(uint64_t tiles, uint64_t *__restrict__ ws,
                                                           uint64_t *__restrict__ counts) {
    __shared__ uint32_t tot[2][kScanWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint64_t carry_r = 0, carry_c = 0;  // the same in every thread
    for (uint64_t base = 0; base < tiles; base += kBlock) {
        const uint64_t t = base + threadIdx.x;
        const bool in = t < tiles;
        const uint32_t r = in ? (uint32_t)ws[2 * t] : 0u, c = in ? (uint32_t)ws[2 * t + 1] : 0u;
        const uint32_t ri = block_inclusive_sum(r, tot[0], lane, wave);
        const uint32_t ci = block_inclusive_sum(c, tot[1], lane, wave);
        if (in) {
            ws[2 * t] = carry_r + (ri - r);
            ws[2 * t + 1] = carry_c + (ci - c);
        }
        // the last thread's inclusive sums, to every thread
        if (threadIdx.x == kBlock - 1) {
            tot[0][0] = ri;
            tot[1][0] = ci;
        }
        __syncthreads();
        carry_r += tot[0][0];
        carry_c += tot[1][0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ws[2 * tiles] = counts[0] = carry_r;
        ws[2 * tiles + 1] = counts[1] = carry_c;
    }
}

// For the callers that also leave each wave's ballots behind the counts (arp_kernels.hip,
// tcprsp_kernels.hip): a pair of 64-bit ballots per wave, four waves per tile; wave w of tile t
// has its pair at [2 * (4 t + w)] behind the tiles + 1 pairs of counts.
__device__ __forceinline__ uint64_t ballots_at(uint64_t tiles) { return 2u * (tiles + 1u); }

// A ballot, the same in every lane of the wave, in scalar registers. (uniform64 of lane_pass.h
// is for indices: readfirstlane gives an int, and a low word with bit 31 set would extend into
// the high one.)
__device__ __forceinline__ uint64_t uniform_bits(uint64_t v) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32 |
           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
}

}  // namespace
}  // namespace aipstack_amd

#endif
