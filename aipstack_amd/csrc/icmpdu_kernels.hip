// aipstack_amd -- received ICMP Destination Unreachable: what the reference does with such a
// message up to and including the TCP handler's find_pcb (recvIcmp4Dgram and
// handleIcmp4DestUnreach, ip/IpStack.h:1093-1249; tcp/IpTcpProto_input.h:154-182) for a batch of
// frames (the rules and the record: icmpdu_common.h). Four stream-ordered launches:
//   1. Rx verify (aipstack_chksum_rx_verify / _slotted), unchanged, into d_verdict;
//   2. icmpdu_decide_kernel, one frame per lane, one block per tile of 256 consecutive frames: the
//      verdict and, only of a frame accepted as ICMP, its header bytes, read as dwords at the
//      frame's own byte alignment and only inside the frame; for a quoted TCP segment of a
//      frag-needed message a binary search of the sorted PCB table, every index inside
//      [0, n_pcbs); the status; the 32-byte record (through LDS in whole lines when d_records is
//      16-byte aligned, 8-byte stores otherwise); the wave's ballot of the frames with a PCB and
//      the tile's number of those and of valid records into the workspace;
//   3. pair_scan_kernel (pair_scan.h), ONE workgroup: the exclusive running sums of the tiles'
//      counts in place, the totals behind them and into d_counts;
//   4. icmpdu_emit_kernel, tiles as in 2: a frame with a PCB has its place j in frame order = its
//      tile's sum + its rank in the tile's four ballots, so its entry of d_pcb_frame; entry i at
//      or beyond the count by lane i (the scheme of udprx_kernels.hip).
// A place is at most the frame's own index (it counts frames in front of the frame), so every
// store lies inside the caller's n entries. No kernel waits for another workgroup.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"
#include "icmp_common.h"
#include "icmpdu_common.h"
#include "lane_pass.h"
#include "pair_scan.h"
#include "rx_frames.h"

namespace aipstack_amd {
namespace {

static_assert(kIcmpDuTile == kBlock && kIcmpDuTileWaves == kBlock / kWave,
              "one tile per block iteration");
constexpr int kWaves = kBlock / kWave;

// LINES: d_records is 16-byte aligned.
template <class Frames, bool LINES>
__global__ __launch_bounds__(kBlock) void icmpdu_decide_kernel(
    const Frames fr, uint64_t n, uint32_t local_addr, uint32_t bcast_addr, uint64_t pcbs,
    uint64_t n_pcbs, const uint8_t *__restrict__ verdict, uint8_t *__restrict__ status,
    uint64_t records, uint64_t *__restrict__ ws) {
    __shared__ LineTiles<2, LINES> tile_lds;
    __shared__ uint32_t part[kWaves][2];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t tiles = icmp_du_tiles(n);
    uint64_t *const ballots = ws + icmp_du_ballot_word(tiles);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t wave_base = uniform64(tile * kIcmpDuTile + wave * kWave);
        const uint64_t i = wave_base + lane;
        const bool active = i < n;
        uint32_t w[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = 0u;
        uint32_t st = AIPSTACK_ICMP_DU_NONE;
        if (active) {
            const uint32_t v = verdict[i];
            // (a frame Rx verify does not accept is not read)
            if (v == AIPSTACK_RX_ACCEPT) {
                uint64_t S;
                uint32_t len;
                fr.frame(i, S, len);
                aipstack_tcp_pcb_key key;
                bool lookup;
                if (icmp_du_build(FrameLoad{S}, len, v, local_addr, bcast_addr, w, key, lookup)) {
                    st = AIPSTACK_ICMP_DU_PARSED;
                    if (lookup) {
                        uint32_t cookie = 0u;
                        const bool found = pcb_table_find(PcbTableLoad{pcbs}, n_pcbs, key, cookie);
                        st = found ? AIPSTACK_ICMP_DU_TCP_PCB : AIPSTACK_ICMP_DU_TCP_NO_PCB;
                        if (found) w[5] = cookie;
                    }
                }
            }
            status[i] = (uint8_t)st;
        }
        if constexpr (LINES) {
            // the records below n
            store_wave_lines<2>(tile_lds[wave], lane, records, wave_base,
                                __builtin_amdgcn_ballot_w64(active), w);
        } else if (active) {
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                __builtin_nontemporal_store(
                    u32x2{w[2 * q], w[2 * q + 1]},
                    reinterpret_cast<global_t<u32x2> *>(records + i * 32u + q * 8u));
        }
        const uint64_t pb = __builtin_amdgcn_ballot_w64(st == AIPSTACK_ICMP_DU_TCP_PCB);
        const uint32_t valid = __popcll(__builtin_amdgcn_ballot_w64(st != AIPSTACK_ICMP_DU_NONE));
        if (lane == 0) {
            ballots[tile * kIcmpDuTileWaves + wave] = pb;
            part[wave][0] = __popcll(pb);
            part[wave][1] = valid;
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            uint32_t s = 0;
#pragma unroll
            for (int k = 0; k < kWaves; ++k) s += part[k][threadIdx.x];
            ws[2 * tile + threadIdx.x] = s;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void icmpdu_emit_kernel(uint64_t n,
                                                             uint64_t *__restrict__ pcb_frame,
                                                             const uint64_t *__restrict__ ws) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t tiles = icmp_du_tiles(n);
    const uint64_t *const ballots = ws + icmp_du_ballot_word(tiles);
    const uint64_t total = ws[2 * tiles];
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * kIcmpDuTile + threadIdx.x;
        uint64_t j = ws[2 * tile];
        uint64_t mine = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            const uint64_t b = ballots[tile * kIcmpDuTileWaves + k];
            if ((uint32_t)k < wave) j += __popcll(b);
            if ((uint32_t)k == wave) mine = b;
        }
        j += __popcll(mine & ((1ull << lane) - 1u));
        // (a ballot has no bit at or beyond n: j counts frames in front of i, so j <= i < n)
        if ((mine >> lane) & 1ull) pcb_frame[j] = i;
        if (i < n && i >= total) pcb_frame[i] = ~0ull;
    }
}

struct Outputs {
    uint8_t *verdict, *status;
    aipstack_icmp_du_record *records;
    uint64_t *pcb_frame, *counts, *ws;
};

template <class Frames>
int launch_unreach(const Frames &fr, uint64_t n, const aipstack_icmp_iface &f,
                   const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs, const Outputs &o,
                   hipStream_t s) {
    unsigned blocks;
    const int st = lane_pass_blocks(n, s, &blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint64_t records = (uint64_t)(uintptr_t)o.records, pcbs = (uint64_t)(uintptr_t)d_pcbs;
    if ((records & 15u) == 0u)
        hipLaunchKernelGGL((icmpdu_decide_kernel<Frames, true>), dim3(blocks), dim3(kBlock), 0, s,
                           fr, n, f.local_addr, f.bcast_addr, pcbs, n_pcbs, o.verdict, o.status,
                           records, o.ws);
    else
        hipLaunchKernelGGL((icmpdu_decide_kernel<Frames, false>), dim3(blocks), dim3(kBlock), 0, s,
                           fr, n, f.local_addr, f.bcast_addr, pcbs, n_pcbs, o.verdict, o.status,
                           records, o.ws);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(kBlock), 0, s, icmp_du_tiles(n), o.ws,
                       o.counts);
    hipLaunchKernelGGL(icmpdu_emit_kernel, dim3(blocks), dim3(kBlock), 0, s, n, o.pcb_frame, o.ws);
    return check_hip(hipGetLastError());
}

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_icmp_rx_unreach(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                                        const aipstack_icmp_iface *h_iface,
                                        const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
                                        uint8_t *d_verdict, uint8_t *d_status,
                                        aipstack_icmp_du_record *d_records, uint64_t *d_pcb_frame,
                                        uint64_t *d_counts, void *d_workspace,
                                        uint64_t workspace_bytes, void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = icmp_rx_unreach_check_args(IcmpUnreachArgs{
        d_base, d_offsets, false, 0, n, h_iface, d_pcbs, n_pcbs, d_verdict, d_status, d_records,
        d_pcb_frame, d_counts, d_workspace, workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_rx_verify(d_base, d_offsets, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const CsrFrames fr{(uint64_t)(uintptr_t)d_base, d_offsets};
    return launch_unreach(fr, n, *h_iface, d_pcbs, n_pcbs,
                          Outputs{d_verdict, d_status, d_records, d_pcb_frame, d_counts,
                                  (uint64_t *)d_workspace},
                          (hipStream_t)stream);
}

extern "C" int aipstack_icmp_rx_unreach_slotted(
    const void *d_base, uint64_t slot_stride, const uint32_t *d_len, uint64_t n,
    const aipstack_icmp_iface *h_iface, const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
    uint8_t *d_verdict, uint8_t *d_status, aipstack_icmp_du_record *d_records,
    uint64_t *d_pcb_frame, uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes,
    void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = icmp_rx_unreach_check_args(IcmpUnreachArgs{
        d_base, d_len, true, slot_stride, n, h_iface, d_pcbs, n_pcbs, d_verdict, d_status,
        d_records, d_pcb_frame, d_counts, d_workspace, workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_rx_verify_slotted(d_base, slot_stride, d_len, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint32_t cap = (uint32_t)(slot_stride < AIPSTACK_CHKSUM_MAX_LEN ? slot_stride
                                                                           : AIPSTACK_CHKSUM_MAX_LEN);
    const SlotFrames fr{(uint64_t)(uintptr_t)d_base, slot_stride, d_len, cap};
    return launch_unreach(fr, n, *h_iface, d_pcbs, n_pcbs,
                          Outputs{d_verdict, d_status, d_records, d_pcb_frame, d_counts,
                                  (uint64_t *)d_workspace},
                          (hipStream_t)stream);
}
