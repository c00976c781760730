// aipstack_amd -- UDP Rx demux: what the reference does with a UDP datagram between its length
// check and the calls of the handlers (IpUdpProto::recvIp4Dgram, udp/IpUdpProto.h:470-621) for a
// batch of frames: the ports, the truncation to the UDP length, the association lookup, the
// listener matches and the decision to send a port unreachable (the rules and the record:
// udprx_common.h). Four stream-ordered launches:
//   1. Rx verify (aipstack_chksum_rx_verify / _slotted), unchanged, into d_verdict;
//   2. udprx_demux_kernel, one frame per lane, one block per tile of 256 consecutive frames: the
//      listener table once per workgroup into LDS; the verdict and, only of a frame accepted as
//      UDP, its header bytes, read as dwords at the frame's own byte alignment and only inside
//      the frame; a binary search of the sorted association table, every index inside
//      [0, n_assocs); a wave-uniform loop over the listeners in which each lane builds its own
//      64-bit mask; the 32-byte record (through LDS in whole lines when d_dgrams is 16-byte
//      aligned, 8-byte stores otherwise) and the unreach code; the wave's delivery ballot and the
//      tile's number of deliveries and of unreach requests into the workspace;
//   3. pair_scan_kernel (pair_scan.h), ONE workgroup: the exclusive running sums of the tiles'
//      counts in place, the totals behind them and into d_counts;
//   4. udprx_emit_kernel, tiles as in 2: a delivered frame's place j in frame order = its tile's
//      sum + its rank in the tile's four ballots, so its entry of d_deliver_frame; entry i at or
//      beyond the count by lane i.
// A place is at most the frame's own index (it counts deliveries in front of the frame), so every
// store lies inside the caller's n entries. No kernel waits for another workgroup.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"
#include "icmp_common.h"
#include "lane_pass.h"
#include "pair_scan.h"
#include "rx_frames.h"
#include "udprx_common.h"

namespace aipstack_amd {
namespace {

static_assert(kUdpRxTile == kBlock && kUdpRxTileWaves == kBlock / kWave, "one tile per block iteration");
constexpr int kWaves = kBlock / kWave;

// LINES: d_dgrams is 16-byte aligned.
template <class Frames, bool LINES>
__global__ __launch_bounds__(kBlock) void udprx_demux_kernel(
    const Frames fr, uint64_t n, uint32_t local_addr, uint32_t bcast_addr, uint64_t assocs,
    uint64_t n_assocs, uint64_t listeners, uint32_t n_lis, const uint8_t *__restrict__ verdict,
    uint64_t dgrams, uint8_t *__restrict__ unreach, uint64_t *__restrict__ ws) {
    __shared__ LineTiles<2, LINES> tile_lds;
    __shared__ UdpLis lis[AIPSTACK_UDP_MAX_LISTENERS];
    __shared__ uint32_t part[kWaves][2];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (threadIdx.x < n_lis) {  // (n_lis <= 64: inside the table and inside lis)
        const u32x2 e = *reinterpret_cast<global_t<const u32x2> *>(listeners + threadIdx.x * 16u);
        lis[threadIdx.x] = UdpLis{e.x, e.y & 0x00FFFFFFu};
    }
    __syncthreads();
    const uint64_t tiles = udp_rx_tiles(n);
    uint64_t *const ballots = ws + udp_rx_ballot_word(tiles);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t wave_base = uniform64(tile * kUdpRxTile + wave * kWave);
        const uint64_t i = wave_base + lane;
        const bool active = i < n;
        uint32_t w[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = 0u;
        UdpRxFacts d{0u, false, false};
        bool valid = false;
        if (active) {
            const uint32_t v = verdict[i];
            // (a frame Rx verify does not accept is not read)
            if (v == AIPSTACK_RX_ACCEPT || v == AIPSTACK_RX_ACCEPT_NO_CHKSUM) {
                uint64_t S;
                uint32_t len;
                fr.frame(i, S, len);
                aipstack_tcp_pcb_key key;
                valid = udp_rx_build(FrameLoad{S}, len, v, local_addr, bcast_addr, w, key, d);
                if (valid) {
                    uint32_t cookie = 0u;
                    const bool found = pcb_table_find(PcbTableLoad{assocs}, n_assocs, key, cookie);
                    w[6] = udp_assoc_of(found, cookie, d.dst_local);
                }
            }
        }
        // the listeners: the same entry for every lane, each lane its own mask
        uint64_t mask = 0;
        if (__builtin_amdgcn_ballot_w64(valid) != 0ull) {
            for (uint32_t k = 0; k < n_lis; ++k) {
                const UdpLis l = lis[k];
                if (valid && udp_listener_matches(l, d, local_addr)) mask |= 1ull << k;
            }
        }
        w[4] = (uint32_t)mask;
        w[5] = (uint32_t)(mask >> 32);
        const bool deliver = valid && (w[6] != AIPSTACK_UDP_NO_ASSOC || mask != 0ull);
        const bool unr = valid && d.dst_local && !deliver;                               // :611
        if (active) unreach[i] = unr ? (uint8_t)3u : (uint8_t)AIPSTACK_ICMP_NO_UNREACH;
        if constexpr (LINES) {
            // the records below n
            store_wave_lines<2>(tile_lds[wave], lane, dgrams, wave_base,
                                __builtin_amdgcn_ballot_w64(active), w);
        } else if (active) {
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                __builtin_nontemporal_store(
                    u32x2{w[2 * q], w[2 * q + 1]},
                    reinterpret_cast<global_t<u32x2> *>(dgrams + i * 32u + q * 8u));
        }
        const uint64_t db = __builtin_amdgcn_ballot_w64(deliver);
        const uint32_t u = __popcll(__builtin_amdgcn_ballot_w64(unr));
        if (lane == 0) {
            ballots[tile * kUdpRxTileWaves + wave] = db;
            part[wave][0] = __popcll(db);
            part[wave][1] = u;
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

__global__ __launch_bounds__(kBlock) void udprx_emit_kernel(uint64_t n,
                                                            uint64_t *__restrict__ deliver_frame,
                                                            const uint64_t *__restrict__ ws) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t tiles = udp_rx_tiles(n);
    const uint64_t *const ballots = ws + udp_rx_ballot_word(tiles);
    const uint64_t total = ws[2 * tiles];
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * kUdpRxTile + threadIdx.x;
        uint64_t j = ws[2 * tile];
        uint64_t mine = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            const uint64_t b = ballots[tile * kUdpRxTileWaves + k];
            if ((uint32_t)k < wave) j += __popcll(b);
            if ((uint32_t)k == wave) mine = b;
        }
        j += __popcll(mine & ((1ull << lane) - 1u));
        // (a ballot has no bit at or beyond n: j counts frames in front of i, so j <= i < n)
        if ((mine >> lane) & 1ull) deliver_frame[j] = i;
        if (i < n && i >= total) deliver_frame[i] = ~0ull;
    }
}

struct Tables {
    uint32_t local_addr, bcast_addr;
    const aipstack_tcp_pcb_key *assocs;
    uint64_t n_assocs;
    const aipstack_udp_listener *listeners;
    uint32_t n_listeners;
};

struct Outputs {
    uint8_t *verdict;
    aipstack_udp_rx_dgram *dgrams;
    uint8_t *unreach;
    uint64_t *deliver_frame, *counts, *ws;
};

template <class Frames>
int launch_demux(const Frames &fr, uint64_t n, const Tables &t, const Outputs &o, hipStream_t s) {
    unsigned blocks;
    const int st = lane_pass_blocks(n, s, &blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint64_t dgrams = (uint64_t)(uintptr_t)o.dgrams;
    const uint64_t assocs = (uint64_t)(uintptr_t)t.assocs, lis = (uint64_t)(uintptr_t)t.listeners;
    if ((dgrams & 15u) == 0u)
        hipLaunchKernelGGL((udprx_demux_kernel<Frames, true>), dim3(blocks), dim3(kBlock), 0, s, fr,
                           n, t.local_addr, t.bcast_addr, assocs, t.n_assocs, lis, t.n_listeners,
                           o.verdict, dgrams, o.unreach, o.ws);
    else
        hipLaunchKernelGGL((udprx_demux_kernel<Frames, false>), dim3(blocks), dim3(kBlock), 0, s,
                           fr, n, t.local_addr, t.bcast_addr, assocs, t.n_assocs, lis,
                           t.n_listeners, o.verdict, dgrams, o.unreach, o.ws);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(kBlock), 0, s, udp_rx_tiles(n), o.ws,
                       o.counts);
    hipLaunchKernelGGL(udprx_emit_kernel, dim3(blocks), dim3(kBlock), 0, s, n, o.deliver_frame,
                       o.ws);
    return check_hip(hipGetLastError());
}

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_udp_rx_demux(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                                     const aipstack_icmp_iface *h_iface,
                                     const aipstack_tcp_pcb_key *d_assocs, uint64_t n_assocs,
                                     const aipstack_udp_listener *d_listeners, uint32_t n_listeners,
                                     uint8_t *d_verdict, aipstack_udp_rx_dgram *d_dgrams,
                                     uint8_t *d_unreach_code, uint64_t *d_deliver_frame,
                                     uint64_t *d_counts, void *d_workspace,
                                     uint64_t workspace_bytes, void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = udp_rx_demux_check_args(UdpRxDemuxArgs{
        d_base, d_offsets, false, 0, n, h_iface, d_assocs, n_assocs, d_listeners, n_listeners,
        d_verdict, d_dgrams, d_unreach_code, d_deliver_frame, d_counts, d_workspace,
        workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_rx_verify(d_base, d_offsets, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const CsrFrames fr{(uint64_t)(uintptr_t)d_base, d_offsets};
    return launch_demux(fr, n,
                        Tables{h_iface->local_addr, h_iface->bcast_addr, d_assocs, n_assocs,
                               d_listeners, n_listeners},
                        Outputs{d_verdict, d_dgrams, d_unreach_code, d_deliver_frame, d_counts,
                                (uint64_t *)d_workspace},
                        (hipStream_t)stream);
}

extern "C" int aipstack_udp_rx_demux_slotted(
    const void *d_base, uint64_t slot_stride, const uint32_t *d_len, uint64_t n,
    const aipstack_icmp_iface *h_iface, const aipstack_tcp_pcb_key *d_assocs, uint64_t n_assocs,
    const aipstack_udp_listener *d_listeners, uint32_t n_listeners, uint8_t *d_verdict,
    aipstack_udp_rx_dgram *d_dgrams, uint8_t *d_unreach_code, uint64_t *d_deliver_frame,
    uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes, void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = udp_rx_demux_check_args(UdpRxDemuxArgs{
        d_base, d_len, true, slot_stride, n, h_iface, d_assocs, n_assocs, d_listeners, n_listeners,
        d_verdict, d_dgrams, d_unreach_code, d_deliver_frame, d_counts, d_workspace,
        workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_rx_verify_slotted(d_base, slot_stride, d_len, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint32_t cap = (uint32_t)(slot_stride < AIPSTACK_CHKSUM_MAX_LEN ? slot_stride
                                                                           : AIPSTACK_CHKSUM_MAX_LEN);
    const SlotFrames fr{(uint64_t)(uintptr_t)d_base, slot_stride, d_len, cap};
    return launch_demux(fr, n,
                        Tables{h_iface->local_addr, h_iface->bcast_addr, d_assocs, n_assocs,
                               d_listeners, n_listeners},
                        Outputs{d_verdict, d_dgrams, d_unreach_code, d_deliver_frame, d_counts,
                                (uint64_t *)d_workspace},
                        (hipStream_t)stream);
}
