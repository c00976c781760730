// aipstack_amd -- ARP on receive: the records of a batch of frames and the replies to the
// requests for the interface's address, as header slots without a chunk (the rules and the
// bytes: arp_common.h). Three stream-ordered launches:
//   1. arp_decide_kernel, one frame per lane, one block per tile of 256 consecutive frames: the
//      frame's bytes 10-33 and 38-41, read as seven dwords at the frame's own byte alignment and
//      only inside the frame; d_status; the 16-byte record (through LDS in whole lines when d_arp lies on a
//      16-byte boundary); per wave the ballot of replies and of seen frames, per tile their
//      counts, into the workspace;
//   2. pair_scan_kernel (pair_scan.h), ONE workgroup: the exclusive running sums of the tiles'
//      counts in place, the totals behind them and into d_counts;
//   3. arp_emit_kernel, tiles as in 1: a frame's place in each list = its tile's sum + the bits
//      below it in the tile's ballots; a reply's slot from the record just written (through LDS
//      in whole lines when the ring is 64-byte slots on a 64-byte boundary, tx_producer.h);
//      d_hdr_len and the zero d_chunk_index of every frame; entry i of each list at or beyond its
//      count by lane i.
// A place is at most the frame's own index (it counts frames in front of it), so every store lies
// inside the caller's n entries. No kernel waits for another workgroup.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "arp_common.h"
#include "chksum_internal.h"
#include "lane_pass.h"
#include "pair_scan.h"
#include "rx_frames.h"
#include "tx_producer.h"

namespace aipstack_amd {
namespace {

static_assert(kArpTile == kBlock && kArpTileWaves == kBlock / kWave, "one tile per block iteration");
constexpr int kWaves = kBlock / kWave;

// (where the ballots lie behind the counts, and how a wave reads one: pair_scan.h)

// LINES: d_arp is stored in whole lines (16-byte aligned).
template <class Frames, bool LINES>
__global__ __launch_bounds__(kBlock) void arp_decide_kernel(const Frames fr, uint64_t n,
                                                            const ArpIface f,
                                                            uint8_t *__restrict__ status,
                                                            uint64_t arp_base,
                                                            uint64_t *__restrict__ ws) {
    __shared__ LineTiles<1, LINES> tile_lds;
    __shared__ uint32_t part[kWaves][2];
    const WaveStride wst;
    const uint32_t lane = wst.lane, wave = wst.wave;
    const uint64_t tiles = (n + kArpTile - 1) / kArpTile;
    uint64_t *__restrict__ ballots = ws + ballots_at(tiles);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t wave_base = tile * kArpTile + wave * kWave;
        const uint64_t i = wave_base + lane;
        const bool active = i < n;
        ArpRecord r{{0u, 0u, 0u, (uint32_t)AIPSTACK_ARP_NONE << 8}};
        if (active) {
            uint64_t S;
            uint32_t len;
            fr.frame(i, S, len);
            r = arp_decide(FrameLoad{S}, len, f);
            status[i] = (uint8_t)r.status();
        }
        const uint64_t rb = __builtin_amdgcn_ballot_w64(active && r.replies());
        const uint64_t sb = __builtin_amdgcn_ballot_w64(active && r.seen());
        if (lane == 0) {
            ballots[2 * (tile * kWaves + wave)] = rb;
            ballots[2 * (tile * kWaves + wave) + 1] = sb;
            part[wave][0] = __popcll(rb);
            part[wave][1] = __popcll(sb);
        }
        if constexpr (LINES) {
            store_wave_lines<1>(tile_lds[wave], lane, arp_base, wave_base,
                                __builtin_amdgcn_ballot_w64(active), r.w);
        } else if (active) {
            *reinterpret_cast<global_t<u32x4, 4> *>(arp_base + i * 16u) =
                u32x4{r.w[0], r.w[1], r.w[2], r.w[3]};
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            uint32_t s = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) s += part[w][threadIdx.x];
            ws[2 * tile + threadIdx.x] = s;
        }
        __syncthreads();
    }
}

// LINES: the header ring is stored in whole lines (ring_in_lines).
template <bool LINES>
__global__ __launch_bounds__(kBlock) void arp_emit_kernel(
    uint64_t n, const ArpIface f, uint64_t arp_base, uint64_t hdr_base, uint64_t hdr_stride,
    uint32_t *__restrict__ hdr_len, uint64_t *__restrict__ chunk_index,
    uint64_t *__restrict__ reply_frame, uint64_t *__restrict__ seen_frame,
    const uint64_t *__restrict__ ws) {
    __shared__ LineTiles<4, LINES> tile_lds;
    const WaveStride wst;
    const uint32_t lane = wst.lane, wave = wst.wave;
    const uint64_t tiles = (n + kArpTile - 1) / kArpTile;
    const uint64_t total_r = ws[2 * tiles], total_s = ws[2 * tiles + 1];
    const uint64_t *__restrict__ ballots = ws + ballots_at(tiles);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t wave_base = tile * kArpTile + wave * kWave;
        const uint64_t i = wave_base + lane;
        const bool active = i < n;
        const uint64_t *__restrict__ b = ballots + 2 * (tile * kWaves);
        const uint64_t rb = uniform_bits(b[2 * wave]), sb = uniform_bits(b[2 * wave + 1]);
        const uint64_t below = (1ull << lane) - 1u;
        uint64_t j = ws[2 * tile] + __popcll(rb & below), k = ws[2 * tile + 1] + __popcll(sb & below);
#pragma unroll
        for (int w = 0; w < kWaves; ++w)
            if ((uint32_t)w < wave) {
                j += __popcll(b[2 * w]);
                k += __popcll(b[2 * w + 1]);
            }
        const bool resp = (rb >> lane & 1ull) != 0u, seen = (sb >> lane & 1ull) != 0u;
        uint32_t o[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) o[q] = 0u;
        if (resp) {  // (a set bit: below n)
            const u32x4 v = *reinterpret_cast<global_t<const u32x4, 4> *>(arp_base + i * 16u);
            arp_build_reply(ArpRecord{{v.x, v.y, v.z, v.w}}, f, o);
            reply_frame[j] = i;
        }
        if (seen) seen_frame[k] = i;
        if (active) {
            hdr_len[i] = resp ? AIPSTACK_ARP_REPLY_HEADER : 0u;
            chunk_index[i] = 0u;
            if (i == n - 1) chunk_index[n] = 0u;
            if (i >= total_r) reply_frame[i] = ~0ull;
            if (i >= total_s) seen_frame[i] = ~0ull;
        }
        store_header_slot<LINES, (int)AIPSTACK_ARP_REPLY_HEADER>(
            tile_lds, wst, hdr_base, hdr_stride, wave_base, resp, AIPSTACK_ARP_REPLY_HEADER, o);
    }
}

struct Outputs {
    uint8_t *status;
    void *arp, *hdr;
    uint64_t hdr_stride;
    uint32_t *hdr_len;
    uint64_t *chunk_index, *reply_frame, *seen_frame, *counts, *ws;
};

template <class Frames>
int launch_respond(const Frames &fr, uint64_t n, const ArpIface &f, const Outputs &o, hipStream_t s) {
    unsigned blocks;
    const int st = lane_pass_blocks(n, s, &blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint64_t tiles = (n + kArpTile - 1) / kArpTile;
    const uint64_t hdr_base = (uint64_t)(uintptr_t)o.hdr, arp_base = (uint64_t)(uintptr_t)o.arp;
    if ((arp_base & 15u) == 0u)
        hipLaunchKernelGGL((arp_decide_kernel<Frames, true>), dim3(blocks), dim3(kBlock), 0, s, fr, n,
                           f, o.status, arp_base, o.ws);
    else
        hipLaunchKernelGGL((arp_decide_kernel<Frames, false>), dim3(blocks), dim3(kBlock), 0, s, fr, n,
                           f, o.status, arp_base, o.ws);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(kBlock), 0, s, tiles, o.ws, o.counts);
    if (ring_in_lines(hdr_base, o.hdr_stride))
        hipLaunchKernelGGL((arp_emit_kernel<true>), dim3(blocks), dim3(kBlock), 0, s, n, f, arp_base,
                           hdr_base, o.hdr_stride, o.hdr_len, o.chunk_index, o.reply_frame,
                           o.seen_frame, o.ws);
    else
        hipLaunchKernelGGL((arp_emit_kernel<false>), dim3(blocks), dim3(kBlock), 0, s, n, f, arp_base,
                           hdr_base, o.hdr_stride, o.hdr_len, o.chunk_index, o.reply_frame,
                           o.seen_frame, o.ws);
    return check_hip(hipGetLastError());
}

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_arp_rx_respond(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                                       const aipstack_arp_iface *h_iface, uint8_t *d_status,
                                       aipstack_arp_record *d_arp, void *d_hdr, uint64_t hdr_stride,
                                       uint32_t *d_hdr_len, uint64_t *d_chunk_index,
                                       uint64_t *d_reply_frame, uint64_t *d_seen_frame,
                                       uint64_t *d_counts, void *d_workspace,
                                       uint64_t workspace_bytes, void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    const int st = arp_rx_respond_check_args(ArpRespondArgs{
        d_base, d_offsets, false, 0, n, h_iface, d_status, d_arp, d_hdr, hdr_stride, d_hdr_len,
        d_chunk_index, d_reply_frame, d_seen_frame, d_counts, d_workspace, workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const CsrFrames fr{(uint64_t)(uintptr_t)d_base, d_offsets};
    return launch_respond(fr, n, arp_iface_of(*h_iface),
                          Outputs{d_status, d_arp, d_hdr, hdr_stride, d_hdr_len, d_chunk_index,
                                  d_reply_frame, d_seen_frame, d_counts, (uint64_t *)d_workspace},
                          (hipStream_t)stream);
}

extern "C" int aipstack_arp_rx_respond_slotted(
    const void *d_base, uint64_t slot_stride, const uint32_t *d_len, uint64_t n,
    const aipstack_arp_iface *h_iface, uint8_t *d_status, aipstack_arp_record *d_arp, void *d_hdr,
    uint64_t hdr_stride, uint32_t *d_hdr_len, uint64_t *d_chunk_index, uint64_t *d_reply_frame,
    uint64_t *d_seen_frame, uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes,
    void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    const int st = arp_rx_respond_check_args(ArpRespondArgs{
        d_base, d_len, true, slot_stride, n, h_iface, d_status, d_arp, d_hdr, hdr_stride, d_hdr_len,
        d_chunk_index, d_reply_frame, d_seen_frame, d_counts, d_workspace, workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint32_t cap = (uint32_t)(slot_stride < AIPSTACK_CHKSUM_MAX_LEN ? slot_stride
                                                                           : AIPSTACK_CHKSUM_MAX_LEN);
    const SlotFrames fr{(uint64_t)(uintptr_t)d_base, slot_stride, d_len, cap};
    return launch_respond(fr, n, arp_iface_of(*h_iface),
                          Outputs{d_status, d_arp, d_hdr, hdr_stride, d_hdr_len, d_chunk_index,
                                  d_reply_frame, d_seen_frame, d_counts, (uint64_t *)d_workspace},
                          (hipStream_t)stream);
}
