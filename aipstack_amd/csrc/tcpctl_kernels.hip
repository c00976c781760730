// aipstack_amd -- TCP segments without data (SYN, SYN-ACK, ACK, FIN, RST): send_tcp_nodata for
// a batch of host-made descriptors, as header slots without a chunk (the bytes: tcpctl_common.h).
// One descriptor per lane, one block per tile of 256 consecutive descriptors, three
// stream-ordered launches:
//   1. tcpctl_plan_kernel: the descriptor's upper 16 bytes (the flags, the options and the
//      reserved fields; the lower half takes no part in the validation), d_status, d_hdr_len and
//      the zero d_chunk_index of every descriptor; per wave the ballot of valid descriptors, per
//      tile the counts of valid and invalid ones, into the workspace;
//   2. pair_scan_kernel (pair_scan.h), ONE workgroup: the exclusive running sums of the tiles'
//      counts in place, the totals behind them and into d_counts;
//   3. tcpctl_emit_kernel, tiles as in 1: a valid descriptor's rank = its tile's sum + the bits
//      below it in the tile's ballots; its two 16-byte halves, the slot image with the Ident from
//      the rank and both checksums as arithmetic on the header words (through LDS in whole lines
//      when the ring is 64-byte slots on a 64-byte boundary, tx_producer.h; else per-lane stores
//      of the header's bytes and zeros up to min(hdr_stride, 64)).
// A set ballot bit lies below n, so every load and store lies inside the caller's n entries. No
// kernel waits for another workgroup; no payload byte is read anywhere.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"
#include "lane_pass.h"
#include "pair_scan.h"
#include "tcpctl_common.h"
#include "tx_producer.h"

namespace aipstack_amd {
namespace {

static_assert(kTcpCtlTile == kBlock && kTcpCtlTileWaves == kBlock / kWave, "one tile per block iteration");
constexpr int kWaves = kBlock / kWave;

// (the ballots lie behind the tiles + 1 pairs of counts, ballots_at of pair_scan.h: one per wave,
// wave w of tile t at [4 t + w])

__global__ __launch_bounds__(kBlock) void tcpctl_plan_kernel(
    uint64_t ctl, uint64_t n, uint32_t *__restrict__ hdr_len, uint64_t *__restrict__ chunk_index,
    uint8_t *__restrict__ status, uint64_t *__restrict__ ws) {
    __shared__ uint32_t part[kWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t tiles = (n + kTcpCtlTile - 1) / kTcpCtlTile;
    uint64_t *__restrict__ ballots = ws + ballots_at(tiles);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t wave_base = uniform64(tile * kTcpCtlTile + wave * kWave);
        const uint64_t i = wave_base + lane;
        const bool active = i < n;
        bool valid = false;
        if (active) {
            const u32x4 hi = *reinterpret_cast<global_t<const u32x4, 8> *>(ctl + i * 32u + 16u);
            valid = tcp_ctl_valid(hi.z, hi.w);
            hdr_len[i] = valid ? tcp_ctl_header_len(hi.z) : 0u;
            status[i] = (uint8_t)(valid ? AIPSTACK_TCP_CTL_EMITTED : AIPSTACK_TCP_CTL_INVALID);
            chunk_index[i] = 0u;
            if (i == n - 1) chunk_index[n] = 0u;
        }
        const uint64_t vb = __builtin_amdgcn_ballot_w64(valid);
        if (lane == 0) {
            ballots[tile * kWaves + wave] = vb;
            part[wave] = __popcll(vb);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t s = 0;
#pragma unroll
            for (int k = 0; k < kWaves; ++k) s += part[k];
            const uint64_t in_tile = n - tile * kTcpCtlTile < kTcpCtlTile ? n - tile * kTcpCtlTile
                                                                          : kTcpCtlTile;
            ws[2 * tile] = s;
            ws[2 * tile + 1] = in_tile - s;
        }
        __syncthreads();
    }
}

// LINES: the header ring is stored in whole lines (ring_in_lines).
template <bool LINES>
__global__ __launch_bounds__(kBlock) void tcpctl_emit_kernel(uint64_t ctl, uint64_t n,
                                                             const TcpRspIface f, uint64_t hdr_base,
                                                             uint64_t hdr_stride,
                                                             const uint64_t *__restrict__ ws) {
    __shared__ LineTiles<4, LINES> tile_lds;
    const WaveStride wst;
    const uint32_t lane = wst.lane, wave = wst.wave;
    const uint64_t tiles = (n + kTcpCtlTile - 1) / kTcpCtlTile;
    const uint64_t *__restrict__ ballots = ws + ballots_at(tiles);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t wave_base = tile * kTcpCtlTile + wave * kWave;
        const uint64_t i = wave_base + lane;
        const uint64_t *__restrict__ b = ballots + tile * kWaves;
        const uint64_t vb = uniform_bits(b[wave]);
        uint64_t j = ws[2 * tile] + __popcll(vb & ((1ull << lane) - 1u));
#pragma unroll
        for (int q = 0; q < kWaves; ++q)
            if ((uint32_t)q < wave) j += __popcll(b[q]);
        const bool valid = (vb >> lane & 1ull) != 0u;
        uint32_t o[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) o[q] = 0u;
        uint32_t hl = AIPSTACK_TCP_SEGMENT_HEADER;
        if (valid) {  // (a set bit: below n)
            const u32x4 lo = *reinterpret_cast<global_t<const u32x4, 8> *>(ctl + i * 32u);
            const u32x4 hi = *reinterpret_cast<global_t<const u32x4, 8> *>(ctl + i * 32u + 16u);
            const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            hl = tcp_ctl_build(d, f.ip_id + (uint32_t)j, f, o);
        }
        if constexpr (LINES) {
            store_header_slot<true, (int)AIPSTACK_TCP_SEGMENT_HEADER>(tile_lds, wst, hdr_base, hdr_stride,
                                                                      wave_base, valid, hl, o);
        } else if (hl == AIPSTACK_TCP_CTL_MAX_HEADER) {
            store_header_slot<false, (int)AIPSTACK_TCP_CTL_MAX_HEADER>(tile_lds, wst, hdr_base, hdr_stride,
                                                                       wave_base, valid, hl, o);
        } else {
            store_header_slot<false, (int)AIPSTACK_TCP_SEGMENT_HEADER,
                              (int)AIPSTACK_TCP_SEGMENT_HEADER + 4>(tile_lds, wst, hdr_base, hdr_stride,
                                                                    wave_base, valid, hl, o);
        }
    }
}

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_tcp_tx_control(const aipstack_tcp_ctl *d_ctl, uint64_t n,
                                       const aipstack_icmp_iface *h_iface, uint32_t tcp_ttl,
                                       void *d_hdr, uint64_t hdr_stride, uint32_t *d_hdr_len,
                                       uint64_t *d_chunk_index, uint8_t *d_status, uint64_t *d_counts,
                                       void *d_workspace, uint64_t workspace_bytes, void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = tcp_tx_control_check_args(TcpControlArgs{d_ctl, n, h_iface, tcp_ttl, d_hdr, hdr_stride,
                                                      d_hdr_len, d_chunk_index, d_status, d_counts,
                                                      d_workspace, workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const hipStream_t s = (hipStream_t)stream;
    unsigned blocks;
    st = lane_pass_blocks(n, s, &blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const TcpRspIface f = tcp_rsp_iface_of(*h_iface, tcp_ttl);
    const uint64_t tiles = (n + kTcpCtlTile - 1) / kTcpCtlTile;
    const uint64_t ctl = (uint64_t)(uintptr_t)d_ctl, hdr_base = (uint64_t)(uintptr_t)d_hdr;
    uint64_t *ws = (uint64_t *)d_workspace;
    hipLaunchKernelGGL(tcpctl_plan_kernel, dim3(blocks), dim3(kBlock), 0, s, ctl, n, d_hdr_len,
                       d_chunk_index, d_status, ws);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(kBlock), 0, s, tiles, ws, d_counts);
    if (ring_in_lines(hdr_base, hdr_stride))
        hipLaunchKernelGGL(tcpctl_emit_kernel<true>, dim3(blocks), dim3(kBlock), 0, s, ctl, n, f,
                           hdr_base, hdr_stride, ws);
    else
        hipLaunchKernelGGL(tcpctl_emit_kernel<false>, dim3(blocks), dim3(kBlock), 0, s, ctl, n, f,
                           hdr_base, hdr_stride, ws);
    return check_hip(hipGetLastError());
}
