// aipstack_amd -- ICMP on receive: echo replies and Destination Unreachable messages for a batch
// of frames, as header slots plus one chunk each that points into the Rx buffer (the decisions
// and the bytes: icmp_common.h). Four stream-ordered launches:
//   1. Rx verify (aipstack_chksum_rx_verify / _slotted), unchanged, into d_verdict;
//   2. icmp_decide_kernel, one frame per lane, one block per tile of 256 consecutive frames: the
//      verdict, the host's unreach code and, only of an accepted frame, its header bytes, read as
//      dwords at the frame's own byte alignment and only inside the frame; d_status; the tile's
//      number of responses and of chunks into the workspace;
//   3. pair_scan_kernel (pair_scan.h), ONE workgroup: the exclusive running sums of the tiles'
//      counts in place, the totals behind them and into d_counts;
//   4. icmp_emit_kernel, tiles as in 2: a responder's place j in frame order = its tile's sum +
//      its rank in the tile (ballots and four wave totals in LDS), so its Ident, its entry of
//      the compact chunk table and of d_response_frame; its slot (through LDS in whole lines when
//      the ring is 64-byte slots on a 64-byte boundary, tx_producer.h); d_hdr_len and
//      d_chunk_index of every frame; entry i of each list at or beyond its count by lane i.
// A place is at most the frame's own index (it counts responders in front of the frame), so every
// store lies inside the caller's n entries. No kernel waits for another workgroup.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"
#include "icmp_common.h"
#include "lane_pass.h"
#include "pair_scan.h"
#include "rx_frames.h"
#include "tx_producer.h"

namespace aipstack_amd {
namespace {

static_assert(kIcmpTile == kBlock, "one tile per block iteration");
constexpr int kWaves = kBlock / kWave;

// Frame i's decision, from its verdict, the host's code and (of an accepted frame) its bytes.
template <class Frames>
__device__ __forceinline__ IcmpPlan plan_of(const Frames &fr, uint64_t i, uint32_t verdict,
                                            uint32_t code, const IcmpIface &f, uint64_t &S) {
    uint32_t len;
    fr.frame(i, S, len);
    return icmp_decide(FrameLoad{S}, len, verdict, code, f);
}

template <class Frames>
__global__ __launch_bounds__(kBlock) void icmp_decide_kernel(
    const Frames fr, uint64_t n, const IcmpIface f, const uint8_t *__restrict__ unreach,
    const uint8_t *__restrict__ verdict, uint8_t *__restrict__ status, uint64_t *__restrict__ ws) {
    __shared__ uint32_t part[kWaves][2];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t tiles = (n + kIcmpTile - 1) / kIcmpTile;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * kIcmpTile + threadIdx.x;
        IcmpPlan p{AIPSTACK_ICMP_NONE, 0u, 0u, 0u};
        if (i < n) {
            const uint32_t v = verdict[i];
            const uint32_t code = unreach ? unreach[i] : (uint32_t)AIPSTACK_ICMP_NO_UNREACH;
            uint64_t S;
            // (a frame Rx verify does not accept is not read)
            if (v == AIPSTACK_RX_ACCEPT || ((v == AIPSTACK_RX_ACCEPT_NO_CHKSUM ||
                                             v == AIPSTACK_RX_ACCEPT_OTHER) &&
                                            code != AIPSTACK_ICMP_NO_UNREACH))
                p = plan_of(fr, i, v, code, f, S);
            status[i] = (uint8_t)p.status;
        }
        const uint32_t r = __popcll(__builtin_amdgcn_ballot_w64(p.responds()));
        const uint32_t c = __popcll(__builtin_amdgcn_ballot_w64(p.has_chunk()));
        if (lane == 0) {
            part[wave][0] = r;
            part[wave][1] = c;
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
template <class Frames, bool LINES>
__global__ __launch_bounds__(kBlock) void icmp_emit_kernel(
    const Frames fr, uint64_t n, const IcmpIface f, const uint8_t *__restrict__ unreach,
    const uint8_t *__restrict__ verdict, const uint8_t *__restrict__ status, uint64_t hdr_base,
    uint64_t hdr_stride, uint32_t *__restrict__ hdr_len, uint64_t *__restrict__ chunk_addr,
    uint32_t *__restrict__ chunk_len, uint64_t *__restrict__ chunk_index,
    uint64_t *__restrict__ response_frame, const uint64_t *__restrict__ ws) {
    __shared__ LineTiles<4, LINES> tile_lds;
    __shared__ uint32_t part[kWaves][2];
    const WaveStride wst;
    const uint32_t lane = wst.lane, wave = wst.wave;
    const uint64_t tiles = (n + kIcmpTile - 1) / kIcmpTile;
    const uint64_t total_r = ws[2 * tiles], total_c = ws[2 * tiles + 1];
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t wave_base = tile * kIcmpTile + wave * kWave;
        const uint64_t i = wave_base + lane;
        const bool active = i < n;
        IcmpPlan p{AIPSTACK_ICMP_NONE, 0u, 0u, 0u};
        uint32_t code = AIPSTACK_ICMP_NO_UNREACH;
        uint64_t S = 0;
        if (active && status[i] != AIPSTACK_ICMP_NONE) {
            code = unreach ? unreach[i] : (uint32_t)AIPSTACK_ICMP_NO_UNREACH;
            p = plan_of(fr, i, verdict[i], code, f, S);
        }
        const bool resp = p.responds(), chunk = p.has_chunk();
        const uint64_t rb = __builtin_amdgcn_ballot_w64(resp), cb = __builtin_amdgcn_ballot_w64(chunk);
        if (lane == 0) {
            part[wave][0] = __popcll(rb);
            part[wave][1] = __popcll(cb);
        }
        __syncthreads();
        const uint64_t below = (1ull << lane) - 1u;
        uint64_t j = ws[2 * tile] + __popcll(rb & below), k = ws[2 * tile + 1] + __popcll(cb & below);
#pragma unroll
        for (int w = 0; w < kWaves; ++w)
            if ((uint32_t)w < wave) {
                j += part[w][0];
                k += part[w][1];
            }
        uint32_t o[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) o[q] = 0u;
        if (resp) {
            icmp_build_slot(FrameLoad{S}, p, code, f.ip_id + (uint32_t)j, f, o);
            response_frame[j] = i;
            if (chunk) {
                chunk_addr[k] = S + p.data_off;
                chunk_len[k] = p.data_len;
            }
        }
        if (active) {
            hdr_len[i] = resp ? AIPSTACK_ICMP_RESPONSE_HEADER : 0u;
            chunk_index[i] = k;
            if (i == n - 1) chunk_index[n] = k + (chunk ? 1u : 0u);
            if (i >= total_r) response_frame[i] = ~0ull;
            if (i >= total_c) {
                chunk_addr[i] = 0u;
                chunk_len[i] = 0u;
            }
        }
        store_header_slot<LINES, (int)AIPSTACK_ICMP_RESPONSE_HEADER>(
            tile_lds, wst, hdr_base, hdr_stride, wave_base, resp, AIPSTACK_ICMP_RESPONSE_HEADER, o);
        __syncthreads();
    }
}

struct Outputs {
    uint8_t *verdict, *status;
    void *hdr;
    uint64_t hdr_stride;
    uint32_t *hdr_len;
    uint64_t *chunk_addr;
    uint32_t *chunk_len;
    uint64_t *chunk_index, *response_frame, *counts, *ws;
};

template <class Frames>
int launch_respond(const Frames &fr, uint64_t n, const IcmpIface &f, const uint8_t *d_unreach,
                   const Outputs &o, hipStream_t s) {
    unsigned blocks;
    const int st = lane_pass_blocks(n, s, &blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint64_t tiles = (n + kIcmpTile - 1) / kIcmpTile;
    const uint64_t hdr_base = (uint64_t)(uintptr_t)o.hdr;
    hipLaunchKernelGGL((icmp_decide_kernel<Frames>), dim3(blocks), dim3(kBlock), 0, s, fr, n, f,
                       d_unreach, o.verdict, o.status, o.ws);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(kBlock), 0, s, tiles, o.ws, o.counts);
    if (ring_in_lines(hdr_base, o.hdr_stride))
        hipLaunchKernelGGL((icmp_emit_kernel<Frames, true>), dim3(blocks), dim3(kBlock), 0, s, fr, n,
                           f, d_unreach, o.verdict, o.status, hdr_base, o.hdr_stride, o.hdr_len,
                           o.chunk_addr, o.chunk_len, o.chunk_index, o.response_frame, o.ws);
    else
        hipLaunchKernelGGL((icmp_emit_kernel<Frames, false>), dim3(blocks), dim3(kBlock), 0, s, fr,
                           n, f, d_unreach, o.verdict, o.status, hdr_base, o.hdr_stride, o.hdr_len,
                           o.chunk_addr, o.chunk_len, o.chunk_index, o.response_frame, o.ws);
    return check_hip(hipGetLastError());
}

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_icmp_rx_respond(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                                        const aipstack_icmp_iface *h_iface,
                                        const uint8_t *d_unreach_code, uint8_t *d_verdict,
                                        uint8_t *d_status, void *d_hdr, uint64_t hdr_stride,
                                        uint32_t *d_hdr_len, uint64_t *d_chunk_addr,
                                        uint32_t *d_chunk_len, uint64_t *d_chunk_index,
                                        uint64_t *d_response_frame, uint64_t *d_counts,
                                        void *d_workspace, uint64_t workspace_bytes, void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = icmp_rx_respond_check_args(IcmpRespondArgs{
        d_base, d_offsets, false, 0, n, h_iface, d_verdict, d_status, d_hdr, hdr_stride, d_hdr_len,
        d_chunk_addr, d_chunk_len, d_chunk_index, d_response_frame, d_counts, d_workspace,
        workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_rx_verify(d_base, d_offsets, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const CsrFrames fr{(uint64_t)(uintptr_t)d_base, d_offsets};
    return launch_respond(fr, n, icmp_iface_of(*h_iface), d_unreach_code,
                          Outputs{d_verdict, d_status, d_hdr, hdr_stride, d_hdr_len, d_chunk_addr,
                                  d_chunk_len, d_chunk_index, d_response_frame, d_counts,
                                  (uint64_t *)d_workspace},
                          (hipStream_t)stream);
}

extern "C" int aipstack_icmp_rx_respond_slotted(
    const void *d_base, uint64_t slot_stride, const uint32_t *d_len, uint64_t n,
    const aipstack_icmp_iface *h_iface, const uint8_t *d_unreach_code, uint8_t *d_verdict,
    uint8_t *d_status, void *d_hdr, uint64_t hdr_stride, uint32_t *d_hdr_len,
    uint64_t *d_chunk_addr, uint32_t *d_chunk_len, uint64_t *d_chunk_index,
    uint64_t *d_response_frame, uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes,
    void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = icmp_rx_respond_check_args(IcmpRespondArgs{
        d_base, d_len, true, slot_stride, n, h_iface, d_verdict, d_status, d_hdr, hdr_stride,
        d_hdr_len, d_chunk_addr, d_chunk_len, d_chunk_index, d_response_frame, d_counts,
        d_workspace, workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_rx_verify_slotted(d_base, slot_stride, d_len, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint32_t cap = (uint32_t)(slot_stride < AIPSTACK_CHKSUM_MAX_LEN ? slot_stride
                                                                           : AIPSTACK_CHKSUM_MAX_LEN);
    const SlotFrames fr{(uint64_t)(uintptr_t)d_base, slot_stride, d_len, cap};
    return launch_respond(fr, n, icmp_iface_of(*h_iface), d_unreach_code,
                          Outputs{d_verdict, d_status, d_hdr, hdr_stride, d_hdr_len, d_chunk_addr,
                                  d_chunk_len, d_chunk_index, d_response_frame, d_counts,
                                  (uint64_t *)d_workspace},
                          (hipStream_t)stream);
}
