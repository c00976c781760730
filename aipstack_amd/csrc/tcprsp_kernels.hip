// aipstack_amd -- TCP segments without a connection: the rest of recvIp4Dgram around find_pcb,
// the top of listen_input and the RSTs of send_rst_reply for a batch of frames, as header slots
// without a chunk (the rules and the bytes: tcprsp_common.h; the record and the PCB lookup are
// those of the TCP Rx parse: tcprx_common.h, pcb_lookup.h). Four stream-ordered launches:
//   1. Rx verify (aipstack_chksum_rx_verify / _slotted), unchanged, into d_verdict;
//   2. tcprsp_decide_kernel, one frame per lane, one block per tile of 256 consecutive frames:
//      the listener table once per workgroup into LDS; the verdict and, only of a frame accepted
//      as TCP, its header bytes, read as dwords at the frame's own byte alignment and only inside
//      the frame; the binary search of the sorted PCB table, every index inside [0, n_pcbs); of a
//      frame that gets as far, the walk of the listeners in LDS, every index inside
//      [0, n_listeners); the verdict byte where it changes, the 32-byte record (through LDS in
//      whole lines when d_segs is 16-byte aligned, 8-byte stores otherwise), d_pcb, d_status,
//      d_listener; per wave the ballot of RSTs and of SYNs, per tile their counts, into the
//      workspace;
//   3. pair_scan_kernel (pair_scan.h), ONE workgroup: the exclusive running sums of the tiles'
//      counts in place, the totals behind them and into d_counts;
//   4. tcprsp_emit_kernel, tiles as in 2: a frame's place in each list = its tile's sum + the
//      bits below it in the tile's ballots; an RST's slot from the record just written and the
//      frame's source MAC, its Ident from its place (through LDS in whole lines when the ring is
//      64-byte slots on a 64-byte boundary, tx_producer.h); d_hdr_len and the zero d_chunk_index
//      of every frame; entry i of each list at or beyond its count by lane i.
// A place is at most the frame's own index (it counts frames in front of it), so every store lies
// inside the caller's n entries. No kernel waits for another workgroup.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"
#include "lane_pass.h"
#include "pair_scan.h"
#include "rx_frames.h"
#include "tcprsp_common.h"
#include "tx_producer.h"

namespace aipstack_amd {
namespace {

static_assert(kTcpRspTile == kBlock && kTcpRspTileWaves == kBlock / kWave, "one tile per block iteration");
static_assert(AIPSTACK_TCP_MAX_LISTENERS <= kBlock, "one listener per thread fills the LDS table");
constexpr int kWaves = kBlock / kWave;

// (where the ballots lie behind the counts, and how a wave reads one: pair_scan.h)

// find_listener_for_rx over the table in LDS: the first entry in list order wins.
struct LdsListeners {
    const TcpRspLis *lis;
    uint32_t n;
    __device__ __forceinline__ bool operator()(uint32_t dst, uint32_t port, uint32_t &cookie) const {
        for (uint32_t k = 0; k < n; ++k) {
            const TcpRspLis l = lis[k];
            if (l.port == port && (l.addr == dst || l.addr == 0u)) {
                cookie = l.cookie;
                return true;
            }
        }
        return false;
    }
};

// LINES: d_segs is 16-byte aligned.
template <class Frames, bool LINES>
__global__ __launch_bounds__(kBlock) void tcprsp_decide_kernel(
    const Frames fr, uint64_t n, const TcpRspIface f, uint64_t pcbs, uint64_t n_pcbs,
    uint64_t listeners, uint32_t n_lis, const uint8_t *__restrict__ rst_request,
    uint8_t *__restrict__ verdict, uint64_t segs, uint32_t *__restrict__ pcb,
    uint8_t *__restrict__ status, uint32_t *__restrict__ listener, uint64_t *__restrict__ ws) {
    __shared__ LineTiles<2, LINES> tile_lds;
    __shared__ TcpRspLis lis[AIPSTACK_TCP_MAX_LISTENERS];
    __shared__ uint32_t part[kWaves][2];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (threadIdx.x < n_lis) {  // (n_lis <= 256: inside the table and inside lis)
        const uint64_t e = listeners + threadIdx.x * 16u;
        const u32x2 a = *reinterpret_cast<global_t<const u32x2> *>(e);
        const uint32_t c = *reinterpret_cast<global_t<const uint32_t> *>(e + 8u);
        lis[threadIdx.x] = TcpRspLis{a.x, a.y & 0xFFFFu, c};
    }
    __syncthreads();
    const uint64_t tiles = (n + kTcpRspTile - 1) / kTcpRspTile;
    uint64_t *__restrict__ ballots = ws + ballots_at(tiles);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t wave_base = uniform64(tile * kTcpRspTile + wave * kWave);
        const uint64_t i = wave_base + lane;
        const bool active = i < n;
        uint32_t w[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = 0u;
        uint32_t cookie = AIPSTACK_TCP_NO_PCB;
        TcpRspPlan p{AIPSTACK_TCP_RSP_NONE, AIPSTACK_TCP_NO_LISTENER};
        if (active) {
            // (a frame Rx verify does not accept is not read)
            if (verdict[i] == AIPSTACK_RX_ACCEPT) {
                uint64_t S;
                uint32_t len;
                fr.frame(i, S, len);
                aipstack_tcp_pcb_key key;
                uint32_t r[8];
                const int res = tcp_rx_build(FrameLoad{S}, len, r, key);
                if (res == kTcpRxValid) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) w[q] = r[q];
                    uint32_t c = 0u;
                    const bool found = pcb_table_find(PcbTableLoad{pcbs}, n_pcbs, key, c);
                    if (found) cookie = c;
                    const bool req = rst_request != nullptr && rst_request[i] != 0u;
                    p = tcp_rsp_decide(r, found, req, f, LdsListeners{lis, n_lis});
                } else if (res == kTcpRxBadOffset) {
                    verdict[i] = (uint8_t)AIPSTACK_RX_DROP_TCP_OFFSET;
                }
            }
            __builtin_nontemporal_store(cookie, &pcb[i]);
            status[i] = (uint8_t)p.status;
            listener[i] = p.listener;
        }
        if constexpr (LINES) {
            // the records below n
            store_wave_lines<2>(tile_lds[wave], lane, segs, wave_base,
                                __builtin_amdgcn_ballot_w64(active), w);
        } else if (active) {
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                *reinterpret_cast<global_t<u32x2> *>(segs + i * 32u + q * 8u) =
                    u32x2{w[2 * q], w[2 * q + 1]};
        }
        const uint64_t rb = __builtin_amdgcn_ballot_w64(p.rst());
        const uint64_t sb = __builtin_amdgcn_ballot_w64(p.syn());
        if (lane == 0) {
            ballots[2 * (tile * kWaves + wave)] = rb;
            ballots[2 * (tile * kWaves + wave) + 1] = sb;
            part[wave][0] = __popcll(rb);
            part[wave][1] = __popcll(sb);
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

// LINES: the header ring is stored in whole lines (ring_in_lines).
template <class Frames, bool LINES>
__global__ __launch_bounds__(kBlock) void tcprsp_emit_kernel(
    const Frames fr, uint64_t n, const TcpRspIface f, uint64_t segs, uint64_t hdr_base,
    uint64_t hdr_stride, uint32_t *__restrict__ hdr_len, uint64_t *__restrict__ chunk_index,
    uint64_t *__restrict__ response_frame, uint64_t *__restrict__ syn_frame,
    const uint64_t *__restrict__ ws) {
    __shared__ LineTiles<4, LINES> tile_lds;
    const WaveStride wst;
    const uint32_t lane = wst.lane, wave = wst.wave;
    const uint64_t tiles = (n + kTcpRspTile - 1) / kTcpRspTile;
    const uint64_t total_r = ws[2 * tiles], total_s = ws[2 * tiles + 1];
    const uint64_t *__restrict__ ballots = ws + ballots_at(tiles);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t wave_base = tile * kTcpRspTile + wave * kWave;
        const uint64_t i = wave_base + lane;
        const bool active = i < n;
        const uint64_t *__restrict__ b = ballots + 2 * (tile * kWaves);
        const uint64_t rb = uniform_bits(b[2 * wave]), sb = uniform_bits(b[2 * wave + 1]);
        const uint64_t below = (1ull << lane) - 1u;
        uint64_t j = ws[2 * tile] + __popcll(rb & below), k = ws[2 * tile + 1] + __popcll(sb & below);
#pragma unroll
        for (int q = 0; q < kWaves; ++q)
            if ((uint32_t)q < wave) {
                j += __popcll(b[2 * q]);
                k += __popcll(b[2 * q + 1]);
            }
        const bool rst = (rb >> lane & 1ull) != 0u, syn = (sb >> lane & 1ull) != 0u;
        uint32_t o[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) o[q] = 0u;
        if (rst) {  // (a set bit: below n, a valid record, so a frame of at least 54 bytes)
            uint32_t w[8];
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const u32x2 v = *reinterpret_cast<global_t<const u32x2> *>(segs + i * 32u + q * 8u);
                w[2 * q] = v.x;
                w[2 * q + 1] = v.y;
            }
            uint64_t S;
            uint32_t len;
            fr.frame(i, S, len);
            const FrameLoad ld{S};
            tcp_rsp_build_rst(w, ld(4u), ld(8u), f.ip_id + (uint32_t)j, f, o);
            response_frame[j] = i;
        }
        if (syn) syn_frame[k] = i;
        if (active) {
            hdr_len[i] = rst ? AIPSTACK_TCP_RSP_HEADER : 0u;
            chunk_index[i] = 0u;
            if (i == n - 1) chunk_index[n] = 0u;
            if (i >= total_r) response_frame[i] = ~0ull;
            if (i >= total_s) syn_frame[i] = ~0ull;
        }
        store_header_slot<LINES, (int)AIPSTACK_TCP_RSP_HEADER>(
            tile_lds, wst, hdr_base, hdr_stride, wave_base, rst, AIPSTACK_TCP_RSP_HEADER, o);
    }
}

struct Tables {
    const aipstack_tcp_pcb_key *pcbs;
    uint64_t n_pcbs;
    const aipstack_tcp_listener *listeners;
    uint32_t n_listeners;
    const uint8_t *rst_request;
};

struct Outputs {
    uint8_t *verdict;
    aipstack_tcp_rx_seg *segs;
    uint32_t *pcb;
    uint8_t *status;
    uint32_t *listener;
    void *hdr;
    uint64_t hdr_stride;
    uint32_t *hdr_len;
    uint64_t *chunk_index, *response_frame, *syn_frame, *counts, *ws;
};

template <class Frames>
int launch_respond(const Frames &fr, uint64_t n, const TcpRspIface &f, const Tables &t,
                   const Outputs &o, hipStream_t s) {
    unsigned blocks;
    const int st = lane_pass_blocks(n, s, &blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint64_t tiles = (n + kTcpRspTile - 1) / kTcpRspTile;
    const uint64_t hdr_base = (uint64_t)(uintptr_t)o.hdr, segs = (uint64_t)(uintptr_t)o.segs;
    const uint64_t pcbs = (uint64_t)(uintptr_t)t.pcbs, lis = (uint64_t)(uintptr_t)t.listeners;
    if ((segs & 15u) == 0u)
        hipLaunchKernelGGL((tcprsp_decide_kernel<Frames, true>), dim3(blocks), dim3(kBlock), 0, s, fr,
                           n, f, pcbs, t.n_pcbs, lis, t.n_listeners, t.rst_request, o.verdict, segs,
                           o.pcb, o.status, o.listener, o.ws);
    else
        hipLaunchKernelGGL((tcprsp_decide_kernel<Frames, false>), dim3(blocks), dim3(kBlock), 0, s,
                           fr, n, f, pcbs, t.n_pcbs, lis, t.n_listeners, t.rst_request, o.verdict,
                           segs, o.pcb, o.status, o.listener, o.ws);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(kBlock), 0, s, tiles, o.ws, o.counts);
    if (ring_in_lines(hdr_base, o.hdr_stride))
        hipLaunchKernelGGL((tcprsp_emit_kernel<Frames, true>), dim3(blocks), dim3(kBlock), 0, s, fr, n,
                           f, segs, hdr_base, o.hdr_stride, o.hdr_len, o.chunk_index,
                           o.response_frame, o.syn_frame, o.ws);
    else
        hipLaunchKernelGGL((tcprsp_emit_kernel<Frames, false>), dim3(blocks), dim3(kBlock), 0, s, fr,
                           n, f, segs, hdr_base, o.hdr_stride, o.hdr_len, o.chunk_index,
                           o.response_frame, o.syn_frame, o.ws);
    return check_hip(hipGetLastError());
}

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_tcp_rx_respond(
    const void *d_base, const uint64_t *d_offsets, uint64_t n, const aipstack_icmp_iface *h_iface,
    uint32_t tcp_ttl, const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
    const aipstack_tcp_listener *d_listeners, uint32_t n_listeners, const uint8_t *d_rst_request,
    uint8_t *d_verdict, aipstack_tcp_rx_seg *d_segs, uint32_t *d_pcb, uint8_t *d_status,
    uint32_t *d_listener, void *d_hdr, uint64_t hdr_stride, uint32_t *d_hdr_len,
    uint64_t *d_chunk_index, uint64_t *d_response_frame, uint64_t *d_syn_frame, uint64_t *d_counts,
    void *d_workspace, uint64_t workspace_bytes, void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = tcp_rx_respond_check_args(TcpRespondArgs{
        d_base, d_offsets, false, 0, n, h_iface, tcp_ttl, d_pcbs, n_pcbs, d_listeners, n_listeners,
        d_verdict, d_segs, d_pcb, d_status, d_listener, d_hdr, hdr_stride, d_hdr_len, d_chunk_index,
        d_response_frame, d_syn_frame, d_counts, d_workspace, workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_rx_verify(d_base, d_offsets, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const CsrFrames fr{(uint64_t)(uintptr_t)d_base, d_offsets};
    return launch_respond(fr, n, tcp_rsp_iface_of(*h_iface, tcp_ttl),
                          Tables{d_pcbs, n_pcbs, d_listeners, n_listeners, d_rst_request},
                          Outputs{d_verdict, d_segs, d_pcb, d_status, d_listener, d_hdr, hdr_stride,
                                  d_hdr_len, d_chunk_index, d_response_frame, d_syn_frame, d_counts,
                                  (uint64_t *)d_workspace},
                          (hipStream_t)stream);
}

extern "C" int aipstack_tcp_rx_respond_slotted(
    const void *d_base, uint64_t slot_stride, const uint32_t *d_len, uint64_t n,
    const aipstack_icmp_iface *h_iface, uint32_t tcp_ttl, const aipstack_tcp_pcb_key *d_pcbs,
    uint64_t n_pcbs, const aipstack_tcp_listener *d_listeners, uint32_t n_listeners,
    const uint8_t *d_rst_request, uint8_t *d_verdict, aipstack_tcp_rx_seg *d_segs, uint32_t *d_pcb,
    uint8_t *d_status, uint32_t *d_listener, void *d_hdr, uint64_t hdr_stride, uint32_t *d_hdr_len,
    uint64_t *d_chunk_index, uint64_t *d_response_frame, uint64_t *d_syn_frame, uint64_t *d_counts,
    void *d_workspace, uint64_t workspace_bytes, void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = tcp_rx_respond_check_args(TcpRespondArgs{
        d_base, d_len, true, slot_stride, n, h_iface, tcp_ttl, d_pcbs, n_pcbs, d_listeners,
        n_listeners, d_verdict, d_segs, d_pcb, d_status, d_listener, d_hdr, hdr_stride, d_hdr_len,
        d_chunk_index, d_response_frame, d_syn_frame, d_counts, d_workspace, workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_rx_verify_slotted(d_base, slot_stride, d_len, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint32_t cap = (uint32_t)(slot_stride < AIPSTACK_CHKSUM_MAX_LEN ? slot_stride
                                                                           : AIPSTACK_CHKSUM_MAX_LEN);
    const SlotFrames fr{(uint64_t)(uintptr_t)d_base, slot_stride, d_len, cap};
    return launch_respond(fr, n, tcp_rsp_iface_of(*h_iface, tcp_ttl),
                          Tables{d_pcbs, n_pcbs, d_listeners, n_listeners, d_rst_request},
                          Outputs{d_verdict, d_segs, d_pcb, d_status, d_listener, d_hdr, hdr_stride,
                                  d_hdr_len, d_chunk_index, d_response_frame, d_syn_frame, d_counts,
                                  (uint64_t *)d_workspace},
                          (hipStream_t)stream);
}
