// aipstack_amd -- TCP Rx parse: what the reference does with a TCP datagram between its
// checksum check and the call of pcb_input (tcp/IpTcpProto_input.h:81-130) for a batch of
// frames: the TcpSegMeta fields, the data offset bound, the options (ParseTcpOptions,
// tcp/TcpOptions.h:63-125) and the PCB lookup (find_pcb, tcp/IpTcpProto.h:806-820). Two
// stream-ordered launches:
//   1. Rx verify (aipstack_chksum_rx_verify / _slotted), unchanged, into d_verdict;
//   2. tcprx_parse_kernel, one frame per lane: the verdict, and only of a frame accepted as TCP
//      its header bytes, read as dwords at the frame's own byte alignment and only inside the
//      frame (tcp_rx_build, tcprx_common.h: the fixed fields, then the options as ten fixed
//      dwords fed to a byte machine -- no array indexed by a run-time position, no scratch);
//      a binary search of the sorted table, one 16-byte entry per step, every index inside
//      [0, n_pcbs); the 32-byte record, the cookie, and the verdict byte where it changes.
//      Records of a 16-byte aligned d_segs go through LDS so that each of the wave's two store
//      instructions covers 1 KiB of contiguous memory; otherwise 8-byte stores per lane.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"
#include "lane_pass.h"
#include "rx_frames.h"
#include "tcprx_common.h"

namespace aipstack_amd {
namespace {

// The cookie of the entry equal to `key` in the table sorted by tcp_pcb_key_compare
// (pcb_table_find, pcb_lookup.h: every entry read lies inside [0, n_pcbs)).
__device__ __forceinline__ uint32_t rxp_lookup(const aipstack_tcp_pcb_key *__restrict__ pcbs,
                                               uint64_t n_pcbs, const aipstack_tcp_pcb_key &key) {
    uint32_t cookie;
    return pcb_table_find(PcbTableLoad{(uint64_t)(uintptr_t)pcbs}, n_pcbs, key, cookie)
               ? cookie
               : AIPSTACK_TCP_NO_PCB;
}

// LINES: d_segs is 16-byte aligned.
template <class Frames, bool LINES>
__global__ __launch_bounds__(kBlock) void tcprx_parse_kernel(
    const Frames fr, uint64_t n, const aipstack_tcp_pcb_key *__restrict__ pcbs, uint64_t n_pcbs,
    uint8_t *__restrict__ verdict, uint64_t segs, uint32_t *__restrict__ pcb) {
    __shared__ LineTiles<2, LINES> tile;
    const WaveStride ws;
    for (uint64_t base = uniform64(ws.first); base < n; base += ws.step) {
        const uint64_t i = base + ws.lane;
        const bool active = i < n;
        uint32_t w[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] = 0u;
        uint32_t cookie = AIPSTACK_TCP_NO_PCB;
        if (active && verdict[i] == AIPSTACK_RX_ACCEPT) {
            uint64_t S;
            uint32_t len;
            fr.frame(i, S, len);
            aipstack_tcp_pcb_key key;
            uint32_t r[8];
            const int res = tcp_rx_build(FrameLoad{S}, len, r, key);
            if (res == kTcpRxValid) {
#pragma unroll
                for (int q = 0; q < 8; ++q) w[q] = r[q];
                cookie = rxp_lookup(pcbs, n_pcbs, key);
            } else if (res == kTcpRxBadOffset) {
                verdict[i] = (uint8_t)AIPSTACK_RX_DROP_TCP_OFFSET;
            }
        }
        if (active) __builtin_nontemporal_store(cookie, &pcb[i]);
        if constexpr (LINES) {
            // the records below n
            store_wave_lines<2>(tile[ws.wave], ws.lane, segs, base,
                                __builtin_amdgcn_ballot_w64(active), w);
        } else if (active) {
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                __builtin_nontemporal_store(
                    u32x2{w[2 * q], w[2 * q + 1]},
                    reinterpret_cast<global_t<u32x2> *>(segs + i * 32u + q * 8u));
        }
    }
}

template <class Frames>
int launch_parse(const Frames &fr, uint64_t n, const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
                 uint8_t *d_verdict, aipstack_tcp_rx_seg *d_segs, uint32_t *d_pcb, hipStream_t s) {
    unsigned blocks;
    const int st = lane_pass_blocks(n, s, &blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint64_t segs = (uint64_t)(uintptr_t)d_segs;
    if ((segs & 15u) == 0u)
        hipLaunchKernelGGL((tcprx_parse_kernel<Frames, true>), dim3(blocks), dim3(kBlock), 0, s, fr,
                           n, d_pcbs, n_pcbs, d_verdict, segs, d_pcb);
    else
        hipLaunchKernelGGL((tcprx_parse_kernel<Frames, false>), dim3(blocks), dim3(kBlock), 0, s,
                           fr, n, d_pcbs, n_pcbs, d_verdict, segs, d_pcb);
    return check_hip(hipGetLastError());
}

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_tcp_rx_parse(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                                     const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
                                     uint8_t *d_verdict, aipstack_tcp_rx_seg *d_segs,
                                     uint32_t *d_pcb, void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = tcp_rx_parse_check_args(d_base, d_offsets, false, 0, n, d_pcbs, n_pcbs, d_verdict,
                                     d_segs, d_pcb);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_rx_verify(d_base, d_offsets, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const CsrFrames fr{(uint64_t)(uintptr_t)d_base, d_offsets};
    return launch_parse(fr, n, d_pcbs, n_pcbs, d_verdict, d_segs, d_pcb, (hipStream_t)stream);
}

extern "C" int aipstack_tcp_rx_parse_slotted(const void *d_base, uint64_t slot_stride,
                                             const uint32_t *d_len, uint64_t n,
                                             const aipstack_tcp_pcb_key *d_pcbs, uint64_t n_pcbs,
                                             uint8_t *d_verdict, aipstack_tcp_rx_seg *d_segs,
                                             uint32_t *d_pcb, void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = tcp_rx_parse_check_args(d_base, d_len, true, slot_stride, n, d_pcbs, n_pcbs,
                                     d_verdict, d_segs, d_pcb);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_rx_verify_slotted(d_base, slot_stride, d_len, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint32_t cap = (uint32_t)(slot_stride < AIPSTACK_CHKSUM_MAX_LEN ? slot_stride
                                                                           : AIPSTACK_CHKSUM_MAX_LEN);
    const SlotFrames fr{(uint64_t)(uintptr_t)d_base, slot_stride, d_len, cap};
    return launch_parse(fr, n, d_pcbs, n_pcbs, d_verdict, d_segs, d_pcb, (hipStream_t)stream);
}
