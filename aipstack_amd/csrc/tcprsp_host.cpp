// aipstack_amd -- TCP segments without a connection, the host side (plain C++, no HIP call): the
// workspace size and the argument checks of aipstack_tcp_rx_respond / _slotted (the launchers
// are in tcprsp_kernels.hip).

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "aipstack_amd/chksum.h"
#include "icmp_common.h"
#include "tcprsp_common.h"

static_assert(sizeof(aipstack_tcp_listener) == 16, "aipstack_tcp_listener is 16 bytes");
static_assert(offsetof(aipstack_tcp_listener, port) == 4 &&
                  offsetof(aipstack_tcp_listener, reserved0) == 6 &&
                  offsetof(aipstack_tcp_listener, cookie) == 8 &&
                  offsetof(aipstack_tcp_listener, reserved1) == 12,
              "aipstack_tcp_listener field offsets");
static_assert(AIPSTACK_TCP_RSP_HEADER == AIPSTACK_TCP_SEGMENT_HEADER, "an RST is a plain segment");

using namespace aipstack_amd;

// One pair of 64-bit counts (RSTs, SYNs) per tile of kTcpRspTile frames and the totals, then per
// tile the ballot pair of each of its waves.
extern "C" uint64_t aipstack_tcp_rx_respond_workspace_bytes(uint64_t n) {
    const uint64_t tiles = (n + kTcpRspTile - 1) / kTcpRspTile;
    return 16u * (tiles + 1) + 16u * kTcpRspTileWaves * tiles;
}

namespace aipstack_amd {

int tcp_rx_respond_check_args(const TcpRespondArgs &a) {
    for (const void *p : {a.d_base, a.frames, (const void *)a.h_iface, a.d_verdict, a.d_segs, a.d_pcb,
                          a.d_status, a.d_listener, a.d_hdr, a.d_hdr_len, a.d_chunk_index,
                          a.d_response_frame, a.d_syn_frame, a.d_counts, a.d_workspace})
        if (!p) return AIPSTACK_CHKSUM_EINVAL;
    if ((a.n_pcbs != 0 && !a.d_pcbs) || (a.n_listeners != 0 && !a.d_listeners))
        return AIPSTACK_CHKSUM_EINVAL;
    if (a.n > kTcpRxMaxCount || a.n_pcbs > kTcpRxMaxCount ||
        a.n_listeners > AIPSTACK_TCP_MAX_LISTENERS)
        return AIPSTACK_CHKSUM_EINVAL;
    if (a.tcp_ttl < 1u || a.tcp_ttl > 255u || a.hdr_stride < AIPSTACK_TCP_RSP_HEADER)
        return AIPSTACK_CHKSUM_EINVAL;
    if (!icmp_iface_valid(*a.h_iface)) return AIPSTACK_CHKSUM_EINVAL;
    for (const void *p : {a.d_segs, a.d_chunk_index, a.d_response_frame, a.d_syn_frame, a.d_counts,
                          a.d_workspace})
        if (((uintptr_t)p & 7u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    for (const void *p : {a.d_pcb, a.d_listener, a.d_hdr_len})
        if (((uintptr_t)p & 3u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    if ((a.n_pcbs != 0 && ((uintptr_t)a.d_pcbs & 7u) != 0) ||
        (a.n_listeners != 0 && ((uintptr_t)a.d_listeners & 7u) != 0))
        return AIPSTACK_CHKSUM_EINVAL;
    if (a.workspace_bytes < aipstack_tcp_rx_respond_workspace_bytes(a.n))
        return AIPSTACK_CHKSUM_EINVAL;
    if (a.slotted && (a.slot_stride == 0 || a.slot_stride > AIPSTACK_CHKSUM_MAX_SLOT_STRIDE))
        return AIPSTACK_CHKSUM_EINVAL;
    return AIPSTACK_CHKSUM_OK;
}

}  // namespace aipstack_amd
