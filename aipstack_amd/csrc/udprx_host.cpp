// aipstack_amd -- UDP Rx demux, the host side (plain C++, no HIP call): the workspace size and
// the argument checks of aipstack_udp_rx_demux / _slotted (the launchers are in
// udprx_kernels.hip).

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "aipstack_amd/chksum.h"
#include "icmp_common.h"
#include "udprx_common.h"

static_assert(sizeof(aipstack_udp_listener) == 16 && offsetof(aipstack_udp_listener, port) == 4 &&
                  offsetof(aipstack_udp_listener, flags) == 6 &&
                  offsetof(aipstack_udp_listener, cookie) == 8,
              "aipstack_udp_listener is 16 bytes");
static_assert(sizeof(aipstack_udp_rx_dgram) == 32, "aipstack_udp_rx_dgram is 32 bytes");
static_assert(offsetof(aipstack_udp_rx_dgram, remote_port) == 8 &&
                  offsetof(aipstack_udp_rx_dgram, data_off) == 12 &&
                  offsetof(aipstack_udp_rx_dgram, data_len) == 14 &&
                  offsetof(aipstack_udp_rx_dgram, listeners) == 16 &&
                  offsetof(aipstack_udp_rx_dgram, assoc) == 24 &&
                  offsetof(aipstack_udp_rx_dgram, flags) == 28 &&
                  offsetof(aipstack_udp_rx_dgram, ttl) == 29 &&
                  offsetof(aipstack_udp_rx_dgram, reserved) == 30,
              "aipstack_udp_rx_dgram field offsets");

using namespace aipstack_amd;

// Per block of kUdpRxTile frames one pair of 64-bit counts (deliveries, unreach requests) and
// four 64-frame delivery ballots; and the pair of totals.
extern "C" uint64_t aipstack_udp_rx_demux_workspace_bytes(uint64_t n) {
    const uint64_t tiles = udp_rx_tiles(n);
    return 8u * (udp_rx_ballot_word(tiles) + kUdpRxTileWaves * tiles);
}

namespace aipstack_amd {

int udp_rx_demux_check_args(const UdpRxDemuxArgs &a) {
    for (const void *p : {a.d_base, a.frames, (const void *)a.h_iface, a.d_verdict, a.d_dgrams,
                          a.d_unreach_code, a.d_deliver_frame, a.d_counts, a.d_workspace})
        if (!p) return AIPSTACK_CHKSUM_EINVAL;
    if ((a.n_assocs != 0 && !a.d_assocs) || (a.n_listeners != 0 && !a.d_listeners))
        return AIPSTACK_CHKSUM_EINVAL;
    if (a.n > kUdpRxMaxCount || a.n_assocs > kUdpRxMaxCount ||
        a.n_listeners > AIPSTACK_UDP_MAX_LISTENERS)
        return AIPSTACK_CHKSUM_EINVAL;
    if (!icmp_iface_valid(*a.h_iface)) return AIPSTACK_CHKSUM_EINVAL;
    for (const void *p : {a.d_dgrams, a.d_deliver_frame, a.d_counts, a.d_workspace})
        if (((uintptr_t)p & 7u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    if ((a.n_assocs != 0 && ((uintptr_t)a.d_assocs & 7u) != 0) ||
        (a.n_listeners != 0 && ((uintptr_t)a.d_listeners & 7u) != 0))
        return AIPSTACK_CHKSUM_EINVAL;
    if (a.workspace_bytes < aipstack_udp_rx_demux_workspace_bytes(a.n))
        return AIPSTACK_CHKSUM_EINVAL;
    if (a.slotted && (a.slot_stride == 0 || a.slot_stride > AIPSTACK_CHKSUM_MAX_SLOT_STRIDE))
        return AIPSTACK_CHKSUM_EINVAL;
    return AIPSTACK_CHKSUM_OK;
}

}  // namespace aipstack_amd
