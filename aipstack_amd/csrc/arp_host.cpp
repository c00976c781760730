// aipstack_amd -- ARP on receive, the host side (plain C++, no HIP call): the workspace size and
// the argument checks of aipstack_arp_rx_respond / _slotted (the launchers are in
// arp_kernels.hip).

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "aipstack_amd/chksum.h"
#include "arp_common.h"

static_assert(sizeof(aipstack_arp_iface) == 32, "aipstack_arp_iface is 32 bytes");
static_assert(offsetof(aipstack_arp_iface, netmask) == 4 && offsetof(aipstack_arp_iface, mac) == 8 &&
                  offsetof(aipstack_arp_iface, flags) == 14 &&
                  offsetof(aipstack_arp_iface, reserved) == 15,
              "aipstack_arp_iface field offsets");
static_assert(sizeof(aipstack_arp_record) == 16, "aipstack_arp_record is 16 bytes");
static_assert(offsetof(aipstack_arp_record, sender_mac) == 4 && offsetof(aipstack_arp_record, op) == 10 &&
                  offsetof(aipstack_arp_record, flags) == 12 &&
                  offsetof(aipstack_arp_record, status) == 13 &&
                  offsetof(aipstack_arp_record, reserved) == 14,
              "aipstack_arp_record field offsets");

using namespace aipstack_amd;

// One pair of 64-bit counts (replies, seen frames) per tile of kArpTile frames and the totals,
// then per tile the ballot pair of each of its waves.
extern "C" uint64_t aipstack_arp_rx_respond_workspace_bytes(uint64_t n) {
    const uint64_t tiles = (n + kArpTile - 1) / kArpTile;
    return 16u * (tiles + 1) + 16u * kArpTileWaves * tiles;
}

namespace aipstack_amd {

int arp_rx_respond_check_args(const ArpRespondArgs &a) {
    for (const void *p : {a.d_base, a.frames, (const void *)a.h_iface, a.d_status, a.d_arp, a.d_hdr,
                          a.d_hdr_len, a.d_chunk_index, a.d_reply_frame, a.d_seen_frame, a.d_counts,
                          a.d_workspace})
        if (!p) return AIPSTACK_CHKSUM_EINVAL;
    if (a.n > kArpMaxCount || a.hdr_stride < AIPSTACK_ARP_REPLY_HEADER) return AIPSTACK_CHKSUM_EINVAL;
    if (!arp_iface_valid(*a.h_iface)) return AIPSTACK_CHKSUM_EINVAL;
    for (const void *p : {a.d_chunk_index, a.d_reply_frame, a.d_seen_frame, a.d_counts, a.d_workspace})
        if (((uintptr_t)p & 7u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    if (((uintptr_t)a.d_hdr_len & 3u) != 0 || ((uintptr_t)a.d_arp & 3u) != 0)
        return AIPSTACK_CHKSUM_EINVAL;
    if (a.workspace_bytes < aipstack_arp_rx_respond_workspace_bytes(a.n)) return AIPSTACK_CHKSUM_EINVAL;
    if (a.slotted && (a.slot_stride == 0 || a.slot_stride > AIPSTACK_CHKSUM_MAX_SLOT_STRIDE))
        return AIPSTACK_CHKSUM_EINVAL;
    return AIPSTACK_CHKSUM_OK;
}

}  // namespace aipstack_amd
