// aipstack_amd -- ICMP on receive, the host side (plain C++, no HIP call): the workspace size
// and the argument checks of aipstack_icmp_rx_respond / _slotted (the launchers are in
// icmp_kernels.hip).

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "aipstack_amd/chksum.h"
#include "icmp_common.h"

static_assert(sizeof(aipstack_icmp_iface) == 32, "aipstack_icmp_iface is 32 bytes");
static_assert(offsetof(aipstack_icmp_iface, bcast_addr) == 4 && offsetof(aipstack_icmp_iface, mtu) == 8 &&
                  offsetof(aipstack_icmp_iface, ip_id) == 10 &&
                  offsetof(aipstack_icmp_iface, ttl) == 12 &&
                  offsetof(aipstack_icmp_iface, flags) == 13 &&
                  offsetof(aipstack_icmp_iface, mac) == 14 &&
                  offsetof(aipstack_icmp_iface, reserved) == 20,
              "aipstack_icmp_iface field offsets");

using namespace aipstack_amd;

// One pair of 64-bit counts (responses, chunks) per block of kIcmpTile frames, and the totals.
extern "C" uint64_t aipstack_icmp_rx_respond_workspace_bytes(uint64_t n) {
    return 16u * ((n + kIcmpTile - 1) / kIcmpTile + 1);
}

namespace aipstack_amd {

int icmp_rx_respond_check_args(const IcmpRespondArgs &a) {
    for (const void *p : {a.d_base, a.frames, (const void *)a.h_iface, a.d_verdict, a.d_status,
                          a.d_hdr, a.d_hdr_len, a.d_chunk_addr, a.d_chunk_len, a.d_chunk_index,
                          a.d_response_frame, a.d_counts, a.d_workspace})
        if (!p) return AIPSTACK_CHKSUM_EINVAL;
    if (a.n > kIcmpMaxCount || a.hdr_stride < AIPSTACK_ICMP_RESPONSE_HEADER)
        return AIPSTACK_CHKSUM_EINVAL;
    if (!icmp_iface_valid(*a.h_iface)) return AIPSTACK_CHKSUM_EINVAL;
    for (const void *p : {a.d_chunk_addr, a.d_chunk_index, a.d_response_frame, a.d_counts, a.d_workspace})
        if (((uintptr_t)p & 7u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    if (((uintptr_t)a.d_hdr_len & 3u) != 0 || ((uintptr_t)a.d_chunk_len & 3u) != 0)
        return AIPSTACK_CHKSUM_EINVAL;
    if (a.workspace_bytes < aipstack_icmp_rx_respond_workspace_bytes(a.n))
        return AIPSTACK_CHKSUM_EINVAL;
    if (a.slotted && (a.slot_stride == 0 || a.slot_stride > AIPSTACK_CHKSUM_MAX_SLOT_STRIDE))
        return AIPSTACK_CHKSUM_EINVAL;
    return AIPSTACK_CHKSUM_OK;
}

}  // namespace aipstack_amd
