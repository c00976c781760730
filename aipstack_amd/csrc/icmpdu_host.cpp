// aipstack_amd -- received ICMP Destination Unreachable, the host side (plain C++, no HIP call):
// the workspace size and the argument checks of aipstack_icmp_rx_unreach / _slotted (the
// launchers are in icmpdu_kernels.hip).

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "aipstack_amd/chksum.h"
#include "icmp_common.h"
#include "icmpdu_common.h"

static_assert(sizeof(aipstack_icmp_du_record) == 32, "aipstack_icmp_du_record is 32 bytes");
static_assert(offsetof(aipstack_icmp_du_record, remote_addr) == 4 &&
                  offsetof(aipstack_icmp_du_record, local_port) == 8 &&
                  offsetof(aipstack_icmp_du_record, remote_port) == 10 &&
                  offsetof(aipstack_icmp_du_record, seq) == 12 &&
                  offsetof(aipstack_icmp_du_record, rest) == 16 &&
                  offsetof(aipstack_icmp_du_record, pcb) == 20 &&
                  offsetof(aipstack_icmp_du_record, ip_off) == 24 &&
                  offsetof(aipstack_icmp_du_record, l4_len) == 26 &&
                  offsetof(aipstack_icmp_du_record, code) == 28 &&
                  offsetof(aipstack_icmp_du_record, proto) == 29 &&
                  offsetof(aipstack_icmp_du_record, ttl) == 30 &&
                  offsetof(aipstack_icmp_du_record, hl) == 31,
              "aipstack_icmp_du_record field offsets");

using namespace aipstack_amd;

// Per block of kIcmpDuTile frames one pair of 64-bit counts (frames with a PCB, valid records) and
// four 64-frame ballots of the frames with a PCB; and the pair of totals.
extern "C" uint64_t aipstack_icmp_rx_unreach_workspace_bytes(uint64_t n) {
    const uint64_t tiles = icmp_du_tiles(n);
    return 8u * (icmp_du_ballot_word(tiles) + kIcmpDuTileWaves * tiles);
}

namespace aipstack_amd {

int icmp_rx_unreach_check_args(const IcmpUnreachArgs &a) {
    for (const void *p : {a.d_base, a.frames, (const void *)a.h_iface, a.d_verdict, a.d_status,
                          a.d_records, a.d_pcb_frame, a.d_counts, a.d_workspace})
        if (!p) return AIPSTACK_CHKSUM_EINVAL;
    if (a.n_pcbs != 0 && !a.d_pcbs) return AIPSTACK_CHKSUM_EINVAL;
    if (a.n > kIcmpDuMaxCount || a.n_pcbs > kIcmpDuMaxCount) return AIPSTACK_CHKSUM_EINVAL;
    if (!icmp_iface_valid(*a.h_iface)) return AIPSTACK_CHKSUM_EINVAL;
    for (const void *p : {a.d_records, a.d_pcb_frame, a.d_counts, a.d_workspace})
        if (((uintptr_t)p & 7u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    if (a.n_pcbs != 0 && ((uintptr_t)a.d_pcbs & 7u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    if (a.workspace_bytes < aipstack_icmp_rx_unreach_workspace_bytes(a.n))
        return AIPSTACK_CHKSUM_EINVAL;
    if (a.slotted && (a.slot_stride == 0 || a.slot_stride > AIPSTACK_CHKSUM_MAX_SLOT_STRIDE))
        return AIPSTACK_CHKSUM_EINVAL;
    return AIPSTACK_CHKSUM_OK;
}

}  // namespace aipstack_amd
