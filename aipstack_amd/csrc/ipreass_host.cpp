// aipstack_amd -- IPv4 reassembly on receive, the host side (plain C++, no HIP call): the
// workspace size and the argument checks of aipstack_ip4_rx_reassemble / _slotted (the launchers
// are in ipreass_kernels.hip).

#include <cstddef>
#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "ipreass_common.h"

static_assert(sizeof(aipstack_ip4_dgram) == 16, "aipstack_ip4_dgram is 16 bytes");
static_assert(offsetof(aipstack_ip4_dgram, last_frame) == 4 &&
                  offsetof(aipstack_ip4_dgram, data_len) == 8 &&
                  offsetof(aipstack_ip4_dgram, proto) == 10 &&
                  offsetof(aipstack_ip4_dgram, verdict) == 11 &&
                  offsetof(aipstack_ip4_dgram, reserved) == 12,
              "aipstack_ip4_dgram field offsets");
static_assert(sizeof(aipstack_amd::ReassRec) == 16, "one fragment record is 16 bytes");

using namespace aipstack_amd;

extern "C" uint64_t aipstack_ip4_reass_workspace_bytes(uint64_t n) {
    return reass_workspace(n).total;
}

namespace aipstack_amd {

int ip4_rx_reassemble_check_args(const void *d_base, const void *frames, bool slotted,
                                 uint64_t slot_stride, uint64_t n, uint32_t max_reass_size,
                                 const void *d_verdict, const void *d_chunk_addr,
                                 const void *d_chunk_len, const void *d_next, const void *d_head,
                                 const void *d_dgram, const void *d_workspace,
                                 uint64_t workspace_bytes) {
    if (!d_base || !frames || !d_verdict || !d_chunk_addr || !d_chunk_len || !d_next || !d_head ||
        !d_dgram || !d_workspace)
        return AIPSTACK_CHKSUM_EINVAL;
    if (n > kReassMaxCount) return AIPSTACK_CHKSUM_EINVAL;
    if (max_reass_size < kReassMinSize || max_reass_size > kReassMaxSize)
        return AIPSTACK_CHKSUM_EINVAL;
    if (((uintptr_t)d_chunk_addr & 7u) != 0 || ((uintptr_t)d_chunk_len & 3u) != 0 ||
        ((uintptr_t)d_next & 3u) != 0 || ((uintptr_t)d_head & 3u) != 0 ||
        ((uintptr_t)d_dgram & 3u) != 0 || ((uintptr_t)d_workspace & 7u) != 0)
        return AIPSTACK_CHKSUM_EINVAL;
    if (workspace_bytes < reass_workspace(n).total) return AIPSTACK_CHKSUM_EINVAL;
    if (slotted && (slot_stride == 0 || slot_stride > AIPSTACK_CHKSUM_MAX_SLOT_STRIDE))
        return AIPSTACK_CHKSUM_EINVAL;
    return AIPSTACK_CHKSUM_OK;
}

}  // namespace aipstack_amd
