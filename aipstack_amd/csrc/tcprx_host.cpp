// aipstack_amd -- TCP Rx parse, the host side (plain C++, no HIP call): the PCB table's sort
// into the order the kernel searches (the comparison of tcprx_common.h) and the argument checks
// of aipstack_tcp_rx_parse / _slotted (the launchers are in tcprx_kernels.hip).

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "tcprx_common.h"

static_assert(sizeof(aipstack_tcp_rx_seg) == 32, "aipstack_tcp_rx_seg is 32 bytes");
static_assert(offsetof(aipstack_tcp_rx_seg, remote_port) == 8 &&
                  offsetof(aipstack_tcp_rx_seg, seq_num) == 12 &&
                  offsetof(aipstack_tcp_rx_seg, flags) == 20 &&
                  offsetof(aipstack_tcp_rx_seg, data_off) == 24 &&
                  offsetof(aipstack_tcp_rx_seg, mss) == 28 &&
                  offsetof(aipstack_tcp_rx_seg, wnd_scale) == 30 &&
                  offsetof(aipstack_tcp_rx_seg, opts) == 31,
              "aipstack_tcp_rx_seg field offsets");
static_assert(sizeof(aipstack_tcp_pcb_key) == 16 && offsetof(aipstack_tcp_pcb_key, local_port) == 8 &&
                  offsetof(aipstack_tcp_pcb_key, remote_port) == 10 &&
                  offsetof(aipstack_tcp_pcb_key, cookie) == 12,
              "aipstack_tcp_pcb_key is 16 bytes");

using namespace aipstack_amd;

extern "C" int aipstack_tcp_pcb_table_sort(aipstack_tcp_pcb_key *h_keys, uint64_t n) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    if (!h_keys || n > kTcpRxMaxCount) return AIPSTACK_CHKSUM_EINVAL;
    // (sorted even when the table is rejected: a permutation of the input either way)
    std::sort(h_keys, h_keys + n, [](const aipstack_tcp_pcb_key &a, const aipstack_tcp_pcb_key &b) {
        return tcp_pcb_key_compare(a, b) < 0;
    });
    for (uint64_t i = 0; i < n; ++i) {
        if (h_keys[i].cookie == AIPSTACK_TCP_NO_PCB) return AIPSTACK_CHKSUM_EINVAL;
        if (i != 0 && tcp_pcb_key_compare(h_keys[i - 1], h_keys[i]) == 0)
            return AIPSTACK_CHKSUM_EINVAL;
    }
    return AIPSTACK_CHKSUM_OK;
}

namespace aipstack_amd {

int tcp_rx_parse_check_args(const void *d_base, const void *frames, bool slotted,
                            uint64_t slot_stride, uint64_t n, const void *d_pcbs, uint64_t n_pcbs,
                            const void *d_verdict, const void *d_segs, const void *d_pcb) {
    if (!d_base || !frames || !d_verdict || !d_segs || !d_pcb || (n_pcbs != 0 && !d_pcbs))
        return AIPSTACK_CHKSUM_EINVAL;
    if (n > kTcpRxMaxCount || n_pcbs > kTcpRxMaxCount) return AIPSTACK_CHKSUM_EINVAL;
    if (((uintptr_t)d_segs & 7u) != 0 || ((uintptr_t)d_pcb & 3u) != 0 ||
        (n_pcbs != 0 && ((uintptr_t)d_pcbs & 7u) != 0))
        return AIPSTACK_CHKSUM_EINVAL;
    if (slotted && (slot_stride == 0 || slot_stride > AIPSTACK_CHKSUM_MAX_SLOT_STRIDE))
        return AIPSTACK_CHKSUM_EINVAL;
    return AIPSTACK_CHKSUM_OK;
}

}  // namespace aipstack_amd
