// aipstack_amd -- TCP segments without data, the host side (plain C++, no HIP call): the
// workspace size and the argument checks of aipstack_tcp_tx_control (the launcher is in
// tcpctl_kernels.hip).

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "aipstack_amd/chksum.h"
#include "icmp_common.h"
#include "tcpctl_common.h"

static_assert(sizeof(aipstack_tcp_ctl) == 32 && alignof(aipstack_tcp_ctl) == 4,
              "aipstack_tcp_ctl is 32 bytes");
static_assert(offsetof(aipstack_tcp_ctl, remote_addr) == 4 && offsetof(aipstack_tcp_ctl, local_port) == 8 &&
                  offsetof(aipstack_tcp_ctl, remote_port) == 10 && offsetof(aipstack_tcp_ctl, seq) == 12 &&
                  offsetof(aipstack_tcp_ctl, ack) == 16 && offsetof(aipstack_tcp_ctl, window) == 20 &&
                  offsetof(aipstack_tcp_ctl, mss) == 22 && offsetof(aipstack_tcp_ctl, flags) == 24 &&
                  offsetof(aipstack_tcp_ctl, options) == 25 &&
                  offsetof(aipstack_tcp_ctl, wnd_scale) == 26 &&
                  offsetof(aipstack_tcp_ctl, reserved0) == 27 &&
                  offsetof(aipstack_tcp_ctl, reserved1) == 28,
              "aipstack_tcp_ctl field offsets");
static_assert(AIPSTACK_TCP_CTL_MAX_HEADER == AIPSTACK_TCP_SEGMENT_HEADER + 8u, "two options of 4 bytes");

using namespace aipstack_amd;

// One pair of 64-bit counts (emitted, invalid) per tile of kTcpCtlTile descriptors and the
// totals, then per tile the ballot of valid descriptors of each of its waves.
extern "C" uint64_t aipstack_tcp_tx_control_workspace_bytes(uint64_t n) {
    const uint64_t tiles = (n + kTcpCtlTile - 1) / kTcpCtlTile;
    return 16u * (tiles + 1) + 8u * kTcpCtlTileWaves * tiles;
}

namespace aipstack_amd {

int tcp_tx_control_check_args(const TcpControlArgs &a) {
    for (const void *p : {a.d_ctl, (const void *)a.h_iface, a.d_hdr, a.d_hdr_len, a.d_chunk_index,
                          a.d_status, a.d_counts, a.d_workspace})
        if (!p) return AIPSTACK_CHKSUM_EINVAL;
    if (a.n > kTcpCtlMaxCount || a.tcp_ttl < 1u || a.tcp_ttl > 255u ||
        a.hdr_stride < AIPSTACK_TCP_CTL_MAX_HEADER)
        return AIPSTACK_CHKSUM_EINVAL;
    if (!icmp_iface_valid(*a.h_iface)) return AIPSTACK_CHKSUM_EINVAL;
    for (const void *p : {a.d_ctl, a.d_chunk_index, a.d_counts, a.d_workspace})
        if (((uintptr_t)p & 7u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    if (((uintptr_t)a.d_hdr_len & 3u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    if (a.workspace_bytes < aipstack_tcp_tx_control_workspace_bytes(a.n))
        return AIPSTACK_CHKSUM_EINVAL;
    return AIPSTACK_CHKSUM_OK;
}

}  // namespace aipstack_amd
