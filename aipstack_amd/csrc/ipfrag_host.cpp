// aipstack_amd -- UDP send with IPv4 fragmentation, the host side (plain C++, no HIP call): the
// layout of a batch of datagrams as running sums, the workspace bound and the argument checks of
// aipstack_udp_tx_fragment (the launcher is in ipfrag_kernels.hip).

#include <cstddef>
#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "ipfrag_common.h"

static_assert(sizeof(aipstack_udp_dgram) == 80, "aipstack_udp_dgram is 80 bytes");
static_assert(alignof(aipstack_udp_dgram) == 8, "aipstack_udp_dgram is 8-byte aligned");
static_assert(offsetof(aipstack_udp_dgram, data_len) == 16 && offsetof(aipstack_udp_dgram, mtu) == 24 &&
                  offsetof(aipstack_udp_dgram, ip_id) == 26 &&
                  offsetof(aipstack_udp_dgram, reserved) == 28 &&
                  offsetof(aipstack_udp_dgram, hdr) == 32,
              "aipstack_udp_dgram field offsets");

using namespace aipstack_amd;

extern "C" int aipstack_udp_dgram_layout(const aipstack_udp_dgram *h_dgrams, uint64_t n_dgrams,
                                         uint64_t *h_frag_index, uint64_t *h_chunk_base,
                                         uint8_t *h_status) {
    if (!h_frag_index || !h_chunk_base || (n_dgrams != 0 && !h_dgrams) || n_dgrams > kTxMaxCount)
        return AIPSTACK_CHKSUM_EINVAL;
    uint64_t frags = 0, chunks = 0;
    h_frag_index[0] = 0;
    h_chunk_base[0] = 0;
    for (uint64_t d = 0; d < n_dgrams; ++d) {
        const UdpDgramShape s = udp_dgram_shape(h_dgrams[d]);
        if (!s.valid) return AIPSTACK_CHKSUM_EINVAL;
        frags += s.S;  // each at most 283 and at most 2^40 of them: no overflow
        chunks += s.C;
        h_frag_index[d + 1] = frags;
        h_chunk_base[d + 1] = chunks;
        if (h_status)
            h_status[d] = (uint8_t)(s.frag_needed ? AIPSTACK_TX_FRAG_NEEDED : AIPSTACK_RX_ACCEPT);
    }
    return AIPSTACK_CHKSUM_OK;
}

extern "C" uint64_t aipstack_udp_tx_fragment_workspace_bytes(uint64_t n_dgrams, uint64_t n_frags) {
    if (n_dgrams > kTxMaxCount) n_dgrams = kTxMaxCount;
    if (n_frags > kTxMaxCount) n_frags = kTxMaxCount;
    return udp_frag_workspace(n_dgrams, n_frags).bytes;
}

namespace aipstack_amd {

int udp_tx_fragment_check_args(const void *d_dgrams, const void *d_frag_index,
                               const void *d_chunk_base, uint64_t n_dgrams, uint64_t n_frags,
                               uint64_t n_chunks, const void *d_hdr, uint64_t hdr_stride,
                               const void *d_hdr_len, const void *d_chunk_addr,
                               const void *d_chunk_len, const void *d_chunk_index,
                               const void *d_status, const void *d_dgram_status,
                               const void *d_workspace, uint64_t workspace_bytes) {
    return tx_producer_check_args({d_dgrams, d_frag_index, d_chunk_base, d_hdr, d_hdr_len,
                                   d_chunk_addr, d_chunk_len, d_chunk_index, d_status,
                                   d_dgram_status},
                                  hdr_stride, AIPSTACK_UDP_FIRST_FRAGMENT_HEADER, n_dgrams, n_frags,
                                  n_chunks, d_workspace, workspace_bytes,
                                  aipstack_udp_tx_fragment_workspace_bytes(n_dgrams, n_frags));
}

}  // namespace aipstack_amd
