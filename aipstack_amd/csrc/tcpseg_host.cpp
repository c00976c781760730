// aipstack_amd -- TCP burst segmentation, the host side (plain C++, no HIP call): the layout of
// a batch of bursts as running sums, the workspace bound and the argument checks of
// aipstack_tcp_tx_segment (the launcher is in tcpseg_kernels.hip).

#include <cstddef>
#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "tcpseg_common.h"

static_assert(sizeof(aipstack_tcp_burst) == 96, "aipstack_tcp_burst is 96 bytes");
static_assert(alignof(aipstack_tcp_burst) == 8, "aipstack_tcp_burst is 8-byte aligned");
static_assert(offsetof(aipstack_tcp_burst, data_len) == 16 && offsetof(aipstack_tcp_burst, seq) == 24 &&
                  offsetof(aipstack_tcp_burst, psh_offset) == 28 &&
                  offsetof(aipstack_tcp_burst, mss) == 32 && offsetof(aipstack_tcp_burst, ip_id) == 34 &&
                  offsetof(aipstack_tcp_burst, flags) == 36 &&
                  offsetof(aipstack_tcp_burst, reserved) == 37 &&
                  offsetof(aipstack_tcp_burst, hdr) == 40,
              "aipstack_tcp_burst field offsets");

using namespace aipstack_amd;

extern "C" int aipstack_tcp_burst_layout(const aipstack_tcp_burst *h_bursts, uint64_t n_bursts,
                                         uint64_t *h_seg_index, uint64_t *h_chunk_base) {
    if (!h_seg_index || !h_chunk_base || (n_bursts != 0 && !h_bursts) || n_bursts > kTxMaxCount)
        return AIPSTACK_CHKSUM_EINVAL;
    uint64_t segs = 0, chunks = 0;
    h_seg_index[0] = 0;
    h_chunk_base[0] = 0;
    for (uint64_t b = 0; b < n_bursts; ++b) {
        const TcpBurstShape s = tcp_burst_shape(h_bursts[b]);
        if (!s.valid) return AIPSTACK_CHKSUM_EINVAL;
        segs += s.S;  // each < 2^32 + 1 and at most 2^40 of them: no overflow
        chunks += s.C;
        h_seg_index[b + 1] = segs;
        h_chunk_base[b + 1] = chunks;
    }
    return AIPSTACK_CHKSUM_OK;
}

// Workspace of n segments: records (8n bytes), seeds (4n), chain sums (2n).
extern "C" uint64_t aipstack_tcp_tx_segment_workspace_bytes(uint64_t n) {
    if (n > kTxMaxCount) n = kTxMaxCount;
    return (14u * n + 7u) & ~(uint64_t)7;
}

namespace aipstack_amd {

int tcp_tx_segment_check_args(const void *d_bursts, const void *d_seg_index,
                              const void *d_chunk_base, uint64_t n_bursts, uint64_t n_segments,
                              uint64_t n_chunks, const void *d_hdr, uint64_t hdr_stride,
                              const void *d_chunk_addr, const void *d_chunk_len,
                              const void *d_chunk_index, const void *d_status,
                              const void *d_workspace, uint64_t workspace_bytes) {
    return tx_producer_check_args({d_bursts, d_seg_index, d_chunk_base, d_hdr, d_chunk_addr,
                                   d_chunk_len, d_chunk_index, d_status},
                                  hdr_stride, AIPSTACK_TCP_SEGMENT_HEADER, n_bursts, n_segments,
                                  n_chunks, d_workspace, workspace_bytes,
                                  aipstack_tcp_tx_segment_workspace_bytes(n_segments));
}

}  // namespace aipstack_amd
