// aipstack_amd -- TCP burst segmentation: what the host layout (tcpseg_host.cpp) and the
// kernels (tcpseg_kernels.hip) share, so that both count a burst's segments and chunks, and
// judge its contract, with the same text.
#ifndef AIPSTACK_AMD_TCPSEG_COMMON_H
#define AIPSTACK_AMD_TCPSEG_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "tx_producer_common.h"

#if defined(__HIPCC__)
#define AIPSTACK_TCPSEG_HD __host__ __device__ inline
#else
#define AIPSTACK_TCPSEG_HD inline
#endif

namespace aipstack_amd {

// A burst as pcb_output_active's loop cuts it (tcp/IpTcpProto_output.h:1069-1090): D data bytes
// in S segments of mss bytes (the last one shorter), C chunks. The range is two pieces of the
// circular send buffer (utils/TcpRingBufferUtils.h:51,113): at most one segment holds bytes of
// both and has two chunks; `straddle` is its number, S when there is none.
struct TcpBurstShape {
    bool valid;
    uint64_t D, S, C, straddle;
};

AIPSTACK_TCPSEG_HD TcpBurstShape tcp_burst_shape(const aipstack_tcp_burst &b) {
    TcpBurstShape s;
    s.D = (uint64_t)b.data_len[0] + b.data_len[1];
    s.valid = b.mss >= 1u && 40u + (uint32_t)b.mss <= 65535u && s.D < (1ull << 32) &&
              (b.flags & ~AIPSTACK_TCP_BURST_FIN) == 0u && b.reserved[0] == 0u &&
              b.reserved[1] == 0u && b.reserved[2] == 0u && b.hdr[12] == 0x08u &&
              b.hdr[13] == 0x00u && b.hdr[14] == 0x45u && b.hdr[23] == 6u;
    s.S = s.C = s.straddle = 0;
    if (!s.valid) return s;
    const uint64_t mss = b.mss;
    if (s.D != 0) {
        s.S = (s.D + mss - 1) / mss;
        const bool two = b.data_len[0] != 0u && b.data_len[1] != 0u && b.data_len[0] % mss != 0u;
        s.straddle = two ? b.data_len[0] / mss : s.S;
        s.C = s.S + (two ? 1u : 0u);
    } else if (b.flags & AIPSTACK_TCP_BURST_FIN) {
        s.S = 1;  // FIN alone: one segment without data
        s.straddle = 1;
    }
    return s;
}

// The argument checks of aipstack_tcp_tx_segment (tcpseg_host.cpp; no HIP call).
int tcp_tx_segment_check_args(const void *d_bursts, const void *d_seg_index,
                              const void *d_chunk_base, uint64_t n_bursts, uint64_t n_segments,
                              uint64_t n_chunks, const void *d_hdr, uint64_t hdr_stride,
                              const void *d_chunk_addr, const void *d_chunk_len,
                              const void *d_chunk_index, const void *d_status,
                              const void *d_workspace, uint64_t workspace_bytes);

}  // namespace aipstack_amd

#endif
