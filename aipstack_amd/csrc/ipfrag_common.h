// aipstack_amd -- UDP send with IPv4 fragmentation: what the host layout (ipfrag_host.cpp) and
// the kernels (ipfrag_kernels.hip) share, so that both count a datagram's fragments and chunks,
// cut its payload and judge its contract with the same text.
#ifndef AIPSTACK_AMD_IPFRAG_COMMON_H
#define AIPSTACK_AMD_IPFRAG_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "tx_producer_common.h"

#if defined(__HIPCC__)
#define AIPSTACK_IPFRAG_HD __host__ __device__ inline
#else
#define AIPSTACK_IPFRAG_HD inline
#endif

namespace aipstack_amd {

// A datagram as sendIp4Dgram / send_fragmented cut it (ip/IpStack.h:404-421, 470-538): the IP
// payload of P = 8 + D bytes (UDP header and data) in S fragments, every one but the last of
// F = Ip4RoundFragLen(20, mtu) - 20 bytes, the last one of up to M = mtu - 20. The data is two
// pieces (as a TCP burst's): at most one fragment holds bytes of both and has two chunks;
// `straddle` is its number, S when there is none.
struct UdpDgramShape {
    bool valid;        // the part of the contract a descriptor alone decides
    bool frag_needed;  // above the MTU with DF set: S = C = 0 (IpErr::FragmentationNeeded, :409-411)
    uint32_t D, P, F, len0;
    uint64_t S, C, straddle;
};

AIPSTACK_IPFRAG_HD UdpDgramShape udp_dgram_shape(const aipstack_udp_dgram &d) {
    UdpDgramShape s;
    const uint64_t D = (uint64_t)d.data_len[0] + d.data_len[1];
    s.valid = d.mtu >= AIPSTACK_UDP_MIN_MTU && 8u + D <= 65535u && d.reserved == 0u &&
              d.hdr[12] == 0x08u && d.hdr[13] == 0x00u && d.hdr[14] == 0x45u && d.hdr[23] == 17u &&
              (d.hdr[20] & ~0x40u) == 0u && d.hdr[21] == 0u;
    s.frag_needed = false;
    s.D = s.P = s.F = s.len0 = 0;
    s.S = s.C = s.straddle = 0;
    if (!s.valid) return s;
    s.D = (uint32_t)D;
    s.P = 8u + s.D;
    s.len0 = d.data_len[0];
    const uint32_t M = (uint32_t)d.mtu - 20u;
    s.F = M & ~7u;  // (M / 8) * 8, at least 232
    const bool both = d.data_len[0] != 0u && d.data_len[1] != 0u;
    if (20u + s.P <= d.mtu) {  // :418-421: the first packet has all the data
        s.S = 1;
        s.straddle = both ? 0u : 1u;
        s.C = s.D == 0u ? 0u : (both ? 2u : 1u);
    } else if ((d.hdr[20] & 0x40u) != 0u) {
        s.frag_needed = true;
    } else {
        s.S = (s.P - M + s.F - 1u) / s.F + 1u;
        // The piece boundary is IP-payload position len0 + 8. It falls between two fragments
        // when that is k * F for a k <= S - 1; else it lies inside fragment (len0 + 8) / F --
        // clamped to S - 1, because the last fragment is longer than F when M % 8 != 0.
        const uint32_t q = (s.len0 + 8u) / s.F, r = (s.len0 + 8u) % s.F;
        const bool two = both && !(r == 0u && q <= s.S - 1u);
        s.straddle = two ? (q < s.S - 1u ? q : s.S - 1u) : s.S;
        s.C = s.S + (two ? 1u : 0u);
    }
    return s;
}

// Fragment k < S of a valid shape: its IP payload is [off, off + len) of the P bytes, its data
// the bytes [a, b) of the UDP payload (fragment 0 starts with the 8 UDP header bytes).
struct UdpFragRange {
    uint32_t off, len, a, b;
};

AIPSTACK_IPFRAG_HD UdpFragRange udp_frag_range(const UdpDgramShape &s, uint64_t k) {
    UdpFragRange f;
    f.off = (uint32_t)k * s.F;  // k < S <= 283, F < 2^16
    f.len = k + 1u < s.S ? s.F : s.P - f.off;
    f.a = k == 0u ? 0u : f.off - 8u;
    f.b = f.off + f.len - 8u;
    return f;
}

// The argument checks of aipstack_udp_tx_fragment (ipfrag_host.cpp; no HIP call).
int udp_tx_fragment_check_args(const void *d_dgrams, const void *d_frag_index,
                               const void *d_chunk_base, uint64_t n_dgrams, uint64_t n_frags,
                               uint64_t n_chunks, const void *d_hdr, uint64_t hdr_stride,
                               const void *d_hdr_len, const void *d_chunk_addr,
                               const void *d_chunk_len, const void *d_chunk_index,
                               const void *d_status, const void *d_dgram_status,
                               const void *d_workspace, uint64_t workspace_bytes);

// The workspace of aipstack_udp_tx_fragment: one 8-byte record per fragment, the chain bounds
// (n_dgrams + 1 entries of 8 bytes), then per datagram the seed (4 bytes) and the chain's sum (2).
struct UdpFragWorkspace {
    uint64_t records, chain_index, seeds, sums, bytes;  // byte offsets, and the total
};

AIPSTACK_IPFRAG_HD UdpFragWorkspace udp_frag_workspace(uint64_t n_dgrams, uint64_t n_frags) {
    UdpFragWorkspace w;
    w.records = 0;
    w.chain_index = 8u * n_frags;
    w.seeds = w.chain_index + 8u * (n_dgrams + 1u);
    w.sums = w.seeds + 4u * n_dgrams;
    w.bytes = (w.sums + 2u * n_dgrams + 7u) & ~(uint64_t)7;
    return w;
}

}  // namespace aipstack_amd

#endif
