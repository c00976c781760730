// aipstack_amd -- UDP Rx demux: what the host code (udprx_host.cpp), the kernels
// (udprx_kernels.hip) and the stand-alone test (tests/cpp/udprx_table_test.cpp) share as plain
// C++: the record of one UDP datagram (IpUdpProto::recvIp4Dgram, udp/IpUdpProto.h:470-506), the
// association's eligibility (:527-537) and the listener match (incomingPacketMatches, :255-289),
// built from the same text wherever the frame's bytes are read from.
#ifndef AIPSTACK_AMD_UDPRX_COMMON_H
#define AIPSTACK_AMD_UDPRX_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "pcb_lookup.h"

#if defined(__HIPCC__)
#define AIPSTACK_UDPRX_HD __host__ __device__ inline
#else
#define AIPSTACK_UDPRX_HD inline
#endif

namespace aipstack_amd {

constexpr uint64_t kUdpRxMaxCount = 1ull << 40;  // frames, table entries of one call
constexpr uint32_t kUdpRxTile = 256;             // frames per block of the counts and the scan
constexpr uint32_t kUdpRxTileWaves = 4;          // 64-frame ballots per tile

// The workspace as 64-bit words: a pair of counts (deliveries, unreach requests) per tile and
// the totals behind them (pair_scan.h), then per tile the four 64-frame delivery ballots.
AIPSTACK_UDPRX_HD uint64_t udp_rx_tiles(uint64_t n) { return (n + kUdpRxTile - 1) / kUdpRxTile; }
AIPSTACK_UDPRX_HD uint64_t udp_rx_ballot_word(uint64_t tiles) { return 2u * (tiles + 1u); }

AIPSTACK_UDPRX_HD uint32_t udprx_bswap32(uint32_t x) {
    return x >> 24 | (x >> 8 & 0xFF00u) | (x << 8 & 0xFF0000u) | x << 24;
}
AIPSTACK_UDPRX_HD uint32_t udprx_be16lo(uint32_t w) {  // the big-endian 16 bits in w's bytes 0-1
    return (w & 0xFFu) << 8 | (w >> 8 & 0xFFu);
}

// A listener as the passes hold it: aipstack_udp_listener's first two dwords (the port in the
// low half of the second, the flags in its bits 16-23; the reserved byte is not looked at).
struct UdpLis {
    uint32_t iface_addr, port_flags;
};

// What the matches below need of one datagram.
struct UdpRxFacts {
    uint32_t dst_port;
    bool dst_local, is_bcast;
};

// incomingPacketMatches (:262-288) for a listener of this interface (or of any: the host
// uploads no other, :266). `local_addr`: the interface's address (ip4AddrIsLocalAddr, :283).
AIPSTACK_UDPRX_HD bool udp_listener_matches(const UdpLis &l, const UdpRxFacts &d,
                                            uint32_t local_addr) {
    const uint32_t port = l.port_flags & 0xFFFFu, flags = l.port_flags >> 16;
    if (port != 0u && d.dst_port != port) return false;                                 // :262
    if ((flags & AIPSTACK_UDP_LIS_BROADCAST) == 0u && d.is_bcast) return false;         // :274
    if ((flags & AIPSTACK_UDP_LIS_NONLOCAL) == 0u && !d.is_bcast && !d.dst_local)       // :278
        return false;
    if (l.iface_addr != 0u && l.iface_addr != local_addr) return false;                 // :282
    return true;
}

// The `assoc` field for the outcome of the table search: the association is eligible when it is
// found and accepts a non-local destination (cookie bit 31) or the destination is local (:535).
AIPSTACK_UDPRX_HD uint32_t udp_assoc_of(bool found, uint32_t cookie, bool dst_local) {
    if (!found) return AIPSTACK_UDP_NO_ASSOC;
    if ((cookie & AIPSTACK_UDP_ASSOC_NONLOCAL) == 0u && !dst_local) return AIPSTACK_UDP_NO_ASSOC;
    return cookie & ~AIPSTACK_UDP_ASSOC_NONLOCAL;
}

// The record of one frame of `len` bytes with Rx verify's `verdict`, read through `ld(off)` = the
// little-endian dword at frame bytes [off, off + 4), which is only called for bytes inside the
// frame (at most the first 82). False: no UDP datagram to dispatch, w stays as it is. True:
// w[8] = the record as dwords (aipstack_udp_rx_dgram, host byte order) with listeners 0 and
// assoc AIPSTACK_UDP_NO_ASSOC, for the caller to complete; key = the association's lookup tuple;
// d = what the listener match needs.
template <class Load>
AIPSTACK_UDPRX_HD bool udp_rx_build(const Load &ld, uint32_t len, uint32_t verdict,
                                    uint32_t local_addr, uint32_t bcast_addr, uint32_t w[8],
                                    aipstack_tcp_pcb_key &key, UdpRxFacts &d) {
    if (verdict != AIPSTACK_RX_ACCEPT && verdict != AIPSTACK_RX_ACCEPT_NO_CHKSUM) return false;
    if (len < 14u + 20u + 8u) return false;
    const uint32_t v = ld(14u);                        // version/IHL, DSCP, total length
    const uint32_t hl = (v & 0xFu) * 4u;
    const uint32_t total = udprx_be16lo(v >> 16);
    const uint32_t tp = ld(20u);                       // flags / offset, TTL, protocol
    if ((tp >> 24) != 17u) return false;
    // what Rx verify has checked of an accepted frame (ip/IpStack.h:938-990,
    // udp/IpUdpProto.h:473-489), restated so that every read below lies inside the frame
    if (hl < 20u || total < hl + 8u || 14u + total > len) return false;
    const uint32_t T = 14u + hl;                       // the UDP header
    const uint32_t ports = ld(T), lc = ld(T + 4u);     // length, checksum
    const uint32_t udp_len = udprx_be16lo(lc);
    if (udp_len < 8u || udp_len > total - hl) return false;                             // :485
    const uint32_t src = udprx_bswap32(ld(26u)), dst = udprx_bswap32(ld(30u));
    const uint32_t sport = udprx_be16lo(ports), dport = udprx_be16lo(ports >> 16);
    d.dst_port = dport;
    d.dst_local = dst == local_addr;                                                    // :504
    d.is_bcast = dst == 0xFFFFFFFFu || dst == bcast_addr;                               // :270
    key.local_addr = dst;                                                               // :527
    key.remote_addr = src;
    key.local_port = (uint16_t)dport;
    key.remote_port = (uint16_t)sport;
    key.cookie = 0u;
    const uint32_t flags = AIPSTACK_UDP_DGRAM_VALID |
                           ((lc >> 16) != 0u ? AIPSTACK_UDP_DGRAM_HAS_CHKSUM : 0u) |    // :637
                           (d.dst_local ? AIPSTACK_UDP_DGRAM_DST_LOCAL : 0u) |
                           (d.is_bcast ? AIPSTACK_UDP_DGRAM_DST_BCAST : 0u);
    w[0] = src;
    w[1] = dst;
    w[2] = sport | dport << 16;
    w[3] = (T + 8u) | (udp_len - 8u) << 16;            // the truncation to the UDP length, :492
    w[4] = w[5] = 0u;
    w[6] = AIPSTACK_UDP_NO_ASSOC;
    w[7] = flags | (tp >> 16 & 0xFFu) << 8;            // TTL (frame byte 22)
    return true;
}

// A whole frame's outcome as the demux pass computes it, for a caller that holds the tables in
// host memory (the stand-alone test; the kernel runs the same steps with the listeners in LDS).
// Returns the unreach code; `deliver`: an eligible association or a matching listener.
template <class Load, class LoadEntry>
AIPSTACK_UDPRX_HD uint32_t udp_rx_demux_frame(const Load &ld, uint32_t len, uint32_t verdict,
                                              uint32_t local_addr, uint32_t bcast_addr,
                                              const LoadEntry &entry, uint64_t n_assocs,
                                              const aipstack_udp_listener *lis, uint32_t n_lis,
                                              uint32_t w[8], bool &deliver) {
    aipstack_tcp_pcb_key key;
    UdpRxFacts d;
    deliver = false;
    for (int q = 0; q < 8; ++q) w[q] = 0u;
    if (!udp_rx_build(ld, len, verdict, local_addr, bcast_addr, w, key, d))
        return AIPSTACK_ICMP_NO_UNREACH;
    uint32_t cookie = 0u;
    const bool found = pcb_table_find(entry, n_assocs, key, cookie);
    w[6] = udp_assoc_of(found, cookie, d.dst_local);
    uint64_t mask = 0;
    for (uint32_t k = 0; k < n_lis; ++k) {
        const UdpLis l{lis[k].iface_addr, (uint32_t)lis[k].port | (uint32_t)lis[k].flags << 16};
        if (udp_listener_matches(l, d, local_addr)) mask |= 1ull << k;
    }
    w[4] = (uint32_t)mask;
    w[5] = (uint32_t)(mask >> 32);
    deliver = w[6] != AIPSTACK_UDP_NO_ASSOC || mask != 0u;
    return d.dst_local && !deliver ? 3u : (uint32_t)AIPSTACK_ICMP_NO_UNREACH;           // :611
}

// The argument checks of aipstack_udp_rx_demux / _slotted (udprx_host.cpp; no HIP call).
// frames: d_offsets or d_len; slot_stride is checked when `slotted`.
struct UdpRxDemuxArgs {
    const void *d_base, *frames;
    bool slotted;
    uint64_t slot_stride, n;
    const aipstack_icmp_iface *h_iface;
    const void *d_assocs;
    uint64_t n_assocs;
    const void *d_listeners;
    uint32_t n_listeners;
    const void *d_verdict, *d_dgrams, *d_unreach_code, *d_deliver_frame, *d_counts, *d_workspace;
    uint64_t workspace_bytes;
};
int udp_rx_demux_check_args(const UdpRxDemuxArgs &a);

}  // namespace aipstack_amd

#endif
