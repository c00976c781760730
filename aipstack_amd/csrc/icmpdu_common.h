// aipstack_amd -- received ICMP Destination Unreachable: what the host code (icmpdu_host.cpp), the
// kernels (icmpdu_kernels.hip) and the stand-alone test (tests/cpp/icmp_du_build_test.cpp) share as
// plain C++: the tests of recvIcmp4Dgram on such a message (ip/IpStack.h:1093-1148), the parse of
// the quoted IPv4 header (handleIcmp4DestUnreach, :1192-1249), and what the TCP handler reads of
// the quoted bytes before find_pcb (tcp/IpTcpProto_input.h:154-182), built from the same text
// wherever the frame's bytes are read from.
#ifndef AIPSTACK_AMD_ICMPDU_COMMON_H
#define AIPSTACK_AMD_ICMPDU_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "icmp_common.h"
#include "pcb_lookup.h"

namespace aipstack_amd {

constexpr uint64_t kIcmpDuMaxCount = 1ull << 40;  // frames, table entries of one call
constexpr uint32_t kIcmpDuTile = 256;             // frames per block of the counts and the scan
constexpr uint32_t kIcmpDuTileWaves = 4;          // 64-frame ballots per tile

// The workspace as 64-bit words: a pair of counts (frames with a PCB, valid records) per tile and
// the totals behind them (pair_scan.h), then per tile the four 64-frame ballots of the frames
// with a PCB.
AIPSTACK_ICMP_HD uint64_t icmp_du_tiles(uint64_t n) { return (n + kIcmpDuTile - 1) / kIcmpDuTile; }
AIPSTACK_ICMP_HD uint64_t icmp_du_ballot_word(uint64_t tiles) { return 2u * (tiles + 1u); }

// The record of one frame of `len` bytes with Rx verify's `verdict`, read through `ld(off)` = the
// little-endian dword at frame bytes [off, off + 4), which is only called for bytes inside the
// frame (at most the first 150). False: no Destination Unreachable the reference would hand to a
// protocol handler, w stays as it is. True: w[8] = the record as dwords (aipstack_icmp_du_record,
// host byte order) with pcb AIPSTACK_TCP_NO_PCB; `lookup`: the TCP handler goes on to find_pcb
// with `key` (quoted protocol 6, code 4, at least 8 quoted L4 bytes).
template <class Load>
AIPSTACK_ICMP_HD bool icmp_du_build(const Load &ld, uint32_t len, uint32_t verdict,
                                    uint32_t local_addr, uint32_t bcast_addr, uint32_t w[8],
                                    aipstack_tcp_pcb_key &key, bool &lookup) {
    lookup = false;
    if (verdict != AIPSTACK_RX_ACCEPT) return false;
    if (len < 14u + 20u + 8u) return false;
    const uint32_t v = ld(14u);  // version/IHL, DSCP, total length
    const uint32_t hl = (v & 0xFu) * 4u;
    const uint32_t total = icmp_bswap16(v >> 16);
    // what Rx verify has checked of a frame accepted as ICMP (ip/IpStack.h:938-990, :1116),
    // restated so that every read below lies inside the frame
    if (hl < 20u || total < hl + 8u || 14u + total > len) return false;
    const uint32_t fp = ld(20u);  // flags / offset, TTL, protocol
    if ((fp >> 24) != 1u) return false;
    if ((icmp_bswap16(fp) & 0x3FFFu) != 0u) return false;  // a fragment (verdict 3 in any case)
    const uint32_t src = icmp_bswap32(ld(26u)), dst = icmp_bswap32(ld(30u));
    if (src == 0xFFFFFFFFu || (src & 0xF0000000u) == 0xE0000000u || src == bcast_addr)  // :838-843
        return false;
    if (dst != local_addr && dst != bcast_addr && dst != 0xFFFFFFFFu) return false;      // :1103-1113
    const uint32_t T = 14u + hl;  // the ICMP header
    const uint32_t tc = ld(T);
    if ((tc & 0xFFu) != 3u) return false;                                                // :1145
    const uint32_t code = tc >> 8 & 0xFFu;
    const uint32_t rest = icmp_bswap32(ld(T + 4u));
    // handleIcmp4DestUnreach: icmp_data = IP-payload bytes [8, total - hl)
    const uint32_t dlen = total - hl - 8u;
    if (dlen < 20u) return false;                                                        // :1196
    const uint32_t Q = T + 8u;  // the quoted IPv4 header
    const uint32_t q0 = ld(Q);  // version/IHL, DSCP, total length
    if ((q0 >> 4 & 0xFu) != 4u) return false;                                            // :1210
    const uint32_t qhl = (q0 & 0xFu) * 4u;
    if (qhl < 20u || qhl > dlen) return false;                                           // :1217
    const uint32_t qtotal = icmp_bswap16(q0 >> 16);
    if (qtotal < qhl) return false;                                                      // :1224
    const uint32_t l4_len = (dlen < qtotal ? dlen : qtotal) - qhl;                       // :1235
    const uint32_t tp = ld(Q + 8u);  // TTL, protocol, checksum
    const uint32_t ttl = tp & 0xFFu, proto = tp >> 8 & 0xFFu;
    const uint32_t qsrc = icmp_bswap32(ld(Q + 12u)), qdst = icmp_bswap32(ld(Q + 16u));
    uint32_t lport = 0u, rport = 0u, seq = 0u;
    if (l4_len >= 8u) {  // bytes [Q + qhl, Q + qhl + 8) lie below Q + dlen = 14 + total
        const uint32_t ports = ld(Q + qhl);
        lport = icmp_bswap16(ports);        // the quoted source side is ours
        rport = icmp_bswap16(ports >> 16);
        seq = icmp_bswap32(ld(Q + qhl + 4u));
    }
    key.local_addr = qsrc;                                   // tcp/IpTcpProto_input.h:178
    key.remote_addr = qdst;
    key.local_port = (uint16_t)lport;
    key.remote_port = (uint16_t)rport;
    key.cookie = 0u;
    lookup = proto == 6u && code == 4u && l4_len >= 8u;      // :159, :165
    w[0] = qsrc;
    w[1] = qdst;
    w[2] = lport | rport << 16;
    w[3] = seq;
    w[4] = rest;
    w[5] = AIPSTACK_TCP_NO_PCB;
    w[6] = Q | l4_len << 16;
    w[7] = code | proto << 8 | ttl << 16 | qhl << 24;
    return true;
}

// A whole frame's outcome as the decide pass computes it, for a caller that holds the table in
// host memory (the stand-alone test). Returns the status; w[8] = the record, zero for _DU_NONE.
template <class Load, class LoadEntry>
AIPSTACK_ICMP_HD uint32_t icmp_du_frame(const Load &ld, uint32_t len, uint32_t verdict,
                                        uint32_t local_addr, uint32_t bcast_addr,
                                        const LoadEntry &entry, uint64_t n_pcbs, uint32_t w[8]) {
    aipstack_tcp_pcb_key key;
    bool lookup;
    for (int q = 0; q < 8; ++q) w[q] = 0u;
    if (!icmp_du_build(ld, len, verdict, local_addr, bcast_addr, w, key, lookup))
        return AIPSTACK_ICMP_DU_NONE;
    if (!lookup) return AIPSTACK_ICMP_DU_PARSED;
    uint32_t cookie = 0u;
    if (!pcb_table_find(entry, n_pcbs, key, cookie)) return AIPSTACK_ICMP_DU_TCP_NO_PCB;
    w[5] = cookie;
    return AIPSTACK_ICMP_DU_TCP_PCB;
}

// The argument checks of aipstack_icmp_rx_unreach / _slotted (icmpdu_host.cpp; no HIP call).
// frames: d_offsets or d_len; slot_stride is checked when `slotted`.
struct IcmpUnreachArgs {
    const void *d_base, *frames;
    bool slotted;
    uint64_t slot_stride, n;
    const aipstack_icmp_iface *h_iface;
    const void *d_pcbs;
    uint64_t n_pcbs;
    const void *d_verdict, *d_status, *d_records, *d_pcb_frame, *d_counts, *d_workspace;
    uint64_t workspace_bytes;
};
int icmp_rx_unreach_check_args(const IcmpUnreachArgs &a);

}  // namespace aipstack_amd

#endif
