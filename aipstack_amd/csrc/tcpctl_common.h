// aipstack_amd -- TCP segments without data (SYN, SYN-ACK, ACK, FIN, RST): what the host code
// (tcpctl_host.cpp), the kernels (tcpctl_kernels.hip) and the stand-alone test
// (tests/cpp/tcp_ctl_build_test.cpp) share as plain C++: the descriptor as eight dwords, its
// validity, and the up to 62 bytes of send_tcp_nodata (tcp/IpTcpProto_output.h:1337-1404) with
// WriteTcpOptions (tcp/TcpOptions.h:141-157) under sendIp4Dgram (ip/IpStack.h:423-453). The
// interface, the 16-bit fold and the byte-order helpers are the TCP responder's (tcprsp_common.h).
#ifndef AIPSTACK_AMD_TCPCTL_COMMON_H
#define AIPSTACK_AMD_TCPCTL_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "tcprsp_common.h"

namespace aipstack_amd {

constexpr uint32_t kTcpCtlTile = 256;     // descriptors per block of the counts and the scan
constexpr uint32_t kTcpCtlTileWaves = 4;  // ballots a tile leaves in the workspace
constexpr uint64_t kTcpCtlMaxCount = 1ull << 40;

// A descriptor (aipstack_tcp_ctl) as its eight little-endian dwords d[0..7]: local_addr,
// remote_addr, local_port | remote_port << 16, seq, ack, window | mss << 16,
// flags | options << 8 | wnd_scale << 16 | reserved0 << 24, reserved1.

// Valid by the upper half alone (d[4..7]): both reserved fields 0, no option bit but the two.
AIPSTACK_TCPRX_HD bool tcp_ctl_valid(uint32_t d6, uint32_t d7) {
    return (d6 >> 24) == 0u && d7 == 0u &&
           ((d6 >> 8) & 0xFFu & ~(AIPSTACK_TCP_OPT_MSS | AIPSTACK_TCP_OPT_WND_SCALE)) == 0u;
}

// The header length of a valid descriptor: 54, 58 or 62.
AIPSTACK_TCPRX_HD uint32_t tcp_ctl_header_len(uint32_t d6) {
    const uint32_t opts = (d6 >> 8) & 3u;
    return AIPSTACK_TCP_SEGMENT_HEADER + 4u * ((opts & 1u) + (opts >> 1));
}

// The slot image o[16] (the 64 slot bytes as little-endian dwords, zero from the header's end) of
// the valid descriptor `d` with Ident `ident`; returns the header length. Bytes 0-5 (the
// destination MAC) are 0: the resolve step writes them.
AIPSTACK_TCPRX_HD uint32_t tcp_ctl_build(const uint32_t (&d)[8], uint32_t ident, const TcpRspIface &f,
                                         uint32_t (&o)[16]) {
    const uint32_t local = d[0], remote = d[1], lport = d[2] & 0xFFFFu, rport = d[2] >> 16;
    const uint32_t seq = d[3], ack = d[4], window = d[5] & 0xFFFFu, mss = d[5] >> 16;
    const uint32_t flags = d[6] & 0xFFu, opts = (d[6] >> 8) & 3u, wscale = (d[6] >> 16) & 0xFFu;
    const bool has_mss = (opts & AIPSTACK_TCP_OPT_MSS) != 0u;
    const bool has_ws = (opts & AIPSTACK_TCP_OPT_WND_SCALE) != 0u;
    const uint32_t olen = 4u * ((has_mss ? 1u : 0u) + (has_ws ? 1u : 0u));
    const uint32_t tflags = (5u + olen / 4u) << 12 | flags;
    // WriteTcpOptions: 02 04 mss, then 01 03 03 scale, as the dwords of their bytes in memory and
    // as the sum of their big-endian words
    const uint32_t mss_w = 0x0402u | tcprx_be16lo(mss) << 16, ws_w = 0x030301u | wscale << 24;
    const uint32_t p0 = has_mss ? mss_w : has_ws ? ws_w : 0u, p1 = has_mss && has_ws ? ws_w : 0u;
    const uint32_t osum = (has_mss ? 0x0204u + mss : 0u) + (has_ws ? 0x0103u + (0x0300u | wscale) : 0u);
    ident &= 0xFFFFu;
    const uint32_t addrs = (local >> 16) + (local & 0xFFFFu) + (remote >> 16) + (remote & 0xFFFFu);
    // sendIp4Dgram: the header checksum over the ten big-endian words
    const uint32_t ipck =
        ~tcp_rsp_fold16(0x4500u + 40u + olen + ident + 0x4000u + (f.ttl << 8 | 6u) + addrs) & 0xFFFFu;
    // send_tcp_nodata: pseudo-header (addresses, protocol 6, length 20 + olen), header, options
    const uint32_t ck =
        ~tcp_rsp_fold16(addrs + 6u + 20u + olen + lport + rport + (seq >> 16) + (seq & 0xFFFFu) +
                        (ack >> 16) + (ack & 0xFFFFu) + tflags + window + osum) &
        0xFFFFu;
    const uint32_t lsrc = tcprx_bswap32(local), rdst = tcprx_bswap32(remote);
    const uint32_t seqbe = tcprx_bswap32(seq), ackbe = tcprx_bswap32(ack);
    o[0] = 0u;
    o[1] = (f.mac_lo & 0xFFFFu) << 16;
    o[2] = f.mac_lo >> 16 | f.mac_hi << 16;
    o[3] = 0x00450008u;                                           // EtherType 0x0800, 0x45, DSCP 0
    o[4] = tcprx_be16lo(40u + olen) | tcprx_be16lo(ident) << 16;  // total length, Ident
    o[5] = 0x0040u | f.ttl << 16 | 6u << 24;                      // DF, TTL, protocol
    o[6] = tcprx_be16lo(ipck) | (lsrc & 0xFFFFu) << 16;
    o[7] = lsrc >> 16 | (rdst & 0xFFFFu) << 16;
    o[8] = rdst >> 16 | tcprx_be16lo(lport) << 16;
    o[9] = tcprx_be16lo(rport) | (seqbe & 0xFFFFu) << 16;
    o[10] = seqbe >> 16 | (ackbe & 0xFFFFu) << 16;
    o[11] = ackbe >> 16 | tcprx_be16lo(tflags) << 16;
    o[12] = tcprx_be16lo(window) | tcprx_be16lo(ck) << 16;
    o[13] = (p0 & 0xFFFFu) << 16;                                 // urgent 0, options from byte 54
    o[14] = p0 >> 16 | (p1 & 0xFFFFu) << 16;
    o[15] = p1 >> 16;
    return AIPSTACK_TCP_SEGMENT_HEADER + olen;
}

// The argument checks of aipstack_tcp_tx_control (tcpctl_host.cpp; no HIP call).
struct TcpControlArgs {
    const void *d_ctl;
    uint64_t n;
    const aipstack_icmp_iface *h_iface;
    uint32_t tcp_ttl;
    const void *d_hdr;
    uint64_t hdr_stride;
    const void *d_hdr_len, *d_chunk_index, *d_status, *d_counts, *d_workspace;
    uint64_t workspace_bytes;
};
int tcp_tx_control_check_args(const TcpControlArgs &a);

}  // namespace aipstack_amd

#endif
