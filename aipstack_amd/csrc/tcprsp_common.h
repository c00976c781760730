// aipstack_amd -- TCP segments without a connection: what the host code (tcprsp_host.cpp), the
// kernels (tcprsp_kernels.hip) and the stand-alone test (tests/cpp/tcp_rsp_build_test.cpp) share
// as plain C++: the rest of recvIp4Dgram around find_pcb (tcp/IpTcpProto_input.h:72, :132-151),
// the top of listen_input (:372-401) with find_listener_for_rx (tcp/IpTcpProto.h:824-837) and
// CalcTcpSndMss (tcp/TcpMiscUtils.h:55-67), and the 54 bytes of the RST (send_rst_reply /
// send_rst / send_tcp_nodata, tcp/IpTcpProto_output.h:989-1018, :1338-1404; sendIp4Dgram,
// ip/IpStack.h:423-453), built from the segment's record (tcp_rx_build, tcprx_common.h) wherever
// the frame's bytes are read from.
#ifndef AIPSTACK_AMD_TCPRSP_COMMON_H
#define AIPSTACK_AMD_TCPRSP_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "tcprx_common.h"

namespace aipstack_amd {

constexpr uint32_t kTcpRspTile = 256;    // frames per block of the counts and the scan
constexpr uint32_t kTcpRspTileWaves = 4; // ballot pairs a tile leaves in the workspace
constexpr uint32_t kTcpRspMinMss = AIPSTACK_UDP_MIN_MTU - 40u;  // MinAllowedMss = MinMTU - 40

// The interface as the kernels take it (by value): the fields of aipstack_icmp_iface the call
// uses, the TCP TTL in place of the ICMP one, the MAC as the little-endian dword of bytes 0-3
// and the half of bytes 4-5.
struct TcpRspIface {
    uint32_t local_addr, bcast_addr, ip_id, ttl, mac_lo, mac_hi;
};

inline TcpRspIface tcp_rsp_iface_of(const aipstack_icmp_iface &f, uint32_t tcp_ttl) {
    return TcpRspIface{f.local_addr,
                       f.bcast_addr,
                       f.ip_id,
                       tcp_ttl,
                       (uint32_t)f.mac[0] | (uint32_t)f.mac[1] << 8 | (uint32_t)f.mac[2] << 16 |
                           (uint32_t)f.mac[3] << 24,
                       (uint32_t)f.mac[4] | (uint32_t)f.mac[5] << 8};
}

// One listener as the decision reads it: the defined fields of aipstack_tcp_listener.
struct TcpRspLis {
    uint32_t addr, port, cookie;
};

// What is due for one frame: d_status[i] and d_listener[i].
struct TcpRspPlan {
    uint32_t status, listener;
    AIPSTACK_TCPRX_HD bool rst() const { return status == AIPSTACK_TCP_RSP_RST; }
    AIPSTACK_TCPRX_HD bool syn() const { return status == AIPSTACK_TCP_RSP_SYN; }
};

// The decision for a frame with a valid record `w` (tcp_rx_build returned kTcpRxValid; a frame
// without one is AIPSTACK_TCP_RSP_NONE), `has_pcb` from the lookup and the host's `rst_request`.
// find(dst, port, cookie): true and the cookie of the first listener in list order with that
// port and that address or the wildcard; only called when a listener is consulted.
template <class FindListener>
AIPSTACK_TCPRX_HD TcpRspPlan tcp_rsp_decide(const uint32_t (&w)[8], bool has_pcb, bool rst_request,
                                            const TcpRspIface &f, const FindListener &find) {
    const uint32_t src = w[0], dst = w[1], flags = w[5] & 0xFFFFu;
    TcpRspPlan p{AIPSTACK_TCP_RSP_NOT_LOCAL, AIPSTACK_TCP_NO_LISTENER};
    if (dst != f.local_addr) return p;                                    // input :72
    p.status = AIPSTACK_TCP_RSP_PCB;
    if (has_pcb && !rst_request) return p;                                // :132-137
    p.status = AIPSTACK_TCP_RSP_DROP;
    if (src == 0xFFFFFFFFu || (src & 0xF0000000u) == 0xE0000000u || src == f.bcast_addr)
        return p;                                                         // checkUnicastSrcAddr
    if (rst_request) {
        p.status = AIPSTACK_TCP_RSP_RST;
        return p;
    }
    uint32_t cookie = 0u;
    if (!find(dst, w[2] >> 16, cookie)) {                                 // :145-151
        if ((flags & 0x04u) == 0u) p.status = AIPSTACK_TCP_RSP_RST;
        return p;
    }
    p.listener = cookie;
    if ((flags & 0x17u) != 0x02u) {                                       // listen_input :372-379
        if ((flags & 0x14u) == 0x10u) p.status = AIPSTACK_TCP_RSP_RST;
        return p;
    }
    // CalcTcpSndMss: min(mtu - 40, the option or 536) >= MinAllowedMss; mtu - 40 always is
    const uint32_t opts = w[7] >> 24, mss = w[7] & 0xFFFFu;
    p.status = (opts & AIPSTACK_TCP_OPT_MSS) != 0u && mss < kTcpRspMinMss ? AIPSTACK_TCP_RSP_RST
                                                                          : AIPSTACK_TCP_RSP_SYN;
    return p;
}

// x mod 0xFFFF with a nonzero multiple as 0xFFFF: zero only for x = 0.
AIPSTACK_TCPRX_HD uint32_t tcp_rsp_fold16(uint32_t x) {
    x = (x & 0xFFFFu) + (x >> 16);
    return (x & 0xFFFFu) + (x >> 16);
}

// The slot image o[16] (the 64 slot bytes as little-endian dwords, bytes 54-63 zero) of the RST
// that answers the segment with record `w`, received in a frame whose bytes 4-7 and 8-11 are
// m0 and m1 (little-endian; bytes 6-11 are its source MAC), with Ident `ident`.
AIPSTACK_TCPRX_HD void tcp_rsp_build_rst(const uint32_t (&w)[8], uint32_t m0, uint32_t m1,
                                         uint32_t ident, const TcpRspIface &f, uint32_t (&o)[16]) {
    const uint32_t remote = w[0], local = w[1], rport = w[2] & 0xFFFFu, lport = w[2] >> 16;
    const uint32_t flags = w[5] & 0xFFFFu, data_len = w[6] >> 16;
    // send_rst_reply: an ACK is answered from its ack_num, anything else acknowledged in full
    const bool has_ack = (flags & 0x10u) != 0u;
    const uint32_t seq = has_ack ? w[4] : 0u;
    const uint32_t ack = has_ack ? 0u : w[3] + data_len + ((flags & 0x03u) != 0u ? 1u : 0u);
    const uint32_t tflags = has_ack ? 0x5004u : 0x5014u;
    ident &= 0xFFFFu;
    const uint32_t addrs = (local >> 16) + (local & 0xFFFFu) + (remote >> 16) + (remote & 0xFFFFu);
    // sendIp4Dgram: the header checksum over the ten big-endian words
    const uint32_t ipck =
        ~tcp_rsp_fold16(0x4500u + 40u + ident + 0x4000u + (f.ttl << 8 | 6u) + addrs) & 0xFFFFu;
    // send_tcp_nodata: pseudo-header (addresses, protocol 6, length 20) and the header
    const uint32_t ck = ~tcp_rsp_fold16(addrs + 6u + 20u + lport + rport + (seq >> 16) +
                                        (seq & 0xFFFFu) + (ack >> 16) + (ack & 0xFFFFu) + tflags) &
                        0xFFFFu;
    const uint32_t lsrc = tcprx_bswap32(local), rdst = tcprx_bswap32(remote);
    const uint32_t seqbe = tcprx_bswap32(seq), ackbe = tcprx_bswap32(ack);
    o[0] = m0 >> 16 | m1 << 16;
    o[1] = m1 >> 16 | (f.mac_lo & 0xFFFFu) << 16;
    o[2] = f.mac_lo >> 16 | f.mac_hi << 16;
    o[3] = 0x00450008u;                                    // EtherType 0x0800, 0x45, DSCP 0
    o[4] = tcprx_be16lo(40u) | tcprx_be16lo(ident) << 16;  // total length, Ident
    o[5] = 0x0040u | f.ttl << 16 | 6u << 24;               // DF, TTL, protocol
    o[6] = tcprx_be16lo(ipck) | (lsrc & 0xFFFFu) << 16;
    o[7] = lsrc >> 16 | (rdst & 0xFFFFu) << 16;
    o[8] = rdst >> 16 | tcprx_be16lo(lport) << 16;
    o[9] = tcprx_be16lo(rport) | (seqbe & 0xFFFFu) << 16;
    o[10] = seqbe >> 16 | (ackbe & 0xFFFFu) << 16;
    o[11] = ackbe >> 16 | tcprx_be16lo(tflags) << 16;
    o[12] = tcprx_be16lo(ck) << 16;                        // window 0, checksum
    o[13] = o[14] = o[15] = 0u;                            // urgent 0
}

// The argument checks of aipstack_tcp_rx_respond / _slotted (tcprsp_host.cpp; no HIP call).
// frames: d_offsets or d_len; slot_stride is checked when `slotted`.
struct TcpRespondArgs {
    const void *d_base, *frames;
    bool slotted;
    uint64_t slot_stride, n;
    const aipstack_icmp_iface *h_iface;
    uint32_t tcp_ttl;
    const void *d_pcbs;
    uint64_t n_pcbs;
    const void *d_listeners;
    uint32_t n_listeners;
    const void *d_verdict, *d_segs, *d_pcb, *d_status, *d_listener, *d_hdr;
    uint64_t hdr_stride;
    const void *d_hdr_len, *d_chunk_index, *d_response_frame, *d_syn_frame, *d_counts, *d_workspace;
    uint64_t workspace_bytes;
};
int tcp_rx_respond_check_args(const TcpRespondArgs &a);

}  // namespace aipstack_amd

#endif
