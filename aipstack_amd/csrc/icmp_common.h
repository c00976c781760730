// aipstack_amd -- ICMP on receive: what the host code (icmp_host.cpp), the kernels
// (icmp_kernels.hip) and the stand-alone test (tests/cpp/icmp_build_test.cpp) share as plain C++:
// the decision whether a frame gets a response (recvIcmp4Dgram, ip/IpStack.h:1093-1148;
// sendIp4DestUnreach, :869-887; checkSendIp4Allowed, :666-690) and the 42 header bytes of the
// response (sendIcmp4Message, :1164-1190; sendIp4Dgram, :423-453), built from the same text
// wherever the frame's bytes are read from.
#ifndef AIPSTACK_AMD_ICMP_COMMON_H
#define AIPSTACK_AMD_ICMP_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"

#if defined(__HIPCC__)
#define AIPSTACK_ICMP_HD __host__ __device__ inline
#else
#define AIPSTACK_ICMP_HD inline
#endif

namespace aipstack_amd {

constexpr uint64_t kIcmpMaxCount = 1ull << 40;  // frames of one call
constexpr uint32_t kIcmpTile = 256;             // frames per block of the counts and the scan

// The interface as the kernels take it (by value): aipstack_icmp_iface without its padding,
// the MAC as the little-endian dword of bytes 0-3 and the half of bytes 4-5.
struct IcmpIface {
    uint32_t local_addr, bcast_addr, mtu, ip_id, ttl, flags, mac_lo, mac_hi;
};

inline IcmpIface icmp_iface_of(const aipstack_icmp_iface &f) {
    return IcmpIface{f.local_addr,
                     f.bcast_addr,
                     f.mtu,
                     f.ip_id,
                     f.ttl,
                     f.flags,
                     (uint32_t)f.mac[0] | (uint32_t)f.mac[1] << 8 | (uint32_t)f.mac[2] << 16 |
                         (uint32_t)f.mac[3] << 24,
                     (uint32_t)f.mac[4] | (uint32_t)f.mac[5] << 8};
}

// What the calls that take an aipstack_icmp_iface accept of it (the ICMP responder, and the UDP
// Rx demux, whose struct goes to the responder next).
inline bool icmp_iface_valid(const aipstack_icmp_iface &f) {
    if (f.mtu < AIPSTACK_UDP_MIN_MTU || (f.flags & ~AIPSTACK_ICMP_ALLOW_BROADCAST_PING) != 0)
        return false;
    for (uint8_t r : f.reserved)
        if (r != 0) return false;
    return true;
}

AIPSTACK_ICMP_HD uint32_t icmp_bswap32(uint32_t x) {
    return x >> 24 | (x >> 8 & 0xFF00u) | (x << 8 & 0xFF0000u) | x << 24;
}
AIPSTACK_ICMP_HD uint32_t icmp_bswap16(uint32_t x) { return (x & 0xFFu) << 8 | (x >> 8 & 0xFFu); }
// x mod 0xFFFF with a nonzero multiple as 0xFFFF: zero only for x = 0.
AIPSTACK_ICMP_HD uint32_t icmp_fold16(uint32_t x) {
    x = (x & 0xFFFFu) + (x >> 16);
    return (x & 0xFFFFu) + (x >> 16);
}

// What is due for one frame: status (AIPSTACK_ICMP_*), and for a response (_ECHO_REPLY, _UNREACH;
// also for _TOO_LARGE) its data as a range of the frame, [data_off, data_off + data_len), and the
// received IPv4 header length.
struct IcmpPlan {
    uint32_t status, hl, data_off, data_len;
    AIPSTACK_ICMP_HD bool responds() const {
        return status == AIPSTACK_ICMP_ECHO_REPLY || status == AIPSTACK_ICMP_UNREACH;
    }
    AIPSTACK_ICMP_HD bool has_chunk() const { return responds() && data_len != 0u; }
};

// The decision for a frame of `len` bytes with Rx verify's `verdict` and the host's unreach
// `code` (AIPSTACK_ICMP_NO_UNREACH: none), read through `ld(off)` = the little-endian dword at
// frame bytes [off, off + 4), which is only called for bytes inside the frame.
template <class Load>
AIPSTACK_ICMP_HD IcmpPlan icmp_decide(const Load &ld, uint32_t len, uint32_t verdict, uint32_t code,
                                      const IcmpIface &f) {
    IcmpPlan p{AIPSTACK_ICMP_NONE, 0u, 0u, 0u};
    if (verdict != AIPSTACK_RX_ACCEPT && verdict != AIPSTACK_RX_ACCEPT_NO_CHKSUM &&
        verdict != AIPSTACK_RX_ACCEPT_OTHER)
        return p;
    if (len < 14u + 20u) return p;
    const uint32_t v = ld(14u);  // version/IHL, DSCP, total length
    const uint32_t hl = (v & 0xFu) * 4u;
    const uint32_t total = icmp_bswap16(v >> 16);
    // what Rx verify has checked of an accepted frame (ip/IpStack.h:938-990), restated so that
    // every read below lies inside the frame
    if (hl < 20u || total < hl || 14u + total > len) return p;
    const uint32_t fp = ld(20u);  // flags / offset, TTL, protocol
    if ((icmp_bswap16(fp) & 0x3FFFu) != 0u) return p;  // a fragment (verdict 3 in any case)
    const uint32_t src = icmp_bswap32(ld(26u)), dst = icmp_bswap32(ld(30u));
    const uint32_t rem = total - hl;  // the IP payload
    p.hl = hl;
    if (verdict == AIPSTACK_RX_ACCEPT && (fp >> 24) == 1u && rem >= 8u) {
        const bool unicast_src = src != 0xFFFFFFFFu && (src & 0xF0000000u) != 0xE0000000u &&
                                 src != f.bcast_addr;                               // :838-843
        const bool bcast_dst = dst == f.bcast_addr || dst == 0xFFFFFFFFu;
        const bool dst_ok = dst == f.local_addr ||
                            (bcast_dst && (f.flags & AIPSTACK_ICMP_ALLOW_BROADCAST_PING) != 0u);
        if (unicast_src && dst_ok && (ld(14u + hl) & 0xFFu) == 8u) {  // EchoRequest, :1137
            p.data_off = 14u + hl + 8u;
            p.data_len = rem - 8u;
            p.status = 28u + p.data_len > f.mtu ? AIPSTACK_ICMP_TOO_LARGE : AIPSTACK_ICMP_ECHO_REPLY;
            return p;
        }
    }
    if (code != AIPSTACK_ICMP_NO_UNREACH && dst == f.local_addr && src != 0xFFFFFFFFu &&
        src != f.bcast_addr) {  // checkSendIp4Allowed({dst, src}), :666-690
        p.data_off = 14u;
        p.data_len = hl + (rem < 8u ? rem : 8u);  // :878-879
        p.status = 28u + p.data_len > f.mtu ? AIPSTACK_ICMP_TOO_LARGE : AIPSTACK_ICMP_UNREACH;
    }
    return p;
}

// True if frame bytes [off, off + n) hold a nonzero byte: whole dwords until the first that is
// not zero, the last 1-3 bytes as the top of the dword that ends with them (off >= 4, so that
// dword lies inside the frame).
template <class Load>
AIPSTACK_ICMP_HD bool icmp_any_nonzero(const Load &ld, uint32_t off, uint32_t n) {
    const uint32_t whole = n & ~3u;
    for (uint32_t k = 0; k < whole; k += 4u)
        if (ld(off + k) != 0u) return true;
    const uint32_t tail = n & 3u;
    return tail != 0u && (ld(off + n - 4u) >> (8u * (4u - tail))) != 0u;
}

// The sum of the little-endian 16-bit words of frame bytes [off, off + n) (n <= 68, off >= 4; an
// odd last byte counts as a low byte: after the final byte swap, the high byte of a padded word).
template <class Load>
AIPSTACK_ICMP_HD uint32_t icmp_sum_le(const Load &ld, uint32_t off, uint32_t n) {
    uint32_t s = 0;
    const uint32_t whole = n & ~3u;
    for (uint32_t k = 0; k < whole; k += 4u) {
        const uint32_t w = ld(off + k);
        s += (w & 0xFFFFu) + (w >> 16);
    }
    const uint32_t tail = n & 3u;
    if (tail != 0u) {
        const uint32_t w = ld(off + n - 4u) >> (8u * (4u - tail));
        s += (w & 0xFFFFu) + (w >> 16);
    }
    return s;
}

// The slot image o[16] (the 64 slot bytes as little-endian dwords, bytes 42-63 zero) of the
// response `p` (p.responds()) to the frame behind `ld`, with Ident `ident` and the host's unreach
// code.
template <class Load>
AIPSTACK_ICMP_HD void icmp_build_slot(const Load &ld, const IcmpPlan &p, uint32_t code,
                                      uint32_t ident, const IcmpIface &f, uint32_t (&o)[16]) {
    const bool echo = p.status == AIPSTACK_ICMP_ECHO_REPLY;
    const uint32_t m0 = ld(4u), m1 = ld(8u);  // bytes 6-11: the frame's source MAC
    const uint32_t rsrc = ld(26u);            // the received source address, as it lies
    const uint32_t lsrc = icmp_bswap32(f.local_addr);
    const uint32_t total = 28u + p.data_len;
    ident &= 0xFFFFu;
    // sendIp4Dgram, :425-453: the header checksum over the ten big-endian words
    const uint32_t ipsum = 0x4500u + total + ident + (f.ttl << 8 | 1u) + (f.local_addr >> 16) +
                           (f.local_addr & 0xFFFFu) + icmp_bswap16(rsrc) + icmp_bswap16(rsrc >> 16);
    const uint32_t ipck = ~icmp_fold16(ipsum) & 0xFFFFu;
    uint32_t type_code, rest, ck;
    if (echo) {
        const uint32_t T = 14u + p.hl;
        const uint32_t h0 = ld(T);
        rest = ld(T + 4u);
        type_code = 0u;
        // The request's sum is good: w0 + field + S = 0 mod 0xFFFF with S the folded sum of rest
        // and data, so the reply's checksum ~S is fold16(w0 + field) unless that is 0xFFFF; there
        // S is 0x0000 (every byte zero) or 0xFFFF, which only the bytes tell.
        const uint32_t r = icmp_fold16(icmp_bswap16(h0) + icmp_bswap16(h0 >> 16));
        if (r != 0xFFFFu) ck = r;
        else ck = rest != 0u || icmp_any_nonzero(ld, p.data_off, p.data_len) ? 0u : 0xFFFFu;
    } else {
        rest = 0u;
        type_code = 3u | (code & 0xFFu) << 8;
        const uint32_t s = icmp_bswap16(icmp_fold16(icmp_sum_le(ld, p.data_off, p.data_len)));
        ck = ~icmp_fold16((0x0300u | (code & 0xFFu)) + s) & 0xFFFFu;
    }
    o[0] = m0 >> 16 | m1 << 16;
    o[1] = m1 >> 16 | (f.mac_lo & 0xFFFFu) << 16;
    o[2] = f.mac_lo >> 16 | f.mac_hi << 16;
    o[3] = 0x00450008u;
    o[4] = icmp_bswap16(total) | icmp_bswap16(ident) << 16;
    o[5] = f.ttl << 16 | 1u << 24;
    o[6] = icmp_bswap16(ipck) | (lsrc & 0xFFFFu) << 16;
    o[7] = lsrc >> 16 | (rsrc & 0xFFFFu) << 16;
    o[8] = rsrc >> 16 | type_code << 16;
    o[9] = icmp_bswap16(ck) | (rest & 0xFFFFu) << 16;
    o[10] = rest >> 16;
    o[11] = o[12] = o[13] = o[14] = o[15] = 0u;
}

// The argument checks of aipstack_icmp_rx_respond / _slotted (icmp_host.cpp; no HIP call).
// frames: d_offsets or d_len; slot_stride is checked when `slotted`.
struct IcmpRespondArgs {
    const void *d_base, *frames;
    bool slotted;
    uint64_t slot_stride, n;
    const aipstack_icmp_iface *h_iface;
    const void *d_verdict, *d_status, *d_hdr;
    uint64_t hdr_stride;
    const void *d_hdr_len, *d_chunk_addr, *d_chunk_len, *d_chunk_index, *d_response_frame, *d_counts,
        *d_workspace;
    uint64_t workspace_bytes;
};
int icmp_rx_respond_check_args(const IcmpRespondArgs &a);

}  // namespace aipstack_amd

#endif
