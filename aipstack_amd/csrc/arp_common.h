// aipstack_amd -- ARP on receive: what the host code (arp_host.cpp), the kernels
// (arp_kernels.hip) and the stand-alone test (tests/cpp/arp_build_test.cpp) share as plain C++:
// the record of a frame (recvArpPacket, eth/EthIpIface.h:474-508, with the address tests of
// save_hw_addr and get_arp_entry, :587-627, :664-698) and the 42 bytes of a reply
// (send_arp_packet, :774-803), built from the same text wherever the frame's bytes are read from.
#ifndef AIPSTACK_AMD_ARP_COMMON_H
#define AIPSTACK_AMD_ARP_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"

#if defined(__HIPCC__)
#define AIPSTACK_ARP_HD __host__ __device__ inline
#else
#define AIPSTACK_ARP_HD inline
#endif

namespace aipstack_amd {

constexpr uint64_t kArpMaxCount = 1ull << 40;  // frames of one call
constexpr uint32_t kArpTile = 256;             // frames per block of the counts and the scan
constexpr uint32_t kArpTileWaves = 4;          // ballot pairs a tile leaves in the workspace

// The interface as the kernels take it (by value): aipstack_arp_iface without its padding, the
// MAC as the little-endian dword of bytes 0-3 and the half of bytes 4-5.
struct ArpIface {
    uint32_t local_addr, netmask, flags, mac_lo, mac_hi;
};

inline ArpIface arp_iface_of(const aipstack_arp_iface &f) {
    return ArpIface{f.local_addr, f.netmask, f.flags,
                    (uint32_t)f.mac[0] | (uint32_t)f.mac[1] << 8 | (uint32_t)f.mac[2] << 16 |
                        (uint32_t)f.mac[3] << 24,
                    (uint32_t)f.mac[4] | (uint32_t)f.mac[5] << 8};
}

inline bool arp_iface_valid(const aipstack_arp_iface &f) {
    if ((f.flags & ~AIPSTACK_ARP_HAVE_ADDR) != 0) return false;
    for (uint8_t r : f.reserved)
        if (r != 0) return false;
    return true;
}

AIPSTACK_ARP_HD uint32_t arp_bswap32(uint32_t x) {
    return x >> 24 | (x >> 8 & 0xFF00u) | (x << 8 & 0xFF0000u) | x << 24;
}
AIPSTACK_ARP_HD uint32_t arp_bswap16(uint32_t x) { return (x & 0xFFu) << 8 | (x >> 8 & 0xFFu); }

// aipstack_arp_record as its four little-endian dwords: w[0] sender_addr, w[1] sender_mac bytes
// 0-3, w[2] sender_mac bytes 4-5 below op, w[3] flags, status << 8, reserved.
struct ArpRecord {
    uint32_t w[4];
    AIPSTACK_ARP_HD uint32_t status() const { return w[3] >> 8 & 0xFFu; }
    AIPSTACK_ARP_HD bool seen() const {
        return status() == AIPSTACK_ARP_SEEN || status() == AIPSTACK_ARP_REPLY;
    }
    AIPSTACK_ARP_HD bool replies() const { return status() == AIPSTACK_ARP_REPLY; }
};

// The record of a frame of `len` bytes, read through `ld(off)` = the little-endian dword at frame
// bytes [off, off + 4), which is only called for bytes inside the frame: bytes 10-13 of a frame
// of at least 14 bytes, bytes 14-33 and 38-41 of an ARP frame of at least 42 (the target hardware
// address, bytes 34-37, is never read).
template <class Load>
AIPSTACK_ARP_HD ArpRecord arp_decide(const Load &ld, uint32_t len, const ArpIface &f) {
    ArpRecord r{{0u, 0u, 0u, (uint32_t)AIPSTACK_ARP_NONE << 8}};
    if (len < 14u) return r;                                    // :370
    if (arp_bswap16(ld(10u) >> 16) != 0x0806u) return r;        // :387
    r.w[3] = (uint32_t)AIPSTACK_ARP_MALFORMED << 8;
    if (len < 14u + 28u) return r;                              // :477
    const uint32_t types = ld(14u), lens_op = ld(18u);
    // HwType 1, ProtoType 0x0800, HwAddrLen 6, ProtoAddrLen 4, as the bytes lie (:483-489)
    if (types != 0x00080100u || (lens_op & 0xFFFFu) != 0x0406u) return r;
    const uint32_t a = ld(22u), b = ld(26u), c = ld(30u), tpa = ld(38u);
    const uint32_t op = arp_bswap16(lens_op >> 16);
    const uint32_t ip = arp_bswap32(b >> 16 | c << 16);         // SrcProtoAddr, frame bytes 28-31
    const uint32_t mac45 = b & 0xFFFFu;
    const bool have = (f.flags & AIPSTACK_ARP_HAVE_ADDR) != 0u;
    const uint32_t netaddr = f.local_addr & f.netmask, bcast = netaddr | ~f.netmask;
    const bool plain = ip != 0xFFFFFFFFu && ip != 0u;
    uint32_t flags = 0u;
    const bool learn = !(a == 0xFFFFFFFFu && mac45 == 0xFFFFu);  // :590
    if (learn) flags |= AIPSTACK_ARP_REC_LEARN;
    if (plain && have && (ip & f.netmask) == netaddr && ip != bcast)  // :675-698
        flags |= AIPSTACK_ARP_REC_NEW_OK;
    if (learn && plain) flags |= AIPSTACK_ARP_REC_NOTIFY;        // :622
    const bool reply = op == 1u && have && arp_bswap32(tpa) == f.local_addr;  // :500-503
    if (reply) flags |= AIPSTACK_ARP_REC_REPLY;
    r.w[0] = ip;
    r.w[1] = a;
    r.w[2] = mac45 | op << 16;
    r.w[3] = flags | (uint32_t)(reply ? AIPSTACK_ARP_REPLY : AIPSTACK_ARP_SEEN) << 8;
    return r;
}

// The slot image o[16] (the 64 slot bytes as little-endian dwords, bytes 42-63 zero) of the reply
// to the request whose record is `r` (r.replies()): send_arp_packet(Reply, src_mac, src_ip_addr).
AIPSTACK_ARP_HD void arp_build_reply(const ArpRecord &r, const ArpIface &f, uint32_t (&o)[16]) {
    const uint32_t mac45 = r.w[2] & 0xFFFFu, spa = arp_bswap32(r.w[0]);
    o[0] = r.w[1];                                   // Ethernet destination: the ARP sender
    o[1] = mac45 | (f.mac_lo & 0xFFFFu) << 16;
    o[2] = f.mac_lo >> 16 | f.mac_hi << 16;
    o[3] = 0x01000608u;                              // EtherType 0x0806, HwType 1
    o[4] = 0x04060008u;                              // ProtoType 0x0800, lengths 6 and 4
    o[5] = 0x0200u | (f.mac_lo & 0xFFFFu) << 16;     // OpType 2, SrcHwAddr
    o[6] = f.mac_lo >> 16 | f.mac_hi << 16;
    o[7] = arp_bswap32(f.local_addr);                // SrcProtoAddr
    o[8] = r.w[1];                                   // DstHwAddr
    o[9] = mac45 | (spa & 0xFFFFu) << 16;            // DstProtoAddr
    o[10] = spa >> 16;
    o[11] = o[12] = o[13] = o[14] = o[15] = 0u;
}

// The argument checks of aipstack_arp_rx_respond / _slotted (arp_host.cpp; no HIP call).
// frames: d_offsets or d_len; slot_stride is checked when `slotted`.
struct ArpRespondArgs {
    const void *d_base, *frames;
    bool slotted;
    uint64_t slot_stride, n;
    const aipstack_arp_iface *h_iface;
    const void *d_status, *d_arp, *d_hdr;
    uint64_t hdr_stride;
    const void *d_hdr_len, *d_chunk_index, *d_reply_frame, *d_seen_frame, *d_counts, *d_workspace;
    uint64_t workspace_bytes;
};
int arp_rx_respond_check_args(const ArpRespondArgs &a);

}  // namespace aipstack_amd

#endif
