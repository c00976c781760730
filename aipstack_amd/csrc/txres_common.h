// aipstack_amd -- Tx resolve: what the host code (txres_host.cpp), the kernels (txres_kernels.hip)
// and the stand-alone test (tests/cpp/tx_resolve_build_test.cpp) share as plain C++: the whole
// decision about one segment -- the route (routeIp4 / routeIp4ForceIface, ip/IpStack.h:713-780),
// the permission tests (checkSendIp4Allowed, :666-690), the ARP lookup with get_arp_entry's
// address tests (eth/EthIpIface.h:511-585, :635-698), the record -- and the 14 bytes of the
// Ethernet header (:420-430) with the stores that put them into a slot at any alignment, built
// from the same text wherever the tables and the slot lie.
#ifndef AIPSTACK_AMD_TXRES_COMMON_H
#define AIPSTACK_AMD_TXRES_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"

#if defined(__HIPCC__)
#define AIPSTACK_TXRES_HD __host__ __device__ inline
#else
#define AIPSTACK_TXRES_HD inline
#endif

namespace aipstack_amd {

constexpr uint64_t kTxResMaxCount = 1ull << 40;  // segments of one call (ARP entries: a 32-bit index)
constexpr uint32_t kTxResTile = 256;             // segments per block of the counts and the scan
constexpr uint32_t kTxResTileWaves = 4;          // ballot pairs a tile leaves in the workspace
constexpr uint32_t kTxResMinHeader = 34;         // Ethernet 14 + IPv4 20: up to the destination address
constexpr uint32_t kTxIfaceWords = 8;            // an aipstack_tx_iface as dwords

AIPSTACK_TXRES_HD uint64_t tx_res_tiles(uint64_t n) { return (n + kTxResTile - 1) / kTxResTile; }

AIPSTACK_TXRES_HD uint32_t txres_bswap32(uint32_t x) {
    return x >> 24 | (x >> 8 & 0xFF00u) | (x << 8 & 0xFF0000u) | x << 24;
}

// An aipstack_tx_iface as its first five little-endian dwords: addr, netmask, gateway,
// prefix | flags << 8 | mac[0] << 16 | mac[1] << 24, mac[2..5].
struct TxIfaceWords {
    uint32_t addr, netmask, gateway, pfm, mac_hi;
    AIPSTACK_TXRES_HD bool have_addr() const { return (pfm >> 8 & AIPSTACK_TX_HAVE_ADDR) != 0u; }
    AIPSTACK_TXRES_HD bool have_gateway() const { return (pfm >> 8 & AIPSTACK_TX_HAVE_GATEWAY) != 0u; }
    AIPSTACK_TXRES_HD int prefix() const { return (int)(pfm & 0xFFu); }
    AIPSTACK_TXRES_HD uint32_t netaddr() const { return addr & netmask; }          // IpIface.h:131
    AIPSTACK_TXRES_HD uint32_t bcastaddr() const { return netaddr() | ~netmask; }  // :132
    AIPSTACK_TXRES_HD bool is_local(uint32_t a) const {                            // ip4AddrIsLocal, :230
        return have_addr() && (a & netmask) == netaddr();
    }
};

// An aipstack_arp_entry as its four little-endian dwords: addr, iface | state << 16 | mac[0] << 24,
// mac[1..4], mac[5] | reserved << 8.
struct ArpEntryWords {
    uint32_t x, y, z, w;
    AIPSTACK_TXRES_HD uint32_t addr() const { return x; }
    AIPSTACK_TXRES_HD uint32_t iface() const { return y & 0xFFFFu; }
    AIPSTACK_TXRES_HD uint32_t state() const { return y >> 16 & 0xFFu; }
    AIPSTACK_TXRES_HD uint32_t mac_lo() const { return y >> 24 | z << 8; }              // bytes 0-3
    AIPSTACK_TXRES_HD uint32_t mac_hi() const { return z >> 24 | (w & 0xFFu) << 8; }   // bytes 4-5
};

// True, and the entry with its index, if the table of `n` entries sorted by (iface, addr) and read
// through `entry(index)` holds (iface, addr). Every entry read has an index in [lo, hi) within
// [0, n), whatever the table holds; the range shrinks by at least one entry per step (the shape
// of pcb_table_find, pcb_lookup.h).
template <class LoadEntry>
AIPSTACK_TXRES_HD bool arp_table_find(const LoadEntry &entry, uint64_t n, uint32_t iface, uint32_t addr,
                                      ArpEntryWords &found, uint64_t &index) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const ArpEntryWords e = entry(mid);
        if (e.iface() == iface && e.addr() == addr) {
            found = e;
            index = mid;
            return true;
        }
        if (e.iface() < iface || (e.iface() == iface && e.addr() < addr)) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// The 14 bytes of an Ethernet header as little-endian dwords (of d the low half; the high is zero).
// (Scalars, not an array: every use names its dword, so the kernels keep them in registers.)
struct EthImage {
    uint32_t a, b, c, d;
};

// The outcome for one segment. r[4]: aipstack_tx_route as dwords (next_hop, arp_index,
// iface | status << 16 | flags << 24, 0). For _SENT: image() = the slot's bytes 0..13, and `used` = the
// entry that resolved it or kTxResMaxCount.
struct TxDecision {
    uint32_t status;
    uint32_t r[4];
    uint32_t oa, ob, oc, od;  // an EthImage's dwords
    uint64_t used;
    AIPSTACK_TXRES_HD EthImage image() const { return EthImage{oa, ob, oc, od}; }
};

// src / dst: the IPv4 addresses in host byte order; send_flags: AIPSTACK_TX_ALLOW_*; force: an
// interface index or AIPSTACK_TX_ROUTE_ANY. iface(k), k < n_ifaces: the table in the order
// m_iface_list iterates. The order of the tests and of the error returns is sendIp4Dgram's.
template <class LoadIface, class LoadEntry>
AIPSTACK_TXRES_HD TxDecision tx_resolve_decide(uint32_t src, uint32_t dst, uint32_t send_flags,
                                               uint32_t force, const LoadIface &iface, uint32_t n_ifaces,
                                               const LoadEntry &entry, uint64_t n_arp) {
    TxDecision d;
    d.used = kTxResMaxCount;
    d.oa = d.ob = d.oc = d.od = 0u;
    uint32_t flags = 0u, hop = 0u, k = force;
    TxIfaceWords f{0u, 0u, 0u, 0u, 0u};
    bool routed = false;
    if (force == AIPSTACK_TX_ROUTE_ANY) {                                  // routeIp4, :713-741
        int best_prefix = -1;
        for (uint32_t q = 0; q < n_ifaces; ++q) {
            const TxIfaceWords g = iface(q);
            if (g.is_local(dst)) {
                if (g.prefix() > best_prefix) {
                    best_prefix = g.prefix();
                    f = g, k = q, routed = true;
                }
            } else if (g.have_gateway() && !routed) {
                f = g, k = q, routed = true;
            }
        }
        if (routed) {
            hop = best_prefix >= 0 ? dst : f.gateway;
            if (best_prefix < 0) flags |= AIPSTACK_TX_ROUTE_GATEWAY;
        }
    } else {                                                               // routeIp4ForceIface, :764-780
        flags |= AIPSTACK_TX_ROUTE_FORCED;
        if (force < n_ifaces) {
            f = iface(force);
            if (dst == 0xFFFFFFFFu || f.is_local(dst)) {
                hop = dst, routed = true;
            } else if (f.have_gateway()) {
                hop = f.gateway, routed = true;
                flags |= AIPSTACK_TX_ROUTE_GATEWAY;
            }
        }
    }
    uint32_t status, arp_index = AIPSTACK_TX_NO_ARP_ENTRY;
    if (!routed) {
        status = AIPSTACK_TX_RES_NO_ROUTE;                                  // :394
    } else if ((send_flags & AIPSTACK_TX_ALLOW_BROADCAST) == 0u &&         // :669-679
               (dst == 0xFFFFFFFFu || (f.have_addr() && dst == f.bcastaddr()))) {
        status = AIPSTACK_TX_RES_BCAST_REJECTED;
    } else if ((send_flags & AIPSTACK_TX_ALLOW_NONLOCAL_SRC) == 0u &&      // :681-687
               (!f.have_addr() || src != f.addr)) {
        status = AIPSTACK_TX_RES_NONLOCAL_SRC;
    } else {                                                               // resolve_hw_addr
        ArpEntryWords e{0u, 0u, 0u, 0u};
        uint64_t index = 0;
        uint32_t mac_lo = 0xFFFFFFFFu, mac_hi = 0xFFFFu;
        if (arp_table_find(entry, n_arp, k, hop, e, index)) {              // eth/EthIpIface.h:650
            arp_index = (uint32_t)index;  // (n_arp < 2^32 - 1: tx_resolve_check_args)
            if (e.state() >= AIPSTACK_ARP_STATE_VALID) {                   // :543
                status = AIPSTACK_TX_RES_SENT;
                mac_lo = e.mac_lo(), mac_hi = e.mac_hi();
                d.used = index;
            } else {
                status = AIPSTACK_TX_RES_ARP_QUERY;                        // :583
            }
        } else if (hop == 0xFFFFFFFFu) {                                   // :675
            status = AIPSTACK_TX_RES_SENT;
            flags |= AIPSTACK_TX_ROUTE_BROADCAST;
        } else if (hop == 0u || !f.have_addr() || (hop & f.netmask) != f.netaddr()) {  // :680-693
            status = AIPSTACK_TX_RES_NO_HW_ROUTE;
        } else if (hop == f.bcastaddr()) {                                 // :696
            status = AIPSTACK_TX_RES_SENT;
            flags |= AIPSTACK_TX_ROUTE_BROADCAST;
        } else {                                                           // :700-712, :566-583
            status = AIPSTACK_TX_RES_ARP_QUERY;
            flags |= AIPSTACK_TX_ROUTE_NEW_ENTRY;
        }
        if (status == AIPSTACK_TX_RES_SENT) {                              // :427-430
            d.oa = mac_lo, d.ob = mac_hi | (f.pfm & 0xFFFF0000u), d.oc = f.mac_hi, d.od = 0x0008u;
        }
    }
    d.status = status;
    d.r[0] = hop;
    d.r[1] = arp_index;
    d.r[2] = (k & 0xFFFFu) | status << 16 | flags << 24;
    d.r[3] = 0u;
    return d;
}

// Whether segment i has something to resolve, from what is known before a slot byte is read.
AIPSTACK_TXRES_HD bool tx_res_candidate(uint32_t hdr_len, uint64_t hdr_stride, uint32_t seg_status) {
    return hdr_len >= kTxResMinHeader && hdr_len <= hdr_stride &&
           seg_status != AIPSTACK_TX_BURST_INVALID && seg_status != AIPSTACK_TX_DGRAM_INVALID;
}

// A whole segment's outcome as the decide pass computes it. ld16(off) / ld32(off): the
// little-endian half / dword at slot bytes [off, off + 2 / 4), called only for bytes 12..13 and
// 26..33 of a candidate. seg_status: 0 where the caller passes none. _RES_NONE: the all-zero
// record and image.
template <class Load16, class Load32, class LoadIface, class LoadEntry>
AIPSTACK_TXRES_HD TxDecision tx_resolve_segment(const Load16 &ld16, const Load32 &ld32, uint32_t hdr_len,
                                                uint64_t hdr_stride, uint32_t seg_status,
                                                uint32_t send_flags, uint32_t force, const LoadIface &iface,
                                                uint32_t n_ifaces, const LoadEntry &entry, uint64_t n_arp) {
    if (tx_res_candidate(hdr_len, hdr_stride, seg_status) && ld16(12u) == 0x0008u)
        return tx_resolve_decide(txres_bswap32(ld32(26u)), txres_bswap32(ld32(30u)), send_flags, force,
                                 iface, n_ifaces, entry, n_arp);
    TxDecision d;
    d.status = AIPSTACK_TX_RES_NONE;
    d.used = kTxResMaxCount;
    d.r[0] = d.r[1] = d.r[2] = d.r[3] = 0u;
    d.oa = d.ob = d.oc = d.od = 0u;
    return d;
}

// The dword of image bytes [at, at + 4), at <= 11.
template <uint32_t at>
AIPSTACK_TXRES_HD uint32_t tx_res_bytes(const EthImage o) {
    static_assert(at <= 11u, "inside the image");
    constexpr uint32_t q = at >> 2, s = (at & 3u) * 8u;
    const uint32_t lo = q == 0u ? o.a : q == 1u ? o.b : o.c, hi = q == 0u ? o.b : q == 1u ? o.c : o.d;
    return (uint32_t)(((uint64_t)lo | (uint64_t)hi << 32) >> s);
}

// Stores the 14 image bytes to a slot whose address is `align` mod 4: st(off, width, value) is a
// store of the low `width` bytes of `value` at slot byte `off`, naturally aligned (off + align is
// a multiple of width), the widest the address allows; together exactly bytes [0, 14).
template <class Store>
AIPSTACK_TXRES_HD void tx_res_store_header(uint32_t align, const EthImage o, const Store &st) {
    switch (align & 3u) {
    case 0u:
        st(0u, 4u, o.a), st(4u, 4u, o.b), st(8u, 4u, o.c), st(12u, 2u, o.d);
        break;
    case 2u:
        st(0u, 2u, o.a), st(2u, 4u, tx_res_bytes<2u>(o)), st(6u, 4u, tx_res_bytes<6u>(o)),
            st(10u, 4u, tx_res_bytes<10u>(o));
        break;
    case 3u:
        st(0u, 1u, o.a), st(1u, 4u, tx_res_bytes<1u>(o)), st(5u, 4u, tx_res_bytes<5u>(o)),
            st(9u, 4u, tx_res_bytes<9u>(o)), st(13u, 1u, o.d >> 8);
        break;
    default:
        st(0u, 1u, o.a), st(1u, 2u, tx_res_bytes<1u>(o)), st(3u, 4u, tx_res_bytes<3u>(o)),
            st(7u, 4u, tx_res_bytes<7u>(o)), st(11u, 2u, tx_res_bytes<11u>(o)), st(13u, 1u, o.d >> 8);
        break;
    }
}

// The argument checks of aipstack_tx_resolve (txres_host.cpp; no HIP call).
struct TxResolveArgs {
    const void *d_hdr;
    uint64_t hdr_stride;
    const void *d_hdr_len;
    uint64_t n;
    const void *d_force_iface, *d_ifaces;
    uint32_t n_ifaces;
    const void *d_arp;
    uint64_t n_arp;
    const void *d_status, *d_route, *d_send_len, *d_arp_used, *d_held_seg, *d_failed_seg, *d_counts,
        *d_workspace;
    uint64_t workspace_bytes;
};
int tx_resolve_check_args(const TxResolveArgs &a);

}  // namespace aipstack_amd

#endif
