// aipstack_amd -- Tx resolve, the host side (plain C++, no HIP call): the sort of the ARP table,
// the workspace size and the argument checks of aipstack_tx_resolve (the launcher is in
// txres_kernels.hip).

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "aipstack_amd/chksum.h"
#include "txres_common.h"

static_assert(sizeof(aipstack_tx_iface) == 32, "aipstack_tx_iface is 32 bytes");
static_assert(offsetof(aipstack_tx_iface, netmask) == 4 && offsetof(aipstack_tx_iface, gateway) == 8 &&
                  offsetof(aipstack_tx_iface, prefix) == 12 && offsetof(aipstack_tx_iface, flags) == 13 &&
                  offsetof(aipstack_tx_iface, mac) == 14 && offsetof(aipstack_tx_iface, reserved) == 20,
              "aipstack_tx_iface field offsets");
static_assert(sizeof(aipstack_arp_entry) == 16, "aipstack_arp_entry is 16 bytes");
static_assert(offsetof(aipstack_arp_entry, iface) == 4 && offsetof(aipstack_arp_entry, state) == 6 &&
                  offsetof(aipstack_arp_entry, mac) == 7 && offsetof(aipstack_arp_entry, reserved) == 13,
              "aipstack_arp_entry field offsets");
static_assert(sizeof(aipstack_tx_route) == 16, "aipstack_tx_route is 16 bytes");
static_assert(offsetof(aipstack_tx_route, arp_index) == 4 && offsetof(aipstack_tx_route, iface) == 8 &&
                  offsetof(aipstack_tx_route, status) == 10 && offsetof(aipstack_tx_route, flags) == 11 &&
                  offsetof(aipstack_tx_route, reserved) == 12,
              "aipstack_tx_route field offsets");

using namespace aipstack_amd;

extern "C" int aipstack_arp_table_sort(aipstack_arp_entry *h_entries, uint64_t n) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    if (!h_entries || n >= AIPSTACK_TX_NO_ARP_ENTRY) return AIPSTACK_CHKSUM_EINVAL;
    // (sorted even when the table is rejected: a permutation of the input either way)
    std::sort(h_entries, h_entries + n, [](const aipstack_arp_entry &a, const aipstack_arp_entry &b) {
        return a.iface != b.iface ? a.iface < b.iface : a.addr < b.addr;
    });
    for (uint64_t i = 0; i < n; ++i) {
        const aipstack_arp_entry &e = h_entries[i];
        if (e.state < AIPSTACK_ARP_STATE_QUERY || e.state > AIPSTACK_ARP_STATE_REFRESHING ||
            e.iface >= AIPSTACK_TX_MAX_IFACES || e.reserved[0] || e.reserved[1] || e.reserved[2])
            return AIPSTACK_CHKSUM_EINVAL;
        if (i != 0 && h_entries[i - 1].iface == e.iface && h_entries[i - 1].addr == e.addr)
            return AIPSTACK_CHKSUM_EINVAL;
    }
    return AIPSTACK_CHKSUM_OK;
}

// One pair of 64-bit counts (held, failed segments) per tile of kTxResTile segments and the
// totals, then per tile the ballot pair of each of its waves.
extern "C" uint64_t aipstack_tx_resolve_workspace(uint64_t n) {
    const uint64_t tiles = tx_res_tiles(n);
    return 16u * (tiles + 1) + 16u * kTxResTileWaves * tiles;
}

namespace aipstack_amd {

int tx_resolve_check_args(const TxResolveArgs &a) {
    for (const void *p : {a.d_hdr, a.d_hdr_len, a.d_ifaces, a.d_status, a.d_route, a.d_send_len,
                          a.d_held_seg, a.d_failed_seg, a.d_counts, a.d_workspace})
        if (!p) return AIPSTACK_CHKSUM_EINVAL;
    if (a.n_arp != 0 && (!a.d_arp || !a.d_arp_used)) return AIPSTACK_CHKSUM_EINVAL;
    if (a.n > kTxResMaxCount || a.n_arp >= AIPSTACK_TX_NO_ARP_ENTRY || a.hdr_stride == 0 ||
        a.n_ifaces > AIPSTACK_TX_MAX_IFACES)
        return AIPSTACK_CHKSUM_EINVAL;
    for (const void *p : {a.d_held_seg, a.d_failed_seg, a.d_counts, a.d_workspace})
        if (((uintptr_t)p & 7u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    for (const void *p : {a.d_hdr_len, a.d_send_len, a.d_route, a.d_ifaces, a.d_arp})
        if (((uintptr_t)p & 3u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    if (((uintptr_t)a.d_force_iface & 1u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    if (a.workspace_bytes < aipstack_tx_resolve_workspace(a.n)) return AIPSTACK_CHKSUM_EINVAL;
    return AIPSTACK_CHKSUM_OK;
}

}  // namespace aipstack_amd
