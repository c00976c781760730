// aipstack_amd -- the search of a table of aipstack_tcp_pcb_key entries sorted by
// tcp_pcb_key_compare (tcprx_common.h), shared by the TCP Rx parse (find_pcb) and the UDP Rx demux
// (m_associations_index.findEntry): plain C++, so that the kernels and the stand-alone host tests
// run one text, wherever an entry is read from.
#ifndef AIPSTACK_AMD_PCB_LOOKUP_H
#define AIPSTACK_AMD_PCB_LOOKUP_H

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "tcprx_common.h"

namespace aipstack_amd {

// One 16-byte table entry as its four little-endian dwords: local_addr, remote_addr,
// local_port | remote_port << 16, cookie.
struct PcbEntryWords {
    uint32_t x, y, z, w;
};

// True, and the entry's cookie, if the table of `n` entries read through `entry(index)` holds one
// equal to `key`. Every entry read has an index in [lo, hi) within [0, n), whatever the table
// holds; the range shrinks by at least one entry per step.
template <class LoadEntry>
AIPSTACK_TCPRX_HD bool pcb_table_find(const LoadEntry &entry, uint64_t n,
                                      const aipstack_tcp_pcb_key &key, uint32_t &cookie) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const PcbEntryWords e = entry(mid);
        aipstack_tcp_pcb_key k;
        k.local_addr = e.x;
        k.remote_addr = e.y;
        k.local_port = (uint16_t)(e.z & 0xFFFFu);
        k.remote_port = (uint16_t)(e.z >> 16);
        const int c = tcp_pcb_key_compare(k, key);
        if (c == 0) {
            cookie = e.w;
            return true;
        }
        if (c < 0) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

}  // namespace aipstack_amd

#endif
