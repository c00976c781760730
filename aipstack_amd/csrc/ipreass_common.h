// aipstack_amd -- IPv4 reassembly on receive: what the host code (ipreass_host.cpp), the kernels
// (ipreass_kernels.hip) and the serial host test (tests/cpp/ipreass_table_test.cpp) share, so
// that a fragment's fields, its key, the hash, the two tables and the datagram verdict are one
// text wherever they run. The table operations take an `Atomics` policy: the kernels give the
// device atomics on global memory, the host test plain loads and stores.
#ifndef AIPSTACK_AMD_IPREASS_COMMON_H
#define AIPSTACK_AMD_IPREASS_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"

#if defined(__HIPCC__)
#define AIPSTACK_REASS_HD __host__ __device__ inline
#else
#define AIPSTACK_REASS_HD inline
#endif

namespace aipstack_amd {

constexpr uint64_t kReassMaxCount = 0xFFFFFFFEull;  // frames of one call: 2^32 - 2
constexpr uint32_t kReassMaxSteps = 8192u;          // fragments of one datagram (65531 / 8 + 1)
constexpr uint32_t kReassMinSize = 1u, kReassMaxSize = 65531u;  // MaxReassSize (IpReassembly.h:96)

// One fragment's record in the workspace (16 bytes). w[0] = source, w[1] = destination (host
// order), w[2] = ident | proto << 16 | flags << 24, w[3] = offset | length << 16 (bytes).
constexpr uint32_t kReassMember = 1u;  // flag: a non-empty fragment inside the size bound
constexpr uint32_t kReassMF = 2u;      // flag: more fragments
struct ReassRec {
    uint32_t w[4];
    AIPSTACK_REASS_HD bool member() const { return (w[2] >> 24 & kReassMember) != 0u; }
    AIPSTACK_REASS_HD bool mf() const { return (w[2] >> 24 & kReassMF) != 0u; }
    AIPSTACK_REASS_HD uint32_t proto() const { return w[2] >> 16 & 0xFFu; }
    AIPSTACK_REASS_HD uint32_t off() const { return w[3] & 0xFFFFu; }
    AIPSTACK_REASS_HD uint32_t len() const { return w[3] >> 16; }
    // the key of find_reass_entry (IpReassembly.h:409-412): addresses, ident, protocol
    AIPSTACK_REASS_HD bool same_key(const ReassRec &o) const {
        return w[0] == o.w[0] && w[1] == o.w[1] && ((w[2] ^ o.w[2]) & 0xFFFFFFu) == 0u;
    }
};

AIPSTACK_REASS_HD uint32_t reass_bswap32(uint32_t x) {
    return x >> 24 | (x >> 8 & 0xFF00u) | (x << 8 & 0xFF0000u) | x << 24;
}
AIPSTACK_REASS_HD uint32_t reass_be16lo(uint32_t w) {  // the big-endian 16 bits in w's bytes 0-1
    return (w & 0xFFu) << 8 | (w >> 8 & 0xFFu);
}

// What a fragment is to the call.
constexpr int kReassNone = 0;      // not a readable fragment: left alone
constexpr int kReassEmpty = 1;     // empty payload: reassembleIp4 returns at once (:189-191)
constexpr int kReassOversize = 2;  // breaks offset <= max && len <= max - offset (:219-223)
constexpr int kReassIn = 3;        // a member that can be linked

// The fields of a frame that Rx verify called a fragment, of `len` bytes, read through `ld(off)`
// = the little-endian dword at frame bytes [off, off + 4); only bytes below 34 are read, and
// only after the lengths verify checked (ip/IpStack.h:938-990) are restated. Fields as
// ip/IpStack.h:1021-1034 takes them. payload_off = 14 + 4*IHL.
template <class Load>
AIPSTACK_REASS_HD int reass_fragment(const Load &ld, uint32_t len, uint32_t max_reass_size,
                                     ReassRec &r, uint32_t &payload_off) {
    r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0u;
    payload_off = 0u;
    if (len < 14u + 20u) return kReassNone;
    const uint32_t v = ld(14u);                  // version/IHL, DSCP, total length
    const uint32_t hl = (v & 0xFu) * 4u;
    const uint32_t total = reass_be16lo(v >> 16);
    if (hl < 20u || total < hl || 14u + total > len) return kReassNone;
    const uint32_t idf = ld(18u);                // ident, flags / offset
    const uint32_t fo = reass_be16lo(idf >> 16);
    if ((fo & 0x3FFFu) == 0u) return kReassNone; // a whole datagram
    const uint32_t proto = ld(20u) >> 24;        // frame byte 23
    const uint32_t off = (fo & 0x1FFFu) * 8u, plen = total - hl;
    const uint32_t mf = (fo & 0x2000u) != 0u ? kReassMF : 0u;
    r.w[0] = reass_bswap32(ld(26u));
    r.w[1] = reass_bswap32(ld(30u));
    r.w[2] = reass_be16lo(idf) | proto << 16 | mf << 24;
    r.w[3] = off | plen << 16;
    payload_off = 14u + hl;
    if (plen == 0u) return kReassEmpty;
    if (off > max_reass_size || plen > max_reass_size - off) return kReassOversize;
    r.w[2] |= kReassMember << 24;
    return kReassIn;
}

// The hash of a key, and of a key with a byte offset.
AIPSTACK_REASS_HD uint32_t reass_mix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
AIPSTACK_REASS_HD uint32_t reass_hash_key(const ReassRec &r) {
    uint32_t h = r.w[0] * 0x9E3779B1u;
    h = (h << 13 | h >> 19) ^ r.w[1] * 0x85EBCA77u;
    h = (h << 13 | h >> 19) ^ (r.w[2] & 0xFFFFFFu) * 0xC2B2AE3Du;
    return reass_mix(h);
}
AIPSTACK_REASS_HD uint32_t reass_hash_key_off(const ReassRec &r, uint32_t off) {
    return reass_mix(reass_hash_key(r) + off * 0x27D4EB2Fu + 1u);
}

// The workspace: byte offsets of its parts. slots = the entries of each table, a power of two,
// at least 4 per frame.
struct ReassWorkspace {
    uint64_t slots, index, recs, succ, sums, pairs, keys, total;
};
AIPSTACK_REASS_HD ReassWorkspace reass_workspace(uint64_t n) {
    if (n > kReassMaxCount) n = kReassMaxCount;
    ReassWorkspace w;
    w.slots = 64u;
    while (w.slots < 4u * n) w.slots <<= 1;
    w.index = 0u;                                // n + 1 x uint64: index[i] = i
    w.recs = w.index + 8u * (n + 1u);            // n x ReassRec
    w.succ = w.recs + 16u * n;                   // n x uint32
    w.sums = w.succ + ((4u * n + 7u) & ~7ull);   // n x uint16
    w.pairs = w.sums + ((2u * n + 7u) & ~7ull);  // the (key, offset) table
    w.keys = w.pairs + 8u * w.slots;             // the key table
    w.total = w.keys + 8u * w.slots;
    return w;
}

// Both tables: `slots` 64-bit entries, open addressing with linear probing; 0 = empty. Bits 0-31
// hold 1 + the frame index of the fragment that claimed the entry. The (key, offset) table:
// bit 32 = poisoned (a second fragment with an equal key and offset came). The key table: bits
// 32-63 count the key's fragments (at most 2^32 - 2: no carry out). Every probe sequence takes
// at most `slots` steps and masks its position into the table; an entry whose index is not
// below n is taken for another key's, whatever else it holds.
constexpr uint64_t kReassPoison = 1ull << 32;
constexpr uint64_t kReassOne = 1ull << 32;

template <class Atomics>
AIPSTACK_REASS_HD void reass_insert_pair(const Atomics &at, uint64_t *table, uint64_t slots,
                                         const ReassRec *recs, uint64_t n, uint32_t i) {
    const ReassRec me = recs[i];
    const uint64_t mask = slots - 1u;
    uint64_t s = reass_hash_key_off(me, me.off()) & mask;
    for (uint64_t step = 0; step < slots; ++step, s = (s + 1u) & mask) {
        uint64_t v = at.load(&table[s]);
        if (v == 0u) {
            v = at.cas(&table[s], 0u, (uint64_t)i + 1u);
            if (v == 0u) return;
        }
        const uint64_t owner = (v & 0xFFFFFFFFu) - 1u;
        if (owner < n && recs[owner].same_key(me) && recs[owner].off() == me.off()) {
            at.fetch_or(&table[s], kReassPoison);
            return;
        }
    }
}

template <class Atomics>
AIPSTACK_REASS_HD void reass_insert_key(const Atomics &at, uint64_t *table, uint64_t slots,
                                        const ReassRec *recs, uint64_t n, uint32_t i) {
    const ReassRec me = recs[i];
    const uint64_t mask = slots - 1u;
    uint64_t s = reass_hash_key(me) & mask;
    for (uint64_t step = 0; step < slots; ++step, s = (s + 1u) & mask) {
        uint64_t v = at.load(&table[s]);
        if (v == 0u) {
            v = at.cas(&table[s], 0u, ((uint64_t)i + 1u) | kReassOne);
            if (v == 0u) return;
        }
        const uint64_t owner = (v & 0xFFFFFFFFu) - 1u;
        if (owner < n && recs[owner].same_key(me)) {
            at.fetch_add(&table[s], kReassOne);
            return;
        }
    }
}

// The frame index under (me's key, off), AIPSTACK_REASS_NONE if there is none or it is poisoned.
AIPSTACK_REASS_HD uint32_t reass_find_pair(const uint64_t *table, uint64_t slots,
                                           const ReassRec *recs, uint64_t n, const ReassRec &me,
                                           uint32_t off) {
    const uint64_t mask = slots - 1u;
    uint64_t s = reass_hash_key_off(me, off) & mask;
    for (uint64_t step = 0; step < slots; ++step, s = (s + 1u) & mask) {
        const uint64_t v = table[s];
        if (v == 0u) break;
        const uint64_t owner = (v & 0xFFFFFFFFu) - 1u;
        if (owner < n && recs[owner].same_key(me) && recs[owner].off() == off)
            return (v & kReassPoison) != 0u ? AIPSTACK_REASS_NONE : (uint32_t)owner;
    }
    return AIPSTACK_REASS_NONE;
}

// How many fragments carry me's key (0 if none was inserted).
AIPSTACK_REASS_HD uint32_t reass_key_count(const uint64_t *table, uint64_t slots,
                                           const ReassRec *recs, uint64_t n, const ReassRec &me) {
    const uint64_t mask = slots - 1u;
    uint64_t s = reass_hash_key(me) & mask;
    for (uint64_t step = 0; step < slots; ++step, s = (s + 1u) & mask) {
        const uint64_t v = table[s];
        if (v == 0u) break;
        const uint64_t owner = (v & 0xFFFFFFFFu) - 1u;
        if (owner < n && recs[owner].same_key(me)) return (uint32_t)(v >> 32);
    }
    return 0u;
}

// The successor of fragment i for the link pass: the member at offset + length, if MF is set.
AIPSTACK_REASS_HD uint32_t reass_successor(const uint64_t *pairs, uint64_t slots,
                                           const ReassRec *recs, uint64_t n, uint32_t i) {
    const ReassRec me = recs[i];
    if (!me.member() || !me.mf()) return AIPSTACK_REASS_NONE;
    const uint32_t end = me.off() + me.len();
    if (end > kReassMaxSize) return AIPSTACK_REASS_NONE;
    return reass_find_pair(pairs, slots, recs, n, me, end);
}

// The walk of the finish pass from the offset-0 member `head` whose key has `count` fragments:
// true iff following the successors reaches a member without MF in exactly `count` members (at
// most kReassMaxSteps). Every index followed is checked against n, every member against the key
// and the offset it must have, so the walk stays in the arrays and ends, whatever the workspace
// holds. On success: last = the member without MF, data_len = the reassembled length, sum = the
// members' sums added with end-around carry (not folded to 16 bits: at most 8192 * 0xFFFF).
AIPSTACK_REASS_HD bool reass_walk(const ReassRec *recs, const uint32_t *succ, const uint16_t *sums,
                                  uint64_t n, uint32_t head, uint32_t count, uint32_t &last,
                                  uint32_t &data_len, uint32_t &sum) {
    const ReassRec h = recs[head];
    if (!h.member() || h.off() != 0u || count < 2u || count > kReassMaxSteps) return false;
    uint32_t cur = head, steps = 1u, at = 0u, total = 0u;
    for (;;) {
        const ReassRec r = recs[cur];
        if (!r.member() || !r.same_key(h) || r.off() != at) return false;
        total += sums[cur];
        at += r.len();
        if (!r.mf()) break;
        const uint32_t nx = succ[cur];
        if (nx >= n || steps == count) return false;
        ++steps;
        cur = nx;
    }
    if (steps != count) return false;
    last = cur;
    data_len = at;
    sum = total;
    return true;
}

AIPSTACK_REASS_HD uint32_t reass_fold16(uint32_t x) {
    x = (x & 0xFFFFu) + (x >> 16);
    return (x & 0xFFFFu) + (x >> 16);
}

// The verdict of a reassembled datagram as recvIp4Dgram's handlers would give it
// (tcp/IpTcpProto_input.h:92-100, udp/IpUdpProto.h:484-489 and :631-652, ip/IpStack.h:1093-1130;
// the length rules of the frame oracle): data_len bytes whose 16-bit words sum to `sum`
// (unfolded), p1 = the little-endian dword at payload bytes 4-7 (UDP length and checksum field;
// used for UDP only).
AIPSTACK_REASS_HD uint32_t reass_dgram_verdict(uint32_t proto, uint32_t src, uint32_t dst,
                                               uint32_t data_len, uint32_t sum, uint32_t p1) {
    const uint32_t pseudo = (src >> 16) + (src & 0xFFFFu) + (dst >> 16) + (dst & 0xFFFFu) + proto;
    if (proto == 6u) {
        if (data_len < 20u) return AIPSTACK_RX_DROP_L4_MALFORMED;
        return reass_fold16(reass_fold16(sum) + reass_fold16(pseudo + data_len)) == 0xFFFFu
                   ? AIPSTACK_RX_ACCEPT : AIPSTACK_RX_DROP_L4_CHKSUM;
    }
    if (proto == 17u) {
        if (data_len < 8u) return AIPSTACK_RX_DROP_L4_MALFORMED;
        const uint32_t ulen = reass_be16lo(p1);
        if (ulen < 8u || ulen > data_len) return AIPSTACK_RX_DROP_L4_MALFORMED;
        if ((p1 >> 16) == 0u) return AIPSTACK_RX_ACCEPT_NO_CHKSUM;
        if (ulen < data_len) return AIPSTACK_RX_REASS_TRUNCATED;
        return reass_fold16(reass_fold16(sum) + reass_fold16(pseudo + ulen)) == 0xFFFFu
                   ? AIPSTACK_RX_ACCEPT : AIPSTACK_RX_DROP_L4_CHKSUM;
    }
    if (proto == 1u) {
        if (data_len < 8u) return AIPSTACK_RX_DROP_L4_MALFORMED;
        return reass_fold16(sum) == 0xFFFFu ? AIPSTACK_RX_ACCEPT : AIPSTACK_RX_DROP_L4_CHKSUM;
    }
    return AIPSTACK_RX_ACCEPT_OTHER;
}

// The argument checks of aipstack_ip4_rx_reassemble / _slotted (ipreass_host.cpp; no HIP call).
// frames: d_offsets or d_len; slot_stride is checked when `slotted`.
int ip4_rx_reassemble_check_args(const void *d_base, const void *frames, bool slotted,
                                 uint64_t slot_stride, uint64_t n, uint32_t max_reass_size,
                                 const void *d_verdict, const void *d_chunk_addr,
                                 const void *d_chunk_len, const void *d_next, const void *d_head,
                                 const void *d_dgram, const void *d_workspace,
                                 uint64_t workspace_bytes);

}  // namespace aipstack_amd

#endif
