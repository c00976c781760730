// aipstack_amd -- what the Tx producers' kernels share (tcpseg_kernels.hip: a burst owns
// segments; ipfrag_kernels.hip: a datagram owns fragments): the owner search over the caller's
// running sums (tx_producer_common.h has its pure part), an owner's ranges and contract, the plan
// pass's record, the header template as dwords with its sums, and the emit pass's slot store. On
// top of lane_pass.h, for the two .hip translation units only, in an anonymous namespace.
#ifndef AIPSTACK_AMD_TX_PRODUCER_H
#define AIPSTACK_AMD_TX_PRODUCER_H

#include "lane_pass.h"
#include "tx_producer_common.h"

namespace aipstack_amd {
namespace {

// One element per lane of the n elements that the running sums `idx` (n_owners + 1 entries)
// share out among the owners: owned(d, i) for element i of owner d (idx[d] <= i < idx[d+1]),
// unowned(j, i) for one the sums give to no owner (they do not run from 0 to n; j = where the
// search ended). The wave's 64 elements mostly share one or two owners: the owners of its first
// and last element are found with wave-uniform searches, and each lane searches only between
// them (no step at all when they agree: d is then wave-uniform, so that the descriptor and index
// loads of owned() are shared).
template <class Owned, class Unowned>
__device__ __forceinline__ void for_each_owned(const uint64_t *__restrict__ idx, uint64_t n_owners,
                                               uint64_t n, const WaveStride &ws, Owned owned,
                                               Unowned unowned) {
    for (uint64_t base = uniform64(ws.first); base < n; base += ws.step) {
        const uint64_t last = base + (kWave - 1) < n ? base + (kWave - 1) : n - 1;
        const uint64_t j0 = uniform64(upper_bound(idx, 0, n_owners + 1, base));
        const uint64_t j1 = uniform64(upper_bound(idx, j0, n_owners + 1, last));
        const uint64_t i = base + ws.lane;
        if (i >= n) continue;
        if (j0 == j1 && j0 >= 1 && j0 <= n_owners) {
            const uint64_t d = j0 - 1;
            if (idx[d] <= base && last < idx[d + 1]) {
                owned(d, i);
                continue;
            }
        }
        const OwnerOf o = owner_of(idx, n_owners, j0, j1, i);
        if (o.owned) owned(o.at, i);
        else unowned(o.at, i);
    }
}

// An owner's view of the caller's two indices: elements [eb, ee), chunks [cb, ce).
struct OwnerRange {
    uint64_t eb, ee, cb, ce;
};

__device__ __forceinline__ OwnerRange owner_range(const uint64_t *__restrict__ idx,
                                                  const uint64_t *__restrict__ chunk_base,
                                                  uint64_t d) {
    return OwnerRange{idx[d], idx[d + 1], chunk_base[d], chunk_base[d + 1]};
}

// The contract: a descriptor that is `valid` by itself, and indices that give it the S elements
// and C chunks of its shape, inside the n elements and n_chunks chunks of the call.
__device__ __forceinline__ bool owner_ok(bool valid, uint64_t S, uint64_t C, const OwnerRange &r,
                                         uint64_t n, uint64_t n_chunks) {
    return valid && r.ee >= r.eb && r.ee - r.eb == S && r.ee <= n && r.ce >= r.cb &&
           r.ce - r.cb == C && r.ce <= n_chunks;
}

// The chunk entries of an owner that breaks the contract, clipped to the table: [c0, c0 + cnt).
__device__ __forceinline__ void clip_chunks(const OwnerRange &r, uint64_t n_chunks, uint64_t &c0,
                                            uint64_t &cnt) {
    c0 = r.cb < n_chunks ? r.cb : n_chunks;
    cnt = r.ce >= r.cb ? r.ce - r.cb : 0u;
    if (cnt > n_chunks - c0) cnt = n_chunks - c0;
}

// The record of element i (workspace, 8 bytes): bits 0-39 the owner, 40-55 the IPv4 header
// checksum, 56 = valid (emit the slot; else the entry point's INVALID status).
constexpr uint64_t kRecOwnerMask = (1ull << 40) - 1u;
constexpr uint64_t kRecValid = 1ull << 56;

__device__ __forceinline__ uint64_t make_record(uint64_t owner, uint32_t ip_checksum, bool valid) {
    return (owner & kRecOwnerMask) | (uint64_t)ip_checksum << 40 | (valid ? kRecValid : 0u);
}
__device__ __forceinline__ uint64_t record_owner(uint64_t rec) { return rec & kRecOwnerMask; }
__device__ __forceinline__ uint32_t record_ip_checksum(uint64_t rec) {
    return (uint32_t)(rec >> 40) & 0xFFFFu;
}
__device__ __forceinline__ bool record_valid(uint64_t rec) { return (rec & kRecValid) != 0u; }

// The first N dwords of a descriptor's header template `hdr` (8-byte aligned): uint2 pairs,
// plus one dword when N is odd.
template <int N>
struct HeaderWords {
    uint32_t t[N];
};

template <int N>
__device__ __forceinline__ HeaderWords<N> load_header_words(const uint8_t *__restrict__ hdr) {
    HeaderWords<N> r;
    const uint2 *p = reinterpret_cast<const uint2 *>(hdr);
#pragma unroll
    for (int q = 0; q < N / 2; ++q) {
        const uint2 v = p[q];
        r.t[2 * q] = v.x;
        r.t[2 * q + 1] = v.y;
    }
    if constexpr (N % 2 != 0) r.t[N - 1] = reinterpret_cast<const uint32_t *>(hdr)[N - 1];
    return r;
}

// Little-endian halves of the source and destination address (frame bytes 26-33).
template <int N>
__device__ __forceinline__ uint32_t addr_halves(const HeaderWords<N> &h) {
    return (h.t[6] >> 16) + (h.t[7] & 0xFFFFu) + (h.t[7] >> 16) + (h.t[8] & 0xFFFFu);
}

// The IPv4 header checksum: version/IHL/DSCP, TTL/protocol and the addresses from the template,
// the field as 0, plus what the producer takes from elsewhere: `le` (little-endian halves of
// further template words) and `be` (the sum of its per-element big-endian words).
template <int N>
__device__ __forceinline__ uint32_t ip_header_checksum(const HeaderWords<N> &h, uint32_t le,
                                                       uint32_t be) {
    le += (h.t[3] >> 16) + (h.t[5] >> 16) + addr_halves(h);
    return ~fold16(bswap16(fold16(le)) + be) & 0xFFFFu;
}

// The first HL bytes of the slot image `o` to P, unaligned, in 16-, 8-, 4- and 2-byte stores.
template <int HL>
__device__ __forceinline__ void store_header_bytes(uint64_t P, const uint32_t (&o)[16]) {
    static_assert(HL % 2 == 0 && HL <= 64, "");
    constexpr int Q = HL / 16, at8 = 16 * Q, at4 = at8 + (HL & 8), at2 = at4 + (HL & 4);
#pragma unroll
    for (int q = 0; q < Q; ++q)
        *reinterpret_cast<global_t<u32x4, 1> *>(P + 16u * q) =
            u32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
    if constexpr ((HL & 8) != 0)
        *reinterpret_cast<global_t<u32x2, 1> *>(P + at8) = u32x2{o[at8 / 4], o[at8 / 4 + 1]};
    if constexpr ((HL & 4) != 0) *reinterpret_cast<global_t<uint32_t, 1> *>(P + at4) = o[at4 / 4];
    if constexpr ((HL & 2) != 0)
        *reinterpret_cast<global_t<uint16_t, 1> *>(P + at2) = (uint16_t)o[at2 / 4];
}

// True if the header ring is stored in whole lines: 64-byte slots from a 64-byte boundary.
inline bool ring_in_lines(uint64_t hdr_base, uint64_t hdr_stride) {
    return hdr_stride == 64u && (hdr_base & 63u) == 0u;
}

// The emit pass's tail: the slot image `o` of element base + lane (`valid`: emit it; its header
// is hl bytes, HL0 or HL1) goes to slot base + lane of the ring. LINES (ring_in_lines): the wave
// passes its 64 slots through LDS and stores them whole; every lane of the wave calls it. Else
// per-lane unaligned stores of exactly hl bytes, then zeros up to min(hdr_stride, 64).
template <bool LINES, int HL0, int HL1 = HL0>
__device__ __forceinline__ void store_header_slot(LineTiles<4, LINES> &tile, const WaveStride &ws,
                                                  uint64_t hdr_base, uint64_t hdr_stride,
                                                  uint64_t base, bool valid, uint32_t hl,
                                                  const uint32_t (&o)[16]) {
    if constexpr (LINES) {
        const uint64_t ok = __builtin_amdgcn_ballot_w64(valid);  // (valid: below n)
        store_wave_lines<4>(tile[ws.wave], ws.lane, hdr_base, base, ok, o);
    } else if (valid) {
        const uint64_t P = hdr_base + (base + ws.lane) * hdr_stride;
        if (HL0 == HL1 || hl == HL0) store_header_bytes<HL0>(P, o);
        else store_header_bytes<HL1>(P, o);
        const uint32_t end = hdr_stride < 64u ? (uint32_t)hdr_stride : 64u;
        for (uint32_t z = hl; z < end; ++z) *reinterpret_cast<global_t<uint8_t> *>(P + z) = 0u;
    }
}

}  // namespace
}  // namespace aipstack_amd

#endif
