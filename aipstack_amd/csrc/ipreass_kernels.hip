// aipstack_amd -- IPv4 reassembly on receive (aipstack_ip4_rx_reassemble / _slotted): the
// fragments of a batch of frames grouped by the key of find_reass_entry (ip/IpReassembly.h:
// 409-412) and, where a group is a complete datagram, linked in offset order and judged as
// recvIp4Dgram's handlers would judge the reassembled payload -- without copying a byte of it.
// Stream-ordered launches, all through the caller's workspace (reass_workspace,
// ipreass_common.h):
//   1. Rx verify (aipstack_chksum_rx_verify / _slotted), unchanged, into d_verdict;
//   2. ipreass_classify_kernel, one frame per lane: of a frame with verdict 3 the IPv4 header
//      (reass_fragment: at most 34 bytes, the lengths restated first), its 16-byte record, its
//      chunk entry, the identity chain index and the default outputs; verdict 15 for an empty or
//      an oversize fragment. The same launch clears the two tables with plain stores in a
//      grid-stride loop of its own, so the call is kernels only and needs no launch for it. A
//      frame with verdict 3 whose restated lengths fail (outside the contract: the verdict byte
//      was not verify's) keeps verdict 3 with an empty chunk and is in no group;
//   3. ipreass_insert_kernel, one fragment per lane: the fragment claimed in the (key, offset)
//      table (atomicCAS; an equal pair found poisons the entry, atomicOr) and counted in the key
//      table (atomicAdd). A pass of its own after the records, so that the record a table entry
//      points to was written by an earlier launch: no ordering between lanes is relied on. An
//      oversize fragment is counted but not claimed: its group can then never be walked in as
//      many steps as it has members, which is what marks it;
//   4. the chained batch, unchanged, over the n one-chunk chains: one folded sum per fragment
//      (an empty chunk reads nothing);
//   5. ipreass_link_kernel, one fragment per lane: the member at offset + length, looked up;
//   6. ipreass_finish_kernel, one offset-0 member per lane: reass_walk over the successors,
//      then, only for a complete group, the datagram verdict, the record and its members'
//      verdicts and links (written by this one lane: a complete group has one head).
// No lane waits for another; every probe is bounded by the table size and masked into the table.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"
#include "ipreass_common.h"
#include "lane_pass.h"

namespace aipstack_amd {
namespace {

// Frame i's start address and length, as Rx verify takes them.
struct CsrFrames {
    uint64_t base;
    const uint64_t *offsets;
    __device__ __forceinline__ void frame(uint64_t i, uint64_t &S, uint32_t &len) const {
        const uint64_t a = offsets[i], b = offsets[i + 1];
        S = base + a;
        const uint64_t l = b - a;  // b < a, or over 65535 bytes: outside the contract, no read
        len = l > (uint64_t)AIPSTACK_CHKSUM_MAX_LEN ? 0u : (uint32_t)l;
    }
};

struct SlotFrames {
    uint64_t base, stride;
    const uint32_t *lens;
    uint32_t cap;  // min(stride, 65535), as verify clamps a slot's length
    __device__ __forceinline__ void frame(uint64_t i, uint64_t &S, uint32_t &len) const {
        S = base + i * stride;
        const uint32_t l = lens[i];
        len = l < cap ? l : cap;
    }
};

// The little-endian dword at bytes [off, off + 4) from S: a load at any byte alignment.
struct ByteLoad {
    uint64_t S;
    __device__ __forceinline__ uint32_t operator()(uint32_t off) const {
        return *reinterpret_cast<global_t<const uint32_t, 1> *>(S + off);
    }
};

// The table operations of ipreass_common.h on global memory, device scope, relaxed.
struct DeviceAtomics {
    __device__ __forceinline__ uint64_t load(uint64_t *p) const {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ uint64_t cas(uint64_t *p, uint64_t expect, uint64_t v) const {
        return atomicCAS(reinterpret_cast<unsigned long long *>(p), (unsigned long long)expect,
                         (unsigned long long)v);
    }
    __device__ __forceinline__ void fetch_or(uint64_t *p, uint64_t v) const {
        atomicOr(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
    }
    __device__ __forceinline__ void fetch_add(uint64_t *p, uint64_t v) const {
        atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
    }
};

struct Outputs {
    uint8_t *verdict;
    uint64_t *chunk_addr;
    uint32_t *chunk_len, *next, *head;
    uint64_t dgram;  // address of the aipstack_ip4_dgram array (4-byte aligned)
};

__device__ __forceinline__ void put_dgram(uint64_t dgram, uint64_t i, uint32_t a, uint32_t b,
                                          uint32_t c, uint32_t d) {
    *reinterpret_cast<global_t<u32x4, 4> *>(dgram + i * 16u) = u32x4{a, b, c, d};
}

template <class Frames>
__global__ __launch_bounds__(kBlock) void ipreass_classify_kernel(
    const Frames fr, uint64_t n, uint32_t max_reass_size, const Outputs o,
    uint64_t *__restrict__ index, ReassRec *__restrict__ recs, uint64_t *__restrict__ tables,
    uint64_t table_entries) {
    const WaveStride ws;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < table_entries; j += ws.step)
        tables[j] = 0u;
    for (uint64_t base = uniform64(ws.first); base < n; base += ws.step) {
        const uint64_t i = base + ws.lane;
        if (i >= n) continue;
        ReassRec r;
        r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0u;
        uint64_t addr = 0;
        uint32_t len = 0;
        if (o.verdict[i] == AIPSTACK_RX_FRAGMENT) {
            uint64_t S;
            uint32_t flen, poff;
            fr.frame(i, S, flen);
            const int kind = reass_fragment(ByteLoad{S}, flen, max_reass_size, r, poff);
            if (kind == kReassIn) {
                addr = S + poff;
                len = r.len();
            } else if (kind == kReassEmpty || kind == kReassOversize) {
                o.verdict[i] = (uint8_t)AIPSTACK_RX_DROP_FRAG;
            }
            if (kind == kReassEmpty) r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0u;  // in no group
        }
        *reinterpret_cast<global_t<u32x4, 8> *>((uint64_t)(uintptr_t)recs + i * 16u) =
            u32x4{r.w[0], r.w[1], r.w[2], r.w[3]};
        index[i] = i;
        if (i + 1 == n) index[n] = n;
        o.chunk_addr[i] = addr;
        o.chunk_len[i] = len;
        o.next[i] = AIPSTACK_REASS_NONE;
        o.head[i] = AIPSTACK_REASS_NONE;
        put_dgram(o.dgram, i, 0u, 0u, 0u, 0u);
    }
}

// A record counts in a group if it holds a fragment at all: every record of a non-empty
// fragment has a nonzero length word.
__device__ __forceinline__ bool in_group(const ReassRec &r) { return r.len() != 0u; }

__global__ __launch_bounds__(kBlock) void ipreass_insert_kernel(
    uint64_t n, const ReassRec *__restrict__ recs, uint64_t slots, uint64_t *pairs,
    uint64_t *keys) {
    const WaveStride ws;
    const DeviceAtomics at;
    for (uint64_t base = uniform64(ws.first); base < n; base += ws.step) {
        const uint64_t i = base + ws.lane;
        if (i >= n) continue;
        const ReassRec me = recs[i];
        if (!in_group(me)) continue;
        reass_insert_key(at, keys, slots, recs, n, (uint32_t)i);
        if (me.member()) reass_insert_pair(at, pairs, slots, recs, n, (uint32_t)i);
    }
}

__global__ __launch_bounds__(kBlock) void ipreass_link_kernel(
    uint64_t n, const ReassRec *__restrict__ recs, uint64_t slots,
    const uint64_t *__restrict__ pairs, uint32_t *__restrict__ succ) {
    const WaveStride ws;
    for (uint64_t base = uniform64(ws.first); base < n; base += ws.step) {
        const uint64_t i = base + ws.lane;
        if (i >= n) continue;
        succ[i] = reass_successor(pairs, slots, recs, n, (uint32_t)i);
    }
}

__global__ __launch_bounds__(kBlock) void ipreass_finish_kernel(
    uint64_t n, const ReassRec *__restrict__ recs, uint64_t slots,
    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ succ,
    const uint16_t *__restrict__ sums, const Outputs o) {
    const WaveStride ws;
    for (uint64_t base = uniform64(ws.first); base < n; base += ws.step) {
        const uint64_t i = base + ws.lane;
        if (i >= n) continue;
        const ReassRec h = recs[i];
        if (!h.member() || h.off() != 0u || !h.mf()) continue;
        const uint32_t count = reass_key_count(keys, slots, recs, n, h);
        uint32_t last, data_len, sum;
        if (!reass_walk(recs, succ, sums, n, (uint32_t)i, count, last, data_len, sum)) continue;
        // (a head with MF in a complete group has a successor at its length: at least 8 bytes)
        const uint32_t p1 = h.len() >= 8u ? ByteLoad{o.chunk_addr[i]}(4u) : 0u;
        const uint32_t v = reass_dgram_verdict(h.proto(), h.w[0], h.w[1], data_len, sum, p1);
        put_dgram(o.dgram, i, count, last, data_len | h.proto() << 16 | v << 24, 0u);
        // the members: exactly `count` of them, as the walk found
        uint32_t cur = (uint32_t)i;
        for (uint32_t k = 0; k < count; ++k) {
            const uint32_t nx = k + 1u < count ? succ[cur] : AIPSTACK_REASS_NONE;
            o.verdict[cur] = (uint8_t)AIPSTACK_RX_FRAG_MEMBER;
            o.head[cur] = (uint32_t)i;
            o.next[cur] = nx;
            cur = nx;
        }
    }
}

template <class Frames>
int reassemble(const Frames &fr, uint64_t n, uint32_t max_reass_size, const Outputs &o,
               void *d_workspace, hipStream_t s) {
    unsigned blocks;
    int st = lane_pass_blocks(n, s, &blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const ReassWorkspace w = reass_workspace(n);
    char *ws = static_cast<char *>(d_workspace);
    uint64_t *index = reinterpret_cast<uint64_t *>(ws + w.index);
    ReassRec *recs = reinterpret_cast<ReassRec *>(ws + w.recs);
    uint32_t *succ = reinterpret_cast<uint32_t *>(ws + w.succ);
    uint16_t *sums = reinterpret_cast<uint16_t *>(ws + w.sums);
    uint64_t *pairs = reinterpret_cast<uint64_t *>(ws + w.pairs);
    uint64_t *keys = reinterpret_cast<uint64_t *>(ws + w.keys);
    hipLaunchKernelGGL(ipreass_classify_kernel<Frames>, dim3(blocks), dim3(kBlock), 0, s, fr, n,
                       max_reass_size, o, index, recs, pairs, 2u * w.slots);  // the tables are adjacent
    st = check_hip(hipGetLastError());
    if (st != AIPSTACK_CHKSUM_OK) return st;
    hipLaunchKernelGGL(ipreass_insert_kernel, dim3(blocks), dim3(kBlock), 0, s, n, recs, w.slots,
                       pairs, keys);
    st = check_hip(hipGetLastError());
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_batch_chain(o.chunk_addr, o.chunk_len, index, nullptr, n, sums, 0u, s);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    hipLaunchKernelGGL(ipreass_link_kernel, dim3(blocks), dim3(kBlock), 0, s, n, recs, w.slots,
                       pairs, succ);
    st = check_hip(hipGetLastError());
    if (st != AIPSTACK_CHKSUM_OK) return st;
    hipLaunchKernelGGL(ipreass_finish_kernel, dim3(blocks), dim3(kBlock), 0, s, n, recs, w.slots,
                       keys, succ, sums, o);
    return check_hip(hipGetLastError());
}

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_ip4_rx_reassemble(const void *d_base, const uint64_t *d_offsets, uint64_t n,
                                          uint32_t max_reass_size, uint8_t *d_verdict,
                                          uint64_t *d_chunk_addr, uint32_t *d_chunk_len,
                                          uint32_t *d_next, uint32_t *d_head,
                                          aipstack_ip4_dgram *d_dgram, void *d_workspace,
                                          uint64_t workspace_bytes, void *stream) {
    int st = ip4_rx_reassemble_check_args(d_base, d_offsets, false, 0, n, max_reass_size, d_verdict,
                                          d_chunk_addr, d_chunk_len, d_next, d_head, d_dgram,
                                          d_workspace, workspace_bytes);
    if (st != AIPSTACK_CHKSUM_OK || n == 0) return st;
    st = aipstack_chksum_rx_verify(d_base, d_offsets, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const CsrFrames fr{(uint64_t)(uintptr_t)d_base, d_offsets};
    const Outputs o{d_verdict, d_chunk_addr, d_chunk_len, d_next, d_head, (uint64_t)(uintptr_t)d_dgram};
    return reassemble(fr, n, max_reass_size, o, d_workspace, (hipStream_t)stream);
}

extern "C" int aipstack_ip4_rx_reassemble_slotted(const void *d_base, uint64_t slot_stride,
                                                  const uint32_t *d_len, uint64_t n,
                                                  uint32_t max_reass_size, uint8_t *d_verdict,
                                                  uint64_t *d_chunk_addr, uint32_t *d_chunk_len,
                                                  uint32_t *d_next, uint32_t *d_head,
                                                  aipstack_ip4_dgram *d_dgram, void *d_workspace,
                                                  uint64_t workspace_bytes, void *stream) {
    int st = ip4_rx_reassemble_check_args(d_base, d_len, true, slot_stride, n, max_reass_size,
                                          d_verdict, d_chunk_addr, d_chunk_len, d_next, d_head,
                                          d_dgram, d_workspace, workspace_bytes);
    if (st != AIPSTACK_CHKSUM_OK || n == 0) return st;
    st = aipstack_chksum_rx_verify_slotted(d_base, slot_stride, d_len, n, d_verdict, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint32_t cap = (uint32_t)(slot_stride < AIPSTACK_CHKSUM_MAX_LEN ? slot_stride
                                                                           : AIPSTACK_CHKSUM_MAX_LEN);
    const SlotFrames fr{(uint64_t)(uintptr_t)d_base, slot_stride, d_len, cap};
    const Outputs o{d_verdict, d_chunk_addr, d_chunk_len, d_next, d_head, (uint64_t)(uintptr_t)d_dgram};
    return reassemble(fr, n, max_reass_size, o, d_workspace, (hipStream_t)stream);
}
