// aipstack_amd -- UDP send with IPv4 fragmentation: the reference's UDP send
// (UdpApi::sendUdpIp4Packet -> IpStack::sendIp4Dgram -> send_fragmented; udp/IpUdpProto.h:152-184,
// ip/IpStack.h:373-464, 467-539) for a batch of datagrams. The host uploads one 80-byte
// descriptor per datagram (aipstack_udp_dgram: the header template Ip4CommonSendParams and
// UdpTxInfo give, and what changes per fragment as arithmetic); the GPU emits every fragment's
// header (42 bytes for the first, 34 for the others), the chunk table of its data, the IPv4
// header checksums and the UDP checksum. Three stream-ordered launches:
//   1. ipfrag_plan_kernel, three loops of one element per lane. Fragments: the datagram that
//      owns the fragment (upper bound in the running fragment counts, minus one: datagrams of no
//      fragment are stepped over), the datagram's contract, the fragment's index entry and the
//      IPv4 header checksum as arithmetic on header words, in one 8-byte record per fragment.
//      Chunk entries: the datagram that owns entry c (the same search in the running chunk
//      counts), the fragment and the piece it stands for, its address and length; an entry of a
//      datagram that breaks the contract, or of none, is written as length 0 at address 0. So
//      every one of the n_chunks entries is written by its own lane in every call, whatever the
//      two indices hold, and the chained batch never follows an address this call did not write.
//      Datagrams: the status, the seed of the UDP sum (pseudo-header and UDP header words) and
//      the chain's bound: chunk_base[d] clamped to n_chunks, the one thing the caller's index
//      lacks to be safe as a chain index.
//   2. the chained batch (aipstack_chksum_batch_chain), unchanged, with one chain per DATAGRAM:
//      a datagram's fragments partition its payload in order, so the chunks
//      [chunk_base[d], chunk_base[d+1]) are its chain; the seeds are its states. The 8 UDP header
//      bytes are an even count, so the payload starts at an even logical position: no swapped
//      seed (hsplit_kernels.hip has the odd case).
//   3. ipfrag_emit_kernel, one fragment per lane: the header from the template and the
//      per-fragment words, the checksums inserted (fragment 0 inverts the chain's sum; 0 is sent
//      as 0xFFFF), the slot stored whole. Slots are never loaded. A 64-byte ring on a 64-byte
//      boundary is stored in whole lines (store_wave_lines<4>); any other stride or alignment:
//      per-lane unaligned stores.
//
// Header words are summed as in tcpseg_kernels.hip: little-endian 16-bit halves of the template's
// dwords (every field lies at an even offset of the 8-byte aligned template), folded and
// byte-swapped once, then the per-fragment big-endian words added.
//
// tx_producer.h has what this file shares with tcpseg_kernels.hip: the owner search, an owner's
// ranges and contract, the record, the template loader and its sums, and the slot store. Here:
// what is UDP's own, and the chunk entries written each from its own lane.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"
#include "ipfrag_common.h"
#include "tx_producer.h"

namespace aipstack_amd {
namespace {

// The template's first 11 dwords (44 of its 48 bytes; the struct is 8-byte aligned and hdr lies
// at offset 32).
using Template = HeaderWords<11>;

// What changes per fragment (ip/IpStack.h:431-440, 497-509).
struct FragWords {
    uint32_t total_len, ident, flags_offset;
};

__device__ __forceinline__ FragWords uf_fragment(const aipstack_udp_dgram *__restrict__ g,
                                                 const Template &h, const UdpDgramShape &s,
                                                 const UdpFragRange &f, uint64_t k) {
    FragWords w;
    w.total_len = 20u + f.len;
    w.ident = g->ip_id;  // one Ident per datagram (m_next_id++ runs once, :434)
    // the template's word is 0 or DF (and 0 whenever S > 1)
    w.flags_offset = bswap16(h.t[5] & 0xFFFFu) | (k + 1u < s.S ? 0x2000u : 0u) | (f.off >> 3);
    return w;
}

// The IPv4 header checksum: what ip_header_checksum takes from the template, and total length,
// ident and flags/fragment offset per fragment. Fragment 0 as :425-453 accumulates it, the others
// as IpChksum over the 20 bytes (:510-515): the same sum.
__device__ __forceinline__ uint32_t uf_ip_checksum(const Template &h, const FragWords &w) {
    return ip_header_checksum(h, 0u, w.total_len + w.ident + w.flags_offset);
}

// The State the datagram's chain is resumed from (udp/IpUdpProto.h:163-174): the pseudo-header
// (addresses, protocol 17, P) and the 8 UDP header bytes (ports from the template, length P, the
// checksum field as 0). 10 words: far below 2^32.
__device__ __forceinline__ uint32_t uf_udp_seed(const Template &h, uint32_t P) {
    const uint32_t le = addr_halves(h) + (h.t[8] >> 16) + (h.t[9] & 0xFFFFu);
    return bswap16(fold16(le)) + 17u + P + P;
}

__device__ __forceinline__ void uf_put_chunk(uint64_t *__restrict__ chunk_addr,
                                             uint32_t *__restrict__ chunk_len, uint64_t c,
                                             uint64_t addr, uint32_t len) {
    __builtin_nontemporal_store(addr, &chunk_addr[c]);
    __builtin_nontemporal_store(len, &chunk_len[c]);
}

__global__ __launch_bounds__(kBlock) void ipfrag_plan_kernel(
    const aipstack_udp_dgram *__restrict__ dgrams, const uint64_t *__restrict__ frag_index,
    const uint64_t *__restrict__ chunk_base, uint64_t n_dgrams, uint64_t n_frags,
    uint64_t n_chunks, uint64_t *__restrict__ chunk_addr, uint32_t *__restrict__ chunk_len,
    uint64_t *__restrict__ chunk_index, uint64_t *__restrict__ records,
    uint64_t *__restrict__ chain_index, uint32_t *__restrict__ seeds,
    uint8_t *__restrict__ dgram_status) {
    const WaveStride ws;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        __builtin_nontemporal_store(n_chunks, &chunk_index[n_frags]);

    // Fragments: the index entry and the record of fragment i.
    for_each_owned(
        frag_index, n_dgrams, n_frags, ws,
        [&](uint64_t d, uint64_t i) {
            const aipstack_udp_dgram *__restrict__ g = dgrams + d;
            const OwnerRange r = owner_range(frag_index, chunk_base, d);
            const UdpDgramShape s = udp_dgram_shape(*g);
            const uint64_t k = i - r.eb;
            uint64_t rec = make_record(d, 0, false), ci;
            if (owner_ok(s.valid, s.S, s.C, r, n_frags, n_chunks)) {
                const Template h = load_header_words<11>(g->hdr);
                const FragWords w = uf_fragment(g, h, s, udp_frag_range(s, k), k);
                ci = r.cb + k + (k > s.straddle ? 1u : 0u);
                rec = make_record(d, uf_ip_checksum(h, w), true);
            } else {
                // its chunk entries are written empty; the fragments the index gives it share
                // them out in order, clipped to the table, so that the index stays in [0, n_chunks]
                uint64_t c0, cnt;
                clip_chunks(r, n_chunks, c0, cnt);
                ci = c0 + (k < cnt ? k : cnt);
            }
            __builtin_nontemporal_store(ci, &chunk_index[i]);
            __builtin_nontemporal_store(rec, &records[i]);
        },
        [&](uint64_t j, uint64_t i) {
            __builtin_nontemporal_store(j == 0 ? (uint64_t)0 : n_chunks, &chunk_index[i]);
            __builtin_nontemporal_store((uint64_t)0, &records[i]);
        });

    // Chunk entries: entry c is entry kc = c - chunk_base[d] of its datagram; fragment k's first
    // entry is k, plus 1 after the straddling fragment, whose two entries are its bytes of piece
    // 0 and of piece 1.
    for_each_owned(
        chunk_base, n_dgrams, n_chunks, ws,
        [&](uint64_t d, uint64_t c) {
            const aipstack_udp_dgram *__restrict__ g = dgrams + d;
            const OwnerRange r = owner_range(frag_index, chunk_base, d);
            const UdpDgramShape s = udp_dgram_shape(*g);
            uint64_t addr = 0;
            uint32_t len = 0;
            if (owner_ok(s.valid, s.S, s.C, r, n_frags, n_chunks)) {
                const uint64_t kc = c - r.cb;  // < C
                const uint64_t k = kc - (kc > s.straddle ? 1u : 0u);
                const UdpFragRange f = udp_frag_range(s, k);
                uint32_t a = f.a, b = f.b;
                if (k == s.straddle) {
                    if (kc == k) b = s.len0;
                    else a = s.len0;
                }
                addr = a < s.len0 ? g->data_addr[0] + a : g->data_addr[1] + (a - s.len0);
                len = b - a;
            }
            uf_put_chunk(chunk_addr, chunk_len, c, addr, len);
        },
        [&](uint64_t, uint64_t c) { uf_put_chunk(chunk_addr, chunk_len, c, 0, 0); });

    // Datagrams: status, seed and chain bound.
    for (uint64_t d = (uint64_t)blockIdx.x * kBlock + threadIdx.x; d < n_dgrams; d += ws.step) {
        const aipstack_udp_dgram *__restrict__ g = dgrams + d;
        const OwnerRange r = owner_range(frag_index, chunk_base, d);
        const UdpDgramShape s = udp_dgram_shape(*g);
        uint32_t seed = 0;
        uint8_t st = AIPSTACK_TX_DGRAM_INVALID;
        if (owner_ok(s.valid, s.S, s.C, r, n_frags, n_chunks)) {
            st = (uint8_t)(s.frag_needed ? AIPSTACK_TX_FRAG_NEEDED : AIPSTACK_RX_ACCEPT);
            seed = uf_udp_seed(load_header_words<11>(g->hdr), s.P);
        }
        dgram_status[d] = st;
        __builtin_nontemporal_store(seed, &seeds[d]);
        __builtin_nontemporal_store(r.cb < n_chunks ? r.cb : n_chunks, &chain_index[d]);
        if (d + 1 == n_dgrams)
            __builtin_nontemporal_store(r.ce < n_chunks ? r.ce : n_chunks, &chain_index[d + 1]);
    }
}

// Emit pass. LINES: ring_in_lines(hdr_base, hdr_stride).
template <bool LINES>
__global__ __launch_bounds__(kBlock) void ipfrag_emit_kernel(
    const aipstack_udp_dgram *__restrict__ dgrams, const uint64_t *__restrict__ frag_index,
    const uint64_t *__restrict__ records, const uint16_t *__restrict__ sums, uint64_t hdr_base,
    uint64_t hdr_stride, uint32_t *__restrict__ hdr_len, uint8_t *__restrict__ status,
    uint64_t n_frags) {
    __shared__ LineTiles<4, LINES> tile;
    const WaveStride ws;
    for (uint64_t base = uniform64(ws.first); base < n_frags; base += ws.step) {
        const uint64_t i = base + ws.lane;
        const bool active = i < n_frags;
        const uint64_t rec = active ? __builtin_nontemporal_load(&records[i]) : 0u;
        const bool valid = record_valid(rec);
        uint32_t hl = 0;
        uint32_t o[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) o[q] = 0u;
        if (valid) {
            const uint64_t d = record_owner(rec);
            const aipstack_udp_dgram *__restrict__ g = dgrams + d;
            const UdpDgramShape s = udp_dgram_shape(*g);
            const uint64_t k = i - frag_index[d];
            const Template h = load_header_words<11>(g->hdr);
            const FragWords w = uf_fragment(g, h, s, udp_frag_range(s, k), k);
            const uint32_t ipchk = record_ip_checksum(rec);
#pragma unroll
            for (int q = 0; q < 8; ++q) o[q] = h.t[q];
            o[4] = bswap16(w.total_len) | bswap16(w.ident) << 16;
            o[5] = bswap16(w.flags_offset) | (h.t[5] & 0xFFFF0000u);
            o[6] = bswap16(ipchk) | (h.t[6] & 0xFFFF0000u);
            o[8] = h.t[8] & 0xFFFFu;
            hl = AIPSTACK_UDP_NEXT_FRAGMENT_HEADER;
            if (k == 0u) {
                // the chain's sum (seed (+) payload, not inverted); a computed 0 goes out as
                // 0xFFFF (udp/IpUdpProto.h:176-178)
                uint32_t l4chk = ~(uint32_t)__builtin_nontemporal_load(&sums[d]) & 0xFFFFu;
                if (l4chk == 0u) l4chk = 0xFFFFu;
                o[8] = h.t[8];
                o[9] = (h.t[9] & 0xFFFFu) | bswap16(s.P) << 16;
                o[10] = bswap16(l4chk);
                hl = AIPSTACK_UDP_FIRST_FRAGMENT_HEADER;
            }
        }
        if (active) {
            status[i] = (uint8_t)(valid ? AIPSTACK_RX_ACCEPT : AIPSTACK_TX_DGRAM_INVALID);
            __builtin_nontemporal_store(hl, &hdr_len[i]);
        }
        store_header_slot<LINES, AIPSTACK_UDP_FIRST_FRAGMENT_HEADER,
                          AIPSTACK_UDP_NEXT_FRAGMENT_HEADER>(tile, ws, hdr_base, hdr_stride, base,
                                                             valid, hl, o);
    }
}

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_udp_tx_fragment(const aipstack_udp_dgram *d_dgrams,
                                        const uint64_t *d_frag_index, const uint64_t *d_chunk_base,
                                        uint64_t n_dgrams, uint64_t n_frags, uint64_t n_chunks,
                                        void *d_hdr, uint64_t hdr_stride, uint32_t *d_hdr_len,
                                        uint64_t *d_chunk_addr, uint32_t *d_chunk_len,
                                        uint64_t *d_chunk_index, uint8_t *d_status,
                                        uint8_t *d_dgram_status, void *d_workspace,
                                        uint64_t workspace_bytes, uint32_t flags, void *stream) {
    if (n_frags == 0) return AIPSTACK_CHKSUM_OK;
    int st = udp_tx_fragment_check_args(d_dgrams, d_frag_index, d_chunk_base, n_dgrams, n_frags,
                                        n_chunks, d_hdr, hdr_stride, d_hdr_len, d_chunk_addr,
                                        d_chunk_len, d_chunk_index, d_status, d_dgram_status,
                                        d_workspace, workspace_bytes);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const hipStream_t s = (hipStream_t)stream;
    uint64_t most = n_frags > n_chunks ? n_frags : n_chunks;
    if (n_dgrams > most) most = n_dgrams;
    unsigned plan_blocks, emit_blocks;
    st = lane_pass_blocks(most, s, &plan_blocks);
    if (st == AIPSTACK_CHKSUM_OK) st = lane_pass_blocks(n_frags, s, &emit_blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const UdpFragWorkspace w = udp_frag_workspace(n_dgrams, n_frags);
    char *ws = static_cast<char *>(d_workspace);
    uint64_t *records = reinterpret_cast<uint64_t *>(ws + w.records);
    uint64_t *chain_index = reinterpret_cast<uint64_t *>(ws + w.chain_index);
    uint32_t *seeds = reinterpret_cast<uint32_t *>(ws + w.seeds);
    uint16_t *sums = reinterpret_cast<uint16_t *>(ws + w.sums);
    hipLaunchKernelGGL(ipfrag_plan_kernel, dim3(plan_blocks), dim3(kBlock), 0, s, d_dgrams,
                       d_frag_index, d_chunk_base, n_dgrams, n_frags, n_chunks, d_chunk_addr,
                       d_chunk_len, d_chunk_index, records, chain_index, seeds, d_dgram_status);
    st = check_hip(hipGetLastError());
    if (st != AIPSTACK_CHKSUM_OK) return st;
    if (n_dgrams != 0) {
        st = aipstack_chksum_batch_chain(d_chunk_addr, d_chunk_len, chain_index, seeds, n_dgrams,
                                         sums, flags & AIPSTACK_CHKSUM_JUST_WRITTEN, stream);
        if (st != AIPSTACK_CHKSUM_OK) return st;
    }
    const uint64_t base = (uint64_t)(uintptr_t)d_hdr;
    const auto emit = ring_in_lines(base, hdr_stride) ? ipfrag_emit_kernel<true>
                                                      : ipfrag_emit_kernel<false>;
    hipLaunchKernelGGL(emit, dim3(emit_blocks), dim3(kBlock), 0, s, d_dgrams, d_frag_index, records,
                       sums, base, hdr_stride, d_hdr_len, d_status, n_frags);
    return check_hip(hipGetLastError());
}
