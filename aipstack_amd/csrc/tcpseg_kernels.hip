// aipstack_amd -- TCP burst segmentation: the reference's send loop for a burst of one
// connection's data (pcb_output_active -> pcb_output_segment -> PcbOutputHelper::sendSegment ->
// IpStack::sendIp4DgramFast; tcp/IpTcpProto_output.h:1056-1120, 1218-1335, ip/IpStack.h:564-663)
// for a batch of bursts. The host uploads one 96-byte descriptor per burst (aipstack_tcp_burst:
// the header template prepareCommon / prepareSendIp4Dgram leave, and what changes per segment
// as arithmetic); the GPU emits every segment's 54-byte header, the chunk table of its data and
// both checksums. Three stream-ordered launches:
//   1. tcpseg_plan_kernel, one segment per lane: the burst that owns the segment (upper bound
//      in the running segment counts, minus one: bursts of no segment are stepped over), the
//      burst's contract, the segment's chunk entries and index entry, the seed of the L4 sum
//      (pseudo-header, the template's TCP words, seq, offset/flags, tcp_len) and the IPv4 header
//      checksum, both as arithmetic on header words. Seeds (dense uint32) and one 8-byte record
//      per segment (owner burst, IPv4 checksum, valid) go to the workspace.
//   2. the chained batch (aipstack_chksum_batch_chain), unchanged, over the table just written
//      with the seeds as its states: seed (+) data, 16 bits per segment. The 20 TCP header bytes
//      are an even count, so the data always starts at an even logical position: no swapped
//      seed (hsplit_kernels.hip has the odd case).
//   3. tcpseg_emit_kernel, one segment per lane: the 54 bytes from the template and the
//      per-segment words, both checksums inserted, the slot stored whole. Slots are never
//      loaded. A 64-byte ring on a 64-byte boundary is stored in whole lines: the wave passes
//      its 64 slots through LDS so that each of its four 16-byte store instructions covers
//      1 KiB of contiguous memory. Any other stride or alignment: per-lane unaligned stores.
//
// Header words are summed as the repository does everywhere: little-endian 16-bit halves of the
// template's dwords (every field lies at an even offset of the 8-byte aligned template), folded
// and byte-swapped once, then the per-segment big-endian words added.
//
// tx_producer.h has what this file shares with ipfrag_kernels.hip: the owner search, an owner's
// ranges and contract, the record, the template loader and its sums, and the slot store. Here:
// what is TCP's own, and the chunk entries written from the segment lanes.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"
#include "tcpseg_common.h"
#include "tx_producer.h"

namespace aipstack_amd {
namespace {

// The template's 14 dwords (56 bytes; the struct is 8-byte aligned and hdr lies at offset 40).
using Template = HeaderWords<14>;

// What changes per segment (tcp/IpTcpProto_output.h:1069-1102, ip/IpStack.h:640-653).
struct SegWords {
    uint64_t start;
    uint32_t len, seq, offset_flags, total_len, ident;
};

__device__ __forceinline__ SegWords ts_segment(const aipstack_tcp_burst *__restrict__ d,
                                               const TcpBurstShape &s, uint64_t k) {
    SegWords w;
    const uint64_t mss = d->mss;
    w.start = k * mss;  // k < S <= 2^32, mss < 2^16
    const uint64_t rest = s.D - w.start;
    w.len = (uint32_t)(rest < mss ? rest : mss);
    w.seq = d->seq + (uint32_t)w.start;
    uint32_t fl = 0x5010u;  // Tcp4EncodeOffset(5) | Ack
    const uint64_t psh = d->psh_offset;
    if (psh > w.start && psh <= w.start + w.len) fl |= 0x08u;                       // Psh
    if ((d->flags & AIPSTACK_TCP_BURST_FIN) != 0u && k + 1 == s.S) fl |= 0x09u;  // Fin|Psh
    w.offset_flags = fl;
    w.total_len = 40u + w.len;
    w.ident = ((uint32_t)d->ip_id + (uint32_t)k) & 0xFFFFu;
    return w;
}

// The IPv4 header checksum: what ip_header_checksum takes from the template, its flags/fragment
// offset word, and total length and ident per segment.
__device__ __forceinline__ uint32_t ts_ip_checksum(const Template &h, const SegWords &w) {
    return ip_header_checksum(h, h.t[5] & 0xFFFFu, w.total_len + w.ident);
}

// The State the data chain is resumed from: the pseudo-header (addresses, protocol 6, tcp_len)
// and the 20 TCP header bytes (ports, ack, window, urgent pointer from the template; seq and
// offset/flags per segment; the checksum field as 0). At most 13 words: far below 2^32.
__device__ __forceinline__ uint32_t ts_l4_seed(const Template &h, const SegWords &w) {
    const uint32_t le = addr_halves(h) + (h.t[8] >> 16) + (h.t[9] & 0xFFFFu) + (h.t[10] >> 16) +
                        (h.t[11] & 0xFFFFu) + (h.t[12] & 0xFFFFu) + (h.t[13] & 0xFFFFu);
    return bswap16(fold16(le)) + 6u + (20u + w.len) + (w.seq >> 16) + (w.seq & 0xFFFFu) +
           w.offset_flags;
}

__device__ __forceinline__ void ts_put_chunk(uint64_t *__restrict__ chunk_addr,
                                             uint32_t *__restrict__ chunk_len, uint64_t c,
                                             uint64_t n_chunks, uint64_t addr, uint32_t len) {
    if (c < n_chunks) {  // (implied by owner_ok; the table is never left whatever happens)
        __builtin_nontemporal_store(addr, &chunk_addr[c]);
        __builtin_nontemporal_store(len, &chunk_len[c]);
    }
}

// Plan pass: segment i of the batch, owned by burst `b` (lane-varying or wave-uniform).
__device__ __forceinline__ void ts_plan_segment(
    const aipstack_tcp_burst *__restrict__ d, const OwnerRange &r, uint64_t b, uint64_t i,
    uint64_t n_segments, uint64_t n_chunks, uint64_t *__restrict__ chunk_addr,
    uint32_t *__restrict__ chunk_len, uint64_t *__restrict__ chunk_index,
    uint32_t *__restrict__ seeds, uint64_t *__restrict__ records) {
    const TcpBurstShape s = tcp_burst_shape(*d);
    const uint64_t k = i - r.eb;
    uint32_t seed = 0;
    uint64_t rec = make_record(b, 0, false), ci;
    if (owner_ok(s.valid, s.S, s.C, r, n_segments, n_chunks)) {
        const SegWords w = ts_segment(d, s, k);
        const Template h = load_header_words<14>(d->hdr);
        ci = r.cb + k + (k > s.straddle ? 1u : 0u);
        const uint64_t len0 = d->data_len[0];
        if (w.len != 0u) {
            if (w.start + w.len <= len0) {
                ts_put_chunk(chunk_addr, chunk_len, ci, n_chunks, d->data_addr[0] + w.start, w.len);
            } else if (w.start >= len0) {
                ts_put_chunk(chunk_addr, chunk_len, ci, n_chunks,
                             d->data_addr[1] + (w.start - len0), w.len);
            } else {  // the segment that straddles the piece boundary
                const uint32_t first = (uint32_t)(len0 - w.start);
                ts_put_chunk(chunk_addr, chunk_len, ci, n_chunks, d->data_addr[0] + w.start, first);
                ts_put_chunk(chunk_addr, chunk_len, ci + 1, n_chunks, d->data_addr[1],
                             w.len - first);
            }
        }
        seed = ts_l4_seed(h, w);
        rec = make_record(b, ts_ip_checksum(h, w), true);
    } else {
        // its chunk entries are emptied by the burst loop below; the segments share them out
        // in order so that the index stays non-decreasing
        uint64_t c0, cnt;
        clip_chunks(r, n_chunks, c0, cnt);
        ci = c0 + (k < cnt ? k : cnt);
    }
    __builtin_nontemporal_store(ci, &chunk_index[i]);
    __builtin_nontemporal_store(seed, &seeds[i]);
    __builtin_nontemporal_store(rec, &records[i]);
}

__global__ __launch_bounds__(kBlock) void tcpseg_plan_kernel(
    const aipstack_tcp_burst *__restrict__ bursts, const uint64_t *__restrict__ seg_index,
    const uint64_t *__restrict__ chunk_base, uint64_t n_bursts, uint64_t n_segments,
    uint64_t n_chunks, uint64_t *__restrict__ chunk_addr, uint32_t *__restrict__ chunk_len,
    uint64_t *__restrict__ chunk_index, uint32_t *__restrict__ seeds,
    uint64_t *__restrict__ records) {
    const WaveStride ws;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        __builtin_nontemporal_store(n_chunks, &chunk_index[n_segments]);
    for_each_owned(
        seg_index, n_bursts, n_segments, ws,
        [&](uint64_t b, uint64_t i) {
            ts_plan_segment(bursts + b, owner_range(seg_index, chunk_base, b), b, i, n_segments,
                            n_chunks, chunk_addr, chunk_len, chunk_index, seeds, records);
        },
        [&](uint64_t j, uint64_t i) {
            __builtin_nontemporal_store(j == 0 ? (uint64_t)0 : n_chunks, &chunk_index[i]);
            __builtin_nontemporal_store(0u, &seeds[i]);
            __builtin_nontemporal_store((uint64_t)0, &records[i]);
        });
    // Bursts that break the contract: their chunk entries are emptied (length 0 at address 0),
    // whether or not the index gives them a segment.
    for (uint64_t b = (uint64_t)blockIdx.x * kBlock + threadIdx.x; b < n_bursts; b += ws.step) {
        const OwnerRange r = owner_range(seg_index, chunk_base, b);
        const TcpBurstShape s = tcp_burst_shape(bursts[b]);
        if (owner_ok(s.valid, s.S, s.C, r, n_segments, n_chunks)) continue;
        uint64_t c0, cnt;
        clip_chunks(r, n_chunks, c0, cnt);
        for (uint64_t c = c0; c < c0 + cnt; ++c) ts_put_chunk(chunk_addr, chunk_len, c, n_chunks, 0, 0);
    }
}

// Emit pass. LINES: ring_in_lines(hdr_base, hdr_stride).
template <bool LINES>
__global__ __launch_bounds__(kBlock) void tcpseg_emit_kernel(
    const aipstack_tcp_burst *__restrict__ bursts, const uint64_t *__restrict__ seg_index,
    const uint64_t *__restrict__ records, const uint16_t *__restrict__ sums, uint64_t hdr_base,
    uint64_t hdr_stride, uint8_t *__restrict__ status, uint64_t n_segments) {
    __shared__ LineTiles<4, LINES> tile;
    const WaveStride ws;
    for (uint64_t base = uniform64(ws.first); base < n_segments; base += ws.step) {
        const uint64_t i = base + ws.lane;
        const bool active = i < n_segments;
        const uint64_t rec = active ? __builtin_nontemporal_load(&records[i]) : 0u;
        const bool valid = record_valid(rec);
        uint32_t o[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) o[q] = 0u;
        if (valid) {
            const uint64_t b = record_owner(rec);
            const aipstack_tcp_burst *__restrict__ d = bursts + b;
            const TcpBurstShape s = tcp_burst_shape(*d);
            const SegWords w = ts_segment(d, s, i - seg_index[b]);
            const Template h = load_header_words<14>(d->hdr);
            const uint32_t ipchk = record_ip_checksum(rec);
            // the chain's sum (seed (+) data, not inverted); a TCP checksum of 0 stays 0
            const uint32_t l4chk = ~(uint32_t)__builtin_nontemporal_load(&sums[i]) & 0xFFFFu;
#pragma unroll
            for (int q = 0; q < 14; ++q) o[q] = h.t[q];
            o[4] = bswap16(w.total_len) | bswap16(w.ident) << 16;
            o[6] = bswap16(ipchk) | (h.t[6] & 0xFFFF0000u);
            o[9] = (h.t[9] & 0xFFFFu) | bswap16(w.seq >> 16) << 16;
            o[10] = bswap16(w.seq & 0xFFFFu) | (h.t[10] & 0xFFFF0000u);
            o[11] = (h.t[11] & 0xFFFFu) | bswap16(w.offset_flags) << 16;
            o[12] = (h.t[12] & 0xFFFFu) | bswap16(l4chk) << 16;
            o[13] = h.t[13] & 0xFFFFu;
        }
        if (active)
            status[i] = (uint8_t)(valid ? AIPSTACK_RX_ACCEPT : AIPSTACK_TX_BURST_INVALID);
        store_header_slot<LINES, AIPSTACK_TCP_SEGMENT_HEADER>(tile, ws, hdr_base, hdr_stride, base,
                                                              valid, AIPSTACK_TCP_SEGMENT_HEADER, o);
    }
}

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_tcp_tx_segment(const aipstack_tcp_burst *d_bursts,
                                       const uint64_t *d_seg_index, const uint64_t *d_chunk_base,
                                       uint64_t n_bursts, uint64_t n_segments, uint64_t n_chunks,
                                       void *d_hdr, uint64_t hdr_stride, uint64_t *d_chunk_addr,
                                       uint32_t *d_chunk_len, uint64_t *d_chunk_index,
                                       uint8_t *d_status, void *d_workspace,
                                       uint64_t workspace_bytes, uint32_t flags, void *stream) {
    if (n_segments == 0) return AIPSTACK_CHKSUM_OK;
    int st = tcp_tx_segment_check_args(d_bursts, d_seg_index, d_chunk_base, n_bursts, n_segments,
                                       n_chunks, d_hdr, hdr_stride, d_chunk_addr, d_chunk_len,
                                       d_chunk_index, d_status, d_workspace, workspace_bytes);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const hipStream_t s = (hipStream_t)stream;
    const uint64_t n = n_segments;
    unsigned blocks;
    st = lane_pass_blocks(n, s, &blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    uint64_t *records = static_cast<uint64_t *>(d_workspace);
    uint32_t *seeds = reinterpret_cast<uint32_t *>(records + n);
    uint16_t *sums = reinterpret_cast<uint16_t *>(seeds + n);
    hipLaunchKernelGGL(tcpseg_plan_kernel, dim3(blocks), dim3(kBlock), 0, s, d_bursts,
                       d_seg_index, d_chunk_base, n_bursts, n, n_chunks, d_chunk_addr, d_chunk_len,
                       d_chunk_index, seeds, records);
    st = check_hip(hipGetLastError());
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_batch_chain(d_chunk_addr, d_chunk_len, d_chunk_index, seeds, n, sums,
                                     flags & AIPSTACK_CHKSUM_JUST_WRITTEN, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const uint64_t base = (uint64_t)(uintptr_t)d_hdr;
    const auto emit = ring_in_lines(base, hdr_stride) ? tcpseg_emit_kernel<true>
                                                      : tcpseg_emit_kernel<false>;
    hipLaunchKernelGGL(emit, dim3(blocks), dim3(kBlock), 0, s, d_bursts, d_seg_index, records, sums,
                       base, hdr_stride, d_status, n);
    return check_hip(hipGetLastError());
}
