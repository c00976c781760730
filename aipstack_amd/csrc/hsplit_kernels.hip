// aipstack_amd -- Tx fill for header-split segments: the send side as the reference builds it,
// a header node in its own buffer followed by chunks of the send ring
// (tcp/IpTcpProto_output.h:1251-1277, udp/IpUdpProto.h:164-179, ip/IpStack.h:632-663).
//
// Segment i is one Ethernet frame in two parts: its first hdr_len[i] bytes in slot i of a dense
// header ring (d_hdr + i * hdr_stride), the rest in the chunks [index[i], index[i+1]) of a chunk
// table (as aipstack_chksum_batch_chain). Three stream-ordered launches:
//   1. hsplit_header_kernel, one segment per lane: the checks of parse_ip4 and the L4 entry
//      checks (frame_kernels.hip parse_lane, oracle/frame_oracle.c), the IPv4 header checksum
//      with its field taken as 0, and the seed of the L4 sum: the pseudo-header words plus the
//      L4 bytes that lie in the slot, the checksum field taken as 0. Seeds (dense uint32) and
//      one 4-byte record per segment go to the workspace.
//   2. the chained batch (aipstack_chksum_batch_chain), unchanged, over the caller's chunk
//      table with the seeds as its states: seed (+) payload, 16 bits per segment.
//   3. hsplit_finish_kernel, one segment per lane: invert, UDP 0 -> 0xFFFF, the two fields
//      stored into the header slot with nontemporal 2-byte stores (as the chain fill's field
//      scatter, chksum_kernels.hip), and the status byte.
//
// Odd split: when an odd number of L4 bytes lies in the slot, the payload starts at an odd
// logical position. With (+) the ones'-complement sum, swap(a (+) b) = swap(a) (+) swap(b): the
// chain kernel gets the byte-swapped seed (folded to 16 bits first; folding keeps zero-ness:
// a nonzero sum never folds to 0x0000) and the finish pass swaps its result back.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"
#include "lane_pass.h"

namespace aipstack_amd {
namespace {

constexpr uint32_t kMaxSplitHeader = AIPSTACK_CHKSUM_MAX_SPLIT_HEADER;

// The record of segment i (workspace, 4 bytes): bits 0-15 the IPv4 header checksum, 16-23 the
// L4 field's offset in the slot (at most 14 + 60 + 16), 24 = write the IPv4 field (slot byte
// 24), 25 = write the L4 field, 26 = UDP (0 is sent as 0xFFFF), 27 = the chain sum comes back
// byte-swapped (odd split), 28-31 the status.
constexpr uint32_t kRecIp = 1u << 24, kRecL4 = 1u << 25, kRecUdp = 1u << 26, kRecSwap = 1u << 27;

// Mask of the bytes [lo, hi) of a dword (byte 0 = bits 0-7), clipped to the dword.
__device__ __forceinline__ uint32_t hs_keep(int lo, int hi) {
    lo = lo < 0 ? 0 : lo;
    hi = hi > 4 ? 4 : hi;
    if (hi <= lo) return 0u;
    const uint32_t below_hi = hi >= 4 ? ~0u : ((1u << (8 * hi)) - 1u);
    return below_hi & ~((1u << (8 * lo)) - 1u);  // lo < hi <= 4
}

__device__ __forceinline__ uint32_t hs_be16(uint32_t le_dword, int byte) {  // byte 0 or 2
    return bswap16(le_dword >> (8 * byte));
}

// Sum of a big-endian byte sequence from a halves-sum (little-endian 16-bit halves at even
// ABSOLUTE addresses) of its bytes: the halves are the byte-swapped words when the sequence
// starts at an even address, the words themselves when it starts at an odd one.
__device__ __forceinline__ uint32_t hs_orient(uint32_t halves_sum, uint32_t start_abs) {
    const uint32_t f = fold16(halves_sum);
    return (start_abs & 1u) ? f : bswap16(f);
}

// The two sums of one aligned 16-byte segment whose byte 0 is slot byte `pos` (may be
// negative): the IPv4 header bytes [14, ip_end) without the checksum field [24, 26), and the
// in-slot L4 bytes [dg, l4_end) without the field [fld, fld + 2).
__device__ __forceinline__ void hs_add_segment(const u32x4 &v, int pos, int ip_end, int dg,
                                               int l4_end, int fld, uint32_t &ip_sum,
                                               uint32_t &l4_sum) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int p = pos + 4 * d;
        const uint32_t mi = hs_keep(14 - p, ip_end - p) & ~hs_keep(24 - p, 26 - p);
        const uint32_t ml = hs_keep(dg - p, l4_end - p) & ~hs_keep(fld - p, fld + 2 - p);
        const uint32_t a = v[d] & mi, b = v[d] & ml;
        ip_sum += (a & 0xFFFFu) + (a >> 16);  // at most 68 dwords: < 2^24
        l4_sum += (b & 0xFFFFu) + (b >> 16);
    }
}

// Header pass. The staged layout rule (chksum.h): every byte the linear fill would parse or
// write lies in the slot, else AIPSTACK_TX_SPLIT_LAYOUT; the verdicts of the linear fill that
// need fewer bytes than a stage asks for come first, as it gives them.
__global__ __launch_bounds__(kBlock) void hsplit_header_kernel(
    uint64_t hdr_base, uint64_t hdr_stride, const uint32_t *__restrict__ hdr_len,
    const uint32_t *__restrict__ chunk_len, const uint64_t *__restrict__ chunk_index, uint64_t n,
    uint32_t *__restrict__ seeds, uint32_t *__restrict__ records) {
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    const uint32_t cap = (uint32_t)(hdr_stride < kMaxSplitHeader ? hdr_stride : kMaxSplitHeader);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
        const uint64_t P = hdr_base + i * hdr_stride;
        const uint32_t H = hdr_len[i];
        // payload bytes: the segment's chunk lengths (usually one or two)
        uint64_t pay = 0;
        for (uint64_t k = chunk_index[i], ke = chunk_index[i + 1]; k < ke; ++k) pay += chunk_len[k];
        uint32_t seed = 0, rec = 0;
        int status = AIPSTACK_TX_SPLIT_LAYOUT;
        if (H <= cap) {
            const uint64_t L = (uint64_t)H + pay;
            // the aligned 16-byte segments holding slot bytes [0, H): the first four go out now
            const uint32_t rs = (uint32_t)P & 15u;
            const uint64_t A0 = P & ~(uint64_t)15;
            const uint32_t nseg = H ? (rs + H + 15u) >> 4 : 0u;  // at most 17
            u32x4 pre[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                pre[k] = (uint32_t)k < nseg ? reinterpret_cast<global_t<const u32x4> *>(A0)[k]
                                            : u32x4{0u, 0u, 0u, 0u};
            // the fixed fields, from the slot at any alignment (the bytes are in the slot:
            // H >= 14 for the EtherType, H >= 34 for the IPv4 header's first 20 bytes)
            const uint32_t ethertype =
                H >= 14u ? bswap16(*reinterpret_cast<global_t<const uint16_t, 1> *>(P + 12)) : 0u;
            u32x4 ip = {0u, 0u, 0u, 0u};
            uint32_t ip4 = 0;
            if (H >= 34u) {
                ip = *reinterpret_cast<global_t<const u32x4, 1> *>(P + 14);
                ip4 = *reinterpret_cast<global_t<const uint32_t, 1> *>(P + 30);
            }
            const uint32_t vihl = ip[0] & 0xFFu;
            const int hl = vihl == 0x45u ? 20 : (int)(vihl & 0xFu) * 4;
            const int total_len = (int)hs_be16(ip[0], 2);
            const uint64_t plen = L - 14u;  // used only when L >= 14
            if (L < 14u) {
                status = AIPSTACK_RX_NOT_IP4;
            } else if (H < 14u) {
                status = AIPSTACK_TX_SPLIT_LAYOUT;
            } else if (ethertype != 0x0800u) {
                status = AIPSTACK_RX_NOT_IP4;
            } else if (plen < 20u) {
                status = AIPSTACK_RX_DROP_IP_MALFORMED;
            } else if (H < 34u) {
                status = AIPSTACK_TX_SPLIT_LAYOUT;
            } else if ((vihl >> 4) != 4u || hl < 20 || (uint64_t)hl > plen || total_len < hl ||
                       (uint64_t)total_len > plen) {
                status = AIPSTACK_RX_DROP_IP_MALFORMED;
            } else if (H < 14u + (uint32_t)hl) {
                status = AIPSTACK_TX_SPLIT_LAYOUT;
            } else {
                // the IPv4 header is good and in the slot: its checksum is written unless the
                // L4 stage finds the layout wanting
                const uint32_t flags_off = hs_be16(ip[1], 2);
                const uint32_t proto = (ip[2] >> 8) & 0xFFu;
                const uint32_t src = __builtin_bswap32(ip[3]), dst = __builtin_bswap32(ip4);
                const uint32_t pseudo =
                    (src >> 16) + (src & 0xFFFFu) + (dst >> 16) + (dst & 0xFFFFu);
                const int dg = 14 + hl;
                const int dlen = total_len - hl;
                int l4len = -1, fo = 0, fixed = 0;
                uint32_t words = 0;
                bool udp = false;
                status = AIPSTACK_RX_ACCEPT_OTHER;
                if ((flags_off & 0x3FFFu) != 0) {
                    status = AIPSTACK_RX_FRAGMENT;
                } else if (proto == 6u) {
                    if (dlen < 20) status = AIPSTACK_RX_DROP_L4_MALFORMED;
                    else { fixed = 20; fo = 16; l4len = dlen; words = pseudo + 6u + (uint32_t)dlen; }
                } else if (proto == 17u) {
                    if (dlen < 8) status = AIPSTACK_RX_DROP_L4_MALFORMED;
                    else { fixed = 8; fo = 6; udp = true; }
                } else if (proto == 1u) {
                    if (dlen < 8) status = AIPSTACK_RX_DROP_L4_MALFORMED;
                    else { fixed = 8; fo = 2; l4len = dlen; }
                }
                bool layout_ok = true;
                if (fixed) {
                    if (H < (uint32_t)(dg + fixed)) {
                        layout_ok = false;
                    } else if (udp) {
                        const int ulen = (int)bswap16(
                            *reinterpret_cast<global_t<const uint16_t, 1> *>(P + (uint64_t)dg + 4));
                        if (ulen < 8 || ulen > dlen) {
                            status = AIPSTACK_RX_DROP_L4_MALFORMED;
                            fixed = 0;
                        } else {
                            l4len = ulen;
                            words = pseudo + 17u + (uint32_t)ulen;
                        }
                    }
                }
                const bool l4 = layout_ok && fixed != 0;
                // the bytes the L4 checksum covers end exactly where the segment does
                if (l4 && (uint64_t)(dg + l4len) != L) layout_ok = false;
                if (!layout_ok) {
                    status = AIPSTACK_TX_SPLIT_LAYOUT;
                } else {
                    if (l4) status = AIPSTACK_RX_ACCEPT;
                    const int fld = l4 ? dg + fo : -8;
                    const int l4_end = l4 ? (int)H : dg;
                    uint32_t ip_sum = 0, l4_sum = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        hs_add_segment(pre[k], 16 * k - (int)rs, dg, dg, l4_end, fld, ip_sum, l4_sum);
                    for (uint32_t k = 4; k < nseg; ++k) {
                        const u32x4 v = reinterpret_cast<global_t<const u32x4> *>(A0)[k];
                        hs_add_segment(v, 16 * (int)k - (int)rs, dg, dg, l4_end, fld, ip_sum, l4_sum);
                    }
                    const uint32_t hchk = ~hs_orient(ip_sum, rs + 14u) & 0xFFFFu;
                    rec = hchk | kRecIp;
                    if (l4) {
                        seed = words + hs_orient(l4_sum, rs + (uint32_t)dg);
                        rec |= (uint32_t)fld << 16 | kRecL4 | (udp ? kRecUdp : 0u);
                        if ((H - (uint32_t)dg) & 1u) {
                            seed = bswap16(fold16(seed));
                            rec |= kRecSwap;
                        }
                    }
                }
            }
        }
        __builtin_nontemporal_store(seed, &seeds[i]);
        __builtin_nontemporal_store(rec | (uint32_t)status << 28, &records[i]);
    }
}

// Finish pass: the chain kernel's sums (seed (+) payload, not inverted) become the field
// values; fields and statuses stored. Rejected segments' sums are discarded.
__global__ __launch_bounds__(kBlock) void hsplit_finish_kernel(
    uint64_t hdr_base, uint64_t hdr_stride, const uint32_t *__restrict__ records,
    const uint16_t *__restrict__ sums, uint8_t *__restrict__ status, uint64_t n) {
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
        const uint32_t rec = __builtin_nontemporal_load(&records[i]);
        const uint64_t P = hdr_base + i * hdr_stride;
        status[i] = (uint8_t)(rec >> 28);
        if (rec & kRecIp)
            __builtin_nontemporal_store((uint16_t)bswap16(rec & 0xFFFFu),
                                        reinterpret_cast<global_t<uint16_t, 1> *>(P + 24));
        if (rec & kRecL4) {
            uint32_t r = __builtin_nontemporal_load(&sums[i]);
            if (rec & kRecSwap) r = bswap16(r);
            uint32_t chk = ~r & 0xFFFFu;
            if ((rec & kRecUdp) && chk == 0) chk = 0xFFFFu;  // udp/IpUdpProto.h:176-178
            __builtin_nontemporal_store((uint16_t)bswap16(chk),
                                        reinterpret_cast<global_t<uint16_t, 1> *>(P + ((rec >> 16) & 0xFFu)));
        }
    }
}

// Workspace layout for n segments: seeds (4n bytes), records (4n), chain sums (2n).
constexpr uint64_t kMaxSegments = 1ull << 40;

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" uint64_t aipstack_chksum_tx_fill_hsplit_workspace_bytes(uint64_t n) {
    if (n > kMaxSegments) n = kMaxSegments;
    return (10u * n + 7u) & ~(uint64_t)7;
}

extern "C" int aipstack_chksum_tx_fill_hsplit(void *d_hdr, uint64_t hdr_stride,
                                              const uint32_t *d_hdr_len,
                                              const uint64_t *d_chunk_addr,
                                              const uint32_t *d_chunk_len,
                                              const uint64_t *d_chunk_index, uint64_t n,
                                              uint8_t *d_status, void *d_workspace,
                                              uint64_t workspace_bytes, uint32_t flags,
                                              void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    if (!d_hdr || !d_hdr_len || !d_chunk_addr || !d_chunk_len || !d_chunk_index || !d_status ||
        !d_workspace)
        return AIPSTACK_CHKSUM_EINVAL;
    if (hdr_stride == 0 || n > kMaxSegments) return AIPSTACK_CHKSUM_EINVAL;
    if (workspace_bytes < aipstack_chksum_tx_fill_hsplit_workspace_bytes(n) ||
        ((uintptr_t)d_workspace & 7u) != 0)
        return AIPSTACK_CHKSUM_EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    unsigned blocks;
    int st = lane_pass_blocks(n, s, &blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    uint32_t *seeds = static_cast<uint32_t *>(d_workspace);
    uint32_t *records = seeds + n;
    uint16_t *sums = reinterpret_cast<uint16_t *>(records + n);
    const uint64_t base = (uint64_t)(uintptr_t)d_hdr;
    hipLaunchKernelGGL(hsplit_header_kernel, dim3(blocks), dim3(kBlock), 0, s, base, hdr_stride,
                       d_hdr_len, d_chunk_len, d_chunk_index, n, seeds, records);
    st = check_hip(hipGetLastError());
    if (st != AIPSTACK_CHKSUM_OK) return st;
    st = aipstack_chksum_batch_chain(d_chunk_addr, d_chunk_len, d_chunk_index, seeds, n, sums,
                                     flags & AIPSTACK_CHKSUM_JUST_WRITTEN, stream);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    hipLaunchKernelGGL(hsplit_finish_kernel, dim3(blocks), dim3(kBlock), 0, s, base, hdr_stride,
                       records, sums, d_status, n);
    return check_hip(hipGetLastError());
}
