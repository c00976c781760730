// aipstack_amd -- TCP Rx parse: what the host code (tcprx_host.cpp) and the kernel
// (tcprx_kernels.hip) share, so that the table is sorted and searched with the same comparison,
// and a frame's record is built from the same text wherever its bytes are read from.
#ifndef AIPSTACK_AMD_TCPRX_COMMON_H
#define AIPSTACK_AMD_TCPRX_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"

#if defined(__HIPCC__)
#define AIPSTACK_TCPRX_HD __host__ __device__ inline
#else
#define AIPSTACK_TCPRX_HD inline
#endif

namespace aipstack_amd {

constexpr uint64_t kTcpRxMaxCount = 1ull << 40;  // frames, table entries of one call

// TcpPcbKeyCompare::CompareKeys (tcp/TcpPcbKey.h:52-86): remote_port, remote_addr, local_port,
// local_addr, each ascending; -1, 0 or +1. The cookie takes no part.
AIPSTACK_TCPRX_HD int tcp_pcb_key_compare(const aipstack_tcp_pcb_key &a,
                                          const aipstack_tcp_pcb_key &b) {
    const uint64_t ar = (uint64_t)a.remote_port << 32 | a.remote_addr;
    const uint64_t br = (uint64_t)b.remote_port << 32 | b.remote_addr;
    if (ar != br) return ar < br ? -1 : 1;
    const uint64_t al = (uint64_t)a.local_port << 32 | a.local_addr;
    const uint64_t bl = (uint64_t)b.local_port << 32 | b.local_addr;
    if (al != bl) return al < bl ? -1 : 1;
    return 0;
}

// ParseTcpOptions (tcp/TcpOptions.h:63-125) as a machine that takes one byte at a time, so that
// the caller can feed it the bytes of fixed dwords (no array indexed by a run-time position).
// `left` = option bytes after the one given. Results: opts (TcpOptionFlags), mss, wnd_scale.
struct TcpOptParser {
    uint32_t opts = 0, mss = 0, wnd_scale = 0;
    uint32_t phase = 0;  // 0 kind, 1 length, 2 data, 3 stopped
    uint32_t kind = 0, dlen = 0, rest = 0, acc = 0;

    AIPSTACK_TCPRX_HD bool live() const { return phase != 3u; }

    AIPSTACK_TCPRX_HD void byte(uint32_t b, uint32_t left) {
        if (phase == 0u) {
            if (b == 0u) phase = 3u;        // End (:73)
            else if (b != 1u) {             // Nop is skipped (:76)
                kind = b;
                phase = 1u;                 // (no length byte left: the bytes run out, :81)
            }
        } else if (phase == 1u) {
            // length below 2, or option data beyond the bytes left: stop (:87-93)
            if (b < 2u || left < b - 2u) phase = 3u;
            else {
                dlen = rest = b - 2u;
                acc = 0u;
                phase = rest != 0u ? 2u : 0u;
            }
        } else if (phase == 2u) {
            acc = acc << 8 | b;
            if (--rest == 0u) {
                // MSS with 2 data bytes, window scale with 1; any other length, or any other
                // kind, is skipped (:98-122)
                if (kind == 2u && dlen == 2u) {
                    opts |= AIPSTACK_TCP_OPT_MSS;
                    mss = acc & 0xFFFFu;
                } else if (kind == 3u && dlen == 1u) {
                    opts |= AIPSTACK_TCP_OPT_WND_SCALE;
                    wnd_scale = acc & 0xFFu;
                }
                phase = 0u;
            }
        }
    }

    // bytes pos .. pos+3 of the n option bytes, little-endian in w
    AIPSTACK_TCPRX_HD void dword(uint32_t w, uint32_t pos, uint32_t n) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < 4u; ++k)
            if (pos + k < n && live()) byte((w >> (8u * k)) & 0xFFu, n - (pos + k) - 1u);
    }
};

// The record of one frame that Rx verify accepted (AIPSTACK_RX_ACCEPT), of `len` bytes, read
// through `ld(off)` = the little-endian dword at frame bytes [off, off + 4), which is only
// called for bytes inside the frame. Returns 0: not TCP (the record stays zero, the verdict as
// it is); 1: a valid record; 2: the data offset is outside [20, datagram length]
// (tcp/IpTcpProto_input.h:108-116): AIPSTACK_RX_DROP_TCP_OFFSET, the record stays zero.
// w[8]: the record as dwords (aipstack_tcp_rx_seg, host byte order); key: the lookup tuple.
constexpr int kTcpRxNotTcp = 0, kTcpRxValid = 1, kTcpRxBadOffset = 2;

AIPSTACK_TCPRX_HD uint32_t tcprx_bswap32(uint32_t x) {
    return x >> 24 | (x >> 8 & 0xFF00u) | (x << 8 & 0xFF0000u) | x << 24;
}
AIPSTACK_TCPRX_HD uint32_t tcprx_be16lo(uint32_t w) {  // the big-endian 16 bits in w's bytes 0-1
    return (w & 0xFFu) << 8 | (w >> 8 & 0xFFu);
}

template <class Load>
AIPSTACK_TCPRX_HD int tcp_rx_build(const Load &ld, uint32_t len, uint32_t w[8],
                                   aipstack_tcp_pcb_key &key) {
    if (len < 14u + 20u + 20u) return kTcpRxNotTcp;
    const uint32_t v = ld(14u);                       // version/IHL, DSCP, total length
    const uint32_t hl = (v & 0xFu) * 4u;
    const uint32_t total = tcprx_be16lo(v >> 16);
    if ((ld(20u) >> 24) != 6u) return kTcpRxNotTcp;   // protocol (frame byte 23)
    // what Rx verify has checked of an accepted frame (ip/IpStack.h:938-990,
    // IpTcpProto_input.h:77), restated so that every read below lies inside the frame
    if (hl < 20u || total < hl + 20u || 14u + total > len) return kTcpRxNotTcp;
    const uint32_t dgram = total - hl;                // dgram.tot_len
    const uint32_t T = 14u + hl;                      // the TCP header
    const uint32_t fw = ld(T + 12u);                  // OffsetFlags, WindowSize
    const uint32_t flags = tcprx_be16lo(fw);
    const uint32_t doff = (flags >> 12) * 4u;
    if (doff < 20u || doff > dgram) return kTcpRxBadOffset;
    const uint32_t ports = ld(T);
    key.remote_addr = tcprx_bswap32(ld(26u));
    key.local_addr = tcprx_bswap32(ld(30u));
    key.remote_port = (uint16_t)tcprx_be16lo(ports);
    key.local_port = (uint16_t)tcprx_be16lo(ports >> 16);
    key.cookie = 0u;
    // the options: 4*offset - 20 bytes, at most 40, as ten fixed dwords
    const uint32_t nopt = doff - 20u;
    uint32_t o[10];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t q = 0; q < 10u; ++q) o[q] = 4u * q < nopt ? ld(T + 20u + 4u * q) : 0u;
    TcpOptParser p;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t q = 0; q < 10u; ++q)
        if (4u * q < nopt && p.live()) p.dword(o[q], 4u * q, nopt);
    w[0] = key.remote_addr;
    w[1] = key.local_addr;
    w[2] = (uint32_t)key.remote_port | (uint32_t)key.local_port << 16;
    w[3] = tcprx_bswap32(ld(T + 4u));
    w[4] = tcprx_bswap32(ld(T + 8u));
    w[5] = flags | tcprx_be16lo(fw >> 16) << 16;
    w[6] = (T + doff) | (dgram - doff) << 16;
    w[7] = p.mss | p.wnd_scale << 16 | (p.opts | AIPSTACK_TCP_SEG_VALID) << 24;
    return kTcpRxValid;
}

// The argument checks of aipstack_tcp_rx_parse / _slotted (tcprx_host.cpp; no HIP call).
// frames: d_offsets or d_len; slot_stride is checked when `slotted`.
int tcp_rx_parse_check_args(const void *d_base, const void *frames, bool slotted,
                            uint64_t slot_stride, uint64_t n, const void *d_pcbs, uint64_t n_pcbs,
                            const void *d_verdict, const void *d_segs, const void *d_pcb);

}  // namespace aipstack_amd

#endif
