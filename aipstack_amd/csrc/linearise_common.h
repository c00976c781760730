// aipstack_amd -- linearising header-split Tx segments: what the kernels
// (linearise_kernels.hip), the host checks (linearise_host.cpp) and the serial host test
// (tests/cpp/linearise_plan_test.cpp) share, so that all three decide a segment's outcome and
// length, and find the piece that holds a frame byte, with the same text.
#ifndef AIPSTACK_AMD_LINEARISE_COMMON_H
#define AIPSTACK_AMD_LINEARISE_COMMON_H

#include <cstdint>

#include "aipstack_amd/chksum.h"

#if defined(__HIPCC__)
#define AIPSTACK_LIN_HD __host__ __device__ inline
#else
#define AIPSTACK_LIN_HD inline
#endif

namespace aipstack_amd {

constexpr uint64_t kLinMaxSegments = 1ull << 40;
constexpr uint32_t kLinMinFrame = 14;        // the Ethernet header (sendFrame's HardwareError)
constexpr uint32_t kLinNoSegStatus = 0x100;  // "no d_seg_status": no status byte has this value
constexpr uint64_t kLinNoRoom = ~0ull;       // "no room to compare with": the slotted form

// Largest header length a segment may have in a ring of `hdr_stride`-byte slots.
AIPSTACK_LIN_HD uint32_t lin_header_cap(uint64_t hdr_stride) {
    return (uint32_t)(hdr_stride < AIPSTACK_CHKSUM_MAX_SPLIT_HEADER ? hdr_stride
                                                                   : AIPSTACK_CHKSUM_MAX_SPLIT_HEADER);
}

// The outcome of one segment: `status` is AIPSTACK_TX_LIN_*, `len` the frame's length L when
// it is written and 0 otherwise; `chunk_len` says that a chunk over 65535 bytes was met (the
// sticky _CHUNK_LEN violation).
struct LinPlan {
    uint32_t len;
    uint8_t status;
    bool chunk_len;
};

// The rule of chksum.h, earliest outcome first. H = d_hdr_len[i], cap = lin_header_cap,
// seg_status = d_seg_status[i] or kLinNoSegStatus, [kbeg, kend) the segment's chunks, len_at(k)
// = d_chunk_len[k], room = d_offsets[i+1] - d_offsets[i] (modulo 2^64) or kLinNoRoom. The chunk
// lengths are summed in order and the walk stops after the first chunk that brings H + sum
// above frame_max (a chunk over 65535 bytes does, frame_max being at most 65535), so an index
// pair that describes far too many chunks costs a bounded walk; chunks behind the stop are not
// looked at.
template <class LenAt>
AIPSTACK_LIN_HD LinPlan lin_plan(uint32_t H, uint32_t cap, uint32_t seg_status, uint64_t kbeg,
                                 uint64_t kend, LenAt len_at, uint32_t frame_max, uint64_t room) {
    LinPlan p = {0u, AIPSTACK_TX_LIN_SKIPPED, false};
    if (H == 0u || seg_status == AIPSTACK_TX_BURST_INVALID || seg_status == AIPSTACK_TX_DGRAM_INVALID)
        return p;
    p.status = AIPSTACK_TX_LIN_INVALID;
    if (H > cap || kend < kbeg) return p;
    uint64_t L = H;  // at most 256 + 65535 + frame_max: no overflow
    for (uint64_t k = kbeg; k < kend && L <= frame_max; ++k) {
        const uint32_t l = len_at(k);
        if (l > AIPSTACK_CHKSUM_MAX_LEN) {
            p.chunk_len = true;
            return p;
        }
        L += l;
    }
    if (L < kLinMinFrame) {
        p.status = AIPSTACK_TX_LIN_TOO_SHORT;
    } else if (L > frame_max) {
        p.status = AIPSTACK_TX_LIN_TOO_LARGE;
    } else if (room != kLinNoRoom && L != room) {
        p.status = AIPSTACK_TX_LIN_WRONG_ROOM;
    } else {
        p.status = AIPSTACK_TX_LIN_WRITTEN;
        p.len = (uint32_t)L;
    }
    return p;
}

// A piece of a frame: the frame bytes [start, start + len) are the piece's bytes in order. The
// header is piece `kbeg - 1` of the walk below (k == kLinHeader), chunk k the piece after it.
constexpr uint64_t kLinHeader = ~0ull;
struct LinPiece {
    uint64_t k;       // kLinHeader, or the chunk's index in the chunk table
    uint32_t start;   // frame position of the piece's first byte
    uint32_t len;     // its length (0 for an empty chunk)
};

AIPSTACK_LIN_HD LinPiece lin_header_piece(uint32_t H) { return LinPiece{kLinHeader, 0u, H}; }

// The piece after `p` in the frame's piece-end prefix (header, then the chunks from kbeg on).
// Only called while the frame has bytes at or behind p's end, so k stays below the frame's kend.
template <class LenAt>
AIPSTACK_LIN_HD LinPiece lin_next_piece(const LinPiece &p, uint64_t kbeg, LenAt len_at) {
    const uint64_t k = p.k == kLinHeader ? kbeg : p.k + 1u;
    return LinPiece{k, p.start + p.len, len_at(k)};
}

// The piece that holds frame byte `pos` of a written frame (pos < L): the first piece whose end
// lies above pos. A serial walk of the prefix from the header on: two or three steps for the
// frames the Tx builders make, as many as there are chunks before pos for any other.
template <class LenAt>
AIPSTACK_LIN_HD LinPiece lin_find_piece(uint32_t H, uint64_t kbeg, LenAt len_at, uint32_t pos) {
    LinPiece p = lin_header_piece(H);
    while (p.start + p.len <= pos) p = lin_next_piece(p, kbeg, len_at);
    return p;
}

// What the entry points check before any work (chksum.h): a stride of 0 stands for "the
// offsets form" in `slot_stride`.
int tx_linearise_check_args(const void *d_hdr, uint64_t hdr_stride, const void *d_hdr_len,
                            const void *d_chunk_addr, const void *d_chunk_len,
                            const void *d_chunk_index, uint64_t n, const void *d_frames,
                            bool slotted, uint64_t slot_stride, const void *d_offsets,
                            uint32_t frame_max, const void *d_frame_len, const void *d_status);

// Segments a wave of the copy pass owns: about 12 KiB of output at frame_max bytes each.
uint32_t tx_linearise_run_frames(uint32_t frame_max);

}  // namespace aipstack_amd

#endif
