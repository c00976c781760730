// aipstack_amd -- how the one-frame-per-lane Rx passes (tcprx_kernels.hip, icmp_kernels.hip,
// udprx_kernels.hip) find and read a frame: its start address and length in the CSR and the
// ring-slot layout, as Rx verify takes them, the unaligned dword load, and the load of an entry
// of the sorted key table. On top of lane_pass.h, for .hip translation units only, in an
// anonymous namespace.
#ifndef AIPSTACK_AMD_RX_FRAMES_H
#define AIPSTACK_AMD_RX_FRAMES_H

#include "lane_pass.h"
#include "pcb_lookup.h"

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

// The little-endian dword at frame bytes [off, off + 4): a load at the frame's own alignment.
struct FrameLoad {
    uint64_t S;
    __device__ __forceinline__ uint32_t operator()(uint32_t off) const {
        return *reinterpret_cast<global_t<const uint32_t, 1> *>(S + off);
    }
};

// Entry `i` of a table of 16-byte aipstack_tcp_pcb_key entries (8-byte aligned) at `table`, for
// pcb_table_find (pcb_lookup.h): one 16-byte load.
struct PcbTableLoad {
    uint64_t table;
    __device__ __forceinline__ PcbEntryWords operator()(uint64_t i) const {
        const u32x4 e = *reinterpret_cast<global_t<const u32x4, 8> *>(table + i * 16u);
        return PcbEntryWords{e.x, e.y, e.z, e.w};
    }
};

}  // namespace
}  // namespace aipstack_amd

#endif
