// aipstack_amd -- Tx resolve: the route, the permission tests, the next-hop MAC and the Ethernet
// header of a batch of header slots (the rules, the record and the bytes: txres_common.h). Four
// stream-ordered launches:
//   1. a memset of d_arp_used;
//   2. txres_decide_kernel, one segment per lane, one block per tile of 256 consecutive segments:
//      the interface table once per workgroup into LDS; of a candidate slot the half at bytes
//      12..13 and the dwords at 26 and 30, at the slot's own byte alignment; a binary search of the
//      sorted ARP table through global loads, every index inside [0, n_arp); d_status, the
//      16-byte record, d_send_len; of a _SENT segment the slot's bytes 0..13 in naturally aligned
//      stores as wide as its address allows, and a 1 into d_arp_used for the entry that resolved
//      it (every lane that stores there stores the same value); per wave the ballot of held and
//      of failed segments, per tile their counts, into the workspace;
//   3. pair_scan_kernel (pair_scan.h), ONE workgroup: the exclusive running sums of the tiles'
//      counts in place, the totals behind them and into d_counts;
//   4. txres_emit_kernel, tiles as in 2: a segment's place in each list = its tile's sum + the
//      bits below it in the tile's ballots; entry i of each list at or beyond its count by lane i.
// A place is at most the segment's own index (it counts segments in front of it), so every store
// lies inside the caller's n entries. No kernel waits for another workgroup.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_internal.h"
#include "lane_pass.h"
#include "pair_scan.h"
#include "txres_common.h"

namespace aipstack_amd {
namespace {

static_assert(kTxResTile == kBlock && kTxResTileWaves == kBlock / kWave, "one tile per block iteration");
static_assert(AIPSTACK_TX_MAX_IFACES * kTxIfaceWords <= kBlock, "one dword of the table per thread");
constexpr int kWaves = kBlock / kWave;

// (where the ballots lie behind the counts, and how a wave reads one: pair_scan.h)

// The slot's bytes at its own alignment.
struct SlotLoad16 {
    uint64_t S;
    __device__ __forceinline__ uint32_t operator()(uint32_t off) const {
        return *reinterpret_cast<global_t<const uint16_t, 1> *>(S + off);
    }
};
struct SlotLoad32 {
    uint64_t S;
    __device__ __forceinline__ uint32_t operator()(uint32_t off) const {
        return *reinterpret_cast<global_t<const uint32_t, 1> *>(S + off);
    }
};
// A naturally aligned store of 1, 2 or 4 bytes (tx_res_store_header).
struct SlotStore {
    uint64_t S;
    __device__ __forceinline__ void operator()(uint32_t off, uint32_t width, uint32_t v) const {
        if (width == 4u) *reinterpret_cast<global_t<uint32_t> *>(S + off) = v;
        else if (width == 2u) *reinterpret_cast<global_t<uint16_t> *>(S + off) = (uint16_t)v;
        else *reinterpret_cast<global_t<uint8_t> *>(S + off) = (uint8_t)v;
    }
};
// Interface k of the workgroup's copy of the table.
struct LdsIfaces {
    const uint32_t *w;
    __device__ __forceinline__ TxIfaceWords operator()(uint32_t k) const {
        const uint32_t *p = w + k * kTxIfaceWords;
        return TxIfaceWords{p[0], p[1], p[2], p[3], p[4]};
    }
};
// Entry i of the ARP table (4-byte aligned): one 16-byte load.
struct ArpTableLoad {
    uint64_t table;
    __device__ __forceinline__ ArpEntryWords operator()(uint64_t i) const {
        const u32x4 e = *reinterpret_cast<global_t<const u32x4, 4> *>(table + i * 16u);
        return ArpEntryWords{e.x, e.y, e.z, e.w};
    }
};

__global__ __launch_bounds__(kBlock) void txres_decide_kernel(
    uint64_t hdr_base, uint64_t hdr_stride, const uint32_t *__restrict__ hdr_len, uint64_t n,
    const uint8_t *__restrict__ seg_status, const uint8_t *__restrict__ send_flags,
    const uint16_t *__restrict__ force_iface, const uint32_t *__restrict__ ifaces, uint32_t n_ifaces,
    uint64_t arp, uint64_t n_arp, uint8_t *__restrict__ status, uint64_t route,
    uint32_t *__restrict__ send_len, uint8_t *__restrict__ arp_used, uint64_t *__restrict__ ws) {
    __shared__ uint32_t iface_lds[AIPSTACK_TX_MAX_IFACES * kTxIfaceWords];
    __shared__ uint32_t part[kWaves][2];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (threadIdx.x < n_ifaces * kTxIfaceWords) iface_lds[threadIdx.x] = ifaces[threadIdx.x];
    __syncthreads();
    const uint64_t tiles = tx_res_tiles(n);
    uint64_t *__restrict__ ballots = ws + ballots_at(tiles);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTxResTile + wave * kWave + lane;
        uint32_t st = AIPSTACK_TX_RES_NONE;
        if (i < n) {
            const uint32_t len = hdr_len[i];
            const uint64_t S = hdr_base + i * hdr_stride;
            const TxDecision d = tx_resolve_segment(
                SlotLoad16{S}, SlotLoad32{S}, len, hdr_stride, seg_status ? seg_status[i] : 0u,
                send_flags ? send_flags[i] : 0u,
                force_iface ? (uint32_t)force_iface[i] : (uint32_t)AIPSTACK_TX_ROUTE_ANY,
                LdsIfaces{iface_lds}, n_ifaces, ArpTableLoad{arp}, n_arp);
            st = d.status;
            status[i] = (uint8_t)st;
            *reinterpret_cast<global_t<u32x4, 4> *>(route + i * 16u) = u32x4{d.r[0], d.r[1], d.r[2], d.r[3]};
            const bool sent = st == AIPSTACK_TX_RES_SENT;
            send_len[i] = sent || st == AIPSTACK_TX_RES_NONE ? len : 0u;
            if (sent) {
                tx_res_store_header((uint32_t)S & 3u, d.image(), SlotStore{S});
                if (d.used < n_arp) arp_used[d.used] = 1u;
            }
        }
        const uint64_t hb = __builtin_amdgcn_ballot_w64(st == AIPSTACK_TX_RES_ARP_QUERY);
        const uint64_t fb = __builtin_amdgcn_ballot_w64(
            st == AIPSTACK_TX_RES_NO_ROUTE || st == AIPSTACK_TX_RES_BCAST_REJECTED ||
            st == AIPSTACK_TX_RES_NONLOCAL_SRC || st == AIPSTACK_TX_RES_NO_HW_ROUTE);
        if (lane == 0) {
            ballots[2 * (tile * kWaves + wave)] = hb;
            ballots[2 * (tile * kWaves + wave) + 1] = fb;
            part[wave][0] = __popcll(hb);
            part[wave][1] = __popcll(fb);
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            uint32_t s = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) s += part[w][threadIdx.x];
            ws[2 * tile + threadIdx.x] = s;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void txres_emit_kernel(uint64_t n, uint64_t *__restrict__ held_seg,
                                                            uint64_t *__restrict__ failed_seg,
                                                            const uint64_t *__restrict__ ws) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t tiles = tx_res_tiles(n);
    const uint64_t total_h = ws[2 * tiles], total_f = ws[2 * tiles + 1];
    const uint64_t *__restrict__ ballots = ws + ballots_at(tiles);
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * kTxResTile + wave * kWave + lane;
        const uint64_t *__restrict__ b = ballots + 2 * (tile * kWaves);
        const uint64_t hb = uniform_bits(b[2 * wave]), fb = uniform_bits(b[2 * wave + 1]);
        const uint64_t below = (1ull << lane) - 1u;
        uint64_t j = ws[2 * tile] + __popcll(hb & below), k = ws[2 * tile + 1] + __popcll(fb & below);
#pragma unroll
        for (int w = 0; w < kWaves; ++w)
            if ((uint32_t)w < wave) {
                j += __popcll(b[2 * w]);
                k += __popcll(b[2 * w + 1]);
            }
        // (a ballot has no bit at or beyond n: a place counts segments in front of i, so <= i < n)
        if (hb >> lane & 1ull) held_seg[j] = i;
        if (fb >> lane & 1ull) failed_seg[k] = i;
        if (i < n) {
            if (i >= total_h) held_seg[i] = ~0ull;
            if (i >= total_f) failed_seg[i] = ~0ull;
        }
    }
}

}  // namespace
}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_tx_resolve(void *d_hdr, uint64_t hdr_stride, const uint32_t *d_hdr_len, uint64_t n,
                                   const uint8_t *d_seg_status, const uint8_t *d_send_flags,
                                   const uint16_t *d_force_iface, const aipstack_tx_iface *d_ifaces,
                                   uint32_t n_ifaces, const aipstack_arp_entry *d_arp, uint64_t n_arp,
                                   uint8_t *d_status, aipstack_tx_route *d_route, uint32_t *d_send_len,
                                   uint8_t *d_arp_used, uint64_t *d_held_seg, uint64_t *d_failed_seg,
                                   uint64_t *d_counts, void *d_workspace, uint64_t workspace_bytes,
                                   uint32_t flags, void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = tx_resolve_check_args(TxResolveArgs{
        d_hdr, hdr_stride, d_hdr_len, n, d_force_iface, d_ifaces, n_ifaces, d_arp, n_arp, d_status,
        d_route, d_send_len, d_arp_used, d_held_seg, d_failed_seg, d_counts, d_workspace,
        workspace_bytes});
    if (st != AIPSTACK_CHKSUM_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    unsigned blocks;
    st = lane_pass_blocks(n, s, &blocks);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    if (n_arp != 0) {
        st = check_hip(hipMemsetAsync(d_arp_used, 0, n_arp, s));
        if (st != AIPSTACK_CHKSUM_OK) return st;
    }
    uint64_t *ws = (uint64_t *)d_workspace;
    hipLaunchKernelGGL(txres_decide_kernel, dim3(blocks), dim3(kBlock), 0, s,
                       (uint64_t)(uintptr_t)d_hdr, hdr_stride, d_hdr_len, n, d_seg_status, d_send_flags,
                       d_force_iface, (const uint32_t *)d_ifaces, n_ifaces, (uint64_t)(uintptr_t)d_arp,
                       n_arp, d_status, (uint64_t)(uintptr_t)d_route, d_send_len, d_arp_used, ws);
    hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(kBlock), 0, s, tx_res_tiles(n), ws, d_counts);
    hipLaunchKernelGGL(txres_emit_kernel, dim3(blocks), dim3(kBlock), 0, s, n, d_held_seg,
                       d_failed_seg, ws);
    return check_hip(hipGetLastError());
}
