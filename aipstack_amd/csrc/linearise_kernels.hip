// aipstack_amd -- linearising header-split Tx segments into send-ring frames: the batched form
// of the copy in the reference's only driver, TapDeviceLinux::sendFrame
// (tap/linux/TapDeviceLinux.cpp:109-140: too short -> HardwareError, too long -> PacketTooLarge,
// else ipBufTakeBytes(frame, len, buffer) into one linear buffer, which it then write()s).
//
// Segment i is what the header-split fill takes (hsplit_kernels.hip): the first hdr_len[i]
// bytes of slot i of a header ring, then the chunks [index[i], index[i+1]) of a chunk table.
// Frame i goes to frames + i * slot_stride (ring slots) or frames + offsets[i] (CSR). Two
// stream-ordered launches:
//   1. linearise_plan_kernel, one segment per lane (lane_pass.h): the rule of
//      linearise_common.h (lin_plan) gives the status and the length L; both are stored for
//      every segment, L as 0 for a segment that is not written.
//   2. linearise_copy_kernel, driven by the destination. A wave owns a run of R consecutive
//      segments (R = about 12 KiB / frame_max, 8 for frame_max 1514; lane j holds segment j's
//      numbers). The aligned 16-byte destination segments of the run's written frames, in
//      order, get compact indices (an exclusive scan of the frames' segment counts); the wave
//      takes them in groups of kLinWindows windows of 64, lane k of window w the index
//      64 w + k. A lane finds its frame from the scan, its frame position from the index, and
//      the piece that holds that position with lin_find_piece (header, then the chunks; the
//      first chunk's length and address come with the frame's numbers, so the frames the Tx
//      builders make need no table load here). It loads the one or two aligned 16-byte source
//      segments that hold the piece's bytes for this destination segment, shifts them into
//      place (v_cndmask by dwords, v_alignbyte by bytes) and ORs them in under a byte mask;
//      a destination segment that spans a seam goes on to the next piece. All first-piece
//      loads of a group are issued before any of its stores. A whole segment is one
//      nontemporal 16-byte store; a frame's first and last partial segments are stored by
//      dwords and bytes, so nothing outside [frame start, frame start + L) is written.
//
// Reads: only aligned 16-byte segments that hold a described byte (of a header's first
// hdr_len bytes or of a chunk), as the chained batch; the tables at the described entries.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "aipstack_amd/chksum.h"
#include "chksum_device.h"
#include "chksum_internal.h"
#include "lane_pass.h"
#include "linearise_common.h"

namespace aipstack_amd {
namespace {

constexpr int kLinWindows = 4;  // windows (1 KiB of output each) a wave has in flight

// d_chunk_len[k]; the frame's first chunk from a register.
struct LinLenAt {
    const uint32_t *len;
    uint64_t kbeg;
    uint32_t len0;
    __device__ __forceinline__ uint32_t operator()(uint64_t k) const {
        return k == kbeg ? len0 : len[k];
    }
};
struct LinPlanLenAt {
    const uint32_t *len;
    __device__ __forceinline__ uint32_t operator()(uint64_t k) const { return len[k]; }
};

template <bool SLOTTED>
__global__ __launch_bounds__(kBlock) void linearise_plan_kernel(
    uint64_t hdr_stride, const uint32_t *__restrict__ hdr_len,
    const uint32_t *__restrict__ chunk_len, const uint64_t *__restrict__ chunk_index, uint64_t n,
    const uint8_t *__restrict__ seg_status, const uint64_t *__restrict__ offsets,
    uint32_t frame_max, uint32_t *__restrict__ frame_len, uint8_t *__restrict__ status) {
    const WaveStride ws;
    const uint32_t cap = lin_header_cap(hdr_stride);
    for (uint64_t base = uniform64(ws.first); base < n; base += ws.step) {
        const uint64_t i = base + ws.lane;
        bool oversize = false;
        if (i < n) {
            const uint32_t ss = seg_status ? (uint32_t)seg_status[i] : kLinNoSegStatus;
            const uint64_t room = SLOTTED ? kLinNoRoom : offsets[i + 1] - offsets[i];
            const LinPlan p = lin_plan(hdr_len[i], cap, ss, chunk_index[i], chunk_index[i + 1],
                                       LinPlanLenAt{chunk_len}, frame_max, room);
            oversize = p.chunk_len;
            frame_len[i] = p.len;
            status[i] = p.status;
        }
        note_violation(oversize, AIPSTACK_CHKSUM_VIOLATION_CHUNK_LEN);
    }
}

__device__ __forceinline__ uint32_t lin_from_lane(uint32_t v, uint32_t j) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(j << 2), (int)v);
}
__device__ __forceinline__ uint64_t lin_from_lane64(uint64_t v, uint32_t j) {
    return ((uint64_t)lin_from_lane((uint32_t)(v >> 32), j) << 32) | lin_from_lane((uint32_t)v, j);
}

// Bytes [sh, sh + 16) of the 48 bytes 0^16 || x || y, sh in 1..31.
__device__ __forceinline__ u32x4 lin_shift(const u32x4 &x, const u32x4 &y, uint32_t sh) {
    const bool s16 = (sh & 16u) != 0, s8 = (sh & 8u) != 0, s4 = (sh & 4u) != 0;
    // named values, not arrays: a select between two elements of a local array becomes one
    // dynamically indexed element, and the array then lives in scratch
    const uint32_t a0 = s16 ? x[0] : 0u, a1 = s16 ? x[1] : 0u, a2 = s16 ? x[2] : 0u,
                   a3 = s16 ? x[3] : 0u, a4 = s16 ? y[0] : x[0], a5 = s16 ? y[1] : x[1],
                   a6 = s16 ? y[2] : x[2], a7 = s16 ? y[3] : x[3];
    const uint32_t b0 = s8 ? a2 : a0, b1 = s8 ? a3 : a1, b2 = s8 ? a4 : a2, b3 = s8 ? a5 : a3,
                   b4 = s8 ? a6 : a4, b5 = s8 ? a7 : a5;
    const uint32_t e0 = s4 ? b1 : b0, e1 = s4 ? b2 : b1, e2 = s4 ? b3 : b2, e3 = s4 ? b4 : b3,
                   e4 = s4 ? b5 : b4;
    const uint32_t r = sh & 3u;
    return u32x4{__builtin_amdgcn_alignbyte(e1, e0, r), __builtin_amdgcn_alignbyte(e2, e1, r),
                 __builtin_amdgcn_alignbyte(e3, e2, r), __builtin_amdgcn_alignbyte(e4, e3, r)};
}

// The part of one destination segment that one piece supplies. The segment's byte 0 is frame
// position p (negative in a frame's first segment); it takes the frame bytes [p + t0, p + t1).
// issue() loads the aligned source segments that hold the piece's share, finish() moves the
// bytes into `out`.
template <bool NT>
struct LinPieceLoad {
    u32x4 x, y;
    int ta, tb;  // the destination bytes [ta, tb) come from this piece
    uint32_t sh;

    __device__ __forceinline__ void issue(const LinPiece &pc, uint64_t addr, int p, int t0, int t1) {
        typedef __attribute__((address_space(1))) const u32x4 gseg;
        const int first = (int)pc.start - p, end = (int)(pc.start + pc.len) - p;
        ta = first > t0 ? first : t0;
        tb = end < t1 ? end : t1;
        x = y = u32x4{0u, 0u, 0u, 0u};
        sh = 16u;
        if (tb > ta) {
            const uint64_t sa = addr + (uint64_t)(int64_t)(ta - first), sb = sa + (uint32_t)(tb - ta);
            const uint64_t B0 = sa & ~(uint64_t)15, B1 = (sb - 1u) & ~(uint64_t)15;
            const bool nt = NT && pc.k != kLinHeader;
            x = nt ? __builtin_nontemporal_load((const gseg *)B0) : *(const gseg *)B0;
            if (B1 != B0) y = nt ? __builtin_nontemporal_load((const gseg *)B1) : *(const gseg *)B1;
            sh = (uint32_t)((int)(uint32_t)(sa - B0) - ta + 16);
        }
    }
    __device__ __forceinline__ void finish(u32x4 &out) const {
        const u32x4 v = lin_shift(x, y, sh);
#pragma unroll
        for (int d = 0; d < 4; ++d) out[d] |= v[d] & dword_keep(ta - 4 * d, tb - 4 * d);
    }
};

// Bytes [t0, t1) of `v` to the aligned segment at `dst`: whole dwords, else single bytes.
__device__ __forceinline__ void lin_store_partial(uint64_t dst, const u32x4 &v, int t0, int t1) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int lo = t0 - 4 * d, hi = t1 - 4 * d;
        if (lo <= 0 && hi >= 4) {
            __builtin_nontemporal_store(v[d], reinterpret_cast<global_t<uint32_t> *>(dst + 4 * d));
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b >= lo && b < hi)
                    __builtin_nontemporal_store(
                        (uint8_t)(v[d] >> (8 * b)),
                        reinterpret_cast<global_t<uint8_t> *>(dst + 4 * d + b));
        }
    }
}

template <bool SLOTTED, bool NT>
__global__ __launch_bounds__(kBlock) void linearise_copy_kernel(
    uint64_t hdr_base, uint64_t hdr_stride, const uint32_t *__restrict__ hdr_len,
    const uint64_t *__restrict__ chunk_addr, const uint32_t *__restrict__ chunk_len,
    const uint64_t *__restrict__ chunk_index, uint64_t n, uint64_t frames, uint64_t slot_stride,
    const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ frame_len, uint32_t R) {
    constexpr int U = kLinWindows;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint64_t runs = (n + R - 1u) / R;
    for (uint64_t run = uniform64((uint64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave);
         run < runs; run += nwaves) {
        // lane j: segment i0 + j of the run
        const uint64_t i0 = run * R;
        const uint32_t cnt = (uint32_t)(n - i0 < R ? n - i0 : R);
        const uint64_t i = i0 + lane;
        const uint32_t L = lane < cnt ? frame_len[i] : 0u;
        uint32_t H = 0, len0 = 0;
        uint64_t kbeg = 0, D = 0, addr0 = 0;
        if (L) {  // written: the plan pass found its numbers within the contract
            H = hdr_len[i];
            kbeg = chunk_index[i];
            D = frames + (SLOTTED ? i * slot_stride : offsets[i]);
            if (L > H) {  // it has a chunk
                len0 = chunk_len[kbeg];
                addr0 = chunk_addr[kbeg];
            }
        }
        const uint32_t ns = L ? (((uint32_t)D & 15u) + L + 15u) >> 4 : 0u;
        const uint32_t incl = wave_incl_scan(ns);
        const uint32_t cs = incl - ns;  // compact index of the frame's first segment
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);

        for (uint32_t g0 = 0; g0 < total; g0 += (uint32_t)(kWave * U)) {
            // the frame of each of this lane's U destination segments: the last one whose
            // first compact index is not above the segment's
            uint32_t c[U], j[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                c[u] = g0 + (uint32_t)(u * kWave) + lane;
                j[u] = 0;
            }
            for (uint32_t f = 1; f < cnt; ++f) {
                const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)cs, (int)f);
#pragma unroll
                for (int u = 0; u < U; ++u) j[u] = c[u] >= s ? f : j[u];
            }
            uint64_t dst[U], kb[U], a0[U], hdr[U];
            uint32_t Hh[U], l0[U];
            int p[U], t0[U], t1[U];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {  // every lane takes part in the permutes
                const uint64_t Dj = lin_from_lane64(D, j[u]);
                const uint32_t Lj = lin_from_lane(L, j[u]), csj = lin_from_lane(cs, j[u]);
                Hh[u] = lin_from_lane(H, j[u]);
                l0[u] = lin_from_lane(len0, j[u]);
                kb[u] = lin_from_lane64(kbeg, j[u]);
                a0[u] = lin_from_lane64(addr0, j[u]);
                hdr[u] = hdr_base + (i0 + j[u]) * hdr_stride;
                live[u] = c[u] < total;
                const uint32_t k = c[u] - csj;
                dst[u] = (Dj & ~(uint64_t)15) + 16ull * k;
                p[u] = (int)(16u * k) - (int)((uint32_t)Dj & 15u);
                t0[u] = p[u] < 0 ? -p[u] : 0;
                const int rest = (int)Lj - p[u];
                t1[u] = live[u] ? (rest < 16 ? rest : 16) : t0[u];
            }
            // the first piece of every segment: found, its loads issued
            LinPiece pc[U];
            LinPieceLoad<NT> ld[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                pc[u] = lin_header_piece(Hh[u]);
                if (live[u]) {
                    const LinLenAt len_at{chunk_len, kb[u], l0[u]};
                    pc[u] = lin_find_piece(Hh[u], kb[u], len_at, (uint32_t)(p[u] + t0[u]));
                    const uint64_t addr = pc[u].k == kLinHeader ? hdr[u]
                                          : pc[u].k == kb[u]    ? a0[u]
                                                                : chunk_addr[pc[u].k];
                    ld[u].issue(pc[u], addr, p[u], t0[u], t1[u]);
                }
            }
            // the bytes into place; a segment across a seam goes on through the pieces
            u32x4 out[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                out[u] = u32x4{0u, 0u, 0u, 0u};
                if (live[u]) {
                    ld[u].finish(out[u]);
                    const LinLenAt len_at{chunk_len, kb[u], l0[u]};
                    LinPiece q = pc[u];
                    while ((int)(q.start + q.len) - p[u] < t1[u]) {
                        q = lin_next_piece(q, kb[u], len_at);
                        if (q.len != 0u) {
                            LinPieceLoad<NT> more;
                            more.issue(q, q.k == kb[u] ? a0[u] : chunk_addr[q.k], p[u], t0[u], t1[u]);
                            more.finish(out[u]);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (live[u]) {
                    if (t0[u] == 0 && t1[u] == 16)
                        __builtin_nontemporal_store(out[u],
                                                    reinterpret_cast<global_t<u32x4> *>(dst[u]));
                    else
                        lin_store_partial(dst[u], out[u], t0[u], t1[u]);
                }
            }
        }
    }
}

template <bool SLOTTED>
int linearise_launch(const void *d_hdr, uint64_t hdr_stride, const uint32_t *d_hdr_len,
                     const uint64_t *d_chunk_addr, const uint32_t *d_chunk_len,
                     const uint64_t *d_chunk_index, uint64_t n, const uint8_t *d_seg_status,
                     void *d_frames, uint64_t slot_stride, const uint64_t *d_offsets,
                     uint32_t frame_max, uint32_t *d_frame_len, uint8_t *d_status, uint32_t flags,
                     void *stream) {
    if (n == 0) return AIPSTACK_CHKSUM_OK;
    int st = tx_linearise_check_args(d_hdr, hdr_stride, d_hdr_len, d_chunk_addr, d_chunk_len,
                                     d_chunk_index, n, d_frames, SLOTTED, slot_stride, d_offsets,
                                     frame_max, d_frame_len, d_status);
    if (st != AIPSTACK_CHKSUM_OK) return st;
    const hipStream_t s = (hipStream_t)stream;
    const int cus = device_cu_count(s);
    if (cus <= 0) return AIPSTACK_CHKSUM_EHIP;
    hipLaunchKernelGGL(linearise_plan_kernel<SLOTTED>, dim3(lane_pass_blocks(n, cus)), dim3(kBlock),
                       0, s, hdr_stride, d_hdr_len, d_chunk_len, d_chunk_index, n, d_seg_status,
                       d_offsets, frame_max, d_frame_len, d_status);
    st = check_hip(hipGetLastError());
    if (st != AIPSTACK_CHKSUM_OK) return st;
    // the copy pass: one run per wave, at most as many blocks as a lane pass launches
    const uint32_t R = tx_linearise_run_frames(frame_max);
    const uint64_t runs = (n + R - 1u) / R;
    const uint64_t want = (runs + kWavesPerBlock - 1u) / kWavesPerBlock, most = tuning_aux_blocks(cus);
    const unsigned blocks = (unsigned)(want < most ? want : most);
    const uint64_t hdr = (uint64_t)(uintptr_t)d_hdr, frames = (uint64_t)(uintptr_t)d_frames;
    if (flags & AIPSTACK_CHKSUM_JUST_WRITTEN)
        hipLaunchKernelGGL((linearise_copy_kernel<SLOTTED, true>), dim3(blocks), dim3(kBlock), 0, s,
                           hdr, hdr_stride, d_hdr_len, d_chunk_addr, d_chunk_len, d_chunk_index, n,
                           frames, slot_stride, d_offsets, d_frame_len, R);
    else
        hipLaunchKernelGGL((linearise_copy_kernel<SLOTTED, false>), dim3(blocks), dim3(kBlock), 0, s,
                           hdr, hdr_stride, d_hdr_len, d_chunk_addr, d_chunk_len, d_chunk_index, n,
                           frames, slot_stride, d_offsets, d_frame_len, R);
    return check_hip(hipGetLastError());
}

}  // namespace

// this unit's violation word joins the ones aipstack_chksum_contract_violations reads
static const bool g_violations_registered = (add_violation_source(&take_violations_here), true);

}  // namespace aipstack_amd

using namespace aipstack_amd;

extern "C" int aipstack_tx_linearise_slotted(const void *d_hdr, uint64_t hdr_stride,
                                             const uint32_t *d_hdr_len,
                                             const uint64_t *d_chunk_addr,
                                             const uint32_t *d_chunk_len,
                                             const uint64_t *d_chunk_index, uint64_t n,
                                             const uint8_t *d_seg_status, void *d_frames,
                                             uint64_t slot_stride, uint32_t frame_max,
                                             uint32_t *d_frame_len, uint8_t *d_status,
                                             uint32_t flags, void *stream) {
    return linearise_launch<true>(d_hdr, hdr_stride, d_hdr_len, d_chunk_addr, d_chunk_len,
                                  d_chunk_index, n, d_seg_status, d_frames, slot_stride, nullptr,
                                  frame_max, d_frame_len, d_status, flags, stream);
}

extern "C" int aipstack_tx_linearise(const void *d_hdr, uint64_t hdr_stride,
                                     const uint32_t *d_hdr_len, const uint64_t *d_chunk_addr,
                                     const uint32_t *d_chunk_len, const uint64_t *d_chunk_index,
                                     uint64_t n, const uint8_t *d_seg_status, void *d_frames,
                                     const uint64_t *d_offsets, uint32_t frame_max,
                                     uint32_t *d_frame_len, uint8_t *d_status, uint32_t flags,
                                     void *stream) {
    return linearise_launch<false>(d_hdr, hdr_stride, d_hdr_len, d_chunk_addr, d_chunk_len,
                                   d_chunk_index, n, d_seg_status, d_frames, 0, d_offsets,
                                   frame_max, d_frame_len, d_status, flags, stream);
}
