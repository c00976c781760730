// aipstack_amd -- the Tx producers (TCP burst segmentation, UDP send with IPv4 fragmentation):
// what their host sides (tcpseg_host.cpp, ipfrag_host.cpp), their kernels (through tx_producer.h)
// and the stand-alone test (tests/cpp/tx_producer_test.cpp) share as plain C++: the count cap,
// the owner search in the caller's running sums and the argument checks of the entry points.
#ifndef AIPSTACK_AMD_TX_PRODUCER_COMMON_H
#define AIPSTACK_AMD_TX_PRODUCER_COMMON_H

#include <cstdint>
#include <initializer_list>

#include "aipstack_amd/chksum.h"

#if defined(__HIPCC__)
#define AIPSTACK_TXP_HD __host__ __device__ inline
#else
#define AIPSTACK_TXP_HD inline
#endif

namespace aipstack_amd {

constexpr uint64_t kTxMaxCount = 1ull << 40;  // owners, elements, chunks of one call

// The first j in [lo, hi] with idx[j] > i (hi if there is none); reads entries in [lo, hi).
AIPSTACK_TXP_HD uint64_t upper_bound(const uint64_t *__restrict__ idx, uint64_t lo, uint64_t hi,
                                     uint64_t i) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (idx[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Who the running sums `idx` (n_owners + 1 entries) give element i to, searched in [lo, hi] (hi
// <= n_owners + 1): `at` is the owner d (idx[d] <= i < idx[d+1]) when `owned`, else where the
// search ended (0: below the first sum). Reads entries in [lo, hi) and, for 1 <= j <= n_owners,
// j - 1 and j: never outside [0, n_owners], whatever the sums hold.
struct OwnerOf {
    bool owned;
    uint64_t at;
};

AIPSTACK_TXP_HD OwnerOf owner_of(const uint64_t *__restrict__ idx, uint64_t n_owners, uint64_t lo,
                                 uint64_t hi, uint64_t i) {
    const uint64_t j = upper_bound(idx, lo, hi, i);
    if (j >= 1 && j <= n_owners && idx[j - 1] <= i && i < idx[j]) return OwnerOf{true, j - 1};
    return OwnerOf{false, j};
}

// Host only (the kernels take the cap and the two searches above, nothing else): the argument
// checks of a producer's entry point. No null pointer among `ptrs` and the workspace, a slot that
// holds the longest header, the counts below the cap, `need` workspace bytes, 8-byte aligned.
inline int tx_producer_check_args(std::initializer_list<const void *> ptrs, uint64_t hdr_stride,
                                  uint64_t min_stride, uint64_t n_owners, uint64_t n,
                                  uint64_t n_chunks, const void *d_workspace,
                                  uint64_t workspace_bytes, uint64_t need) {
    for (const void *p : ptrs)
        if (!p) return AIPSTACK_CHKSUM_EINVAL;
    if (!d_workspace || hdr_stride < min_stride || n > kTxMaxCount || n_chunks > kTxMaxCount ||
        n_owners > kTxMaxCount)
        return AIPSTACK_CHKSUM_EINVAL;
    if (workspace_bytes < need || ((uintptr_t)d_workspace & 7u) != 0) return AIPSTACK_CHKSUM_EINVAL;
    return AIPSTACK_CHKSUM_OK;
}

}  // namespace aipstack_amd

#endif
