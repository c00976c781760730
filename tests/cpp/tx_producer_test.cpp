// The owner search of the Tx producers (aipstack_amd/csrc/tx_producer_common.h: upper_bound and
// owner_of, the pure part of what tcpseg_kernels.hip and ipfrag_kernels.hip share), run serially
// on the host and built with ASan + UBSan (tests/cpp/tx_producer.mk). Every element i < n is
// searched the way a wave of for_each_owned does it -- the wave's first and last element over the
// whole index, then the lane between the two results, or the whole wave to one owner when the two
// agree and its range holds the wave -- and compared with a linear scan. The
// index is a heap block of exactly n_owners + 1 entries, so a read outside [0, n_owners] is
// caught by the sanitizer, whatever the index holds: proper running sums (owners of no element
// among them), sums that do not start at 0, that end below or above n, and that decrease.
#include <cstdint>
#include <cstdio>
#include <memory>

#include "tx_producer_common.h"

using aipstack_amd::OwnerOf;
using aipstack_amd::owner_of;
using aipstack_amd::upper_bound;

static int failures = 0;
static long checked = 0, fast_waves = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// upper_bound over a range that is sorted (the contract of a binary search): the first j in
// [lo, hi] with idx[j] > i, by a linear scan.
static uint64_t scan_upper_bound(const uint64_t *idx, uint64_t lo, uint64_t hi, uint64_t i) {
    while (lo < hi && idx[lo] <= i) ++lo;
    return lo;
}

static bool sorted(const uint64_t *idx, uint64_t count) {
    for (uint64_t j = 1; j < count; ++j)
        if (idx[j - 1] > idx[j]) return false;
    return true;
}

// The owners a linear scan gives element i: every d < n_owners with idx[d] <= i < idx[d+1].
static uint64_t scan_owners(const uint64_t *idx, uint64_t n_owners, uint64_t i, uint64_t *first) {
    uint64_t count = 0;
    for (uint64_t d = 0; d < n_owners; ++d)
        if (idx[d] <= i && i < idx[d + 1]) {
            if (count++ == 0) *first = d;
        }
    return count;
}

static void check_index(const uint64_t *idx, uint64_t n_owners, uint64_t n) {
    const bool is_sorted = sorted(idx, n_owners + 1);
    for (uint64_t base = 0; base < n; base += 64) {
        const uint64_t last = base + 63 < n ? base + 63 : n - 1;
        const uint64_t j0 = upper_bound(idx, 0, n_owners + 1, base);
        const uint64_t j1 = upper_bound(idx, j0, n_owners + 1, last);
        CHECK(j0 <= j1 && j1 <= n_owners + 1);
        if (is_sorted) {
            CHECK(j0 == scan_upper_bound(idx, 0, n_owners + 1, base));
            CHECK(j1 == scan_upper_bound(idx, 0, n_owners + 1, last));
        }
        // for_each_owned's uniform fast path: the two searches agree on an owner whose range
        // holds the whole wave (its last reads of the index: j0 - 1 and j0)
        const bool fast = j0 == j1 && j0 >= 1 && j0 <= n_owners && idx[j0 - 1] <= base && last < idx[j0];
        if (fast) ++fast_waves;
        for (uint64_t i = base; i <= last; ++i) {
            const OwnerOf o = owner_of(idx, n_owners, j0, j1, i);
            if (fast) CHECK(o.owned && o.at == j0 - 1);  // the per-lane search gives the same owner
            uint64_t first = 0;
            const uint64_t owners = scan_owners(idx, n_owners, i, &first);
            ++checked;
            if (o.owned) {  // whatever the index holds: an owner is one the scan finds too
                CHECK(o.at < n_owners && idx[o.at] <= i && i < idx[o.at + 1]);
                CHECK(owners >= 1);
            } else {
                CHECK(j0 <= o.at && o.at <= j1);
            }
            if (is_sorted) {  // sorted sums: at most one owner, and the search finds it
                CHECK(owners <= 1 && o.owned == (owners == 1));
                if (o.owned) CHECK(o.at == first);
                else CHECK(o.at == scan_upper_bound(idx, 0, n_owners + 1, i));
            }
        }
    }
}

// Running sums of n_owners counts that add up to about n; `zeros`: per mille of owners with no
// element.
static void fill_sums(uint64_t *idx, uint64_t n_owners, uint64_t n, unsigned zeros) {
    idx[0] = 0;
    uint64_t left = n;
    for (uint64_t d = 0; d < n_owners; ++d) {
        uint64_t c = 0;
        if (d + 1 == n_owners) c = left;
        else if (rnd() % 1000 >= zeros && left != 0) c = 1 + rnd() % (1 + 2 * left / (n_owners - d));
        if (c > left) c = left;
        left -= c;
        idx[d + 1] = idx[d] + c;
    }
}

int main() {
    const uint64_t owners[] = {0, 1, 2, 65, 300};
    const uint64_t sizes[] = {0, 1, 63, 64, 65, 128, 257, 1000, 1537};
    for (uint64_t n_owners : owners)
        for (uint64_t n : sizes)
            for (int shape = 0; shape < 8; ++shape) {
                // exactly n_owners + 1 entries on the heap
                std::unique_ptr<uint64_t[]> idx(new uint64_t[n_owners + 1]);
                fill_sums(idx.get(), n_owners, n, shape == 1 ? 700 : shape == 2 ? 0 : 200);
                switch (shape) {
                case 0: case 1: case 2: break;  // proper running sums
                case 3:  // do not start at 0
                    for (uint64_t j = 0; j <= n_owners; ++j) idx[j] += 5;
                    break;
                case 4:  // end below n
                    for (uint64_t j = 0; j <= n_owners; ++j) idx[j] = idx[j] * 2 / 3;
                    break;
                case 5:  // end above n
                    for (uint64_t j = 0; j <= n_owners; ++j) idx[j] = idx[j] * 3 / 2 + j;
                    break;
                case 6:  // decrease: reversed
                    for (uint64_t j = 0; j < (n_owners + 1) / 2; ++j) {
                        const uint64_t t = idx[j];
                        idx[j] = idx[n_owners - j];
                        idx[n_owners - j] = t;
                    }
                    break;
                case 7:  // decrease here and there: any values, some huge
                    for (uint64_t j = 0; j <= n_owners; ++j)
                        idx[j] = rnd() % 16 == 0 ? ~0ull - rnd() % 4 : rnd() % (n + 2);
                    break;
                }
                check_index(idx.get(), n_owners, n);
            }
    CHECK(checked > 100000 && fast_waves > 100);
    if (failures) return 1;
    std::printf("tx_producer_test: OK (%ld elements)\n", checked);
    return 0;
}
