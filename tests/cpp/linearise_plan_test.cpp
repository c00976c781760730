// The rule that decides a segment's status and length (lin_plan) and the piece lookup
// (lin_find_piece / lin_next_piece) of aipstack_amd/csrc/linearise_common.h, run serially on the
// host against a byte-wise gather: every frame byte is fetched through the lookup, as a lane of
// the copy pass fetches it, from heap blocks of exactly the described sizes, so that
// AddressSanitizer sees any read outside a header's first hdr_len bytes or outside a chunk.
// Also the argument checks and the run length of linearise_host.cpp.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "aipstack_amd/chksum.h"
#include "linearise_common.h"

using namespace aipstack_amd;

static int g_fail = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                              \
        }                                                          \
    } while (0)

struct LenAt {
    const uint32_t *len;
    uint32_t operator()(uint64_t k) const { return len[k]; }
};

struct Segment {
    uint8_t *hdr = nullptr;  // exactly H bytes
    uint32_t H = 0;
    std::vector<uint8_t *> chunk;  // each exactly its length (null for an empty one)
    std::vector<uint32_t> len;
};

static void run_random(uint32_t seed, uint32_t frame_max) {
    std::mt19937 rng(seed);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
    for (int it = 0; it < 400; ++it) {
        Segment s;
        const int kind = (int)pick(0, 7);
        s.H = kind == 0 ? pick(1, 13) : pick(14, 256);
        const uint32_t nch = kind == 1 ? 0 : kind == 2 ? pick(65, 300) : pick(0, 4);
        for (uint32_t c = 0; c < nch; ++c)
            s.len.push_back(kind == 2 ? pick(0, 3) : kind == 3 ? pick(0, frame_max) : pick(0, 400));
        if (kind == 4) s.len.push_back(65536u + pick(0, 3));  // never read
        s.hdr = (uint8_t *)std::malloc(s.H);
        for (uint32_t b = 0; b < s.H; ++b) s.hdr[b] = (uint8_t)rng();
        for (uint32_t l : s.len) {
            uint8_t *p = l && l <= 65535u ? (uint8_t *)std::malloc(l) : nullptr;
            for (uint32_t b = 0; p && b < l; ++b) p[b] = (uint8_t)rng();
            s.chunk.push_back(p);
        }
        // the rule, against the list of chksum.h written out here
        uint64_t total = s.H;
        bool oversize = false;
        for (uint32_t l : s.len) {
            if (total > frame_max) break;
            if (l > 65535u) { oversize = true; break; }
            total += l;
        }
        const uint32_t cap = lin_header_cap(256);
        const LenAt len_at{s.len.data()};
        const LinPlan p = lin_plan(s.H, cap, kLinNoSegStatus, 0, s.len.size(), len_at, frame_max, kLinNoRoom);
        const int want = oversize ? AIPSTACK_TX_LIN_INVALID
                         : total < 14 ? AIPSTACK_TX_LIN_TOO_SHORT
                         : total > frame_max ? AIPSTACK_TX_LIN_TOO_LARGE
                                             : AIPSTACK_TX_LIN_WRITTEN;
        CHECK(p.status == want);
        CHECK(p.chunk_len == oversize);
        CHECK(p.len == (want == AIPSTACK_TX_LIN_WRITTEN ? total : 0));
        if (p.status == AIPSTACK_TX_LIN_WRITTEN) {
            // byte-wise gather (sendFrame's copy) against the lookup, every position on its own
            std::vector<uint8_t> lin(s.hdr, s.hdr + s.H);
            for (size_t c = 0; c < s.len.size(); ++c) lin.insert(lin.end(), s.chunk[c], s.chunk[c] + s.len[c]);
            CHECK(lin.size() == p.len);
            for (uint32_t pos = 0; pos < p.len; ++pos) {
                const LinPiece pc = lin_find_piece(s.H, 0, len_at, pos);
                CHECK(pc.start <= pos && pos < pc.start + pc.len);
                const uint8_t *src = pc.k == kLinHeader ? s.hdr : s.chunk[pc.k];
                CHECK(src[pos - pc.start] == lin[pos]);
            }
            // the walk a destination segment across seams makes: piece after piece to the end
            LinPiece q = lin_header_piece(s.H);
            uint32_t seen = q.len;
            while (q.start + q.len < p.len) {
                q = lin_next_piece(q, 0, len_at);
                CHECK(q.start == seen);
                seen += q.len;
            }
            CHECK(seen == p.len);
        }
        // the same segment in a room of its own: right, one short, one long
        const LinPlan r0 = lin_plan(s.H, cap, kLinNoSegStatus, 0, s.len.size(), len_at, frame_max, total);
        const LinPlan r1 = lin_plan(s.H, cap, kLinNoSegStatus, 0, s.len.size(), len_at, frame_max, total + 1);
        CHECK(r0.status == want);
        CHECK(r1.status == (want == AIPSTACK_TX_LIN_WRITTEN ? AIPSTACK_TX_LIN_WRONG_ROOM : want));
        std::free(s.hdr);
        for (uint8_t *c : s.chunk) std::free(c);
    }
}

static void run_order() {
    const uint32_t len[3] = {10, 70000, 5};
    const LenAt at{len};
    // skipped beats everything
    CHECK(lin_plan(0, 64, kLinNoSegStatus, 5, 2, at, 1514, 3).status == AIPSTACK_TX_LIN_SKIPPED);
    CHECK(lin_plan(300, 64, AIPSTACK_TX_BURST_INVALID, 0, 3, at, 1514, kLinNoRoom).status == AIPSTACK_TX_LIN_SKIPPED);
    CHECK(lin_plan(54, 64, AIPSTACK_TX_DGRAM_INVALID, 0, 1, at, 1514, kLinNoRoom).status == AIPSTACK_TX_LIN_SKIPPED);
    CHECK(lin_plan(54, 64, AIPSTACK_TX_SPLIT_LAYOUT, 0, 1, at, 1514, kLinNoRoom).status == AIPSTACK_TX_LIN_WRITTEN);
    // invalid: header above the cap, index decreasing, an oversized chunk (with its bit)
    CHECK(lin_plan(65, 64, kLinNoSegStatus, 0, 1, at, 1514, kLinNoRoom).status == AIPSTACK_TX_LIN_INVALID);
    CHECK(lin_plan(257, lin_header_cap(300), kLinNoSegStatus, 0, 1, at, 1514, kLinNoRoom).status == AIPSTACK_TX_LIN_INVALID);
    CHECK(lin_plan(54, 64, kLinNoSegStatus, 2, 1, at, 1514, kLinNoRoom).status == AIPSTACK_TX_LIN_INVALID);
    const LinPlan big = lin_plan(54, 64, kLinNoSegStatus, 0, 3, at, 1514, kLinNoRoom);
    CHECK(big.status == AIPSTACK_TX_LIN_INVALID && big.chunk_len && big.len == 0);
    // the sum stops once it is above frame_max: the oversized chunk behind is not looked at
    const LinPlan stop = lin_plan(54, 64, kLinNoSegStatus, 0, 3, at, 60, kLinNoRoom);
    CHECK(stop.status == AIPSTACK_TX_LIN_TOO_LARGE && !stop.chunk_len);
    CHECK(lin_plan(3, 64, kLinNoSegStatus, 0, 1, at, 1514, 13).status == AIPSTACK_TX_LIN_TOO_SHORT);
    CHECK(lin_plan(4, 64, kLinNoSegStatus, 0, 1, at, 1514, 14).status == AIPSTACK_TX_LIN_WRITTEN);
}

static void run_args() {
    char x[8];
    const void *p = x;
    auto chk = [&](const void *hdr, uint64_t hs, uint64_t n, bool slotted, uint64_t ss, const void *off,
                   uint32_t fm) {
        return tx_linearise_check_args(hdr, hs, p, p, p, p, n, p, slotted, ss, off, fm, p, p);
    };
    CHECK(chk(p, 64, 1, true, 2048, nullptr, 1514) == AIPSTACK_CHKSUM_OK);
    CHECK(chk(p, 64, 1, false, 0, p, 65535) == AIPSTACK_CHKSUM_OK);
    CHECK(chk(nullptr, 64, 1, true, 2048, nullptr, 1514) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(chk(p, 0, 1, true, 2048, nullptr, 1514) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(chk(p, 64, 1, true, 0, nullptr, 1514) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(chk(p, 64, 1, true, 65537, nullptr, 1514) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(chk(p, 64, 1, true, 1513, nullptr, 1514) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(chk(p, 64, 1, true, 2048, nullptr, 0) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(chk(p, 64, 1, false, 0, p, 65536) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(chk(p, 64, 1, false, 0, nullptr, 1514) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(chk(p, 64, (1ull << 40) + 1, true, 2048, nullptr, 1514) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(chk(p, 64, 1ull << 40, true, 2048, nullptr, 1514) == AIPSTACK_CHKSUM_OK);
    CHECK(tx_linearise_run_frames(1514) == 8 && tx_linearise_run_frames(65535) == 1 &&
          tx_linearise_run_frames(100) == 64 && tx_linearise_run_frames(200) == 61);
}

int main() {
    run_order();
    run_args();
    run_random(1, 1514);
    run_random(2, 300);
    run_random(3, 65535);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("linearise_plan_test: ok\n");
    return 0;
}
