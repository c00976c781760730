// TCP burst segmentation, the host code alone (aipstack_amd/csrc/tcpseg_host.cpp: the burst
// layout and the argument checks of aipstack_tcp_tx_segment), built with ASan + UBSan
// (tests/cpp/tcpseg.mk). Index arrays are heap blocks of exactly n_bursts + 1 entries, so a
// write or read past them is caught.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "aipstack_amd/chksum.h"
#include "tcpseg_common.h"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static aipstack_tcp_burst good(uint32_t len0, uint32_t len1, uint16_t mss, uint8_t flags) {
    aipstack_tcp_burst b;
    std::memset(&b, 0, sizeof b);
    b.data_addr[0] = 0x1000;
    b.data_addr[1] = 0x9000;
    b.data_len[0] = len0;
    b.data_len[1] = len1;
    b.mss = mss;
    b.flags = flags;
    b.hdr[12] = 0x08;
    b.hdr[14] = 0x45;
    b.hdr[23] = 6;
    return b;
}

static int layout(const std::vector<aipstack_tcp_burst> &v, std::vector<uint64_t> &si,
                  std::vector<uint64_t> &cb) {
    si.assign(v.size() + 1, 0xDEAD);
    cb.assign(v.size() + 1, 0xDEAD);
    return aipstack_tcp_burst_layout(v.empty() ? nullptr : v.data(), v.size(), si.data(), cb.data());
}

int main() {
    std::vector<uint64_t> si, cb;
    // counts: data in mss steps, the straddling segment has two chunks, FIN alone is one segment
    std::vector<aipstack_tcp_burst> v = {
        good(1000, 3000, 1460, 0),                   // 3 segments, 4 chunks
        good(0, 0, 1460, 0),                         // nothing
        good(0, 0, 1460, AIPSTACK_TCP_BURST_FIN),    // 1 segment, no chunk
        good(2920, 100, 1460, 0),                    // boundary on a segment edge: 3 / 3
        good(1, 0, 1, 0),                            // 1 / 1
        good(0xFFFFFFFFu, 0, 65495, 0),              // the largest D and mss
    };
    CHECK(layout(v, si, cb) == AIPSTACK_CHKSUM_OK);
    const uint64_t big = (0xFFFFFFFFull + 65494) / 65495;
    const uint64_t want_s[] = {0, 3, 3, 4, 7, 8, 8 + big}, want_c[] = {0, 4, 4, 4, 7, 8, 8 + big};
    for (size_t i = 0; i < si.size(); ++i) CHECK(si[i] == want_s[i] && cb[i] == want_c[i]);
    v.clear();
    CHECK(layout(v, si, cb) == AIPSTACK_CHKSUM_OK && si[0] == 0 && cb[0] == 0);
    // every invalid class, in the middle of valid bursts
    for (int cls = 0; cls < 9; ++cls) {
        aipstack_tcp_burst b = good(500, 0, 100, 0);
        switch (cls) {
        case 0: b.mss = 0; break;
        case 1: b.mss = 65496; break;
        case 2: b.reserved[2] = 1; break;
        case 3: b.flags = 2; break;
        case 4: b.hdr[13] = 6; break;
        case 5: b.hdr[14] = 0x46; break;
        case 6: b.hdr[23] = 17; break;
        case 7: b.data_len[0] = 0xFFFFFFFFu; b.data_len[1] = 1; break;
        case 8: b.reserved[0] = 0x80; break;
        }
        v = {good(10, 0, 5, 0), b, good(10, 0, 5, 0)};
        CHECK(layout(v, si, cb) == AIPSTACK_CHKSUM_EINVAL);
        CHECK(!aipstack_amd::tcp_burst_shape(b).valid);
    }
    v = {good(10, 0, 5, 0)};
    si.assign(2, 0);
    cb.assign(2, 0);
    CHECK(aipstack_tcp_burst_layout(nullptr, 1, si.data(), cb.data()) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(aipstack_tcp_burst_layout(v.data(), 1, nullptr, cb.data()) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(aipstack_tcp_burst_layout(v.data(), 1, si.data(), nullptr) == AIPSTACK_CHKSUM_EINVAL);

    // workspace bound
    CHECK(aipstack_tcp_tx_segment_workspace_bytes(0) == 0);
    for (uint64_t n : {1ull, 2ull, 63ull, 64ull, 4097ull, 1ull << 20, 1ull << 40, ~0ull}) {
        const uint64_t w = aipstack_tcp_tx_segment_workspace_bytes(n);
        const uint64_t m = n > (1ull << 40) ? 1ull << 40 : n;
        CHECK(w % 8 == 0 && w >= 14 * m && w <= 16 * m + 256);
    }

    // the argument checks (pointers are only compared, never followed)
    using aipstack_amd::tcp_tx_segment_check_args;
    alignas(8) static char mem[64];
    const void *p = mem;
    const uint64_t need = aipstack_tcp_tx_segment_workspace_bytes(4);
    auto call = [&](int null_at, uint64_t stride, uint64_t nseg, uint64_t nchunk, const void *ws,
                    uint64_t ws_bytes) {
        const void *a[9];
        for (int i = 0; i < 9; ++i) a[i] = i == null_at ? nullptr : p;
        if (null_at != 8) a[8] = ws;
        return tcp_tx_segment_check_args(a[0], a[1], a[2], 1, nseg, nchunk, a[3], stride, a[4], a[5],
                                         a[6], a[7], a[8], ws_bytes);
    };
    CHECK(call(-1, 64, 4, 4, p, need) == AIPSTACK_CHKSUM_OK);
    CHECK(call(-1, 54, 4, 4, p, need) == AIPSTACK_CHKSUM_OK);
    for (int i = 0; i < 9; ++i) CHECK(call(i, 64, 4, 4, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, 53, 4, 4, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, 64, 4, 4, p, need - 1) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, 64, 4, 4, mem + 4, need + 8) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, 64, (1ull << 40) + 1, 4, p, ~0ull) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, 64, 4, (1ull << 40) + 1, p, need) == AIPSTACK_CHKSUM_EINVAL);

    if (failures) return 1;
    std::printf("tcpseg_layout_test: OK\n");
    return 0;
}
