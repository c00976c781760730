// UDP send with IPv4 fragmentation, the host code alone (aipstack_amd/csrc/ipfrag_host.cpp: the
// datagram layout and the argument checks of aipstack_udp_tx_fragment), built with ASan + UBSan
// (tests/cpp/ipfrag.mk). Descriptors, index and status arrays are heap blocks of exactly their
// size, so a write or read past them is caught.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "aipstack_amd/chksum.h"
#include "ipfrag_common.h"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static aipstack_udp_dgram good(uint32_t len0, uint32_t len1, uint16_t mtu, bool df) {
    aipstack_udp_dgram d;
    std::memset(&d, 0, sizeof d);
    d.data_addr[0] = 0x1000;
    d.data_addr[1] = 0x90000;
    d.data_len[0] = len0;
    d.data_len[1] = len1;
    d.mtu = mtu;
    d.hdr[12] = 0x08;
    d.hdr[14] = 0x45;
    d.hdr[20] = df ? 0x40 : 0;
    d.hdr[23] = 17;
    return d;
}

static int layout(const std::vector<aipstack_udp_dgram> &v, std::vector<uint64_t> &fi,
                  std::vector<uint64_t> &cb, std::vector<uint8_t> &st) {
    fi.assign(v.size() + 1, 0xDEAD);
    cb.assign(v.size() + 1, 0xDEAD);
    st.assign(v.size(), 0xEE);
    return aipstack_udp_dgram_layout(v.empty() ? nullptr : v.data(), v.size(), fi.data(), cb.data(),
                                     st.empty() ? nullptr : st.data());
}

int main() {
    std::vector<uint64_t> fi, cb;
    std::vector<uint8_t> st;
    // mtu 1500: M = F = 1480; mtu 256: M = 236, F = 232
    std::vector<aipstack_udp_dgram> v = {
        good(1472, 0, 1500, false),     // P = M: 1 fragment, 1 chunk
        good(1473, 0, 1500, false),     // P = M + 1: 2 / 2
        good(1000, 1952, 1500, false),  // P = M + F: 2 / 3 (the boundary inside fragment 0)
        good(1472, 1481, 1500, false),  // P = M + F + 1: 3 / 3 (the boundary on a fragment edge)
        good(0, 0, 1500, false),        // D = 0: 1 / 0
        good(1473, 0, 1500, true),      // DF, above the mtu: 0 / 0, FRAG_NEEDED
        good(1472, 0, 1500, true),      // DF, fits: 1 / 1
        good(65527, 0, 256, false),     // 283 fragments
        good(689, 2, 256, false),       // P = 699 = 2F + 235: 3 fragments, the clamped straddle
        good(460, 231, 256, false),     // the same sizes, the boundary inside fragment 2: 3 / 4
        good(456, 235, 256, false),     // len0 + 8 = 2F: on the edge, 3 / 3
    };
    CHECK(layout(v, fi, cb, st) == AIPSTACK_CHKSUM_OK);
    const uint64_t S[] = {1, 2, 2, 3, 1, 0, 1, 283, 3, 3, 3}, C[] = {1, 2, 3, 3, 0, 0, 1, 283, 4, 4, 3};
    uint64_t s = 0, c = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        s += S[i];
        c += C[i];
        CHECK(fi[i + 1] == s && cb[i + 1] == c);
        CHECK(st[i] == (i == 5 ? AIPSTACK_TX_FRAG_NEEDED : AIPSTACK_RX_ACCEPT));
    }
    CHECK(fi[0] == 0 && cb[0] == 0);
    {
        const aipstack_amd::UdpDgramShape sh = aipstack_amd::udp_dgram_shape(v[8]);
        CHECK(sh.valid && sh.S == 3 && sh.straddle == 2 && (sh.len0 + 8) / sh.F == 3);
        const aipstack_amd::UdpFragRange last = aipstack_amd::udp_frag_range(sh, 2);
        CHECK(last.off == 464 && last.len == 235 && last.a == 456 && last.b == 691);
        const aipstack_amd::UdpFragRange first = aipstack_amd::udp_frag_range(sh, 0);
        CHECK(first.off == 0 && first.len == 232 && first.a == 0 && first.b == 224);
    }
    v.clear();
    CHECK(layout(v, fi, cb, st) == AIPSTACK_CHKSUM_OK && fi[0] == 0 && cb[0] == 0);
    // every contract breach, in the middle of valid datagrams
    for (int cls = 0; cls < 10; ++cls) {
        aipstack_udp_dgram b = good(500, 0, 576, false);
        switch (cls) {
        case 0: b.mtu = 255; break;
        case 1: b.data_len[0] = 65000; b.data_len[1] = 528; break;
        case 2: b.reserved = 1; break;
        case 3: b.reserved = 0x80000000u; break;
        case 4: b.hdr[13] = 6; break;
        case 5: b.hdr[14] = 0x46; break;
        case 6: b.hdr[23] = 6; break;
        case 7: b.hdr[20] = 0x20; break;
        case 8: b.hdr[21] = 1; break;
        case 9: b.data_len[0] = 0xFFFFFFFFu; b.data_len[1] = 0xFFFFFFFFu; break;
        }
        v = {good(10, 0, 256, false), b, good(10, 0, 256, true)};
        CHECK(layout(v, fi, cb, st) == AIPSTACK_CHKSUM_EINVAL);
        CHECK(!aipstack_amd::udp_dgram_shape(b).valid);
    }
    v = {good(10, 0, 256, false)};
    fi.assign(2, 0);
    cb.assign(2, 0);
    CHECK(aipstack_udp_dgram_layout(nullptr, 1, fi.data(), cb.data(), nullptr) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(aipstack_udp_dgram_layout(v.data(), 1, nullptr, cb.data(), nullptr) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(aipstack_udp_dgram_layout(v.data(), 1, fi.data(), nullptr, nullptr) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(aipstack_udp_dgram_layout(v.data(), 1, fi.data(), cb.data(), nullptr) == AIPSTACK_CHKSUM_OK);

    // workspace bound
    for (uint64_t nd : {0ull, 1ull, 1000ull, 1ull << 40, ~0ull})
        for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 4097ull, 1ull << 40, ~0ull}) {
            const uint64_t w = aipstack_udp_tx_fragment_workspace_bytes(nd, n);
            const uint64_t md = nd > (1ull << 40) ? 1ull << 40 : nd, m = n > (1ull << 40) ? 1ull << 40 : n;
            CHECK(w % 8 == 0 && w >= 8 * m + 14 * md + 8 && w <= 16 * (m + md) + 256);
        }

    // the argument checks (pointers are only compared, never followed)
    using aipstack_amd::udp_tx_fragment_check_args;
    alignas(8) static char mem[64];
    const void *p = mem;
    const uint64_t need = aipstack_udp_tx_fragment_workspace_bytes(2, 4);
    auto call = [&](int null_at, uint64_t stride, uint64_t nd, uint64_t nfrag, uint64_t nchunk,
                    const void *ws, uint64_t ws_bytes) {
        const void *a[11];
        for (int i = 0; i < 11; ++i) a[i] = i == null_at ? nullptr : p;
        if (null_at != 10) a[10] = ws;
        return udp_tx_fragment_check_args(a[0], a[1], a[2], nd, nfrag, nchunk, a[3], stride, a[4], a[5],
                                          a[6], a[7], a[8], a[9], a[10], ws_bytes);
    };
    CHECK(call(-1, 64, 2, 4, 4, p, need) == AIPSTACK_CHKSUM_OK);
    CHECK(call(-1, 42, 2, 4, 4, p, need) == AIPSTACK_CHKSUM_OK);
    for (int i = 0; i < 11; ++i) CHECK(call(i, 64, 2, 4, 4, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, 41, 2, 4, 4, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, 64, 2, 4, 4, p, need - 1) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, 64, 2, 4, 4, mem + 4, need + 8) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, 64, 2, (1ull << 40) + 1, 4, p, ~0ull) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, 64, 2, 4, (1ull << 40) + 1, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, 64, (1ull << 40) + 1, 4, 4, p, ~0ull) == AIPSTACK_CHKSUM_EINVAL);

    if (failures) return 1;
    std::printf("ipfrag_layout_test: OK\n");
    return 0;
}
