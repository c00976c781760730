// TCP Rx parse, the host code alone (aipstack_amd/csrc/tcprx_host.cpp: the PCB table's sort and
// the argument checks of aipstack_tcp_rx_parse / _slotted), built with ASan + UBSan
// (tests/cpp/tcprx.mk). Tables are heap blocks of exactly n entries, so a read or write past
// them is caught. The shared header's option machine and record builder run here too, on frames
// held in heap blocks of exactly their length.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "aipstack_amd/chksum.h"
#include "tcprx_common.h"

using namespace aipstack_amd;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static aipstack_tcp_pcb_key key(uint32_t la, uint32_t ra, uint16_t lp, uint16_t rp, uint32_t cookie) {
    aipstack_tcp_pcb_key k;
    k.local_addr = la;
    k.remote_addr = ra;
    k.local_port = lp;
    k.remote_port = rp;
    k.cookie = cookie;
    return k;
}

static bool sorted_unique(const std::vector<aipstack_tcp_pcb_key> &v) {
    for (size_t i = 1; i < v.size(); ++i)
        if (tcp_pcb_key_compare(v[i - 1], v[i]) >= 0) return false;
    return true;
}

static uint64_t cookie_sum(const std::vector<aipstack_tcp_pcb_key> &v) {
    uint64_t s = 0;
    for (const auto &k : v) s += (uint64_t)k.cookie * 2654435761u + k.remote_port + k.local_addr;
    return s;
}

static int sort(std::vector<aipstack_tcp_pcb_key> &v) {
    return aipstack_tcp_pcb_table_sort(v.empty() ? nullptr : v.data(), v.size());
}

struct FrameBytes {
    const std::vector<unsigned char> *f;
    uint32_t operator()(uint32_t off) const {
        uint32_t w;
        std::memcpy(&w, f->data() + off, 4);   // past the block: ASan reports it
        return w;
    }
};

int main() {
    // the order: remote_port, remote_addr, local_port, local_addr; the cookie takes no part
    CHECK(tcp_pcb_key_compare(key(9, 9, 9, 1, 0), key(0, 0, 0, 2, 0)) == -1);
    CHECK(tcp_pcb_key_compare(key(9, 1, 9, 5, 0), key(0, 2, 0, 5, 0)) == -1);
    CHECK(tcp_pcb_key_compare(key(9, 7, 1, 5, 0), key(0, 7, 2, 5, 0)) == -1);
    CHECK(tcp_pcb_key_compare(key(1, 7, 3, 5, 0), key(2, 7, 3, 5, 0)) == -1);
    CHECK(tcp_pcb_key_compare(key(2, 7, 3, 5, 0), key(1, 7, 3, 5, 0)) == 1);
    CHECK(tcp_pcb_key_compare(key(1, 7, 3, 5, 4), key(1, 7, 3, 5, 8)) == 0);
    CHECK(tcp_pcb_key_compare(key(0, 0x80000000u, 0, 0, 0), key(0, 0x7FFFFFFFu, 0, 0, 0)) == 1);

    std::vector<aipstack_tcp_pcb_key> v;
    CHECK(sort(v) == AIPSTACK_CHKSUM_OK);                                   // empty
    CHECK(aipstack_tcp_pcb_table_sort(nullptr, 1) == AIPSTACK_CHKSUM_EINVAL);
    v = {key(1, 2, 3, 4, 5)};
    CHECK(sort(v) == AIPSTACK_CHKSUM_OK && v[0].cookie == 5);               // single
    v = {key(1, 2, 3, 4, AIPSTACK_TCP_NO_PCB)};
    CHECK(sort(v) == AIPSTACK_CHKSUM_EINVAL);                               // bad cookie
    v.clear();
    for (uint32_t i = 0; i < 100; ++i) v.push_back(key(i % 3, i % 7, (uint16_t)(i % 5), (uint16_t)(i / 4), i));
    std::vector<aipstack_tcp_pcb_key> w = v;
    CHECK(sort(v) == AIPSTACK_CHKSUM_OK && sorted_unique(v) && cookie_sum(v) == cookie_sum(w));
    w = v;
    CHECK(sort(v) == AIPSTACK_CHKSUM_OK && std::memcmp(v.data(), w.data(), 16 * v.size()) == 0);   // sorted
    std::reverse(v.begin(), v.end());
    CHECK(sort(v) == AIPSTACK_CHKSUM_OK && std::memcmp(v.data(), w.data(), 16 * v.size()) == 0);   // reversed
    v.push_back(key(w[40].local_addr, w[40].remote_addr, w[40].local_port, w[40].remote_port, 777));
    const uint64_t before = cookie_sum(v);
    CHECK(sort(v) == AIPSTACK_CHKSUM_EINVAL && cookie_sum(v) == before);    // duplicate: a permutation
    v = w;
    v[99].cookie = AIPSTACK_TCP_NO_PCB;
    CHECK(sort(v) == AIPSTACK_CHKSUM_EINVAL);
    // 10,000 random keys (duplicates removed by the model first)
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    v.clear();
    for (uint32_t i = 0; i < 10000; ++i)
        v.push_back(key((uint32_t)rnd() % 4, (uint32_t)rnd(), (uint16_t)(rnd() % 3), (uint16_t)(rnd() % 200), i));
    std::vector<aipstack_tcp_pcb_key> m = v;
    std::stable_sort(m.begin(), m.end(), [](const aipstack_tcp_pcb_key &a, const aipstack_tcp_pcb_key &b) {
        if (a.remote_port != b.remote_port) return a.remote_port < b.remote_port;
        if (a.remote_addr != b.remote_addr) return a.remote_addr < b.remote_addr;
        if (a.local_port != b.local_port) return a.local_port < b.local_port;
        return a.local_addr < b.local_addr;
    });
    CHECK(sorted_unique(m));   // (32 random address bits: no duplicate among 10,000)
    CHECK(sort(v) == AIPSTACK_CHKSUM_OK && std::memcmp(v.data(), m.data(), 16 * v.size()) == 0);

    // the option machine on the branches of ParseTcpOptions
    struct { std::vector<unsigned char> b; uint32_t opts, mss, ws; } oc[] = {
        {{}, 0, 0, 0},
        {{2, 4, 5, 0xB4, 1, 3, 3, 7}, 3, 1460, 7},
        {{3, 3, 7, 0, 2, 4, 5, 0xB4}, 2, 0, 7},            // End stops
        {{2, 4, 5, 0xB4, 3}, 1, 1460, 0},                  // no length byte left: the flag stays
        {{2, 1, 5, 0xB4}, 0, 0, 0},                        // length below 2
        {{2, 4, 5}, 0, 0, 0},                              // data beyond the bytes left
        {{2, 3, 9, 2, 4, 5, 0xB4}, 1, 1460, 0},            // wrong length: skipped
        {{3, 4, 9, 9, 3, 3, 2}, 2, 0, 2},
        {{8, 10, 1, 2, 3, 4, 5, 6, 7, 8, 2, 4, 1, 0}, 1, 256, 0},
        {{2, 4, 5, 0xB4, 2, 4, 2, 0x18, 3, 3, 1, 3, 3, 14}, 3, 536, 14},   // later ones override
    };
    for (const auto &c : oc) {
        std::vector<unsigned char> padded = c.b;
        while (padded.size() % 4) padded.push_back(0x55);   // never read: past n
        TcpOptParser p;
        for (uint32_t q = 0; 4 * q < c.b.size(); ++q) {
            uint32_t word;
            std::memcpy(&word, padded.data() + 4 * q, 4);
            if (p.live()) p.dword(word, 4 * q, (uint32_t)c.b.size());
        }
        CHECK(p.opts == c.opts && p.mss == c.mss && p.wnd_scale == c.ws);
    }

    // the record builder on frames of exactly their length: IHL 15, offset 15, no data (134
    // bytes, the last option byte is the frame's last), and a bad offset
    {
        std::vector<unsigned char> f(134, 1);
        f[12] = 0x08; f[13] = 0x00; f[14] = 0x4F; f[16] = 0; f[17] = 120; f[23] = 6;
        const unsigned char addr[8] = {10, 0, 0, 1, 10, 0, 0, 2};
        std::memcpy(&f[26], addr, 8);
        unsigned char *t = &f[74];
        t[0] = 0x9C; t[1] = 0x40; t[2] = 0; t[3] = 80;
        t[4] = 1; t[5] = 2; t[6] = 3; t[7] = 4; t[8] = 5; t[9] = 6; t[10] = 7; t[11] = 8;
        t[12] = 0xF0; t[13] = 0x18; t[14] = 0x20; t[15] = 0x00;
        f[130] = 2; f[131] = 4; f[132] = 0x02; f[133] = 0x18;
        uint32_t w[8];
        aipstack_tcp_pcb_key k;
        CHECK(tcp_rx_build(FrameBytes{&f}, (uint32_t)f.size(), w, k) == kTcpRxValid);
        aipstack_tcp_rx_seg s;
        std::memcpy(&s, w, 32);
        CHECK(s.remote_addr == 0x0A000001u && s.local_addr == 0x0A000002u && s.remote_port == 40000 &&
              s.local_port == 80 && s.seq_num == 0x01020304u && s.ack_num == 0x05060708u &&
              s.flags == 0xF018 && s.window_size == 0x2000 && s.data_off == 134 && s.data_len == 0 &&
              s.mss == 536 && s.wnd_scale == 0 && s.opts == (AIPSTACK_TCP_SEG_VALID | AIPSTACK_TCP_OPT_MSS));
        CHECK(k.local_addr == s.local_addr && k.remote_addr == s.remote_addr && k.local_port == 80 &&
              k.remote_port == 40000);
        f[17] = 116;   // the datagram is 56 bytes: offset 60 is beyond it
        f.resize(130);
        CHECK(tcp_rx_build(FrameBytes{&f}, (uint32_t)f.size(), w, k) == kTcpRxBadOffset);
        f[86] = 0x40;  // offset 4
        CHECK(tcp_rx_build(FrameBytes{&f}, (uint32_t)f.size(), w, k) == kTcpRxBadOffset);
        f[23] = 17;
        CHECK(tcp_rx_build(FrameBytes{&f}, (uint32_t)f.size(), w, k) == kTcpRxNotTcp);
        f.resize(40);
        CHECK(tcp_rx_build(FrameBytes{&f}, (uint32_t)f.size(), w, k) == kTcpRxNotTcp);
    }

    // the argument checks (pointers are only compared, never followed)
    alignas(16) static char mem[64];
    const void *p = mem;
    auto call = [&](int null_at, bool slotted, uint64_t stride, uint64_t n, uint64_t np,
                    const void *segs, const void *pcb, const void *tbl) {
        const void *a[3];
        for (int i = 0; i < 3; ++i) a[i] = i == null_at ? nullptr : p;
        return tcp_rx_parse_check_args(a[0], a[1], slotted, stride, n, tbl, np, a[2], segs, pcb);
    };
    CHECK(call(-1, false, 0, 4, 2, p, p, p) == AIPSTACK_CHKSUM_OK);
    CHECK(call(-1, false, 0, 4, 0, p, p, nullptr) == AIPSTACK_CHKSUM_OK);
    CHECK(call(-1, true, 2048, 4, 2, mem + 8, mem + 4, mem + 8) == AIPSTACK_CHKSUM_OK);
    CHECK(call(-1, true, 65536, 4, 2, p, p, p) == AIPSTACK_CHKSUM_OK);
    for (int i = 0; i < 3; ++i) CHECK(call(i, false, 0, 4, 2, p, p, p) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, false, 0, 4, 2, nullptr, p, p) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, false, 0, 4, 2, p, nullptr, p) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, false, 0, 4, 2, p, p, nullptr) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, false, 0, 4, 2, mem + 4, p, p) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, false, 0, 4, 2, p, mem + 2, p) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, false, 0, 4, 2, p, p, mem + 4) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, false, 0, (1ull << 40) + 1, 2, p, p, p) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, false, 0, 4, (1ull << 40) + 1, p, p, p) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, true, 0, 4, 2, p, p, p) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(-1, true, 65537, 4, 2, p, p, p) == AIPSTACK_CHKSUM_EINVAL);

    if (failures) return 1;
    std::printf("tcprx_table_test: OK\n");
    return 0;
}
