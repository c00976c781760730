// Stand-alone test (its own main, built under ASan + UBSan by tcp_ctl.mk, no GPU): the validity
// rule and the builder of the TCP segments without data (aipstack_amd/csrc/tcpctl_common.h), as
// the kernels compile them, over the cases of a text file that tests/test_tcp_ctl_host.py writes
// from the reference-recorded fixture and the model, and the argument checks of the entry point
// (tcpctl_host.cpp). Every descriptor lies in a heap block of exactly its 32 bytes.
//
// One case per line:
//   <mac hex> <ip_id> <ttl> <rank> <32 descriptor bytes hex> <valid 0|1> <header bytes hex, or ->
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "aipstack_amd/chksum.h"
#include "icmp_common.h"
#include "tcpctl_common.h"

using namespace aipstack_amd;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static std::vector<uint8_t> unhex(const std::string &h) {
    if (h == "-") return {};
    std::vector<uint8_t> v(h.size() / 2);
    for (size_t k = 0; k < v.size(); ++k) v[k] = (uint8_t)std::stoul(h.substr(2 * k, 2), nullptr, 16);
    return v;
}

static int run_cases(const char *path) {
    std::ifstream in(path);
    std::string line;
    int n = 0;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        unsigned long ip_id, ttl, rank, valid;
        std::string mac, ctl_hex, hdr_hex;
        s >> mac >> ip_id >> ttl >> rank >> ctl_hex >> valid >> hdr_hex;
        if (!s) continue;
        aipstack_icmp_iface hf;
        std::memset(&hf, 0, sizeof(hf));
        hf.mtu = 1500;
        hf.ip_id = (uint16_t)ip_id;
        hf.ttl = 1;  // the ICMP TTL: not used
        const std::vector<uint8_t> m = unhex(mac);
        CHECK(m.size() == 6);
        std::memcpy(hf.mac, m.data(), 6);
        CHECK(icmp_iface_valid(hf));
        const TcpRspIface f = tcp_rsp_iface_of(hf, (uint32_t)ttl);
        const std::vector<uint8_t> bytes = unhex(ctl_hex);
        CHECK(bytes.size() == sizeof(aipstack_tcp_ctl));
        std::unique_ptr<uint8_t[]> block(new uint8_t[32]);
        std::memcpy(block.get(), bytes.data(), 32);
        uint32_t d[8];
        std::memcpy(d, block.get(), 32);
        const bool ok = tcp_ctl_valid(d[6], d[7]);
        if (ok != (valid != 0)) {
            std::printf("FAIL: case %d: valid %d, want %lu\n", n, (int)ok, valid);
            ++failures;
        }
        CHECK(ok == (hdr_hex != "-"));
        if (ok && hdr_hex != "-") {
            uint32_t o[16];
            std::memset(o, 0xA5, sizeof(o));
            const uint32_t hl = tcp_ctl_build(d, f.ip_id + (uint32_t)rank, f, o);
            uint8_t img[64];
            std::memcpy(img, o, 64);
            const std::vector<uint8_t> want = unhex(hdr_hex);
            CHECK(hl == want.size() && hl == tcp_ctl_header_len(d[6]));
            CHECK(hl == 54 || hl == 58 || hl == 62);
            if (hl != want.size() || std::memcmp(img, want.data(), hl) != 0) {
                std::printf("FAIL: header of case %d differs\n", n);
                ++failures;
            }
            for (uint32_t k = hl; k < 64; ++k) CHECK(img[k] == 0);
        }
        ++n;
    }
    return n;
}

static void arg_checks() {
    alignas(16) static uint8_t buf[256];
    aipstack_icmp_iface f;
    std::memset(&f, 0, sizeof(f));
    f.mtu = 1500;
    const uint64_t n = 600, need = aipstack_tcp_tx_control_workspace_bytes(n);
    CHECK(need == 16u * 4u + 32u * 3u);
    CHECK(aipstack_tcp_tx_control_workspace_bytes(0) == 16u);
    CHECK(aipstack_tcp_tx_control_workspace_bytes(256) == 32u + 32u);
    CHECK(aipstack_tcp_tx_control_workspace_bytes(257) == 48u + 64u);
    const TcpControlArgs good{buf, n, &f, 64, buf, 64, buf, buf, buf, buf, buf, need};
    CHECK(tcp_tx_control_check_args(good) == AIPSTACK_CHKSUM_OK);
    auto bad = [&](auto change) {
        TcpControlArgs a = good;
        aipstack_icmp_iface g = f;
        a.h_iface = &g;
        change(a, g);
        CHECK(tcp_tx_control_check_args(a) == AIPSTACK_CHKSUM_EINVAL);
    };
    using A = TcpControlArgs;
    using I = aipstack_icmp_iface;
    bad([](A &a, I &) { a.d_ctl = nullptr; });
    bad([](A &a, I &) { a.h_iface = nullptr; });
    bad([](A &a, I &) { a.d_hdr = nullptr; });
    bad([](A &a, I &) { a.d_hdr_len = nullptr; });
    bad([](A &a, I &) { a.d_chunk_index = nullptr; });
    bad([](A &a, I &) { a.d_status = nullptr; });
    bad([](A &a, I &) { a.d_counts = nullptr; });
    bad([](A &a, I &) { a.d_workspace = nullptr; });
    bad([](A &a, I &) { a.hdr_stride = 61; });
    bad([](A &a, I &) { a.hdr_stride = 54; });
    bad([](A &a, I &) { a.hdr_stride = 0; });
    bad([](A &a, I &) { a.tcp_ttl = 0; });
    bad([](A &a, I &) { a.tcp_ttl = 256; });
    bad([](A &, I &g) { g.mtu = 255; });
    bad([](A &, I &g) { g.flags = 2; });
    bad([](A &, I &g) { g.reserved[0] = 1; });
    bad([](A &, I &g) { g.reserved[11] = 1; });
    bad([](A &a, I &) { a.n = (1ull << 40) + 1; a.workspace_bytes = ~0ull; });
    bad([](A &a, I &) { a.workspace_bytes -= 1; });
    bad([](A &a, I &) { a.d_workspace = buf + 4; });
    bad([](A &a, I &) { a.d_ctl = buf + 4; });
    bad([](A &a, I &) { a.d_chunk_index = buf + 4; });
    bad([](A &a, I &) { a.d_counts = buf + 4; });
    bad([](A &a, I &) { a.d_hdr_len = buf + 2; });
    A edge = good;  // the bounds themselves; the ring and the status bytes at any alignment
    edge.hdr_stride = 62;
    edge.tcp_ttl = 255;
    edge.d_hdr = buf + 1;
    edge.d_status = buf + 3;
    edge.d_hdr_len = buf + 4;
    edge.d_ctl = buf + 8;
    f.mtu = 256;
    f.flags = AIPSTACK_ICMP_ALLOW_BROADCAST_PING;
    edge.n = 1ull << 40;
    edge.workspace_bytes = aipstack_tcp_tx_control_workspace_bytes(edge.n);
    CHECK(tcp_tx_control_check_args(edge) == AIPSTACK_CHKSUM_OK);
    edge.tcp_ttl = 1;
    CHECK(tcp_tx_control_check_args(edge) == AIPSTACK_CHKSUM_OK);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::printf("usage: tcp_ctl_build_test <cases file>\n");
        return 2;
    }
    const int n = run_cases(argv[1]);
    CHECK(n > 0);
    arg_checks();
    if (failures) return 1;
    std::printf("OK %d cases\n", n);
    return 0;
}
