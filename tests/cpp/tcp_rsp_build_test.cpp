// Stand-alone test (its own main, built under ASan + UBSan by tcp_rsp.mk, no GPU): the decision and
// the RST builder of the TCP responder (aipstack_amd/csrc/tcprsp_common.h) on top of the record
// builder of the TCP Rx parse (tcprx_common.h), as the kernels compile them, over the cases of a
// text file that tests/test_tcp_rsp_host.py writes from the reference-recorded fixture and the
// model, and the argument checks of the two entry points (tcprsp_host.cpp). Every frame lies in a
// heap block of exactly its length, and the load functor refuses a dword that is not inside it or
// beyond the first 134 bytes.
//
// One case per line:
//   <local> <bcast> <mtu> <ip_id> <ttl> <mac hex> <accepted 0|1> <has_pcb 0|1> <rst_request 0|1>
//   <ident> <status> <listener> <32 record bytes hex, or -> <frame hex, or -> <54 RST bytes hex, or ->
//   <n listeners> then <addr> <port> <cookie> per listener, in table order
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
#include "tcprsp_common.h"

using namespace aipstack_amd;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++failures;                                                 \
        }                                                               \
    } while (0)

struct HeapLoad {
    const uint8_t *p;
    uint32_t len;
    uint32_t operator()(uint32_t off) const {
        if ((uint64_t)off + 4u > len || off + 4u > 134u) {
            std::printf("FAIL: load of [%u, %u) of a frame of %u bytes\n", off, off + 4u, len);
            std::abort();
        }
        uint32_t w;
        std::memcpy(&w, p + off, 4);
        return w;
    }
};

struct VectorListeners {
    const std::vector<TcpRspLis> *lis;
    bool operator()(uint32_t dst, uint32_t port, uint32_t &cookie) const {
        for (const TcpRspLis &l : *lis)
            if (l.port == port && (l.addr == dst || l.addr == 0u)) {
                cookie = l.cookie;
                return true;
            }
        return false;
    }
};

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
        unsigned long local, bcast, mtu, ip_id, ttl, accepted, has_pcb, req, ident, status, listener, nlis;
        std::string mac, rec_hex, frame_hex, slot_hex;
        s >> local >> bcast >> mtu >> ip_id >> ttl >> mac >> accepted >> has_pcb >> req >> ident >>
            status >> listener >> rec_hex >> frame_hex >> slot_hex >> nlis;
        if (!s) continue;
        std::vector<TcpRspLis> lis(nlis);
        for (TcpRspLis &l : lis) {
            unsigned long a, p, c;
            s >> a >> p >> c;
            l = TcpRspLis{(uint32_t)a, (uint32_t)p, (uint32_t)c};
        }
        CHECK((bool)s);
        aipstack_icmp_iface hf;
        std::memset(&hf, 0, sizeof(hf));
        hf.local_addr = (uint32_t)local;
        hf.bcast_addr = (uint32_t)bcast;
        hf.mtu = (uint16_t)mtu;
        hf.ip_id = (uint16_t)ip_id;
        hf.ttl = 1;  // the ICMP TTL: not used
        const std::vector<uint8_t> m = unhex(mac);
        std::memcpy(hf.mac, m.data(), 6);
        CHECK(icmp_iface_valid(hf));
        const TcpRspIface f = tcp_rsp_iface_of(hf, (uint32_t)ttl);
        const std::vector<uint8_t> bytes = unhex(frame_hex);
        std::unique_ptr<uint8_t[]> block(new uint8_t[bytes.size() ? bytes.size() : 1]);
        if (!bytes.empty()) std::memcpy(block.get(), bytes.data(), bytes.size());
        const HeapLoad ld{block.get(), (uint32_t)bytes.size()};
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        aipstack_tcp_pcb_key key;
        TcpRspPlan p{AIPSTACK_TCP_RSP_NONE, AIPSTACK_TCP_NO_LISTENER};
        const bool valid = accepted != 0 && tcp_rx_build(ld, ld.len, w, key) == kTcpRxValid;
        CHECK(valid == (rec_hex != "-"));
        if (valid) {
            const std::vector<uint8_t> want_rec = unhex(rec_hex);
            CHECK(want_rec.size() == sizeof(aipstack_tcp_rx_seg));
            if (want_rec.size() != 32 || std::memcmp(w, want_rec.data(), 32) != 0) {
                std::printf("FAIL: record of case %d differs\n", n);
                ++failures;
            }
            p = tcp_rsp_decide(w, has_pcb != 0, req != 0, f, VectorListeners{&lis});
        }
        if (p.status != status || p.listener != (uint32_t)listener) {
            std::printf("FAIL: case %d: status %u listener %u, want %lu %lu\n", n, p.status, p.listener,
                        status, listener);
            ++failures;
        }
        CHECK(p.rst() == (slot_hex != "-"));
        CHECK(!(p.rst() && p.syn()));
        if (p.rst() && slot_hex != "-") {
            uint32_t o[16];
            tcp_rsp_build_rst(w, ld(4u), ld(8u), f.ip_id + (uint32_t)ident, f, o);
            uint8_t img[64];
            std::memcpy(img, o, 64);
            const std::vector<uint8_t> want = unhex(slot_hex);
            CHECK(want.size() == AIPSTACK_TCP_RSP_HEADER);
            if (want.size() != 54 || std::memcmp(img, want.data(), 54) != 0) {
                std::printf("FAIL: RST of case %d differs\n", n);
                ++failures;
            }
            for (int k = AIPSTACK_TCP_RSP_HEADER; k < 64; ++k) CHECK(img[k] == 0);
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
    const uint64_t n = 600, need = aipstack_tcp_rx_respond_workspace_bytes(n);
    CHECK(need == 16u * 4u + 64u * 3u);
    CHECK(aipstack_tcp_rx_respond_workspace_bytes(0) == 16u);
    CHECK(aipstack_tcp_rx_respond_workspace_bytes(256) == 32u + 64u);
    CHECK(aipstack_tcp_rx_respond_workspace_bytes(257) == 48u + 128u);
    const TcpRespondArgs good{buf, buf, true, 2048, n,   &f,  64,  buf, 10,  buf, 256, buf,  buf,
                              buf, buf, buf,  buf,  64,  buf, buf, buf, buf, buf, buf, need};
    CHECK(tcp_rx_respond_check_args(good) == AIPSTACK_CHKSUM_OK);
    auto bad = [&](auto change) {
        TcpRespondArgs a = good;
        aipstack_icmp_iface g = f;
        a.h_iface = &g;
        change(a, g);
        CHECK(tcp_rx_respond_check_args(a) == AIPSTACK_CHKSUM_EINVAL);
    };
    using A = TcpRespondArgs;
    using I = aipstack_icmp_iface;
    bad([](A &a, I &) { a.d_base = nullptr; });
    bad([](A &a, I &) { a.frames = nullptr; });
    bad([](A &a, I &) { a.h_iface = nullptr; });
    bad([](A &a, I &) { a.d_pcbs = nullptr; });
    bad([](A &a, I &) { a.d_listeners = nullptr; });
    bad([](A &a, I &) { a.d_verdict = nullptr; });
    bad([](A &a, I &) { a.d_segs = nullptr; });
    bad([](A &a, I &) { a.d_pcb = nullptr; });
    bad([](A &a, I &) { a.d_status = nullptr; });
    bad([](A &a, I &) { a.d_listener = nullptr; });
    bad([](A &a, I &) { a.d_hdr = nullptr; });
    bad([](A &a, I &) { a.d_hdr_len = nullptr; });
    bad([](A &a, I &) { a.d_chunk_index = nullptr; });
    bad([](A &a, I &) { a.d_response_frame = nullptr; });
    bad([](A &a, I &) { a.d_syn_frame = nullptr; });
    bad([](A &a, I &) { a.d_counts = nullptr; });
    bad([](A &a, I &) { a.d_workspace = nullptr; });
    bad([](A &a, I &) { a.hdr_stride = 53; });
    bad([](A &a, I &) { a.tcp_ttl = 0; });
    bad([](A &a, I &) { a.tcp_ttl = 256; });
    bad([](A &a, I &) { a.n_listeners = 257; });
    bad([](A &a, I &) { a.n_pcbs = (1ull << 40) + 1; });
    bad([](A &, I &g) { g.mtu = 255; });
    bad([](A &, I &g) { g.flags = 2; });
    bad([](A &, I &g) { g.reserved[11] = 1; });
    bad([](A &a, I &) { a.n = (1ull << 40) + 1; a.workspace_bytes = ~0ull; });
    bad([](A &a, I &) { a.workspace_bytes -= 1; });
    bad([](A &a, I &) { a.d_workspace = buf + 4; });
    bad([](A &a, I &) { a.d_segs = buf + 4; });
    bad([](A &a, I &) { a.d_pcbs = buf + 4; });
    bad([](A &a, I &) { a.d_listeners = buf + 4; });
    bad([](A &a, I &) { a.d_chunk_index = buf + 4; });
    bad([](A &a, I &) { a.d_response_frame = buf + 4; });
    bad([](A &a, I &) { a.d_syn_frame = buf + 4; });
    bad([](A &a, I &) { a.d_counts = buf + 4; });
    bad([](A &a, I &) { a.d_hdr_len = buf + 2; });
    bad([](A &a, I &) { a.d_pcb = buf + 2; });
    bad([](A &a, I &) { a.d_listener = buf + 2; });
    bad([](A &a, I &) { a.slot_stride = 0; });
    bad([](A &a, I &) { a.slot_stride = 65537; });
    A csr = good;  // the CSR form does not look at the stride
    csr.slotted = false;
    csr.slot_stride = 0;
    CHECK(tcp_rx_respond_check_args(csr) == AIPSTACK_CHKSUM_OK);
    A edge = good;  // no tables, the smallest stride, the bounds themselves
    edge.d_pcbs = edge.d_listeners = nullptr;
    edge.n_pcbs = 0;
    edge.n_listeners = 0;
    edge.hdr_stride = 54;
    edge.tcp_ttl = 255;
    f.mtu = 256;
    f.flags = AIPSTACK_ICMP_ALLOW_BROADCAST_PING;
    edge.n = 1ull << 40;
    edge.workspace_bytes = aipstack_tcp_rx_respond_workspace_bytes(edge.n);
    CHECK(tcp_rx_respond_check_args(edge) == AIPSTACK_CHKSUM_OK);
    edge.tcp_ttl = 1;
    edge.n_listeners = 256;
    edge.d_listeners = buf + 8;
    CHECK(tcp_rx_respond_check_args(edge) == AIPSTACK_CHKSUM_OK);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::printf("usage: tcp_rsp_build_test <cases file>\n");
        return 2;
    }
    const int n = run_cases(argv[1]);
    CHECK(n > 0);
    arg_checks();
    if (failures) return 1;
    std::printf("OK %d cases\n", n);
    return 0;
}
