// Stand-alone test (its own main, built under ASan + UBSan by icmp.mk, no GPU): the decision and
// the slot builder of the ICMP responder (aipstack_amd/csrc/icmp_common.h), as the kernels
// compile them, over the cases of a text file that tests/test_icmp_host.py writes from the
// reference-recorded fixture and the model, and the argument checks of the two entry points
// (icmp_host.cpp). Every frame lies in a heap block of exactly its length, and the load functor
// refuses a dword that is not inside it.
//
// One case per line:
//   <local> <bcast> <mtu> <ttl> <flags> <mac hex> <verdict> <code> <ident> <status> <data_off>
//   <data_len> <frame hex, or - for an empty frame> <42 header bytes hex, or ->
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
        if ((uint64_t)off + 4u > len) {
            std::printf("FAIL: load of [%u, %u) outside a frame of %u bytes\n", off, off + 4u, len);
            std::abort();
        }
        uint32_t w;
        std::memcpy(&w, p + off, 4);
        return w;
    }
};

static std::vector<uint8_t> unhex(const std::string &h) {
    if (h == "-") return {};  // a frame of no bytes at all
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
        unsigned long local, bcast, mtu, ttl, flags, verdict, code, ident, status, data_off, data_len;
        std::string mac, frame_hex, slot_hex;
        s >> local >> bcast >> mtu >> ttl >> flags >> mac >> verdict >> code >> ident >> status >>
            data_off >> data_len >> frame_hex >> slot_hex;
        if (!s) continue;
        aipstack_icmp_iface hf;
        std::memset(&hf, 0, sizeof(hf));
        hf.local_addr = (uint32_t)local;
        hf.bcast_addr = (uint32_t)bcast;
        hf.mtu = (uint16_t)mtu;
        hf.ttl = (uint8_t)ttl;
        hf.flags = (uint8_t)flags;
        const std::vector<uint8_t> m = unhex(mac);
        std::memcpy(hf.mac, m.data(), 6);
        const IcmpIface f = icmp_iface_of(hf);
        const std::vector<uint8_t> bytes = unhex(frame_hex);
        std::unique_ptr<uint8_t[]> block(new uint8_t[bytes.size()]);  // exactly the frame
        if (!bytes.empty()) std::memcpy(block.get(), bytes.data(), bytes.size());
        const HeapLoad ld{block.get(), (uint32_t)bytes.size()};
        const IcmpPlan p = icmp_decide(ld, ld.len, (uint32_t)verdict, (uint32_t)code, f);
        CHECK(p.status == status);
        if (status != AIPSTACK_ICMP_NONE) CHECK(p.data_off == data_off && p.data_len == data_len);
        CHECK(p.responds() == (slot_hex != "-"));
        if (p.responds() && slot_hex != "-") {
            uint32_t o[16];
            icmp_build_slot(ld, p, (uint32_t)code, (uint32_t)ident, f, o);
            uint8_t img[64];
            std::memcpy(img, o, 64);
            const std::vector<uint8_t> want = unhex(slot_hex);
            CHECK(want.size() == AIPSTACK_ICMP_RESPONSE_HEADER);
            if (std::memcmp(img, want.data(), want.size()) != 0) {
                std::printf("FAIL: slot of case %d differs\n", n);
                ++failures;
            }
            for (int k = AIPSTACK_ICMP_RESPONSE_HEADER; k < 64; ++k) CHECK(img[k] == 0);
            // the Ident wraps at 2^16, whatever the caller's sum holds above it
            uint32_t o2[16];
            icmp_build_slot(ld, p, (uint32_t)code, (uint32_t)ident + 0x30000u, f, o2);
            CHECK(std::memcmp(o, o2, 64) == 0);
        }
        // every verdict that is no acceptance: nothing, and nothing read
        for (uint32_t v : {0u, 1u, 2u, 3u, 4u, 5u, 11u, 14u, 15u}) {
            const HeapLoad none{block.get(), 0};
            CHECK(icmp_decide(none, 0, v, (uint32_t)code, f).status == AIPSTACK_ICMP_NONE);
        }
        // a frame cut short behind any byte is never read past its end
        for (uint32_t cut = 0; cut < ld.len && cut < 96; ++cut) {
            std::unique_ptr<uint8_t[]> part(new uint8_t[cut ? cut : 1]);
            std::memcpy(part.get(), bytes.data(), cut);
            const HeapLoad pl{part.get(), cut};
            const IcmpPlan q = icmp_decide(pl, cut, (uint32_t)verdict, (uint32_t)code, f);
            if (q.responds()) {
                uint32_t o[16];
                icmp_build_slot(pl, q, (uint32_t)code, 1u, f, o);
                CHECK(q.data_off + q.data_len <= cut);
            }
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
    const uint64_t n = 600, need = aipstack_icmp_rx_respond_workspace_bytes(n);
    CHECK(need == 16u * 4u);
    CHECK(aipstack_icmp_rx_respond_workspace_bytes(0) == 16u);
    CHECK(aipstack_icmp_rx_respond_workspace_bytes(256) == 32u);
    CHECK(aipstack_icmp_rx_respond_workspace_bytes(257) == 48u);
    const IcmpRespondArgs good{buf, buf, true, 2048, n, &f, buf, buf, buf, 64, buf, buf, buf, buf, buf,
                               buf, buf, need};
    CHECK(icmp_rx_respond_check_args(good) == AIPSTACK_CHKSUM_OK);
    auto bad = [&](auto change) {
        IcmpRespondArgs a = good;
        aipstack_icmp_iface g = f;
        a.h_iface = &g;
        change(a, g);
        CHECK(icmp_rx_respond_check_args(a) == AIPSTACK_CHKSUM_EINVAL);
    };
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_base = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.frames = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.h_iface = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_verdict = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_status = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_hdr = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_hdr_len = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_chunk_addr = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_chunk_len = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_chunk_index = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_response_frame = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_counts = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_workspace = nullptr; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.hdr_stride = 41; });
    bad([](IcmpRespondArgs &, aipstack_icmp_iface &g) { g.mtu = 255; });
    bad([](IcmpRespondArgs &, aipstack_icmp_iface &g) { g.flags = 2; });
    bad([](IcmpRespondArgs &, aipstack_icmp_iface &g) { g.flags = 0x81; });
    bad([](IcmpRespondArgs &, aipstack_icmp_iface &g) { g.reserved[0] = 1; });
    bad([](IcmpRespondArgs &, aipstack_icmp_iface &g) { g.reserved[11] = 1; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.n = (1ull << 40) + 1; a.workspace_bytes = ~0ull; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.workspace_bytes -= 1; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_workspace = buf + 4; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_chunk_addr = buf + 4; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_chunk_index = buf + 4; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_response_frame = buf + 4; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_counts = buf + 4; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_hdr_len = buf + 2; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.d_chunk_len = buf + 2; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.slot_stride = 0; });
    bad([](IcmpRespondArgs &a, aipstack_icmp_iface &) { a.slot_stride = 65537; });
    IcmpRespondArgs csr = good;  // the CSR form does not look at the stride
    csr.slotted = false;
    csr.slot_stride = 0;
    CHECK(icmp_rx_respond_check_args(csr) == AIPSTACK_CHKSUM_OK);
    IcmpRespondArgs edge = good;
    f.mtu = 256;
    f.flags = AIPSTACK_ICMP_ALLOW_BROADCAST_PING;
    edge.hdr_stride = 42;
    edge.n = 1ull << 40;
    edge.workspace_bytes = aipstack_icmp_rx_respond_workspace_bytes(edge.n);
    CHECK(icmp_rx_respond_check_args(edge) == AIPSTACK_CHKSUM_OK);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::printf("usage: icmp_build_test <cases file>\n");
        return 2;
    }
    const int n = run_cases(argv[1]);
    CHECK(n > 0);
    arg_checks();
    if (failures) return 1;
    std::printf("OK %d cases\n", n);
    return 0;
}
