// Stand-alone test (its own main, built under ASan + UBSan by arp.mk, no GPU): the record and the
// reply builder of ARP on receive (aipstack_amd/csrc/arp_common.h), as the kernels compile them,
// over the cases of a text file that tests/test_arp_host.py writes from the reference-recorded
// fixture and the model, and the argument checks of the two entry points (arp_host.cpp). Every
// frame lies in a heap block of exactly its length, and the load functor refuses a dword that is
// not inside it.
//
// One case per line:
//   <local> <netmask> <flags> <mac hex> <16 record bytes hex> <frame hex, or - for an empty frame>
//   <42 reply bytes hex, or ->
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
#include "arp_common.h"

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
        if ((uint64_t)off + 4u > len || off + 4u > 42u) {
            std::printf("FAIL: load of [%u, %u) of a frame of %u bytes\n", off, off + 4u, len);
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
        unsigned long local, mask, flags;
        std::string mac, rec_hex, frame_hex, slot_hex;
        s >> local >> mask >> flags >> mac >> rec_hex >> frame_hex >> slot_hex;
        if (!s) continue;
        aipstack_arp_iface hf;
        std::memset(&hf, 0, sizeof(hf));
        hf.local_addr = (uint32_t)local;
        hf.netmask = (uint32_t)mask;
        hf.flags = (uint8_t)flags;
        const std::vector<uint8_t> m = unhex(mac);
        std::memcpy(hf.mac, m.data(), 6);
        CHECK(arp_iface_valid(hf));
        const ArpIface f = arp_iface_of(hf);
        const std::vector<uint8_t> bytes = unhex(frame_hex);
        std::unique_ptr<uint8_t[]> block(new uint8_t[bytes.size()]);  // exactly the frame
        if (!bytes.empty()) std::memcpy(block.get(), bytes.data(), bytes.size());
        const HeapLoad ld{block.get(), (uint32_t)bytes.size()};
        const ArpRecord r = arp_decide(ld, ld.len, f);
        const std::vector<uint8_t> want_rec = unhex(rec_hex);
        CHECK(want_rec.size() == sizeof(aipstack_arp_record));
        aipstack_arp_record rec;  // the dwords are the struct
        std::memcpy(&rec, r.w, sizeof(rec));
        if (std::memcmp(&rec, want_rec.data(), sizeof(rec)) != 0) {
            std::printf("FAIL: record of case %d differs\n", n);
            ++failures;
        }
        CHECK(rec.status == r.status() && rec.reserved == 0);
        CHECK(r.replies() == (slot_hex != "-"));
        CHECK(r.replies() == ((rec.flags & AIPSTACK_ARP_REC_REPLY) != 0));
        CHECK(!r.replies() || r.seen());
        if (r.replies() && slot_hex != "-") {
            uint32_t o[16];
            arp_build_reply(r, f, o);
            uint8_t img[64];
            std::memcpy(img, o, 64);
            const std::vector<uint8_t> want = unhex(slot_hex);
            CHECK(want.size() == AIPSTACK_ARP_REPLY_HEADER);
            if (std::memcmp(img, want.data(), want.size()) != 0) {
                std::printf("FAIL: reply of case %d differs\n", n);
                ++failures;
            }
            for (int k = AIPSTACK_ARP_REPLY_HEADER; k < 64; ++k) CHECK(img[k] == 0);
        }
        // a frame cut short behind any byte is never read past its end, and never replies
        for (uint32_t cut = 0; cut < ld.len && cut < 42; ++cut) {
            std::unique_ptr<uint8_t[]> part(new uint8_t[cut ? cut : 1]);
            if (cut) std::memcpy(part.get(), bytes.data(), cut);
            const ArpRecord q = arp_decide(HeapLoad{part.get(), cut}, cut, f);
            CHECK(!q.seen() && q.w[0] == 0 && q.w[1] == 0 && q.w[2] == 0 && (q.w[3] & 0xFFFF00FFu) == 0);
        }
        ++n;
    }
    return n;
}

static void arg_checks() {
    alignas(16) static uint8_t buf[256];
    aipstack_arp_iface f;
    std::memset(&f, 0, sizeof(f));
    f.flags = AIPSTACK_ARP_HAVE_ADDR;
    const uint64_t n = 600, need = aipstack_arp_rx_respond_workspace_bytes(n);
    CHECK(need == 16u * 4u + 64u * 3u);
    CHECK(aipstack_arp_rx_respond_workspace_bytes(0) == 16u);
    CHECK(aipstack_arp_rx_respond_workspace_bytes(256) == 32u + 64u);
    CHECK(aipstack_arp_rx_respond_workspace_bytes(257) == 48u + 128u);
    const ArpRespondArgs good{buf, buf, true, 2048, n, &f, buf, buf, buf, 64, buf, buf, buf, buf, buf,
                              buf, need};
    CHECK(arp_rx_respond_check_args(good) == AIPSTACK_CHKSUM_OK);
    auto bad = [&](auto change) {
        ArpRespondArgs a = good;
        aipstack_arp_iface g = f;
        a.h_iface = &g;
        change(a, g);
        CHECK(arp_rx_respond_check_args(a) == AIPSTACK_CHKSUM_EINVAL);
    };
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_base = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.frames = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.h_iface = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_status = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_arp = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_hdr = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_hdr_len = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_chunk_index = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_reply_frame = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_seen_frame = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_counts = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_workspace = nullptr; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.hdr_stride = 41; });
    bad([](ArpRespondArgs &, aipstack_arp_iface &g) { g.flags = 2; });
    bad([](ArpRespondArgs &, aipstack_arp_iface &g) { g.flags = 0x81; });
    bad([](ArpRespondArgs &, aipstack_arp_iface &g) { g.reserved[0] = 1; });
    bad([](ArpRespondArgs &, aipstack_arp_iface &g) { g.reserved[16] = 1; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.n = (1ull << 40) + 1; a.workspace_bytes = ~0ull; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.workspace_bytes -= 1; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_workspace = buf + 4; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_chunk_index = buf + 4; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_reply_frame = buf + 4; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_seen_frame = buf + 4; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_counts = buf + 4; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_hdr_len = buf + 2; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.d_arp = buf + 2; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.slot_stride = 0; });
    bad([](ArpRespondArgs &a, aipstack_arp_iface &) { a.slot_stride = 65537; });
    ArpRespondArgs csr = good;  // the CSR form does not look at the stride
    csr.slotted = false;
    csr.slot_stride = 0;
    CHECK(arp_rx_respond_check_args(csr) == AIPSTACK_CHKSUM_OK);
    ArpRespondArgs edge = good;
    f.flags = 0;
    edge.hdr_stride = 42;
    edge.d_arp = buf + 4;
    edge.n = 1ull << 40;
    edge.workspace_bytes = aipstack_arp_rx_respond_workspace_bytes(edge.n);
    CHECK(arp_rx_respond_check_args(edge) == AIPSTACK_CHKSUM_OK);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::printf("usage: arp_build_test <cases file>\n");
        return 2;
    }
    const int n = run_cases(argv[1]);
    CHECK(n > 0);
    arg_checks();
    if (failures) return 1;
    std::printf("OK %d cases\n", n);
    return 0;
}
