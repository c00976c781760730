// Stand-alone test (its own main, built under ASan + UBSan by udprx.mk, no GPU): the record
// builder, the association search and the listener match of the UDP Rx demux
// (aipstack_amd/csrc/udprx_common.h, pcb_lookup.h), as the kernels compile them, over the cases
// of a text file that tests/test_udprx_host.py writes from the reference-recorded fixture and the
// model, and the workspace size and argument checks of the two entry points (udprx_host.cpp).
// Every frame and every table lies in a heap block of exactly its length; the load functors
// refuse a dword outside the frame and an entry outside the table.
//
// The file: "T <local> <bcast> <assoc table hex or -> <listener table hex or ->" starts a set;
// then one frame per line: "F <verdict> <frame hex or -> <32 record bytes hex> <unreach code>
// <delivered 0|1>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "aipstack_amd/chksum.h"
#include "udprx_common.h"

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
        if ((uint64_t)off + 4u > len || off + 4u > 82u) {
            std::printf("FAIL: load of [%u, %u) of a frame of %u bytes\n", off, off + 4u, len);
            std::abort();
        }
        uint32_t w;
        std::memcpy(&w, p + off, 4);
        return w;
    }
};

struct TableLoad {
    const std::vector<aipstack_tcp_pcb_key> *t;
    PcbEntryWords operator()(uint64_t i) const {
        if (i >= t->size()) {
            std::printf("FAIL: entry %llu of a table of %zu\n", (unsigned long long)i, t->size());
            std::abort();
        }
        PcbEntryWords e;
        std::memcpy(&e, t->data() + i, 16);   // past the block: ASan reports it
        return e;
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
    uint32_t local = 0, bcast = 0;
    std::vector<aipstack_tcp_pcb_key> assocs, shuffled;
    std::vector<aipstack_udp_listener> lis;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string what;
        s >> what;
        if (what == "T") {
            std::string a, l;
            s >> local >> bcast >> a >> l;
            const std::vector<uint8_t> ab = unhex(a), lb = unhex(l);
            assocs.assign(ab.size() / 16, aipstack_tcp_pcb_key{});
            if (!ab.empty()) std::memcpy(assocs.data(), ab.data(), ab.size());
            assocs.shrink_to_fit();
            lis.assign(lb.size() / 16, aipstack_udp_listener{});
            if (!lb.empty()) std::memcpy(lis.data(), lb.data(), lb.size());
            lis.shrink_to_fit();
            shuffled = assocs;                      // an unsorted table: reversed
            std::reverse(shuffled.begin(), shuffled.end());
            shuffled.shrink_to_fit();
        } else if (what == "F") {
            uint32_t verdict, code, delivered;
            std::string fh, rh;
            s >> verdict >> fh >> rh >> code >> delivered;
            std::vector<uint8_t> frame = unhex(fh);
            frame.shrink_to_fit();
            const std::vector<uint8_t> want = unhex(rh);
            uint32_t w[8];
            bool deliver = false;
            const HeapLoad ld{frame.data(), (uint32_t)frame.size()};
            const uint32_t got = udp_rx_demux_frame(ld, ld.len, verdict, local, bcast, TableLoad{&assocs},
                                                    assocs.size(), lis.data(), (uint32_t)lis.size(), w,
                                                    deliver);
            if (want.size() != 32 || std::memcmp(w, want.data(), 32) != 0 || got != code ||
                deliver != (delivered != 0)) {
                std::printf("FAIL case %d: code %u (want %u), delivered %d (want %u), record", n, got,
                            code, (int)deliver, delivered);
                for (int q = 0; q < 8; ++q) std::printf(" %08x", w[q]);
                std::printf("\n");
                ++failures;
            }
            // the unsorted table: any answer, no access outside it; everything but assoc as before
            uint32_t u[8];
            udp_rx_demux_frame(ld, ld.len, verdict, local, bcast, TableLoad{&shuffled}, shuffled.size(),
                               lis.data(), (uint32_t)lis.size(), u, deliver);
            u[6] = w[6];
            CHECK(std::memcmp(u, w, 32) == 0);
            ++n;
        }
    }
    return n;
}

int main(int argc, char **argv) {
    // the workspace: a pair of counts and four ballots per tile, and the totals
    CHECK(aipstack_udp_rx_demux_workspace_bytes(0) == 16);
    CHECK(aipstack_udp_rx_demux_workspace_bytes(1) == 16 * 2 + 32);
    CHECK(aipstack_udp_rx_demux_workspace_bytes(256) == 16 * 2 + 32);
    CHECK(aipstack_udp_rx_demux_workspace_bytes(257) == 16 * 3 + 64);
    CHECK(aipstack_udp_rx_demux_workspace_bytes(1ull << 40) == 16 * ((1ull << 32) + 1) + (32ull << 32));

    // the argument checks (pointers are only compared, never followed, but the interface's)
    alignas(16) static char mem[64];
    aipstack_icmp_iface f;
    std::memset(&f, 0, sizeof f);
    f.mtu = 1500;
    auto args = [&]() {
        return UdpRxDemuxArgs{mem, mem, false, 0, 4, &f, mem, 2, mem, 3, mem, mem, mem, mem, mem, mem, 1024};
    };
    UdpRxDemuxArgs a = args();
    CHECK(udp_rx_demux_check_args(a) == AIPSTACK_CHKSUM_OK);
    a.d_assocs = nullptr; a.n_assocs = 0; a.d_listeners = nullptr; a.n_listeners = 0;
    CHECK(udp_rx_demux_check_args(a) == AIPSTACK_CHKSUM_OK);
    a = args(); a.d_dgrams = mem + 8; a.d_verdict = mem + 1; a.d_unreach_code = mem + 3;
    CHECK(udp_rx_demux_check_args(a) == AIPSTACK_CHKSUM_OK);
    a = args(); a.slotted = true; a.slot_stride = 65536;
    CHECK(udp_rx_demux_check_args(a) == AIPSTACK_CHKSUM_OK);
    a = args(); a.n_listeners = 64; a.workspace_bytes = 64;
    CHECK(udp_rx_demux_check_args(a) == AIPSTACK_CHKSUM_OK);
#define BAD(stmt) do { a = args(); stmt; CHECK(udp_rx_demux_check_args(a) == AIPSTACK_CHKSUM_EINVAL); } while (0)
    BAD(a.d_base = nullptr); BAD(a.frames = nullptr); BAD(a.h_iface = nullptr);
    BAD(a.d_verdict = nullptr); BAD(a.d_dgrams = nullptr); BAD(a.d_unreach_code = nullptr);
    BAD(a.d_deliver_frame = nullptr); BAD(a.d_counts = nullptr); BAD(a.d_workspace = nullptr);
    BAD(a.d_assocs = nullptr); BAD(a.d_listeners = nullptr);
    BAD(a.n = (1ull << 40) + 1; a.workspace_bytes = ~0ull);
    BAD(a.n_assocs = (1ull << 40) + 1); BAD(a.n_listeners = 65);
    BAD(a.d_dgrams = mem + 4); BAD(a.d_deliver_frame = mem + 4); BAD(a.d_counts = mem + 4);
    BAD(a.d_workspace = mem + 4); BAD(a.d_assocs = mem + 4); BAD(a.d_listeners = mem + 4);
    BAD(a.workspace_bytes = 63);
    BAD(a.slotted = true); BAD(a.slotted = true; a.slot_stride = 65537);
    BAD(f.mtu = 255); f.mtu = 1500;
    BAD(f.flags = 2); f.flags = 0;
    BAD(f.reserved[11] = 1); f.reserved[11] = 0;

    int n = 0;
    if (argc > 1) n = run_cases(argv[1]);
    if (failures) return 1;
    std::printf("udprx_table_test: OK %d cases\n", n);
    return 0;
}
