// Stand-alone test (its own main, built under ASan + UBSan by tx_resolve.mk, no GPU): the whole
// decision of Tx resolve (aipstack_amd/csrc/txres_common.h: route, permission tests, the table
// search, the record, the Ethernet header and its stores) as the kernels compile it, over the
// cases of a text file that tests/test_tx_resolve_host.py writes from the reference-recorded
// fixture and the model, and the host code (txres_host.cpp: the table sort, the workspace size,
// the argument checks). Every slot lies in a heap block of exactly its header's length, and the
// load functors refuse anything but bytes 12..13 and 26..33 inside it; a table lies in a block of
// exactly its entries and an index outside it aborts.
//
// The file: "I <n>" and n lines "<addr> <netmask> <gateway> <prefix> <flags> <mac hex>" (the
// interfaces, in table order), "T <n>" and n lines "<addr> <iface> <state> <mac hex>" (the ARP
// table as given: sorted unless the test says otherwise), then one case per line:
//   C <stride> <seg_status> <send_flags> <force> <status, or 0 for unspecified> <16 record bytes hex>
//     <14 header bytes hex, or -> <the slot's header bytes hex, or ->
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
#include "txres_common.h"

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
    uint32_t len, width;
    uint32_t operator()(uint32_t off) const {
        const bool field = (off >= 12u && off + width <= 14u) || (off >= 26u && off + width <= 34u);
        if ((uint64_t)off + width > len || !field) {
            std::printf("FAIL: load of [%u, %u) of a header of %u bytes\n", off, off + width, len);
            std::abort();
        }
        uint32_t w = 0;
        std::memcpy(&w, p + off, width);
        return w;
    }
};

struct IfaceLoad {
    const aipstack_tx_iface *t;
    uint32_t n;
    TxIfaceWords operator()(uint32_t k) const {
        if (k >= n) {
            std::printf("FAIL: interface %u of %u\n", k, n);
            std::abort();
        }
        uint32_t w[8];
        std::memcpy(w, &t[k], 32);
        return TxIfaceWords{w[0], w[1], w[2], w[3], w[4]};
    }
};

struct EntryLoad {
    const aipstack_arp_entry *t;
    uint64_t n;
    ArpEntryWords operator()(uint64_t i) const {
        if (i >= n) {
            std::printf("FAIL: entry %llu of a table of %llu\n", (unsigned long long)i, (unsigned long long)n);
            std::abort();
        }
        uint32_t w[4];
        std::memcpy(w, &t[i], 16);
        return ArpEntryWords{w[0], w[1], w[2], w[3]};
    }
};

// The stores of one header into a guarded block at a given alignment.
struct CheckedStore {
    uint8_t *slot;
    uint32_t align;
    uint8_t *written;  // 14 flags
    void operator()(uint32_t off, uint32_t width, uint32_t v) const {
        if ((width != 1u && width != 2u && width != 4u) || off + width > 14u || (off + align) % width != 0u) {
            std::printf("FAIL: store of %u bytes at %u, alignment %u\n", width, off, align);
            std::abort();
        }
        for (uint32_t k = 0; k < width; ++k) {
            if (written[off + k]) {
                std::printf("FAIL: byte %u stored twice\n", off + k);
                std::abort();
            }
            written[off + k] = 1;
            slot[off + k] = (uint8_t)(v >> (8u * k));
        }
    }
};

static std::vector<uint8_t> unhex(const std::string &h) {
    if (h == "-") return {};
    std::vector<uint8_t> v(h.size() / 2);
    for (size_t k = 0; k < v.size(); ++k) v[k] = (uint8_t)std::stoul(h.substr(2 * k, 2), nullptr, 16);
    return v;
}

static void check_stores(const TxDecision &d, const std::vector<uint8_t> &want) {
    for (uint32_t align = 0; align < 4; ++align) {
        // a heap block of exactly 14 bytes behind `align` bytes: ASan guards both ends
        std::unique_ptr<uint8_t[]> block(new uint8_t[align + 14]);
        std::memset(block.get(), 0x77, align + 14);
        uint8_t written[14] = {0};
        tx_res_store_header(align, d.image(), CheckedStore{block.get() + align, align, written});
        for (uint32_t k = 0; k < 14; ++k) CHECK(written[k] == 1);
        for (uint32_t k = 0; k < align; ++k) CHECK(block[k] == 0x77);
        CHECK(std::memcmp(block.get() + align, want.data(), 14) == 0);
    }
}

static int run_cases(const char *path) {
    std::ifstream in(path);
    std::string line;
    std::vector<aipstack_tx_iface> ifaces;
    std::vector<aipstack_arp_entry> table;
    int n = 0;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string what;
        s >> what;
        if (what == "I" || what == "T") {
            unsigned long count;
            s >> count;
            if (what == "I") ifaces.assign(count, aipstack_tx_iface{});
            else table.assign(count, aipstack_arp_entry{});
            for (unsigned long k = 0; k < count; ++k) {
                std::getline(in, line);
                std::istringstream e(line);
                std::string mac;
                if (what == "I") {
                    unsigned long a, m, g, p, f;
                    e >> a >> m >> g >> p >> f >> mac;
                    aipstack_tx_iface &x = ifaces[k];
                    x.addr = (uint32_t)a, x.netmask = (uint32_t)m, x.gateway = (uint32_t)g;
                    x.prefix = (uint8_t)p, x.flags = (uint8_t)f;
                    std::memcpy(x.mac, unhex(mac).data(), 6);
                } else {
                    unsigned long a, i, st;
                    e >> a >> i >> st >> mac;
                    aipstack_arp_entry &x = table[k];
                    x.addr = (uint32_t)a, x.iface = (uint16_t)i, x.state = (uint8_t)st;
                    std::memcpy(x.mac, unhex(mac).data(), 6);
                }
            }
            continue;
        }
        if (what != "C") continue;
        unsigned long stride, seg_status, send_flags, force, status;
        std::string rec_hex, hdr_hex, slot_hex;
        s >> stride >> seg_status >> send_flags >> force >> status >> rec_hex >> hdr_hex >> slot_hex;
        if (!s) {
            std::printf("FAIL: bad case line %d\n", n);
            ++failures;
            continue;
        }
        // the tables as the kernel sees them: exactly their entries, nothing readable behind
        std::unique_ptr<aipstack_tx_iface[]> ib(new aipstack_tx_iface[ifaces.size() ? ifaces.size() : 1]);
        if (!ifaces.empty()) std::memcpy(ib.get(), ifaces.data(), ifaces.size() * sizeof(ifaces[0]));
        std::unique_ptr<aipstack_arp_entry[]> tb(new aipstack_arp_entry[table.size() ? table.size() : 1]);
        if (!table.empty()) std::memcpy(tb.get(), table.data(), table.size() * sizeof(table[0]));
        const IfaceLoad iface{ib.get(), (uint32_t)ifaces.size()};
        const EntryLoad entry{tb.get(), table.size()};
        const std::vector<uint8_t> bytes = unhex(slot_hex);
        // the header as given, then every shorter length of it (0..64 for the longest cases)
        for (size_t cut = bytes.size() + 1; cut-- > 0;) {
            std::unique_ptr<uint8_t[]> block(new uint8_t[cut ? cut : 1]);
            if (cut) std::memcpy(block.get(), bytes.data(), cut);
            const TxDecision d = tx_resolve_segment(
                HeapLoad{block.get(), (uint32_t)cut, 2}, HeapLoad{block.get(), (uint32_t)cut, 4},
                (uint32_t)cut, stride, (uint32_t)seg_status, (uint32_t)send_flags, (uint32_t)force, iface,
                iface.n, entry, entry.n);
            CHECK(d.status >= AIPSTACK_TX_RES_NONE && d.status <= AIPSTACK_TX_RES_ARP_QUERY);
            CHECK((d.used < entry.n) == (d.status == AIPSTACK_TX_RES_SENT && d.r[1] != AIPSTACK_TX_NO_ARP_ENTRY));
            if (cut < 34) CHECK(d.status == AIPSTACK_TX_RES_NONE);
            if (d.status == AIPSTACK_TX_RES_NONE)
                CHECK((d.r[0] | d.r[1] | d.r[2] | d.r[3] | d.oa | d.ob | d.oc | d.od) == 0u);
            if (cut != bytes.size() || status == 0) continue;
            if (d.status != status) {
                std::printf("FAIL: case %d: status %u, want %lu\n", n, d.status, status);
                ++failures;
            }
            const std::vector<uint8_t> want = unhex(rec_hex);
            if (want.size() != 16 || std::memcmp(d.r, want.data(), 16) != 0) {
                std::printf("FAIL: record of case %d differs\n", n);
                ++failures;
            }
            const std::vector<uint8_t> hdr = unhex(hdr_hex);
            CHECK((d.status == AIPSTACK_TX_RES_SENT) == (hdr.size() == 14));
            if (hdr.size() == 14) check_stores(d, hdr);
        }
        ++n;
    }
    return n;
}

static void table_sort() {
    auto e = [](uint32_t addr, uint16_t iface, uint8_t state) {
        aipstack_arp_entry x{};
        x.addr = addr, x.iface = iface, x.state = state;
        return x;
    };
    std::vector<aipstack_arp_entry> v = {e(5, 1, 2), e(9, 0, 1), e(0xFFFFFFF0u, 0, 3), e(1, 1, 2), e(7, 0, 2)};
    CHECK(aipstack_arp_table_sort(v.data(), v.size()) == AIPSTACK_CHKSUM_OK);
    const uint32_t want[5][2] = {{0, 7}, {0, 9}, {0, 0xFFFFFFF0u}, {1, 1}, {1, 5}};
    for (int k = 0; k < 5; ++k) CHECK(v[k].iface == want[k][0] && v[k].addr == want[k][1]);
    CHECK(aipstack_arp_table_sort(nullptr, 0) == AIPSTACK_CHKSUM_OK);
    CHECK(aipstack_arp_table_sort(nullptr, 1) == AIPSTACK_CHKSUM_EINVAL);
    v = {e(5, 1, 2), e(5, 1, 1)};
    CHECK(aipstack_arp_table_sort(v.data(), 2) == AIPSTACK_CHKSUM_EINVAL);   // duplicate key
    v = {e(5, 1, 2), e(5, 0, 2)};
    CHECK(aipstack_arp_table_sort(v.data(), 2) == AIPSTACK_CHKSUM_OK && v[0].iface == 0);
    for (uint8_t state : {(uint8_t)0, (uint8_t)4}) {
        v = {e(5, 1, state)};
        CHECK(aipstack_arp_table_sort(v.data(), 1) == AIPSTACK_CHKSUM_EINVAL);
    }
    v = {e(5, 16, 2)};
    CHECK(aipstack_arp_table_sort(v.data(), 1) == AIPSTACK_CHKSUM_EINVAL);
    v = {e(5, 15, 2)};
    CHECK(aipstack_arp_table_sort(v.data(), 1) == AIPSTACK_CHKSUM_OK);
    v[0].reserved[2] = 1;
    CHECK(aipstack_arp_table_sort(v.data(), 1) == AIPSTACK_CHKSUM_EINVAL);
}

static void arg_checks() {
    alignas(16) static uint8_t buf[256];
    const uint64_t n = 600, need = aipstack_tx_resolve_workspace(n);
    CHECK(need == 16u * 4u + 64u * 3u);
    CHECK(aipstack_tx_resolve_workspace(0) == 16u);
    CHECK(aipstack_tx_resolve_workspace(256) == 32u + 64u);
    CHECK(aipstack_tx_resolve_workspace(257) == 48u + 128u);
    const TxResolveArgs good{buf, 64, buf, n, buf, buf, 16, buf, 10, buf, buf, buf, buf, buf, buf, buf, buf, need};
    CHECK(tx_resolve_check_args(good) == AIPSTACK_CHKSUM_OK);
    auto bad = [&](auto change) {
        TxResolveArgs a = good;
        change(a);
        CHECK(tx_resolve_check_args(a) == AIPSTACK_CHKSUM_EINVAL);
    };
    using A = TxResolveArgs;
    bad([](A &a) { a.d_hdr = nullptr; });
    bad([](A &a) { a.d_hdr_len = nullptr; });
    bad([](A &a) { a.d_ifaces = nullptr; });
    bad([](A &a) { a.d_arp = nullptr; });
    bad([](A &a) { a.d_arp_used = nullptr; });
    bad([](A &a) { a.d_status = nullptr; });
    bad([](A &a) { a.d_route = nullptr; });
    bad([](A &a) { a.d_send_len = nullptr; });
    bad([](A &a) { a.d_held_seg = nullptr; });
    bad([](A &a) { a.d_failed_seg = nullptr; });
    bad([](A &a) { a.d_counts = nullptr; });
    bad([](A &a) { a.d_workspace = nullptr; });
    bad([](A &a) { a.n_ifaces = 17; });
    bad([](A &a) { a.hdr_stride = 0; });
    bad([](A &a) { a.n = (1ull << 40) + 1; a.workspace_bytes = ~0ull; });
    bad([](A &a) { a.n_arp = 0xFFFFFFFFull; });
    bad([](A &a) { a.workspace_bytes -= 1; });
    bad([](A &a) { a.d_workspace = buf + 4; });
    bad([](A &a) { a.d_held_seg = buf + 4; });
    bad([](A &a) { a.d_failed_seg = buf + 4; });
    bad([](A &a) { a.d_counts = buf + 4; });
    bad([](A &a) { a.d_hdr_len = buf + 2; });
    bad([](A &a) { a.d_send_len = buf + 2; });
    bad([](A &a) { a.d_route = buf + 2; });
    bad([](A &a) { a.d_ifaces = buf + 2; });
    bad([](A &a) { a.d_arp = buf + 2; });
    bad([](A &a) { a.d_force_iface = buf + 1; });
    A edge = good;  // the optional pointer absent, no table, any ring address, the bounds themselves
    edge.d_force_iface = nullptr;
    edge.d_arp = edge.d_arp_used = nullptr;
    edge.n_arp = 0;
    edge.d_hdr = buf + 1;
    edge.d_status = buf + 3;
    edge.n_ifaces = 0;
    edge.hdr_stride = 1;
    edge.n = 1ull << 40;
    edge.workspace_bytes = aipstack_tx_resolve_workspace(edge.n);
    CHECK(tx_resolve_check_args(edge) == AIPSTACK_CHKSUM_OK);
    edge.n_arp = 0xFFFFFFFEull;
    edge.d_arp = buf + 4;
    edge.d_arp_used = buf + 1;
    CHECK(tx_resolve_check_args(edge) == AIPSTACK_CHKSUM_OK);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        std::printf("usage: tx_resolve_build_test <cases file>\n");
        return 2;
    }
    const int n = run_cases(argv[1]);
    CHECK(n > 0);
    table_sort();
    arg_checks();
    if (failures) return 1;
    std::printf("OK %d cases\n", n);
    return 0;
}
