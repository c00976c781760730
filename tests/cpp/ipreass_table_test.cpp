// Stand-alone test (its own main; built with -fsanitize=address,undefined by ipreass.mk) of the
// text the reassembly kernels share with the host: the fragment fields, the two tables (insert,
// poison, count, lookup), the walk and the datagram verdict of ipreass_common.h, run serially in
// the order of the kernels' passes on crafted batches whose frames lie in heap blocks of exactly
// their length, plus the argument checks and the workspace size of ipreass_host.cpp.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "aipstack_amd/chksum.h"
#include "ipreass_common.h"

using namespace aipstack_amd;

static int failures = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            ++failures;                                                  \
        }                                                                \
    } while (0)

struct HostAtomics {
    uint64_t load(uint64_t *p) const { return *p; }
    uint64_t cas(uint64_t *p, uint64_t expect, uint64_t v) const {
        const uint64_t old = *p;
        if (old == expect) *p = v;
        return old;
    }
    void fetch_or(uint64_t *p, uint64_t v) const { *p |= v; }
    void fetch_add(uint64_t *p, uint64_t v) const { *p += v; }
};

// A frame in a heap block of exactly its length: a read past it is an ASan report.
struct Frame {
    uint8_t *p;
    uint32_t len;
};
struct HeapLoad {
    const uint8_t *p;
    uint32_t operator()(uint32_t off) const {
        uint32_t v;
        std::memcpy(&v, p + off, 4);
        return v;
    }
};

static uint32_t sum16(const uint8_t *d, size_t n, uint32_t s = 0) {
    for (size_t i = 0; i + 1 < n; i += 2) s += (uint32_t)d[i] << 8 | d[i + 1];
    if (n & 1) s += (uint32_t)d[n - 1] << 8;
    while (s >> 16) s = (s & 0xFFFF) + (s >> 16);
    return s;
}

static Frame make_frame(uint32_t src, uint32_t dst, uint16_t ident, uint8_t proto, uint32_t off,
                        bool mf, const std::vector<uint8_t> &payload, unsigned ihl = 5) {
    const uint32_t hl = 4 * ihl, total = hl + (uint32_t)payload.size();
    Frame f{(uint8_t *)std::malloc(14 + total), 14 + total};
    std::memset(f.p, 2, 12);
    f.p[12] = 0x08;
    f.p[13] = 0x00;
    uint8_t *ip = f.p + 14;
    std::memset(ip, 1, hl);
    ip[0] = (uint8_t)(0x40 | ihl);
    ip[1] = 0;
    ip[2] = (uint8_t)(total >> 8);
    ip[3] = (uint8_t)total;
    ip[4] = (uint8_t)(ident >> 8);
    ip[5] = (uint8_t)ident;
    const uint32_t fo = (mf ? 0x2000u : 0u) | off / 8;
    ip[6] = (uint8_t)(fo >> 8);
    ip[7] = (uint8_t)fo;
    ip[8] = 64;
    ip[9] = proto;
    ip[10] = ip[11] = 0;
    for (int k = 0; k < 4; ++k) {
        ip[12 + k] = (uint8_t)(src >> (24 - 8 * k));
        ip[16 + k] = (uint8_t)(dst >> (24 - 8 * k));
    }
    const uint32_t c = ~sum16(ip, hl) & 0xFFFF;
    ip[10] = (uint8_t)(c >> 8);
    ip[11] = (uint8_t)c;
    if (!payload.empty()) std::memcpy(ip + hl, payload.data(), payload.size());
    return f;
}

struct Piece {
    uint32_t off;
    std::vector<uint8_t> data;
    bool mf;
};

static std::vector<Piece> cut(const std::vector<uint8_t> &body, const std::vector<uint32_t> &cuts) {
    std::vector<uint32_t> e{0};
    e.insert(e.end(), cuts.begin(), cuts.end());
    e.push_back((uint32_t)body.size());
    std::vector<Piece> out;
    for (size_t k = 0; k + 1 < e.size(); ++k)
        out.push_back({e[k], std::vector<uint8_t>(body.begin() + e[k], body.begin() + e[k + 1]),
                       e[k + 1] != body.size()});
    return out;
}

static std::vector<uint8_t> udp_body(uint32_t src, uint32_t dst, size_t n, int ulen = -1,
                                     bool no_chk = false) {
    std::vector<uint8_t> b(8 + n);
    for (size_t k = 0; k < n; ++k) b[8 + k] = (uint8_t)(k * 31 + 7);
    const uint32_t ul = ulen < 0 ? (uint32_t)b.size() : (uint32_t)ulen;
    b[0] = 0; b[1] = 7; b[2] = 0; b[3] = 9;
    b[4] = (uint8_t)(ul >> 8); b[5] = (uint8_t)ul; b[6] = b[7] = 0;
    if (!no_chk) {
        uint32_t ps = (src >> 16) + (src & 0xFFFF) + (dst >> 16) + (dst & 0xFFFF) + 17 + ul;
        uint32_t c = ~sum16(b.data(), ul <= b.size() ? ul : b.size(), ps) & 0xFFFF;
        if (c == 0) c = 0xFFFF;
        b[6] = (uint8_t)(c >> 8); b[7] = (uint8_t)c;
    }
    return b;
}

struct Group {
    std::string name;
    std::vector<Frame> frames;
    int verdict;       // the datagram verdict, or -1: must stay incomplete
    uint32_t n_drop;   // members that must get AIPSTACK_RX_DROP_FRAG
};

struct Result {
    std::vector<uint8_t> verdict;
    std::vector<uint32_t> head, next;
    std::vector<aipstack_ip4_dgram> dgram;
};

// The passes of ipreass_kernels.hip, serially; `slots` = the tables' size (0: reass_workspace's).
static Result run(const std::vector<Frame> &fr, uint32_t max_reass, uint64_t slots = 0) {
    const uint64_t n = fr.size();
    if (slots == 0) slots = reass_workspace(n).slots;
    CHECK((slots & (slots - 1)) == 0 && slots >= n);
    Result r;
    r.verdict.assign(n, AIPSTACK_RX_FRAGMENT);
    r.head.assign(n, AIPSTACK_REASS_NONE);
    r.next.assign(n, AIPSTACK_REASS_NONE);
    r.dgram.assign(n, aipstack_ip4_dgram{});
    std::vector<ReassRec> recs(n);
    std::vector<uint32_t> poff(n), succ(n);
    std::vector<uint16_t> sums(n);
    std::vector<uint64_t> pairs(slots, 0), keys(slots, 0);
    const HostAtomics at;
    for (uint64_t i = 0; i < n; ++i) {                                   // classify
        const int kind = reass_fragment(HeapLoad{fr[i].p}, fr[i].len, max_reass, recs[i], poff[i]);
        if (kind == kReassEmpty || kind == kReassOversize) r.verdict[i] = AIPSTACK_RX_DROP_FRAG;
        if (kind == kReassNone) r.verdict[i] = AIPSTACK_RX_NOT_IP4;      // (a runt: no fragment)
        if (kind == kReassEmpty || kind == kReassNone) recs[i] = ReassRec{{0, 0, 0, 0}};
        sums[i] = kind == kReassIn ? (uint16_t)sum16(fr[i].p + poff[i], recs[i].len()) : 0;
    }
    for (uint64_t i = 0; i < n; ++i) {                                   // insert
        if (recs[i].len() == 0) continue;
        reass_insert_key(at, keys.data(), slots, recs.data(), n, (uint32_t)i);
        if (recs[i].member()) reass_insert_pair(at, pairs.data(), slots, recs.data(), n, (uint32_t)i);
    }
    for (uint64_t i = 0; i < n; ++i)                                     // link
        succ[i] = reass_successor(pairs.data(), slots, recs.data(), n, (uint32_t)i);
    for (uint64_t i = 0; i < n; ++i) {                                   // finish
        const ReassRec h = recs[i];
        if (!h.member() || h.off() != 0 || !h.mf()) continue;
        const uint32_t count = reass_key_count(keys.data(), slots, recs.data(), n, h);
        uint32_t last, data_len, sum;
        if (!reass_walk(recs.data(), succ.data(), sums.data(), n, (uint32_t)i, count, last, data_len, sum))
            continue;
        uint32_t p1 = 0;
        if (h.len() >= 8) std::memcpy(&p1, fr[i].p + poff[i] + 4, 4);
        r.dgram[i].n_frags = count;
        r.dgram[i].last_frame = last;
        r.dgram[i].data_len = (uint16_t)data_len;
        r.dgram[i].proto = (uint8_t)h.proto();
        r.dgram[i].verdict = (uint8_t)reass_dgram_verdict(h.proto(), h.w[0], h.w[1], data_len, sum, p1);
        uint32_t cur = (uint32_t)i;
        for (uint32_t k = 0; k < count; ++k) {
            const uint32_t nx = k + 1 < count ? succ[cur] : AIPSTACK_REASS_NONE;
            r.verdict[cur] = AIPSTACK_RX_FRAG_MEMBER;
            r.head[cur] = (uint32_t)i;
            r.next[cur] = nx;
            cur = nx;
        }
    }
    return r;
}

static const uint32_t A = 0xC0A80001u, B = 0xC0A80002u;

static std::vector<Group> crafted() {
    std::vector<Group> g;
    uint16_t ident = 100;
    auto add = [&](const char *name, uint8_t proto, std::vector<Piece> pieces, int verdict,
                   uint32_t n_drop = 0, unsigned ihl = 5) {
        Group x{name, {}, verdict, n_drop};
        ++ident;
        for (const Piece &p : pieces) x.frames.push_back(make_frame(A, B, ident, proto, p.off, p.mf, p.data, ihl));
        g.push_back(x);
    };
    const std::vector<uint8_t> u = udp_body(A, B, 100);
    auto P = cut(u, {40, 80});
    add("ok", 17, P, AIPSTACK_RX_ACCEPT);
    add("reversed", 17, {P[2], P[1], P[0]}, AIPSTACK_RX_ACCEPT);
    add("ihl15", 17, {P[1], P[0], P[2]}, AIPSTACK_RX_ACCEPT, 0, 15);
    add("missing_first", 17, {P[1], P[2]}, -1);
    add("missing_middle", 17, {P[0], P[2]}, -1);
    add("missing_last", 17, {P[0], P[1]}, -1);
    add("duplicate", 17, {P[0], P[1], P[1], P[2]}, -1);
    add("overlap", 17, {P[0], P[1], P[2], Piece{32, std::vector<uint8_t>(16, 0x55), true}}, -1);
    add("extra", 17, {P[0], P[1], P[2], Piece{200, std::vector<uint8_t>(8, 0x55), false}}, -1);
    add("two_dgrams", 17, {P[0], P[1], P[2], P[0], P[1], P[2]}, -1);
    add("empty", 17, {P[0], P[1], P[2], Piece{16, {}, true}}, AIPSTACK_RX_ACCEPT, 1);
    add("oversize", 17, {P[0], P[1], P[2], Piece{65528, std::vector<uint8_t>(8, 1), false}}, -1, 1);
    add("lone_mf", 17, {Piece{0, u, true}}, -1);
    add("lone_tail", 17, {Piece{48, u, false}}, -1);
    auto C = P;
    C[1].data[3] ^= 1;
    add("corrupt", 17, C, AIPSTACK_RX_DROP_L4_CHKSUM);
    add("udp_chk0", 17, cut(udp_body(A, B, 100, -1, true), {40}), AIPSTACK_RX_ACCEPT_NO_CHKSUM);
    add("udp_short", 17, cut(udp_body(A, B, 100, 60), {40}), AIPSTACK_RX_REASS_TRUNCATED);
    add("udp_long", 17, cut(udp_body(A, B, 100, 109), {40}), AIPSTACK_RX_DROP_L4_MALFORMED);
    add("udp_below_8", 17, cut(udp_body(A, B, 100, 7), {40}), AIPSTACK_RX_DROP_L4_MALFORMED);
    add("tcp_below_20", 6, cut(std::vector<uint8_t>(19, 0x11), {8, 16}), AIPSTACK_RX_DROP_L4_MALFORMED);
    {
        std::vector<uint8_t> t(61, 0x21);                                // TCP, 8-byte first fragments
        t[16] = t[17] = 0;
        const uint32_t ps = (A >> 16) + (A & 0xFFFF) + (B >> 16) + (B & 0xFFFF) + 6 + 61;
        const uint32_t c = ~sum16(t.data(), t.size(), ps) & 0xFFFF;
        t[16] = (uint8_t)(c >> 8); t[17] = (uint8_t)c;
        add("tcp_header_8", 6, cut(t, {8, 16, 24}), AIPSTACK_RX_ACCEPT);
        t[60] ^= 4;
        add("tcp_bad", 6, cut(t, {16}), AIPSTACK_RX_DROP_L4_CHKSUM);
    }
    {
        std::vector<uint8_t> ic(77, 0x42);
        ic[2] = ic[3] = 0;
        const uint32_t c = ~sum16(ic.data(), ic.size()) & 0xFFFF;
        ic[2] = (uint8_t)(c >> 8); ic[3] = (uint8_t)c;
        add("icmp", 1, cut(ic, {24, 48}), AIPSTACK_RX_ACCEPT);
    }
    add("proto47", 47, cut(std::vector<uint8_t>(99, 9), {32}), AIPSTACK_RX_ACCEPT_OTHER);
    return g;
}

static void check_groups(const std::vector<Group> &groups, uint32_t max_reass, uint64_t slots,
                         unsigned rotate) {
    // the groups' frames interleaved round-robin, rotated: arrival order must not matter
    std::vector<Frame> fr;
    std::vector<size_t> owner;
    for (size_t k = 0;; ++k) {
        bool any = false;
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            const size_t g = (gi + rotate) % groups.size();
            if (k < groups[g].frames.size()) {
                fr.push_back(groups[g].frames[k]);
                owner.push_back(g);
                any = true;
            }
        }
        if (!any) break;
    }
    const Result r = run(fr, max_reass, slots);
    for (size_t g = 0; g < groups.size(); ++g) {
        uint32_t heads = 0, members = 0, drops = 0, left = 0;
        int verdict = -1;
        for (size_t i = 0; i < fr.size(); ++i) {
            if (owner[i] != g) continue;
            if (r.dgram[i].n_frags) {
                ++heads;
                verdict = r.dgram[i].verdict;
                // the links: from the head, n_frags members in strictly increasing offset order
                uint32_t cur = (uint32_t)i, seen = 0;
                while (cur != AIPSTACK_REASS_NONE && seen <= r.dgram[i].n_frags) {
                    CHECK(owner[cur] == g && r.head[cur] == i);
                    if (r.next[cur] == AIPSTACK_REASS_NONE) CHECK(cur == r.dgram[i].last_frame);
                    cur = r.next[cur];
                    ++seen;
                }
                CHECK(seen == r.dgram[i].n_frags);
            }
            members += r.verdict[i] == AIPSTACK_RX_FRAG_MEMBER;
            drops += r.verdict[i] == AIPSTACK_RX_DROP_FRAG;
            left += r.verdict[i] == AIPSTACK_RX_FRAGMENT;
        }
        const Group &x = groups[g];
        const bool ok = verdict == x.verdict && heads == (x.verdict >= 0 ? 1u : 0u) &&
                        drops == x.n_drop &&
                        (x.verdict >= 0 ? members + drops == x.frames.size() && left == 0
                                        : members == 0 && left + drops == x.frames.size());
        if (!ok) {
            std::printf("FAIL group %s (slots %llu, rotate %u): verdict %d want %d, heads %u members %u "
                        "drops %u left %u\n", x.name.c_str(), (unsigned long long)slots, rotate, verdict,
                        x.verdict, heads, members, drops, left);
            ++failures;
        }
    }
}

static void test_tables() {
    // many keys in a table with hardly a free slot: every insert and lookup probes far, every
    // count is right, poison hits exactly the doubled pair
    const uint32_t n = 250;
    std::vector<ReassRec> recs(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t key = i / 5;                       // 50 keys of 5 fragments
        recs[i].w[0] = 0x0A000000u + key % 7;
        recs[i].w[1] = 0x0B000000u + key % 3;
        recs[i].w[2] = (key & 0xFFFFu) | 17u << 16 | (kReassMember | kReassMF) << 24;
        recs[i].w[3] = (i % 5 == 4 ? 8u : (i % 5) * 8u) | 8u << 16;   // the fifth doubles offset 8
    }
    const uint64_t slots = 256;
    std::vector<uint64_t> pairs(slots, 0), keys(slots, 0);
    const HostAtomics at;
    for (uint32_t i = 0; i < n; ++i) {
        reass_insert_key(at, keys.data(), slots, recs.data(), n, i);
        reass_insert_pair(at, pairs.data(), slots, recs.data(), n, i);
    }
    for (uint32_t i = 0; i < n; ++i) {
        CHECK(reass_key_count(keys.data(), slots, recs.data(), n, recs[i]) == 5);
        const uint32_t f = reass_find_pair(pairs.data(), slots, recs.data(), n, recs[i], recs[i].off());
        if (recs[i].off() == 8) CHECK(f == AIPSTACK_REASS_NONE);     // poisoned
        else CHECK(f == i);
        CHECK(reass_find_pair(pairs.data(), slots, recs.data(), n, recs[i], 4000) == AIPSTACK_REASS_NONE);
    }
    ReassRec other = recs[0];
    other.w[0] ^= 0x100;
    CHECK(reass_key_count(keys.data(), slots, recs.data(), n, other) == 0);
    // a table of garbage: every probe stays inside it and ends
    std::vector<uint64_t> junk(64, ~0ull);
    CHECK(reass_find_pair(junk.data(), 64, recs.data(), n, recs[0], 0) == AIPSTACK_REASS_NONE);
    CHECK(reass_key_count(junk.data(), 64, recs.data(), n, recs[0]) == 0);
    reass_insert_pair(at, junk.data(), 64, recs.data(), n, 0);
    reass_insert_key(at, junk.data(), 64, recs.data(), n, 0);
    // a successor array of garbage: the walk stays inside the arrays and ends
    std::vector<uint32_t> succ(n, 3);
    std::vector<uint16_t> sums(n, 1);
    uint32_t a, b, c;
    CHECK(!reass_walk(recs.data(), succ.data(), sums.data(), n, 0, 5, a, b, c));
    std::fill(succ.begin(), succ.end(), 0xFFFFFFF0u);
    CHECK(!reass_walk(recs.data(), succ.data(), sums.data(), n, 0, 5, a, b, c));
}

static void test_host() {
    CHECK(aipstack_ip4_reass_workspace_bytes(0) % 8 == 0);
    uint64_t prev = 0;
    for (uint64_t n : {0ull, 1ull, 15ull, 16ull, 17ull, 1000ull, 1ull << 20, 0xFFFFFFFEull}) {
        const ReassWorkspace w = reass_workspace(n);
        CHECK((w.slots & (w.slots - 1)) == 0 && w.slots >= 4 * n && w.slots < 8 * n + 128);
        CHECK(w.total == aipstack_ip4_reass_workspace_bytes(n) && w.total % 8 == 0 && w.total >= prev);
        CHECK(w.recs % 8 == 0 && w.succ % 8 == 0 && w.sums % 8 == 0 && w.pairs % 8 == 0);
        prev = w.total;
    }
    alignas(16) static char buf[4096];
    void *p = buf;
    const uint64_t need = aipstack_ip4_reass_workspace_bytes(4);
    auto call = [&](const void *base, const void *fr, uint64_t n, uint32_t max, const void *v,
                    const void *ca, const void *cl, const void *nx, const void *hd, const void *dg,
                    const void *ws, uint64_t wsb) {
        return ip4_rx_reassemble_check_args(base, fr, false, 0, n, max, v, ca, cl, nx, hd, dg, ws, wsb);
    };
    CHECK(call(p, p, 4, 65531, p, p, p, p, p, p, p, need) == AIPSTACK_CHKSUM_OK);
    CHECK(call(p, p, 4, 1, p, p, p, p, p, p, p, need) == AIPSTACK_CHKSUM_OK);
    CHECK(call(p, p, 4, 0, p, p, p, p, p, p, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(p, p, 4, 65532, p, p, p, p, p, p, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(p, p, 4, 65531, p, p, p, p, p, p, p, need - 1) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(p, p, 0xFFFFFFFFull, 65531, p, p, p, p, p, p, p, ~0ull) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(p, p, 4, 65531, p, buf + 4, p, p, p, p, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(p, p, 4, 65531, p, p, buf + 2, p, p, p, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(p, p, 4, 65531, p, p, p, buf + 2, p, p, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(p, p, 4, 65531, p, p, p, p, buf + 1, p, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(p, p, 4, 65531, p, p, p, p, p, buf + 2, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(p, p, 4, 65531, p, p, p, p, p, p, buf + 4, need + 4) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(nullptr, p, 4, 65531, p, p, p, p, p, p, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(call(p, p, 4, 65531, p, p, p, p, p, nullptr, p, need) == AIPSTACK_CHKSUM_EINVAL);
    CHECK(ip4_rx_reassemble_check_args(p, p, true, 0, 4, 65531, p, p, p, p, p, p, p, need) ==
          AIPSTACK_CHKSUM_EINVAL);
    CHECK(ip4_rx_reassemble_check_args(p, p, true, 65537, 4, 65531, p, p, p, p, p, p, p, need) ==
          AIPSTACK_CHKSUM_EINVAL);
    CHECK(ip4_rx_reassemble_check_args(p, p, true, 2048, 4, 65531, p, p, p, p, p, p, p, need) ==
          AIPSTACK_CHKSUM_OK);
}

int main(int argc, char **argv) {
    if (argc == 7 && std::string(argv[1]) == "--hash") {   // the hashes of one key, for the model
        ReassRec r{{(uint32_t)std::strtoul(argv[2], nullptr, 0), (uint32_t)std::strtoul(argv[3], nullptr, 0),
                    (uint32_t)std::strtoul(argv[4], nullptr, 0) | (uint32_t)std::strtoul(argv[5], nullptr, 0) << 16,
                    0}};
        std::printf("%u %u\n", reass_hash_key(r), reass_hash_key_off(r, (uint32_t)std::strtoul(argv[6], nullptr, 0)));
        return 0;
    }
    std::vector<Group> groups = crafted();
    size_t n = 0;
    for (const Group &g : groups) n += g.frames.size();
    uint64_t tight = 1;
    while (tight < n) tight <<= 1;                       // hardly a free slot: long probes
    for (unsigned rotate = 0; rotate < 5; ++rotate) {
        check_groups(groups, 65531, 0, rotate);
        check_groups(groups, 65531, tight, rotate);
    }
    {   // both sides of a small max_reass_size
        std::vector<Group> s;
        auto mk = [&](const char *name, uint16_t id, std::vector<Piece> ps, int v, uint32_t drop) {
            Group x{name, {}, v, drop};
            for (const Piece &p : ps) x.frames.push_back(make_frame(A, B, id, 47, p.off, p.mf, p.data));
            s.push_back(x);
        };
        mk("len_at_max", 1, cut(std::vector<uint8_t>(104, 3), {96}), AIPSTACK_RX_ACCEPT_OTHER, 0);
        mk("len_past_max", 2, cut(std::vector<uint8_t>(105, 3), {96}), -1, 1);
        mk("off_at_max", 3, {Piece{0, std::vector<uint8_t>(104, 3), true}, Piece{104, {1}, false}}, -1, 1);
        mk("off_past_max", 4, {Piece{0, std::vector<uint8_t>(96, 3), true}, Piece{112, {1}, false}}, -1, 1);
        check_groups(s, 104, 0, 0);
        for (Group &g : s)
            for (Frame &f : g.frames) std::free(f.p);
    }
    {   // runts and truncated frames: nothing past a frame's own length is read
        std::vector<Frame> fr;
        const Frame whole = make_frame(A, B, 9, 17, 0, true, std::vector<uint8_t>(16, 5), 15);
        for (uint32_t len = 0; len <= whole.len; ++len) {
            Frame f{(uint8_t *)std::malloc(len ? len : 1), len};
            std::memcpy(f.p, whole.p, len);
            fr.push_back(f);
        }
        const Result r = run(fr, 65531);
        for (size_t i = 0; i + 1 < fr.size(); ++i) CHECK(r.verdict[i] == AIPSTACK_RX_NOT_IP4);
        CHECK(r.verdict.back() == AIPSTACK_RX_FRAGMENT);
        for (Frame &f : fr) std::free(f.p);
        std::free(whole.p);
    }
    test_tables();
    test_host();
    for (Group &g : groups)
        for (Frame &f : g.frames) std::free(f.p);
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
