// TEST INFRASTRUCTURE -- what the reference stack puts on the wire: the reference's own IpStack
// with IpTcpProto and IpUdpProto, instantiated on a stub platform and a capture driver of this
// project's (only reference headers are included; `make -C oracle ref` builds it where the
// reference tree exists). tests/golden/stack_tx_ref.py drives it and records the answers in
// tests/golden/stack_tx_ref_cases.json.
//
// The platform: a clock that stands still unless the script moves it; timers that record
// setAt / unset in a registry, of which the script fires those that are due, in time order
// (the reference defers TCP output to a timer of 0 ticks). The interface is a bare
// IpDriverIface (no Ethernet, no ARP) whose send_ip4_packet copies each IP packet into a
// capture list and returns success.
//
// One request per line; every answer ends with a line ".":
//   S <mtu> <local addr> <clock>          a fresh stack, interface <local addr>/8, clock set
//   U <src port> <dst port> <dst addr> <len0> <len1> <salt> <fix>
//        UdpApi::sendUdpIp4Packet of a payload of two nodes (one if len1 is 0): byte k is
//        (salt + 3k) & 0xFF; with fix >= 0 bytes 0 and 1 are fix's high and low byte.
//        -> "U <IpErr>", then per captured packet
//           "F <20 IP header bytes> <8 UDP header bytes, or - beyond the first> <data length> <FNV-1a 64>"
//   C <dst addr> <dst port> <peer mss, 0 = no option> <peer window> <peer window shift, -1 = no option>
//     <ring size> <salt> <peer isn>
//        TcpConnection::startConnection, the SYN captured, a SYN-ACK injected (checksums by the
//        reference's IpChksum), the send ring set: a circular IpBufNode of <ring size> bytes
//        -> "P <kind> ..." per captured packet, then "C <snd_mss> <established>"
//   B <token>...    tokens: <n> = write n bytes to the ring and extendSendBuf(n), P = sendPush,
//                   F = closeSending; then the due timers fire, the burst is captured, and the
//                   scripted peer ACKs every segment on its own with its window
//        -> "B <off0> <len0> <off1> <len1> <snd_mss> <push index> <fin> <seq> <stream index>"
//           (the ring range from getSendBuf, snd_mss from getSndBufOverhead, the push index and
//           FIN from what the script did, seq from the clock at connect and the bytes handed over),
//           then "P <kind> <20 IP header bytes> <TCP header with options> <data length> <FNV>"
//           per captured packet, "I" where the ACK injections begin
//        kind: S = SYN, D = data or FIN first sent, A = no data and no SYN / FIN, R = retransmit
//   R <port> <n>    followed by n lines of hex IP packets: a UdpListener on <port>, the packets
//                   injected in order -> "R <calls>" and "L <length> <FNV>" per listener call
// Stream byte k of a connection is (salt + 3k) & 0xFF at ring position k % <ring size>.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include <aipstack/misc/Function.h>
#include <aipstack/structure/index/AvlTreeIndex.h>
#include <aipstack/platform/PlatformFacade.h>
#include <aipstack/infra/Buf.h>
#include <aipstack/infra/BufUtils.h>
#include <aipstack/infra/Chksum.h>
#include <aipstack/infra/Err.h>
#include <aipstack/proto/Ip4Proto.h>
#include <aipstack/proto/Tcp4Proto.h>
#include <aipstack/proto/Udp4Proto.h>
#include <aipstack/ip/IpAddr.h>
#include <aipstack/ip/IpStack.h>
#include <aipstack/ip/IpDriverIface.h>
#include <aipstack/ip/IpPathMtuCache.h>
#include <aipstack/ip/IpReassembly.h>
#include <aipstack/tcp/IpTcpProto.h>
#include <aipstack/tcp/TcpApi.h>
#include <aipstack/tcp/TcpConnection.h>
#include <aipstack/udp/IpUdpProto.h>

using namespace AIpStack;

// ---- the platform ---------------------------------------------------------------------------

struct StubPlatform {
    inline static constexpr bool ImplIsStatic = true;
    using TimeType = std::uint64_t;
    inline static constexpr double TimeFreq = 1000.0;
    inline static constexpr TimeType RelativeTimeLimit = ~TimeType(0);

    class Timer;
    inline static TimeType now = 1000;
    inline static std::vector<Timer *> timers;
    inline static unsigned long n_set = 0, n_unset = 0, n_fired = 0, order = 0;

    static TimeType getTime() { return now; }
    static TimeType getEventTime() { return now; }

    class Timer {
    public:
        Timer(PlatformRef<StubPlatform>, Function<void()> handler) : m_handler(handler) {
            timers.push_back(this);
        }
        Timer(Timer const &) = delete;
        Timer &operator=(Timer const &) = delete;
        ~Timer() { timers.erase(std::find(timers.begin(), timers.end(), this)); }
        PlatformRef<StubPlatform> ref() const { return PlatformRef<StubPlatform>(); }
        bool isSet() const { return m_set; }
        TimeType getSetTime() const { return m_time; }
        void unset() {
            n_unset += m_set;
            m_set = false;
        }
        void setAt(TimeType t) {
            m_set = true;
            m_time = t;
            m_order = ++order;
            ++n_set;
        }
        void fire() {
            m_set = false;
            ++n_fired;
            m_handler();
        }
        unsigned long setOrder() const { return m_order; }

    private:
        Function<void()> m_handler;
        bool m_set = false;
        TimeType m_time = 0;
        unsigned long m_order = 0;
    };

    // The timers due at `now`, earliest first (ties in the order they were set), until none is.
    static void fireDue() {
        for (int guard = 0; guard < 100000; ++guard) {
            Timer *best = nullptr;
            for (Timer *t : timers) {
                if (!t->isSet() || (std::int64_t)(t->getSetTime() - now) > 0) continue;
                if (best == nullptr ||
                    (std::int64_t)(t->getSetTime() - best->getSetTime()) < 0 ||
                    (t->getSetTime() == best->getSetTime() && t->setOrder() < best->setOrder()))
                    best = t;
            }
            if (best == nullptr) return;
            best->fire();
        }
        std::fprintf(stderr, "stack_ref_gen: timers keep firing\n");
        std::exit(2);
    }
};

// ---- the stack ------------------------------------------------------------------------------

using IndexService = AvlTreeIndexService;
using StackService = IpStackService<
    IpStackOptions::HeaderBeforeIp::Is<14>,
    IpStackOptions::PathMtuCacheService::Is<IpPathMtuCacheService<
        IpPathMtuCacheOptions::NumMtuEntries::Is<16>,
        IpPathMtuCacheOptions::MtuIndexService::Is<IndexService>>>,
    IpStackOptions::ReassemblyService::Is<IpReassemblyService<
        IpReassemblyOptions::MaxReassEntrys::Is<16>,
        IpReassemblyOptions::MaxReassSize::Is<65531>,
        IpReassemblyOptions::MaxReassHoles::Is<250>>>>;
using ProtocolServices = MakeTypeList<
    IpTcpProtoService<IpTcpProtoOptions::NumTcpPcbs::Is<16>,
                      IpTcpProtoOptions::PcbIndexService::Is<IndexService>>,
    IpUdpProtoService<IpUdpProtoOptions::UdpIndexService::Is<IndexService>>>;
class StackArg : public StackService::template Compose<StubPlatform, ProtocolServices> {};
using Stack = IpStack<StackArg>;
using TcpArg = typename Stack::template GetProtoArg<TcpApi>;
using UdpArg = typename Stack::template GetProtoArg<UdpApi>;

static std::uint64_t fnv(const char *p, std::size_t n) {
    std::uint64_t f = 0xcbf29ce484222325ull;
    for (std::size_t i = 0; i < n; ++i) f = (f ^ (unsigned char)p[i]) * 0x100000001b3ull;
    return f;
}

static std::string hex(const char *p, std::size_t n) {
    static const char d[] = "0123456789abcdef";
    std::string s;
    for (std::size_t i = 0; i < n; ++i) {
        s += d[(unsigned char)p[i] >> 4];
        s += d[(unsigned char)p[i] & 15];
    }
    return s;
}

static std::uint32_t be32(const char *p) {
    return (std::uint32_t)(unsigned char)p[0] << 24 | (std::uint32_t)(unsigned char)p[1] << 16 |
           (std::uint32_t)(unsigned char)p[2] << 8 | (unsigned char)p[3];
}

struct World {
    PlatformFacade<StubPlatform> platform{};
    std::unique_ptr<Stack> stack;
    std::unique_ptr<IpDriverIface<StackArg>> iface;
    std::vector<std::vector<char>> captured;
    std::uint32_t local_addr = 0;

    World(std::size_t mtu, std::uint32_t addr) : local_addr(addr) {
        stack.reset(new Stack(platform));
        IpIfaceDriverParams params;
        params.ip_mtu = mtu;
        params.send_ip4_packet = [this](IpBufRef pkt, Ip4Addr, IpSendRetryRequest *) {
            std::vector<char> copy(pkt.tot_len);
            ipBufTakeBytes(pkt, pkt.tot_len, copy.data());
            captured.push_back(std::move(copy));
            return IpErr::Success;
        };
        params.get_state = []() { return IpIfaceDriverState{}; };
        iface.reset(new IpDriverIface<StackArg>(stack.get(), params));
        iface->iface().setIp4Addr(IpIfaceIp4AddrSetting(8, Ip4Addr(addr)));
    }
    ~World() {
        iface.reset();
        stack.reset();
    }
    void inject(std::vector<char> &pkt) {
        IpBufNode node{pkt.data(), pkt.size(), nullptr};
        iface->recvIp4Packet(IpBufRef{&node, 0, pkt.size()});
    }
};

// An IPv4 packet of the scripted peer: header and checksums by the reference's own code.
static std::vector<char> peerPacket(std::uint32_t src, std::uint32_t dst, std::uint8_t proto,
                                    std::uint16_t ident, const std::vector<char> &l4) {
    std::vector<char> p(20 + l4.size());
    auto h = Ip4Header::MakeRef(p.data());
    h.set(Ip4Header::VersionIhlDscpEcn(), (std::uint16_t)0x4500);
    h.set(Ip4Header::TotalLen(), (std::uint16_t)p.size());
    h.set(Ip4Header::Ident(), ident);
    h.set(Ip4Header::FlagsOffset(), Ip4Flags::DF);
    h.set(Ip4Header::Ttl(), (std::uint8_t)64);
    h.set(Ip4Header::Proto(), Ip4Protocol(proto));
    h.set(Ip4Header::HeaderChksum(), (std::uint16_t)0);
    h.set(Ip4Header::SrcAddr(), Ip4Addr(src));
    h.set(Ip4Header::DstAddr(), Ip4Addr(dst));
    h.set(Ip4Header::HeaderChksum(), IpChksum(p.data(), 20));
    std::memcpy(p.data() + 20, l4.data(), l4.size());
    return p;
}

static std::vector<char> peerTcp(std::uint32_t src, std::uint32_t dst, std::uint16_t sport,
                                 std::uint16_t dport, std::uint32_t seq, std::uint32_t ack,
                                 std::uint16_t flags, std::uint16_t window,
                                 const std::vector<char> &options) {
    std::vector<char> t(20 + options.size());
    auto h = Tcp4Header::MakeRef(t.data());
    h.set(Tcp4Header::SrcPort(), sport);
    h.set(Tcp4Header::DstPort(), dport);
    h.set(Tcp4Header::SeqNum(), TcpSeqNum(seq));
    h.set(Tcp4Header::AckNum(), TcpSeqNum(ack));
    h.set(Tcp4Header::OffsetFlags(), Tcp4Flags((std::uint16_t)((5 + options.size() / 4) << 12 | flags)));
    h.set(Tcp4Header::WindowSize(), window);
    h.set(Tcp4Header::Checksum(), (std::uint16_t)0);
    h.set(Tcp4Header::UrgentPtr(), (std::uint16_t)0);
    std::memcpy(t.data() + 20, options.data(), options.size());
    IpChksumAccumulator acc;
    acc.addWord(WrapType<std::uint32_t>(), src);
    acc.addWord(WrapType<std::uint32_t>(), dst);
    acc.addWord(WrapType<std::uint16_t>(), (std::uint16_t)6);
    acc.addWord(WrapType<std::uint16_t>(), (std::uint16_t)t.size());
    IpBufNode node{t.data(), t.size(), nullptr};
    h.set(Tcp4Header::Checksum(), acc.getChksum(IpBufRef{&node, 0, t.size()}));
    return peerPacket(src, dst, 6, 0, t);
}

// ---- TCP ------------------------------------------------------------------------------------

class Conn : public TcpConnection<TcpArg> {
public:
    bool established = false, aborted = false;
    std::size_t sent = 0;

private:
    void connectionAborted() override { aborted = true; }
    void connectionEstablished() override { established = true; }
    void dataReceived(std::size_t) override {}
    void dataSent(std::size_t amount) override { sent += amount; }
};

struct TcpSession {
    std::unique_ptr<Conn> con;
    std::vector<char> ring;
    IpBufNode ring_node{};
    std::uint32_t peer_addr = 0, peer_isn = 0, iss = 0;
    std::uint16_t peer_port = 0, peer_window = 0;
    unsigned salt = 0;
    std::uint64_t handed = 0;        // stream bytes handed to the ring so far
    std::uint32_t high_end = 0;      // highest sequence end seen (for the retransmit mark)
    bool closed = false;
};

// Prints the packets captured since `from`; returns the (seq, seqlen) of the D ones.
static std::vector<std::pair<std::uint32_t, std::uint32_t>> printTcp(World &w, TcpSession &s,
                                                                     std::size_t from) {
    std::vector<std::pair<std::uint32_t, std::uint32_t>> data;
    for (std::size_t i = from; i < w.captured.size(); ++i) {
        const std::vector<char> &p = w.captured[i];
        const char *t = p.data() + 20;
        const unsigned fl = (unsigned char)t[13], hl = ((unsigned char)t[12] >> 4) * 4;
        const std::size_t dl = p.size() - 20 - hl;
        const std::uint32_t seq = be32(t + 4);
        const std::uint32_t seqlen = (std::uint32_t)dl + ((fl & 0x03) ? 1 : 0);
        char kind;
        if (fl & 0x02) kind = 'S';
        else if (seqlen == 0) kind = 'A';
        else if ((std::int32_t)(seq + seqlen - s.high_end) <= 0) kind = 'R';
        else kind = 'D';
        if (seqlen && (std::int32_t)(seq + seqlen - s.high_end) > 0) s.high_end = seq + seqlen;
        if (kind == 'D') data.emplace_back(seq, seqlen);
        std::printf("P %c %s %s %zu %016llx\n", kind, hex(p.data(), 20).c_str(), hex(t, hl).c_str(),
                    dl, (unsigned long long)fnv(t + hl, dl));
    }
    return data;
}

int main() {
    std::unique_ptr<World> w;
    std::unique_ptr<TcpSession> s;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "S") {
            unsigned long mtu, addr;
            unsigned long long clock;
            in >> mtu >> addr >> clock;
            s.reset();
            w.reset();
            StubPlatform::now = clock;
            w.reset(new World(mtu, (std::uint32_t)addr));
        } else if (what == "U") {
            unsigned long sport, dport, dst, l0, l1, salt;
            long fix;
            in >> sport >> dport >> dst >> l0 >> l1 >> salt >> fix;
            // node 0: room for the headers, then piece 0; node 1: piece 1
            const std::size_t room = UdpApi<UdpArg>::HeaderBeforeUdpData;
            std::vector<char> b0(room + l0), b1(l1 ? l1 : 1);
            for (unsigned long k = 0; k < l0 + l1; ++k) {
                char v = (char)((salt + 3 * k) & 0xFF);
                if (fix >= 0 && k < 2) v = (char)(k == 0 ? fix >> 8 : fix & 0xFF);
                (k < l0 ? b0[room + k] : b1[k - l0]) = v;
            }
            IpBufNode n1{b1.data(), l1, nullptr};
            IpBufNode n0{b0.data(), b0.size(), l1 ? &n1 : nullptr};
            const std::size_t from = w->captured.size();
            UdpTxInfo<UdpArg> info{(std::uint16_t)sport, (std::uint16_t)dport};
            IpErr err = w->stack->getProtoApi<UdpApi>().sendUdpIp4Packet(
                Ip4AddrPair{Ip4Addr(w->local_addr), Ip4Addr((std::uint32_t)dst)}, info,
                IpBufRef{&n0, room, l0 + l1}, nullptr, nullptr, IpSendFlags());
            std::printf("U %d\n", (int)err);
            for (std::size_t i = from; i < w->captured.size(); ++i) {
                const std::vector<char> &p = w->captured[i];
                const bool first = (be32(p.data() + 4) & 0x1FFF) == 0;
                const std::size_t h = 20 + (first ? 8 : 0);
                std::printf("F %s %s %zu %016llx\n", hex(p.data(), 20).c_str(),
                            first ? hex(p.data() + 20, 8).c_str() : "-", p.size() - h,
                            (unsigned long long)fnv(p.data() + h, p.size() - h));
            }
            w->captured.clear();
        } else if (what == "C") {
            unsigned long dst, dport, mss, wnd, ring, salt, pisn;
            long ws;
            in >> dst >> dport >> mss >> wnd >> ws >> ring >> salt >> pisn;
            s.reset(new TcpSession());
            s->con.reset(new Conn());
            s->ring.assign(ring, 0);
            s->ring_node = IpBufNode{s->ring.data(), ring, &s->ring_node};
            s->peer_addr = (std::uint32_t)dst;
            s->peer_port = (std::uint16_t)dport;
            s->peer_window = (std::uint16_t)wnd;
            s->peer_isn = (std::uint32_t)pisn;
            s->salt = (unsigned)salt;
            s->iss = (std::uint32_t)StubPlatform::now;       // make_iss: the clock's low 32 bits
            s->high_end = s->iss;
            const std::size_t from = w->captured.size();
            TcpStartConnectionArgs<TcpArg> args;
            args.addr = Ip4Addr((std::uint32_t)dst);
            args.port = (std::uint16_t)dport;
            args.rcv_wnd = 8192;
            IpErr err = s->con->startConnection(w->stack->getProtoApi<TcpApi>(), args);
            StubPlatform::fireDue();
            if (err == IpErr::Success) {
                std::vector<char> opts;
                if (mss) {
                    const char o[] = {2, 4, (char)(mss >> 8), (char)(mss & 0xFF)};
                    opts.insert(opts.end(), o, o + 4);
                }
                if (ws >= 0) {
                    const char o[] = {1, 3, 3, (char)ws};
                    opts.insert(opts.end(), o, o + 4);
                }
                std::vector<char> synack = peerTcp(
                    s->peer_addr, w->local_addr, s->peer_port, s->con->getLocalPort(), s->peer_isn,
                    s->iss + 1, 0x12, s->peer_window, opts);
                w->inject(synack);
                StubPlatform::fireDue();
            }
            printTcp(*w, *s, from);
            w->captured.clear();
            const bool up = err == IpErr::Success && s->con->established && !s->con->aborted;
            if (up) s->con->setSendBuf(IpBufRef{&s->ring_node, 0, 0});
            std::printf("C %zu %d\n", up ? s->con->getSndBufOverhead() + 1 : (std::size_t)0, (int)up);
        } else if (what == "B") {
            std::size_t push = 0;
            bool fin = false;
            const std::uint64_t start = s->handed;
            std::string tok;
            while (in >> tok) {
                if (tok == "P") {
                    s->con->sendPush();
                    push = (std::size_t)(s->handed - start);
                } else if (tok == "F") {
                    s->con->closeSending();
                    push = (std::size_t)(s->handed - start);   // closeSending pushes all of it
                    fin = s->closed = true;
                } else {
                    const unsigned long n = std::stoul(tok);
                    for (unsigned long k = 0; k < n; ++k, ++s->handed)
                        s->ring[s->handed % s->ring.size()] = (char)((s->salt + 3 * s->handed) & 0xFF);
                    s->con->extendSendBuf(n);
                }
            }
            const IpBufRef sb = s->con->getSendBuf();
            const std::size_t l0 = std::min(sb.tot_len, s->ring.size() - sb.offset);
            std::printf("B %zu %zu %d %zu %zu %zu %d %lu %llu\n", sb.offset, l0, 0, sb.tot_len - l0,
                        s->con->getSndBufOverhead() + 1, push, (int)fin,
                        (unsigned long)(std::uint32_t)(s->iss + 1 + start), (unsigned long long)start);
            const std::size_t from = w->captured.size();
            StubPlatform::fireDue();
            auto data = printTcp(*w, *s, from);
            std::printf("I\n");
            const std::size_t from2 = w->captured.size();
            for (auto &d : data) {
                std::vector<char> ack = peerTcp(s->peer_addr, w->local_addr, s->peer_port,
                                                s->con->getLocalPort(), s->peer_isn + 1,
                                                d.first + d.second, 0x10, s->peer_window, {});
                w->inject(ack);
                StubPlatform::fireDue();
            }
            printTcp(*w, *s, from2);
            w->captured.clear();
        } else if (what == "R") {
            unsigned long port, n;
            in >> port >> n;
            std::vector<std::pair<std::size_t, std::uint64_t>> got;
            UdpListener<UdpArg> lis([&](IpRxInfoIp4<StackArg> const &, UdpRxInfo<UdpArg> const &,
                                        IpBufRef data) {
                std::vector<char> copy(data.tot_len);
                ipBufTakeBytes(data, data.tot_len, copy.data());
                got.emplace_back(copy.size(), fnv(copy.data(), copy.size()));
                return UdpRecvResult::AcceptStop;
            });
            UdpListenParams<UdpArg> lp;
            lp.port = (std::uint16_t)port;
            lis.startListening(w->stack->getProtoApi<UdpApi>(), lp);
            for (unsigned long i = 0; i < n; ++i) {
                std::getline(std::cin, line);
                std::vector<char> pkt(line.size() / 2);
                for (std::size_t k = 0; k < pkt.size(); ++k)
                    pkt[k] = (char)std::stoul(line.substr(2 * k, 2), nullptr, 16);
                w->inject(pkt);
            }
            std::printf("R %zu\n", got.size());
            for (auto &g : got) std::printf("L %zu %016llx\n", g.first, (unsigned long long)g.second);
            w->captured.clear();
        }
        std::printf(".\n");
    }
    s.reset();
    w.reset();
    return 0;
}
