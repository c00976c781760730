// TEST INFRASTRUCTURE -- the TCP segments without data that the reference stack sends on behalf of
// its connections (SYN, SYN-ACK, empty ACK, window update, FIN, RST): the reference's own
// EthIpIface (its ARP table included) over its IpStack with IpTcpProto, TcpListeners that accept
// and TcpConnections, instantiated on a platform and a capture driver of this project's. Only
// reference headers are included; tests/golden/tcp_ctl_ref.py compiles it against the reference
// tree, drives it and records what was sent in tests/golden/tcp_ctl_ref_cases.json.
//
// The platform: a clock that only moves when told to, and timers that fire, in the order of their
// times, while it moves. The ISS is the clock's value (IpTcpProto::make_iss). The driver's
// send_frame copies each Ethernet frame into the event list and returns success.
//
// One request per line; every one but S, L and Q answers "T <hex>" per frame sent, in full, in
// the order they happened, then ".":
//   S <addr> <prefix> <gateway, or 0 for none> <mac hex> <clock>
//        a fresh stack and an interface <addr>/<prefix> with the MAC, the clock at <clock>.
//   L <addr, or 0 for any> <port> <initial receive window> <receive buffer>
//        a TcpListener (max_pcbs 8) whose handler accepts into a new connection (numbered in the
//        order connections arise) with a ring buffer of <receive buffer> bytes.
//   Q <hex>
//        the Ethernet frame is injected and whatever it causes is thrown away (the ARP packet
//        that makes the next hop's MAC known).
//   F <hex>                  the Ethernet frame is injected (EthIpIface::recvFrame).
//   C <addr> <port> <rcv_wnd> <receive buffer>
//        a new connection (the next number) and startConnection to <addr>:<port>.
//   A <ticks>                the clock advances by <ticks> (1000 per second).
//   X <connection> <bytes>   the application has read <bytes>: extendRecvBuf.
//   R <connection> <0|1>     TcpConnection::reset(have_unprocessed_data).
#include <algorithm>
#include <array>
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
#include <aipstack/structure/minimum/LinkedHeap.h>
#include <aipstack/platform/PlatformFacade.h>
#include <aipstack/infra/Buf.h>
#include <aipstack/infra/BufUtils.h>
#include <aipstack/infra/Err.h>
#include <aipstack/ip/IpAddr.h>
#include <aipstack/ip/IpStack.h>
#include <aipstack/ip/IpPathMtuCache.h>
#include <aipstack/ip/IpReassembly.h>
#include <aipstack/tcp/IpTcpProto.h>
#include <aipstack/tcp/TcpApi.h>
#include <aipstack/tcp/TcpListener.h>
#include <aipstack/tcp/TcpConnection.h>
#include <aipstack/eth/MacAddr.h>
#include <aipstack/eth/EthHw.h>
#include <aipstack/eth/EthIpIface.h>

using namespace AIpStack;

struct SimPlatform {
    inline static constexpr bool ImplIsStatic = true;
    using TimeType = std::uint64_t;
    inline static constexpr double TimeFreq = 1000.0;
    inline static constexpr TimeType RelativeTimeLimit = ~TimeType(0) / 4;
    class Timer;
    inline static TimeType now = 1000;
    inline static std::vector<Timer *> timers;
    static TimeType getTime() { return now; }
    static TimeType getEventTime() { return now; }
    class Timer {
    public:
        Timer(PlatformRef<SimPlatform>, Function<void()> handler) : m_handler(handler) {
            timers.push_back(this);
        }
        ~Timer() { timers.erase(std::find(timers.begin(), timers.end(), this)); }
        Timer(const Timer &) = delete;
        Timer &operator=(const Timer &) = delete;
        PlatformRef<SimPlatform> ref() const { return PlatformRef<SimPlatform>(); }
        bool isSet() const { return m_set; }
        TimeType getSetTime() const { return m_time; }
        void unset() { m_set = false; }
        void setAt(TimeType t) {
            m_set = true;
            m_time = t;
        }
        void fire() {
            m_set = false;
            m_handler();
        }

    private:
        Function<void()> m_handler;
        bool m_set = false;
        TimeType m_time = 0;
    };
    // Move the clock to now + ticks; a timer due on the way fires at its own time.
    static void advance(TimeType ticks) {
        const TimeType target = now + ticks;
        for (;;) {
            Timer *next = nullptr;
            for (Timer *t : timers)
                if (t->isSet() && t->getSetTime() <= target &&
                    (next == nullptr || t->getSetTime() < next->getSetTime()))
                    next = t;
            if (next == nullptr) break;
            if (next->getSetTime() > now) now = next->getSetTime();
            next->fire();
        }
        now = target;
    }
};

static std::string hex(const char *p, std::size_t n) {
    static const char d[] = "0123456789abcdef";
    std::string s;
    for (std::size_t k = 0; k < n; ++k) {
        s += d[(unsigned char)p[k] >> 4];
        s += d[(unsigned char)p[k] & 15];
    }
    return s;
}

struct World {
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
    using ProtocolServices = MakeTypeList<IpTcpProtoService<
        IpTcpProtoOptions::NumTcpPcbs::Is<64>, IpTcpProtoOptions::PcbIndexService::Is<IndexService>>>;
    class StackArg : public StackService::template Compose<SimPlatform, ProtocolServices> {};
    using Stack = IpStack<StackArg>;
    using TcpArg = typename Stack::template GetProtoArg<TcpApi>;
    using EthService = EthIpIfaceService<
        EthIpIfaceOptions::NumArpEntries::Is<16>, EthIpIfaceOptions::ArpProtectCount::Is<8>,
        EthIpIfaceOptions::HeaderBeforeEth::Is<0>,
        EthIpIfaceOptions::TimersStructureService::Is<LinkedHeapService>>;
    class EthArg : public EthService::template Compose<SimPlatform, StackArg> {};
    using Eth = EthIpIface<EthArg>;

    struct Conn : public TcpConnection<TcpArg> {
        std::vector<char> ring;
        IpBufNode node;
        explicit Conn(std::size_t room) : ring(room ? room : 1) {
            node = IpBufNode{ring.data(), ring.size(), &node};
        }
        ~Conn() { this->reset(); }
        void giveRecvBuf(std::size_t room) { this->setRecvBuf(IpBufRef{&node, 0, room}); }
        void connectionAborted() override {}
        void dataReceived(std::size_t) override {}
        void dataSent(std::size_t) override {}
    };

    struct Lis {
        World *world;
        std::size_t room;
        TcpListener<TcpArg> lis;
        Lis(World *w, std::size_t room_)
            : world(w), room(room_), lis(AIPSTACK_BIND_MEMBER(&Lis::established, this)) {}
        void established() {
            std::unique_ptr<Conn> c(new Conn(room));
            if (c->acceptConnection(lis) != IpErr::Success) {
                std::fprintf(stderr, "tcp_ctl_ref_gen: acceptConnection failed\n");
                std::exit(2);
            }
            c->giveRecvBuf(room);
            world->conns.push_back(std::move(c));
        }
    };

    PlatformFacade<SimPlatform> platform{};
    MacAddr mac;
    std::vector<std::string> events;
    std::unique_ptr<Stack> stack;
    std::unique_ptr<Eth> eth;
    std::vector<std::unique_ptr<Lis>> listeners;
    std::vector<std::unique_ptr<Conn>> conns;

    World(std::uint32_t addr, unsigned prefix, std::uint32_t gateway, MacAddr mac_) : mac(mac_) {
        stack.reset(new Stack(platform));
        EthIfaceDriverParams params;
        params.eth_mtu = 1514;
        params.mac_addr = &mac;
        params.send_frame = [this](IpBufRef frame) {
            std::vector<char> copy(frame.tot_len);
            ipBufTakeBytes(frame, frame.tot_len, copy.data());
            events.push_back("T " + hex(copy.data(), copy.size()));
            return IpErr::Success;
        };
        params.get_eth_state = []() {
            EthIfaceState st = {};
            st.link_up = true;
            return st;
        };
        eth.reset(new Eth(platform, stack.get(), params));
        eth->iface().setIp4Addr(IpIfaceIp4AddrSetting((std::uint8_t)prefix, Ip4Addr(addr)));
        if (gateway != 0) eth->iface().setIp4Gateway(IpIfaceIp4GatewaySetting(Ip4Addr(gateway)));
    }
    ~World() {
        conns.clear();
        listeners.clear();
        eth.reset();
        stack.reset();
    }

    bool listen(std::uint32_t addr, unsigned port, std::size_t wnd, std::size_t room) {
        listeners.emplace_back(new Lis(this, room));
        TcpListenParams lp;
        lp.addr = Ip4Addr(addr);
        lp.port = (std::uint16_t)port;
        lp.max_pcbs = 8;
        if (!listeners.back()->lis.startListening(stack->template getProtoApi<TcpApi>(), lp)) return false;
        listeners.back()->lis.setInitialReceiveWindow(wnd);
        return true;
    }

    bool connect(std::uint32_t addr, unsigned port, std::size_t wnd, std::size_t room) {
        conns.emplace_back(new Conn(room));
        TcpStartConnectionArgs<TcpArg> args;
        args.addr = Ip4Addr(addr);
        args.port = (std::uint16_t)port;
        args.rcv_wnd = wnd;
        if (conns.back()->startConnection(stack->template getProtoApi<TcpApi>(), args) != IpErr::Success)
            return false;
        conns.back()->giveRecvBuf(room);
        return true;
    }

    void inject(std::vector<char> &frame) {
        // a heap block of exactly the frame's length
        IpBufNode node{frame.data(), frame.size(), nullptr};
        eth->recvFrame(IpBufRef{&node, 0, frame.size()});
    }
};

static std::vector<char> unhex(const std::string &h) {
    if (h == "-") return {};
    std::vector<char> v(h.size() / 2);
    for (std::size_t k = 0; k < v.size(); ++k) v[k] = (char)std::stoul(h.substr(2 * k, 2), nullptr, 16);
    return v;
}

static int fail(const char *what) {
    std::fprintf(stderr, "tcp_ctl_ref_gen: %s\n", what);
    return 2;
}

int main() {
    std::unique_ptr<World> w;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        bool answer = true;
        if (what == "S") {
            unsigned long addr, prefix, gateway;
            unsigned long long clock;
            std::string mac;
            in >> addr >> prefix >> gateway >> mac >> clock;
            const std::vector<char> m = unhex(mac);
            std::array<std::uint8_t, 6> bytes;
            std::memcpy(bytes.data(), m.data(), 6);
            w.reset();
            SimPlatform::now = clock;
            w.reset(new World((std::uint32_t)addr, (unsigned)prefix, (std::uint32_t)gateway,
                              MacAddr(bytes)));
            answer = false;
        } else if (what == "L") {
            unsigned long addr, port, wnd, room;
            in >> addr >> port >> wnd >> room;
            if (!w->listen((std::uint32_t)addr, (unsigned)port, wnd, room)) return fail("startListening failed");
            answer = false;
        } else if (what == "Q" || what == "F") {
            std::string h;
            in >> h;
            std::vector<char> frame = unhex(h);
            w->inject(frame);
            answer = what == "F";
        } else if (what == "C") {
            unsigned long addr, port, wnd, room;
            in >> addr >> port >> wnd >> room;
            if (!w->connect((std::uint32_t)addr, (unsigned)port, wnd, room)) return fail("startConnection failed");
        } else if (what == "A") {
            unsigned long long ticks;
            in >> ticks;
            SimPlatform::advance(ticks);
        } else if (what == "X" || what == "R") {
            unsigned long c, v;
            in >> c >> v;
            if (c >= w->conns.size()) return fail("no such connection");
            if (what == "X") w->conns[c]->extendRecvBuf(v);
            else w->conns[c]->reset(v != 0);
        } else {
            continue;
        }
        if (answer) {
            for (auto &e : w->events) std::printf("%s\n", e.c_str());
            std::printf(".\n");
            std::fflush(stdout);  // the driver reads each answer before it writes the next request
        }
        w->events.clear();
    }
    w.reset();
    return 0;
}
