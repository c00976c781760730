// TEST INFRASTRUCTURE -- what the reference stack does with a SESSION of received Ethernet frames:
// the reference's own EthIpIface (its ARP table included) over its IpStack with IpUdpProto, one
// stack that keeps its state from frame to frame, instantiated on a stub platform and a capture
// driver of this project's, with UdpListeners and UdpAssociations whose handlers record their
// calls and accept. Only reference headers are included; tests/golden/rx_loop_ref.py compiles it
// against the reference tree, drives it and records the answers in
// tests/golden/rx_loop_ref_cases.json.
//
// The platform: a clock that stands still and timers that never fire. The driver's send_frame
// copies each Ethernet frame into the event list and returns success. The interface has no
// gateway, so only its own subnet has a route.
//
// One request per line:
//   S <allow> <addr> <prefix> <mac hex>
//        a fresh stack with IpStackOptions::AllowBroadcastPing = <allow> (0 / 1) and an interface
//        <addr>/<prefix> with the MAC. No answer.
//   L <iface_addr> <port> <accept_broadcast> <accept_nonlocal_dst>
//        a UdpListener, number = how many came before. No answer.
//   A <local_addr> <remote_addr> <local_port> <remote_port> <accept_nonlocal_dst>
//        a UdpAssociation, numbered likewise. No answer.
//   F <hex, or - for no bytes>
//        the Ethernet frame is injected (EthIpIface::recvFrame) -> "C <L|A><number> <data length>"
//        per handler call and "T <hex>" per frame sent, in full, in the order they happened, then "."
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
#include <aipstack/udp/IpUdpProto.h>
#include <aipstack/eth/MacAddr.h>
#include <aipstack/eth/EthHw.h>
#include <aipstack/eth/EthIpIface.h>

using namespace AIpStack;

struct StubPlatform {
    inline static constexpr bool ImplIsStatic = true;
    using TimeType = std::uint64_t;
    inline static constexpr double TimeFreq = 1000.0;
    inline static constexpr TimeType RelativeTimeLimit = ~TimeType(0);
    static TimeType getTime() { return 1000; }
    static TimeType getEventTime() { return 1000; }
    class Timer {
    public:
        Timer(PlatformRef<StubPlatform>, Function<void()>) {}
        PlatformRef<StubPlatform> ref() const { return PlatformRef<StubPlatform>(); }
        bool isSet() const { return m_set; }
        TimeType getSetTime() const { return m_time; }
        void unset() { m_set = false; }
        void setAt(TimeType t) {
            m_set = true;
            m_time = t;
        }

    private:
        bool m_set = false;
        TimeType m_time = 0;
    };
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
    std::vector<std::string> events;
    virtual ~World() {}
    virtual bool listen(std::uint32_t iface_addr, unsigned port, bool bcast, bool nonlocal) = 0;
    virtual bool associate(std::uint32_t la, std::uint32_t ra, unsigned lp, unsigned rp, bool nonlocal) = 0;
    virtual void inject(std::vector<char> &frame) = 0;
};

template <bool AllowBcastPing>
struct WorldOf : World {
    using IndexService = AvlTreeIndexService;
    using StackService = IpStackService<
        IpStackOptions::HeaderBeforeIp::Is<14>,
        IpStackOptions::AllowBroadcastPing::Is<AllowBcastPing>,
        IpStackOptions::PathMtuCacheService::Is<IpPathMtuCacheService<
            IpPathMtuCacheOptions::NumMtuEntries::Is<16>,
            IpPathMtuCacheOptions::MtuIndexService::Is<IndexService>>>,
        IpStackOptions::ReassemblyService::Is<IpReassemblyService<
            IpReassemblyOptions::MaxReassEntrys::Is<16>,
            IpReassemblyOptions::MaxReassSize::Is<65531>,
            IpReassemblyOptions::MaxReassHoles::Is<250>>>>;
    using ProtocolServices =
        MakeTypeList<IpUdpProtoService<IpUdpProtoOptions::UdpIndexService::Is<IndexService>>>;
    class StackArg : public StackService::template Compose<StubPlatform, ProtocolServices> {};
    using Stack = IpStack<StackArg>;
    using UdpArg = typename Stack::template GetProtoArg<UdpApi>;
    using EthService = EthIpIfaceService<
        EthIpIfaceOptions::NumArpEntries::Is<16>, EthIpIfaceOptions::ArpProtectCount::Is<8>,
        EthIpIfaceOptions::HeaderBeforeEth::Is<0>,
        EthIpIfaceOptions::TimersStructureService::Is<LinkedHeapService>>;
    class EthArg : public EthService::template Compose<StubPlatform, StackArg> {};
    using Eth = EthIpIface<EthArg>;

    // What a handler knows of itself (the reference's Function holds one pointer).
    struct Tag {
        WorldOf *world;
        char kind;
        unsigned number;
    };

    PlatformFacade<StubPlatform> platform{};
    MacAddr mac;
    std::vector<std::unique_ptr<Tag>> tags;
    std::unique_ptr<Stack> stack;
    std::unique_ptr<Eth> eth;
    std::vector<std::unique_ptr<UdpListener<UdpArg>>> listeners;
    std::vector<std::unique_ptr<UdpAssociation<UdpArg>>> assocs;

    WorldOf(std::uint32_t addr, unsigned prefix, MacAddr mac_) : mac(mac_) {
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
    }
    ~WorldOf() override {
        listeners.clear();
        assocs.clear();
        eth.reset();
        stack.reset();
    }

    UdpRecvResult record(Tag *tag, IpBufRef data) {
        events.push_back(std::string("C ") + tag->kind + std::to_string(tag->number) + " " +
                         std::to_string(data.tot_len));
        return UdpRecvResult::AcceptContinue;
    }

    bool listen(std::uint32_t iface_addr, unsigned port, bool bcast, bool nonlocal) override {
        tags.emplace_back(new Tag{this, 'L', (unsigned)listeners.size()});
        Tag *tag = tags.back().get();
        listeners.emplace_back(new UdpListener<UdpArg>(
            [tag](IpRxInfoIp4<StackArg> const &, UdpRxInfo<UdpArg> const &, IpBufRef data) {
                return tag->world->record(tag, data);
            }));
        UdpListenParams<UdpArg> lp;
        lp.iface_addr = Ip4Addr(iface_addr);
        lp.port = (std::uint16_t)port;
        lp.accept_broadcast = bcast;
        lp.accept_nonlocal_dst = nonlocal;
        return listeners.back()->startListening(stack->template getProtoApi<UdpApi>(), lp) == IpErr::Success;
    }

    bool associate(std::uint32_t la, std::uint32_t ra, unsigned lp, unsigned rp, bool nonlocal) override {
        tags.emplace_back(new Tag{this, 'A', (unsigned)assocs.size()});
        Tag *tag = tags.back().get();
        assocs.emplace_back(new UdpAssociation<UdpArg>(
            [tag](IpRxInfoIp4<StackArg> const &, UdpRxInfo<UdpArg> const &, IpBufRef data) {
                return tag->world->record(tag, data);
            }));
        UdpAssociationParams<UdpArg> ap;
        ap.key = UdpAssociationKey{Ip4Addr(la), Ip4Addr(ra), (std::uint16_t)lp, (std::uint16_t)rp};
        ap.accept_nonlocal_dst = nonlocal;
        return assocs.back()->associate(stack->template getProtoApi<UdpApi>(), ap) == IpErr::Success;
    }

    void inject(std::vector<char> &frame) override {
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

int main() {
    std::unique_ptr<World> w;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "S") {
            unsigned long allow, addr, prefix;
            std::string mac;
            in >> allow >> addr >> prefix >> mac;
            const std::vector<char> m = unhex(mac);
            std::array<std::uint8_t, 6> bytes;
            std::memcpy(bytes.data(), m.data(), 6);
            w.reset();
            if (allow) w.reset(new WorldOf<true>((std::uint32_t)addr, (unsigned)prefix, MacAddr(bytes)));
            else w.reset(new WorldOf<false>((std::uint32_t)addr, (unsigned)prefix, MacAddr(bytes)));
        } else if (what == "L") {
            unsigned long iface_addr, port, bcast, nonlocal;
            in >> iface_addr >> port >> bcast >> nonlocal;
            if (!w->listen((std::uint32_t)iface_addr, (unsigned)port, bcast != 0, nonlocal != 0)) {
                std::fprintf(stderr, "rx_loop_ref_gen: startListening failed\n");
                return 2;
            }
        } else if (what == "A") {
            unsigned long la, ra, lp, rp, nonlocal;
            in >> la >> ra >> lp >> rp >> nonlocal;
            if (!w->associate((std::uint32_t)la, (std::uint32_t)ra, (unsigned)lp, (unsigned)rp, nonlocal != 0)) {
                std::fprintf(stderr, "rx_loop_ref_gen: associate failed\n");
                return 2;
            }
        } else if (what == "F") {
            std::string h;
            in >> h;
            std::vector<char> frame = unhex(h);
            w->inject(frame);
            for (auto &e : w->events) std::printf("%s\n", e.c_str());
            w->events.clear();
            std::printf(".\n");
        }
    }
    w.reset();
    return 0;
}
