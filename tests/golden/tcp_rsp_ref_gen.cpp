// TEST INFRASTRUCTURE -- what the reference stack answers to received Ethernet frames that carry
// TCP segments of no connection: the reference's own EthIpIface (its ARP table included) over its
// IpStack with IpTcpProto, instantiated on a stub platform and a capture driver of this
// project's, with TcpListeners that never accept. Only reference headers are included;
// tests/golden/tcp_rsp_ref.py compiles it against the reference tree, drives it and records the
// answers in tests/golden/tcp_rsp_ref_cases.json.
//
// The platform: a clock that stands still and timers that never fire. The driver's send_frame
// copies each Ethernet frame into the event list and returns success.
//
// One request per line:
//   S <addr> <prefix> <gateway, or 0 for none> <mac hex>
//        a fresh stack and an interface <addr>/<prefix> with the MAC. No answer.
//   L <addr, or 0 for any> <port>
//        a TcpListener (max_pcbs 8); a later one stands in front of an earlier one. No answer.
//   Q <hex>
//        the Ethernet frame is injected and whatever it causes is thrown away: the ARP packet that
//        makes the next hop's MAC known, so that the answer is not held back by ARP resolution.
//   F <hex, or - for no bytes>
//        the Ethernet frame is injected (EthIpIface::recvFrame) -> "T <hex>" per frame sent, in
//        full, in the order they happened, then "."
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
        IpTcpProtoOptions::NumTcpPcbs::Is<16>, IpTcpProtoOptions::PcbIndexService::Is<IndexService>>>;
    class StackArg : public StackService::template Compose<StubPlatform, ProtocolServices> {};
    using Stack = IpStack<StackArg>;
    using TcpArg = typename Stack::template GetProtoArg<TcpApi>;
    using EthService = EthIpIfaceService<
        EthIpIfaceOptions::NumArpEntries::Is<16>, EthIpIfaceOptions::ArpProtectCount::Is<8>,
        EthIpIfaceOptions::HeaderBeforeEth::Is<0>,
        EthIpIfaceOptions::TimersStructureService::Is<LinkedHeapService>>;
    class EthArg : public EthService::template Compose<StubPlatform, StackArg> {};
    using Eth = EthIpIface<EthArg>;

    PlatformFacade<StubPlatform> platform{};
    MacAddr mac;
    std::vector<std::string> events;
    std::unique_ptr<Stack> stack;
    std::unique_ptr<Eth> eth;
    std::vector<std::unique_ptr<TcpListener<TcpArg>>> listeners;

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
        listeners.clear();
        eth.reset();
        stack.reset();
    }

    bool listen(std::uint32_t addr, unsigned port) {
        listeners.emplace_back(new TcpListener<TcpArg>([]() {}));
        TcpListenParams lp;
        lp.addr = Ip4Addr(addr);
        lp.port = (std::uint16_t)port;
        lp.max_pcbs = 8;
        return listeners.back()->startListening(stack->template getProtoApi<TcpApi>(), lp);
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

int main() {
    std::unique_ptr<World> w;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "S") {
            unsigned long addr, prefix, gateway;
            std::string mac;
            in >> addr >> prefix >> gateway >> mac;
            const std::vector<char> m = unhex(mac);
            std::array<std::uint8_t, 6> bytes;
            std::memcpy(bytes.data(), m.data(), 6);
            w.reset();
            w.reset(new World((std::uint32_t)addr, (unsigned)prefix, (std::uint32_t)gateway,
                              MacAddr(bytes)));
        } else if (what == "L") {
            unsigned long addr, port;
            in >> addr >> port;
            if (!w->listen((std::uint32_t)addr, (unsigned)port)) {
                std::fprintf(stderr, "tcp_rsp_ref_gen: startListening failed\n");
                return 2;
            }
        } else if (what == "Q" || what == "F") {
            std::string h;
            in >> h;
            std::vector<char> frame = unhex(h);
            w->inject(frame);
            if (what == "F") {
                for (auto &e : w->events) std::printf("%s\n", e.c_str());
                std::printf(".\n");
            }
            w->events.clear();
        }
    }
    w.reset();
    return 0;
}
