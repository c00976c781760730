// TEST INFRASTRUCTURE -- what the reference stack hands its protocol handlers for received ICMP
// Destination Unreachable messages: the reference's own EthIpIface over its IpStack, instantiated
// on a stub platform and a capture driver of this project's, with two recording protocol handlers
// of this project's (the interface of ip/IpProtocolHandlerStub.h) for the protocol numbers 6 and
// 17. Only reference headers are included; tests/golden/icmp_du_ref.py compiles it against the
// reference tree, drives it and records the calls in tests/golden/icmp_du_ref_cases.json.
//
// The platform: a clock that stands still and timers that never fire. The driver's send_frame
// throws the frame away.
//
// One request per line:
//   S <addr> <prefix> <gateway, or 0 for none> <mac hex>
//        a fresh stack and an interface <addr>/<prefix> with the MAC. No answer.
//   F <hex, or - for no bytes>
//        the Ethernet frame is injected (EthIpIface::recvFrame) -> one line per handler call, in
//        the order they happened, then ".":
//          "D <handler> <code> <rest hex> <src_addr> <dst_addr> <ttl> <proto> <header_len>
//             <dgram_initial hex, or ->"        handleIp4DestUnreach
//          "R <handler>"                        recvIp4Dgram
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
#include <aipstack/misc/NonCopyable.h>
#include <aipstack/structure/index/AvlTreeIndex.h>
#include <aipstack/structure/minimum/LinkedHeap.h>
#include <aipstack/platform/PlatformFacade.h>
#include <aipstack/infra/Buf.h>
#include <aipstack/infra/BufUtils.h>
#include <aipstack/infra/Err.h>
#include <aipstack/infra/Instance.h>
#include <aipstack/ip/IpAddr.h>
#include <aipstack/ip/IpStack.h>
#include <aipstack/ip/IpPathMtuCache.h>
#include <aipstack/ip/IpReassembly.h>
#include <aipstack/proto/Ip4Proto.h>
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
    return s.empty() ? "-" : s;
}

static std::vector<std::string> g_events;

// A protocol handler that records what the stack calls it with.
template <typename Arg>
class RecordingHandler : private NonCopyable<RecordingHandler<Arg>> {
public:
    using StackArg = typename Arg::StackArg;
    inline static constexpr unsigned Number = (unsigned)Arg::Params::IpProtocolNumber;

    RecordingHandler(IpProtocolHandlerArgs<StackArg>) {}
    RecordingHandler<Arg> &getApi() { return *this; }

    void recvIp4Dgram(IpRxInfoIp4<StackArg> const &, IpBufRef) {
        g_events.push_back("R " + std::to_string(Number));
    }

    void handleIp4DestUnreach(Ip4DestUnreachMeta const &du_meta, IpRxInfoIp4<StackArg> const &ip_info,
                              IpBufRef dgram_initial) {
        std::vector<char> copy(dgram_initial.tot_len);
        ipBufTakeBytes(dgram_initial, dgram_initial.tot_len, copy.data());
        std::ostringstream o;
        o << "D " << Number << ' ' << (unsigned)du_meta.icmp_code << ' '
          << hex(du_meta.icmp_rest.data(), 4) << ' ' << ip_info.src_addr.value() << ' '
          << ip_info.dst_addr.value() << ' ' << (unsigned)ip_info.ttl << ' ' << (unsigned)ip_info.proto
          << ' ' << (unsigned)ip_info.header_len << ' ' << hex(copy.data(), copy.size());
        g_events.push_back(o.str());
    }
};

template <unsigned P>
struct RecordingService {
    inline static constexpr Ip4Protocol IpProtocolNumber = Ip4Protocol(P);
    template <typename PlatformImpl_, typename StackArg_>
    struct Compose {
        using PlatformImpl = PlatformImpl_;
        using StackArg = StackArg_;
        using Params = RecordingService;
        AIPSTACK_DEF_INSTANCE(Compose, RecordingHandler)
    };
};

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
    using ProtocolServices = MakeTypeList<RecordingService<6>, RecordingService<17>>;
    class StackArg : public StackService::template Compose<StubPlatform, ProtocolServices> {};
    using Stack = IpStack<StackArg>;
    using EthService = EthIpIfaceService<
        EthIpIfaceOptions::NumArpEntries::Is<16>, EthIpIfaceOptions::ArpProtectCount::Is<8>,
        EthIpIfaceOptions::HeaderBeforeEth::Is<0>,
        EthIpIfaceOptions::TimersStructureService::Is<LinkedHeapService>>;
    class EthArg : public EthService::template Compose<StubPlatform, StackArg> {};
    using Eth = EthIpIface<EthArg>;

    PlatformFacade<StubPlatform> platform{};
    MacAddr mac;
    std::unique_ptr<Stack> stack;
    std::unique_ptr<Eth> eth;

    World(std::uint32_t addr, unsigned prefix, std::uint32_t gateway, MacAddr mac_) : mac(mac_) {
        stack.reset(new Stack(platform));
        EthIfaceDriverParams params;
        params.eth_mtu = 1514;
        params.mac_addr = &mac;
        params.send_frame = [](IpBufRef) { return IpErr::Success; };
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
        eth.reset();
        stack.reset();
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
        } else if (what == "F") {
            std::string h;
            in >> h;
            std::vector<char> frame = unhex(h);
            g_events.clear();
            w->inject(frame);
            for (auto &e : g_events) std::printf("%s\n", e.c_str());
            std::printf(".\n");
            g_events.clear();
        }
    }
    w.reset();
    return 0;
}
