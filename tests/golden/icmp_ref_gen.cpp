// TEST INFRASTRUCTURE -- what the reference stack answers to received IPv4 packets with ICMP: the
// reference's own IpStack with IpUdpProto (no listener: every UDP datagram for the interface's
// address finds a closed port), instantiated on a stub platform and a capture driver of this
// project's. Only reference headers are included; tests/golden/icmp_ref.py compiles it against
// the reference tree, drives it and records the answers in tests/golden/icmp_ref_cases.json.
//
// The platform: a clock that stands still and timers that never fire. The interface is a bare
// IpDriverIface (no Ethernet, no ARP) whose send_ip4_packet copies each IP packet into a capture
// list and returns success; it has a gateway, so that every destination has a route.
//
// One request per line:
//   S <allow> <mtu> <addr> <prefix> <gateway> <warm>
//        a fresh stack with IpStackOptions::AllowBroadcastPing = <allow> (0 / 1), the interface
//        <addr>/<prefix>; then <warm> echo requests from the gateway are injected and their
//        replies dropped, which leaves the stack's next Ident at <warm> mod 2^16. No answer.
//   I <hex>
//        the IP packet is injected -> "P <hex>" per captured packet, in full, then "."
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
#include <aipstack/proto/Icmp4Proto.h>
#include <aipstack/ip/IpAddr.h>
#include <aipstack/ip/IpStack.h>
#include <aipstack/ip/IpDriverIface.h>
#include <aipstack/ip/IpPathMtuCache.h>
#include <aipstack/ip/IpReassembly.h>
#include <aipstack/udp/IpUdpProto.h>

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

struct World {
    virtual ~World() {}
    virtual void inject(std::vector<char> &pkt) = 0;
    std::vector<std::vector<char>> captured;
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

    PlatformFacade<StubPlatform> platform{};
    std::unique_ptr<Stack> stack;
    std::unique_ptr<IpDriverIface<StackArg>> iface;

    WorldOf(std::size_t mtu, std::uint32_t addr, unsigned prefix, std::uint32_t gateway) {
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
        iface->iface().setIp4Addr(IpIfaceIp4AddrSetting((std::uint8_t)prefix, Ip4Addr(addr)));
        iface->iface().setIp4Gateway(IpIfaceIp4GatewaySetting(Ip4Addr(gateway)));
    }
    ~WorldOf() override {
        iface.reset();
        stack.reset();
    }
    void inject(std::vector<char> &pkt) override {
        // a heap block of exactly the packet's length
        IpBufNode node{pkt.data(), pkt.size(), nullptr};
        iface->recvIp4Packet(IpBufRef{&node, 0, pkt.size()});
    }
};

static std::string hex(const std::vector<char> &p) {
    static const char d[] = "0123456789abcdef";
    std::string s;
    for (char c : p) {
        s += d[(unsigned char)c >> 4];
        s += d[(unsigned char)c & 15];
    }
    return s;
}

// An echo request without data from `src` to `dst`: header and checksums by the reference's code.
static std::vector<char> ping(std::uint32_t src, std::uint32_t dst) {
    std::vector<char> p(28, 0);
    auto h = Ip4Header::MakeRef(p.data());
    h.set(Ip4Header::VersionIhlDscpEcn(), (std::uint16_t)0x4500);
    h.set(Ip4Header::TotalLen(), (std::uint16_t)p.size());
    h.set(Ip4Header::Ident(), (std::uint16_t)0);
    h.set(Ip4Header::FlagsOffset(), Ip4Flags((std::uint16_t)0));
    h.set(Ip4Header::Ttl(), (std::uint8_t)64);
    h.set(Ip4Header::Proto(), Ip4Protocol::Icmp);
    h.set(Ip4Header::HeaderChksum(), (std::uint16_t)0);
    h.set(Ip4Header::SrcAddr(), Ip4Addr(src));
    h.set(Ip4Header::DstAddr(), Ip4Addr(dst));
    h.set(Ip4Header::HeaderChksum(), IpChksum(p.data(), 20));
    auto ic = Icmp4Header::MakeRef(p.data() + 20);
    ic.set(Icmp4Header::Type(), Icmp4Type::EchoRequest);
    ic.set(Icmp4Header::Chksum(), (std::uint16_t)0);
    ic.set(Icmp4Header::Chksum(), IpChksum(p.data() + 20, 8));
    return p;
}

int main() {
    std::unique_ptr<World> w;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "S") {
            unsigned long allow, mtu, addr, prefix, gateway, warm;
            in >> allow >> mtu >> addr >> prefix >> gateway >> warm;
            w.reset();
            if (allow) w.reset(new WorldOf<true>(mtu, (std::uint32_t)addr, (unsigned)prefix, (std::uint32_t)gateway));
            else w.reset(new WorldOf<false>(mtu, (std::uint32_t)addr, (unsigned)prefix, (std::uint32_t)gateway));
            std::vector<char> p = ping((std::uint32_t)gateway, (std::uint32_t)addr);
            for (unsigned long k = 0; k < warm; ++k) {
                w->inject(p);
                if (w->captured.size() != 1) {
                    std::fprintf(stderr, "icmp_ref_gen: a warm-up request got no reply\n");
                    return 2;
                }
                w->captured.clear();
            }
        } else if (what == "I") {
            std::string h;
            in >> h;
            std::vector<char> pkt(h.size() / 2);
            for (std::size_t k = 0; k < pkt.size(); ++k)
                pkt[k] = (char)std::stoul(h.substr(2 * k, 2), nullptr, 16);
            w->inject(pkt);
            for (auto &c : w->captured) std::printf("P %s\n", hex(c).c_str());
            w->captured.clear();
            std::printf(".\n");
        }
    }
    w.reset();
    return 0;
}
