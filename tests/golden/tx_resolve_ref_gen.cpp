// TEST INFRASTRUCTURE -- what the reference stack does with a datagram handed to
// IpStack::sendIp4Dgram: the route, the permission tests, the ARP lookup of
// EthIpIface::driverSendIp4Packet and the Ethernet header. The reference's own IpStack with one to
// three of its EthIpIface, instantiated on a stub platform and capture drivers of this project's.
// Only reference headers are included; tests/golden/tx_resolve_ref.py compiles it against the
// reference tree, drives it and records the answers in tests/golden/tx_resolve_ref_cases.json.
//
// The platform: a clock that stands still and timers that never fire, so no ARP entry times out.
// Each driver's send_frame notes which interface was handed the frame and returns success.
//
// One request per line:
//   S <n> then n times: <have> <addr> <prefix> <have_gw> <gateway> <mac hex>
//        a fresh stack and n interfaces, constructed in this order (the stack's list iterates
//        them last-constructed first, ip/IpIface.h:97). No answer.
//   F <k> <hex>
//        the Ethernet frame is injected into interface k (EthIpIface::recvFrame)
//   D <src> <dst> <send flags> <k, or -1 for no interface>
//        sendIp4Dgram of 8 payload bytes, protocol 17, TTL 64 -> "E <IpErr>" first
// Both answer with one line per frame a driver was handed, in order, then ".":
//   "T <k> <hex of the first 14 bytes>" for EtherType 0x0800, "Q <k> <hex of the whole frame>"
//   for any other (the ARP requests and replies).
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
#include <aipstack/infra/TxAllocHelper.h>
#include <aipstack/ip/IpAddr.h>
#include <aipstack/ip/IpStack.h>
#include <aipstack/ip/IpPathMtuCache.h>
#include <aipstack/ip/IpReassembly.h>
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

struct IfaceSpec {
    bool have, have_gw;
    std::uint32_t addr, gateway;
    unsigned prefix;
    MacAddr mac;
};

struct World;
// What a driver's send_frame captures (a reference Function holds one pointer).
struct Port {
    World *world;
    std::size_t k;
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
    class StackArg : public StackService::template Compose<StubPlatform, MakeTypeList<>> {};
    using Stack = IpStack<StackArg>;
    using EthService = EthIpIfaceService<
        EthIpIfaceOptions::NumArpEntries::Is<16>, EthIpIfaceOptions::ArpProtectCount::Is<8>,
        EthIpIfaceOptions::HeaderBeforeEth::Is<0>,
        EthIpIfaceOptions::TimersStructureService::Is<LinkedHeapService>>;
    class EthArg : public EthService::template Compose<StubPlatform, StackArg> {};
    using Eth = EthIpIface<EthArg>;

    PlatformFacade<StubPlatform> platform{};
    std::vector<IfaceSpec> specs;
    std::vector<std::string> events;
    std::unique_ptr<Stack> stack;
    std::vector<std::unique_ptr<Port>> ports;
    std::vector<std::unique_ptr<Eth>> eths;

    explicit World(std::vector<IfaceSpec> specs_) : specs(std::move(specs_)) {
        stack.reset(new Stack(platform));
        for (std::size_t k = 0; k < specs.size(); ++k) {
            ports.emplace_back(new Port{this, k});
            Port *port = ports[k].get();
            EthIfaceDriverParams params;
            params.eth_mtu = 1514;
            params.mac_addr = &specs[k].mac;
            params.send_frame = [port](IpBufRef frame) {
                std::vector<char> copy(frame.tot_len);
                ipBufTakeBytes(frame, frame.tot_len, copy.data());
                const bool ip4 = copy.size() >= 14 && copy[12] == 0x08 && copy[13] == 0x00;
                port->world->events.push_back(std::string(ip4 ? "T " : "Q ") +
                                              std::to_string(port->k) + " " +
                                              hex(copy.data(), ip4 ? 14 : copy.size()));
                return IpErr::Success;
            };
            params.get_eth_state = []() {
                EthIfaceState st = {};
                st.link_up = true;
                return st;
            };
            eths.emplace_back(new Eth(platform, stack.get(), params));
            if (specs[k].have)
                eths[k]->iface().setIp4Addr(
                    IpIfaceIp4AddrSetting((std::uint8_t)specs[k].prefix, Ip4Addr(specs[k].addr)));
            if (specs[k].have_gw)
                eths[k]->iface().setIp4Gateway(IpIfaceIp4GatewaySetting(Ip4Addr(specs[k].gateway)));
        }
    }
    ~World() {
        eths.clear();
        stack.reset();
    }
    void inject(std::size_t k, std::vector<char> &frame) {
        IpBufNode node{frame.data(), frame.size(), nullptr};
        eths.at(k)->recvFrame(IpBufRef{&node, 0, frame.size()});
    }
    IpErr send(std::uint32_t src, std::uint32_t dst, unsigned flags, long k) {
        TxAllocHelper<8, Stack::HeaderBeforeIp4Dgram> alloc(8);
        std::memset(alloc.getPtr(), 0x5A, 8);
        const Ip4AddrPair addrs{Ip4Addr(src), Ip4Addr(dst)};
        return stack->sendIp4Dgram(
            alloc.getBufRef(), k < 0 ? nullptr : &eths.at((std::size_t)k)->iface(), nullptr,
            Ip4CommonSendParams{addrs, 64, Ip4Protocol::Udp, (IpSendFlags)flags});
    }
    void answer() {
        for (auto &e : events) std::printf("%s\n", e.c_str());
        events.clear();
        std::printf(".\n");
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
            unsigned long n;
            in >> n;
            std::vector<IfaceSpec> specs;
            for (unsigned long k = 0; k < n; ++k) {
                unsigned long have, addr, prefix, have_gw, gw;
                std::string mac;
                in >> have >> addr >> prefix >> have_gw >> gw >> mac;
                const std::vector<char> m = unhex(mac);
                std::array<std::uint8_t, 6> bytes;
                std::memcpy(bytes.data(), m.data(), 6);
                specs.push_back(IfaceSpec{have != 0, have_gw != 0, (std::uint32_t)addr,
                                          (std::uint32_t)gw, (unsigned)prefix, MacAddr(bytes)});
            }
            w.reset();
            w.reset(new World(std::move(specs)));
        } else if (what == "F") {
            unsigned long k;
            std::string h;
            in >> k >> h;
            std::vector<char> frame = unhex(h);
            w->inject(k, frame);
            w->answer();
        } else if (what == "D") {
            unsigned long src, dst, flags;
            long k;
            in >> src >> dst >> flags >> k;
            const IpErr err = w->send((std::uint32_t)src, (std::uint32_t)dst, (unsigned)flags, k);
            std::printf("E %d\n", (int)err);
            w->answer();
        }
    }
    w.reset();
    return 0;
}
