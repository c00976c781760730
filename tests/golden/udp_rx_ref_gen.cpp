// TEST INFRASTRUCTURE -- which UDP handlers the reference stack calls for a received IPv4 packet,
// and whether it answers with a port unreachable: the reference's own IpStack with IpUdpProto,
// instantiated on a stub platform and a capture driver of this project's, with UdpListeners and
// UdpAssociations whose handlers record their calls. Only reference headers are included;
// tests/golden/udp_rx_ref.py compiles it against the reference tree, drives it and records the
// answers in tests/golden/udp_rx_ref_cases.json.
//
// The platform: a clock that stands still and timers that never fire. The interface is a bare
// IpDriverIface (no Ethernet, no ARP) whose send_ip4_packet copies each IP packet into a capture
// list and returns success; it has a gateway, so that every destination has a route.
//
// One request per line:
//   S <addr> <prefix> <gateway>
//        a fresh stack, the interface <addr>/<prefix>. No answer.
//   L <iface_addr> <port> <accept_broadcast> <accept_nonlocal_dst>
//        a UdpListener (UdpListenParams with a null iface), number = how many came before. No answer.
//   A <local_addr> <remote_addr> <local_port> <remote_port> <accept_nonlocal_dst>
//        a UdpAssociation, numbered likewise. No answer.
//   I <mode> <hex>
//        the IP packet is injected; every handler returns AcceptContinue (mode 0) or Reject
//        (mode 1) -> "C <L|A> <number> <data length> <FNV-1a 64 of the data> <has_checksum>" per
//        handler call in call order, "P <hex>" per captured packet, in full, then "."
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
#include <aipstack/infra/Err.h>
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
using ProtocolServices =
    MakeTypeList<IpUdpProtoService<IpUdpProtoOptions::UdpIndexService::Is<IndexService>>>;
class StackArg : public StackService::template Compose<StubPlatform, ProtocolServices> {};
using Stack = IpStack<StackArg>;
using UdpArg = typename Stack::template GetProtoArg<UdpApi>;

static std::uint64_t fnv(const char *p, std::size_t n) {
    std::uint64_t h = 1469598103934665603ull;
    for (std::size_t k = 0; k < n; ++k) {
        h ^= (unsigned char)p[k];
        h *= 1099511628211ull;
    }
    return h;
}

struct Call {
    char kind;
    unsigned number;
    std::size_t len;
    std::uint64_t hash;
    bool has_checksum;
};

struct World;

// What a handler knows of itself (the reference's Function holds one pointer).
struct Tag {
    World *world;
    char kind;
    unsigned number;
};

struct World {
    PlatformFacade<StubPlatform> platform{};
    std::vector<std::unique_ptr<Tag>> tags;
    std::unique_ptr<Stack> stack;
    std::unique_ptr<IpDriverIface<StackArg>> iface;
    std::vector<std::unique_ptr<UdpListener<UdpArg>>> listeners;
    std::vector<std::unique_ptr<UdpAssociation<UdpArg>>> assocs;
    std::vector<std::vector<char>> captured;
    std::vector<Call> calls;
    UdpRecvResult answer = UdpRecvResult::AcceptContinue;

    World(std::uint32_t addr, unsigned prefix, std::uint32_t gateway) {
        stack.reset(new Stack(platform));
        IpIfaceDriverParams params;
        params.ip_mtu = 1500;
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
    ~World() {
        listeners.clear();
        assocs.clear();
        iface.reset();
        stack.reset();
    }

    UdpRecvResult record(char kind, unsigned number, UdpRxInfo<UdpArg> const &info, IpBufRef data) {
        std::vector<char> copy(data.tot_len);
        ipBufTakeBytes(data, data.tot_len, copy.data());
        calls.push_back(Call{kind, number, copy.size(), fnv(copy.data(), copy.size()), info.has_checksum});
        return answer;
    }

    bool listen(std::uint32_t iface_addr, unsigned port, bool bcast, bool nonlocal) {
        tags.emplace_back(new Tag{this, 'L', (unsigned)listeners.size()});
        Tag *tag = tags.back().get();
        listeners.emplace_back(new UdpListener<UdpArg>(
            [tag](IpRxInfoIp4<StackArg> const &, UdpRxInfo<UdpArg> const &info, IpBufRef data) {
                return tag->world->record(tag->kind, tag->number, info, data);
            }));
        UdpListenParams<UdpArg> lp;
        lp.iface_addr = Ip4Addr(iface_addr);
        lp.port = (std::uint16_t)port;
        lp.accept_broadcast = bcast;
        lp.accept_nonlocal_dst = nonlocal;
        return listeners.back()->startListening(stack->getProtoApi<UdpApi>(), lp) == IpErr::Success;
    }

    bool associate(std::uint32_t la, std::uint32_t ra, unsigned lp, unsigned rp, bool nonlocal) {
        tags.emplace_back(new Tag{this, 'A', (unsigned)assocs.size()});
        Tag *tag = tags.back().get();
        assocs.emplace_back(new UdpAssociation<UdpArg>(
            [tag](IpRxInfoIp4<StackArg> const &, UdpRxInfo<UdpArg> const &info, IpBufRef data) {
                return tag->world->record(tag->kind, tag->number, info, data);
            }));
        UdpAssociationParams<UdpArg> ap;
        ap.key = UdpAssociationKey{Ip4Addr(la), Ip4Addr(ra), (std::uint16_t)lp, (std::uint16_t)rp};
        ap.accept_nonlocal_dst = nonlocal;
        return assocs.back()->associate(stack->getProtoApi<UdpApi>(), ap) == IpErr::Success;
    }

    void inject(std::vector<char> &pkt) {
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

int main() {
    std::unique_ptr<World> w;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "S") {
            unsigned long addr, prefix, gateway;
            in >> addr >> prefix >> gateway;
            w.reset();
            w.reset(new World((std::uint32_t)addr, (unsigned)prefix, (std::uint32_t)gateway));
        } else if (what == "L") {
            unsigned long iface_addr, port, bcast, nonlocal;
            in >> iface_addr >> port >> bcast >> nonlocal;
            if (!w->listen((std::uint32_t)iface_addr, (unsigned)port, bcast != 0, nonlocal != 0)) {
                std::fprintf(stderr, "udp_rx_ref_gen: startListening failed\n");
                return 2;
            }
        } else if (what == "A") {
            unsigned long la, ra, lp, rp, nonlocal;
            in >> la >> ra >> lp >> rp >> nonlocal;
            if (!w->associate((std::uint32_t)la, (std::uint32_t)ra, (unsigned)lp, (unsigned)rp, nonlocal != 0)) {
                std::fprintf(stderr, "udp_rx_ref_gen: associate failed\n");
                return 2;
            }
        } else if (what == "I") {
            unsigned long mode;
            std::string h;
            in >> mode >> h;
            std::vector<char> pkt(h.size() / 2);
            for (std::size_t k = 0; k < pkt.size(); ++k)
                pkt[k] = (char)std::stoul(h.substr(2 * k, 2), nullptr, 16);
            w->answer = mode ? UdpRecvResult::Reject : UdpRecvResult::AcceptContinue;
            w->inject(pkt);
            for (auto &c : w->calls)
                std::printf("C %c %u %zu %016llx %d\n", c.kind, c.number, c.len,
                            (unsigned long long)c.hash, c.has_checksum ? 1 : 0);
            for (auto &c : w->captured) std::printf("P %s\n", hex(c).c_str());
            w->calls.clear();
            w->captured.clear();
            std::printf(".\n");
        }
    }
    w.reset();
    return 0;
}
