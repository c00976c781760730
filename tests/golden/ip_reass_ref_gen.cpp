// TEST INFRASTRUCTURE -- answers of the reference's own IPv4 reassembly
// (ip/IpReassembly.h: IpReassembly::reassembleIp4), compiled against the reference tree by
// tests/golden/ip_reass_ref.py, which records them in tests/golden/ip_reass_ref_cases.json.
// Only IpReassembly.h is included (it needs misc / infra / proto headers and PlatformFacade);
// the platform below is this project's stub: a clock that stands still and a timer that does
// nothing, so no entry ever expires. Reads one request per line:
//   S <config>     a fresh reassembler: 0 = MaxReassSize 65531, 1 = 2000, 2 = 576, the smallest allowed (each with 8
//                  entries, 250 holes), 3 = 2000 with MaxReassHoles 2
//   F <ident> <src> <dst> <ttl> <proto> <mf> <offset> <len> <salt>   (decimal)
//                  -> one call of reassembleIp4 with a fragment whose payload byte k is
//                     (salt + 3 * (offset + k)) & 0xFF, in a heap block of exactly len bytes;
//                     prints "0", or "1 <length> <FNV-1a 64 of the reassembled bytes, hex>"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include <aipstack/ip/IpReassembly.h>

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
        bool isSet() const { return false; }
        TimeType getSetTime() const { return 0; }
        void unset() {}
        void setAt(TimeType) {}
    };
};

struct Reassembler {
    virtual ~Reassembler() {}
    virtual bool feed(std::uint16_t ident, std::uint32_t src, std::uint32_t dst, std::uint8_t ttl,
                      std::uint8_t proto, bool mf, std::uint16_t off, const char *header,
                      IpBufRef &dgram) = 0;
};

template <std::uint16_t Size, std::uint8_t Holes>
struct ReassemblerOf : Reassembler {
    using Service = IpReassemblyService<IpReassemblyOptions::MaxReassEntrys::Is<8>,
                                        IpReassemblyOptions::MaxReassSize::Is<Size>,
                                        IpReassemblyOptions::MaxReassHoles::Is<Holes>>;
    using Impl = IpReassembly<typename Service::template Compose<StubPlatform>>;
    Impl impl{PlatformFacade<StubPlatform>()};
    bool feed(std::uint16_t ident, std::uint32_t src, std::uint32_t dst, std::uint8_t ttl,
              std::uint8_t proto, bool mf, std::uint16_t off, const char *header,
              IpBufRef &dgram) override {
        return impl.reassembleIp4(ident, Ip4Addr(src), Ip4Addr(dst), ttl, Ip4Protocol(proto), mf, off,
                                  header, dgram);
    }
};

int main() {
    std::unique_ptr<Reassembler> r;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "S") {
            int cfg;
            in >> cfg;
            if (cfg == 0) r.reset(new ReassemblerOf<65531, 250>());
            else if (cfg == 1) r.reset(new ReassemblerOf<2000, 250>());
            else if (cfg == 2) r.reset(new ReassemblerOf<576, 250>());
            else r.reset(new ReassemblerOf<2000, 2>());
        } else if (what == "F") {
            unsigned long ident, src, dst, ttl, proto, mf, off, len, salt;
            in >> ident >> src >> dst >> ttl >> proto >> mf >> off >> len >> salt;
            std::vector<char> data(len);         // a heap block of exactly the payload
            for (unsigned long k = 0; k < len; ++k) data[k] = (char)((salt + 3 * (off + k)) & 0xFF);
            char header[Ip4Header::Size];
            std::memset(header, 0, sizeof(header));
            auto h = Ip4Header::MakeRef(header);
            h.set(Ip4Header::VersionIhlDscpEcn(), (std::uint16_t)0x4500);
            h.set(Ip4Header::TotalLen(), (std::uint16_t)(20 + len));
            h.set(Ip4Header::Ident(), (std::uint16_t)ident);
            h.set(Ip4Header::FlagsOffset(), Ip4Flags((std::uint16_t)((mf ? 0x2000u : 0u) | off / 8)));
            h.set(Ip4Header::Ttl(), (std::uint8_t)ttl);
            h.set(Ip4Header::Proto(), Ip4Protocol((std::uint8_t)proto));
            h.set(Ip4Header::SrcAddr(), Ip4Addr((std::uint32_t)src));
            h.set(Ip4Header::DstAddr(), Ip4Addr((std::uint32_t)dst));
            IpBufNode node{data.data(), len, nullptr};
            IpBufRef dgram{&node, 0, len};
            const bool done = r->feed((std::uint16_t)ident, (std::uint32_t)src, (std::uint32_t)dst,
                                      (std::uint8_t)ttl, (std::uint8_t)proto, mf != 0,
                                      (std::uint16_t)off, header, dgram);
            if (!done) {
                std::printf("0\n");
            } else {
                std::vector<char> out(dgram.tot_len);
                IpBufRef rest = ipBufTakeBytes(dgram, dgram.tot_len, out.data());
                (void)rest;
                std::uint64_t f = 0xcbf29ce484222325ull;
                for (char c : out) f = (f ^ (unsigned char)c) * 0x100000001b3ull;
                std::printf("1 %zu %016llx\n", out.size(), (unsigned long long)f);
            }
        }
    }
    return 0;
}
