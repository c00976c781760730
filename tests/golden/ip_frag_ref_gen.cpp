// TEST INFRASTRUCTURE -- answers of the reference's own fragment-length rounding and checksum
// code (proto/Ip4Proto.h Ip4RoundFragLen; infra/Chksum.h IpChksum and IpChksumAccumulator),
// compiled against the reference tree by tests/golden/ip_frag_ref.py, which records them in
// tests/golden/ip_frag_ref_cases.json. send_fragmented itself needs the whole stack: it is not
// called here but by oracle/stack_ref_gen.cpp, which runs the reference's IpStack on a capture
// driver (tests/golden/stack_tx_ref_cases.json). Reads one request per line:
//   R <mtu>                                  -> Ip4RoundFragLen(20, mtu)
//   H <40 hex digits: 20 header bytes>       -> IpChksum(header, 20)
//   U <src> <dst> <sport> <dport> <hex payload, or ->   (hex fields)
//        -> the UDP checksum as udp/IpUdpProto.h:163-179 computes it: the 8 header bytes written
//           in front of the payload (length = 8 + payload, checksum 0), the accumulator fed
//           local address, remote address, protocol 17, length, then getChksum over header and
//           payload; 0 becomes 0xFFFF
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include <aipstack/infra/Chksum.h>
#include <aipstack/proto/Ip4Proto.h>

using namespace AIpStack;

static std::vector<char> unhex(const std::string &hex) {
    std::vector<char> bytes;
    if (hex != "-")
        for (std::size_t i = 0; i + 1 < hex.size(); i += 2)
            bytes.push_back((char)std::stoul(hex.substr(i, 2), nullptr, 16));
    return bytes;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "R") {
            unsigned mtu;
            in >> mtu;
            std::printf("%u\n", (unsigned)Ip4RoundFragLen(20, (std::uint16_t)mtu));
        } else if (what == "H") {
            std::string hex;
            in >> hex;
            std::vector<char> h = unhex(hex);   // a heap block of exactly the 20 bytes
            std::printf("%u\n", (unsigned)IpChksum(h.data(), h.size()));
        } else if (what == "U") {
            unsigned long src, dst, sport, dport;
            std::string hex;
            in >> std::hex >> src >> dst >> sport >> dport >> hex;
            std::vector<char> pay = unhex(hex);
            const std::size_t tot = 8 + pay.size();
            std::vector<char> dgram(tot);       // header and payload, a heap block of exactly tot
            const unsigned char hdr[8] = {
                (unsigned char)(sport >> 8), (unsigned char)sport, (unsigned char)(dport >> 8),
                (unsigned char)dport, (unsigned char)(tot >> 8), (unsigned char)tot, 0, 0};
            std::memcpy(dgram.data(), hdr, 8);
            if (!pay.empty()) std::memcpy(dgram.data() + 8, pay.data(), pay.size());
            IpBufNode node{dgram.data(), tot, nullptr};
            IpChksumAccumulator acc;
            acc.addWord(WrapType<std::uint32_t>(), (std::uint32_t)src);
            acc.addWord(WrapType<std::uint32_t>(), (std::uint32_t)dst);
            acc.addWord(WrapType<std::uint16_t>(), (std::uint16_t)17);
            acc.addWord(WrapType<std::uint16_t>(), (std::uint16_t)tot);
            std::uint16_t c = acc.getChksum(IpBufRef{&node, 0, tot});
            if (c == 0) c = 0xFFFF;
            std::printf("%u\n", (unsigned)c);
        }
    }
    return 0;
}
