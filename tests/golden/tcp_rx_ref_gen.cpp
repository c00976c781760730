// TEST INFRASTRUCTURE -- answers of the reference's own option parser and PCB key comparison
// (tcp/TcpOptions.h ParseTcpOptions, tcp/TcpPcbKey.h TcpPcbKeyCompare::CompareKeys), compiled
// against the reference tree by tests/golden/tcp_rx_ref.py, which records them in
// tests/golden/tcp_rx_ref_cases.json. Reads one request per line:
//   O <hex option bytes, or ->          -> "<options flags> <mss> <wnd_scale>" (mss / wnd_scale
//                                           preset to 0: the parser leaves them alone unless set)
//   K <la> <ra> <lp> <rp> <la> <ra> <lp> <rp>  (hex)  -> CompareKeys(op1, op2)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include <aipstack/tcp/TcpOptions.h>
#include <aipstack/tcp/TcpPcbKey.h>

using namespace AIpStack;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "O") {
            std::string hex;
            in >> hex;
            std::vector<char> bytes;
            if (hex != "-")
                for (std::size_t i = 0; i + 1 < hex.size(); i += 2)
                    bytes.push_back((char)std::stoul(hex.substr(i, 2), nullptr, 16));
            // a heap block of exactly the option bytes (at least one, so that the pointer is valid)
            std::vector<char> block(bytes.empty() ? 1 : bytes.size());
            if (!bytes.empty()) std::memcpy(block.data(), bytes.data(), bytes.size());
            IpBufNode node{block.data(), bytes.size(), nullptr};
            IpBufRef ref{&node, 0, bytes.size()};
            TcpOptions o;
            o.options = TcpOptionFlags(0);
            o.mss = 0;
            o.wnd_scale = 0;
            ParseTcpOptions(ref, o);
            std::printf("%u %u %u\n", (unsigned)o.options, (unsigned)o.mss, (unsigned)o.wnd_scale);
        } else if (what == "K") {
            unsigned long v[8];
            for (auto &x : v) in >> std::hex >> x;
            TcpPcbKey a(Ip4Addr((std::uint32_t)v[0]), Ip4Addr((std::uint32_t)v[1]),
                        (PortNum)v[2], (PortNum)v[3]);
            TcpPcbKey b(Ip4Addr((std::uint32_t)v[4]), Ip4Addr((std::uint32_t)v[5]),
                        (PortNum)v[6], (PortNum)v[7]);
            std::printf("%d\n", TcpPcbKeyCompare::CompareKeys(a, b));
        }
    }
    return 0;
}
