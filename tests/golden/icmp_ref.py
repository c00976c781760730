"""TEST INFRASTRUCTURE -- reference-produced answers for ICMP on receive: the reference's own
IpStack with IpUdpProto and no listener (icmp_ref_gen.cpp only includes reference headers; the
platform and the capture driver are stubs of this project's), compiled from the reference tree and
fed the IP packets below. The answers are recorded in icmp_ref_cases.json:

  {"stacks": [{"allow": 0|1, "mtu": .., "addr": .., "prefix": .., "gateway": .., "warm": ..,
               "cases": [{"name": .., "in": "<hex IP packet>", "out": ["<hex IP packet>", ...]}]}]}

A stack answers its cases in order, so the Ident runs on within it; "warm" echo requests were
answered before the first case (the stack's next Ident is then warm mod 2^16).

    python3 tests/golden/icmp_ref.py <reference tree>      # rewrites the fixture
"""
import json
import os
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "icmp_ref_cases.json")
GEN_SRC = os.path.join(HERE, "icmp_ref_gen.cpp")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "icmp_ref_gen")

LOCAL = 0x0A141E28        # 10.20.30.40 (frame_cases.LOCAL_IP)
PREFIX = 24
BCAST = 0x0A141EFF
GATEWAY = 0x0A141E01
PEER = 0x0A141E64         # 10.20.30.100 (frame_cases.peer_ip(0))
ALL_ONES = 0xFFFFFFFF

# (allow broadcast ping, mtu, warm-up echo requests)
STACKS = ((0, 576, 0), (0, 1500, 65530), (1, 1500, 3))


def be_sum(data):
    if len(data) & 1:
        data = data + b"\0"
    return sum(struct.unpack(">%dH" % (len(data) // 2), data))


def chksum(data):
    s = be_sum(data)
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return (~s) & 0xFFFF


def ip_packet(proto, l4, *, src=PEER, dst=LOCAL, ihl=5, flags_off=0, ident=0x4242, ttl=61,
              trailing=b""):
    """An IPv4 packet (options: Nops) with a good header checksum, then `trailing` bytes beyond
    its total length."""
    h = bytearray(struct.pack(">BBHHHBBHII", 0x40 | ihl, 0, 4 * ihl + len(l4), ident, flags_off, ttl,
                              proto, 0, src, dst) + bytes([1]) * (4 * (ihl - 5)))
    struct.pack_into(">H", h, 10, chksum(bytes(h)))
    return bytes(h) + l4 + trailing


def icmp(type_, code, rest, data, *, bad=False):
    m = bytearray(struct.pack(">BBH", type_, code, 0) + rest + data)
    struct.pack_into(">H", m, 2, chksum(bytes(m)) ^ (0x0100 if bad else 0))
    return bytes(m)


def udp(data, *, src=PEER, dst=LOCAL, sport=40000, dport=9, with_chksum=True, bad=False):
    u = bytearray(struct.pack(">HHHH", sport, dport, 8 + len(data), 0) + data)
    if with_chksum:
        c = chksum(struct.pack(">IIHH", src, dst, 17, len(u)) + bytes(u)) or 0xFFFF
        struct.pack_into(">H", u, 6, c ^ (0x0100 if bad else 0))
    return bytes(u)


def pattern(n, salt):
    return bytes((salt + 7 * k) & 0xFF for k in range(n))


REST = bytes([0x12, 0x34, 0x00, 0x07])


def echo(data=b"", *, rest=REST, code=0, **ip):
    return ip_packet(1, icmp(8, code, rest, data), **ip)


def cases(mtu, allow):
    """[(name, IP packet)] for a stack of `mtu`; the names carry what the case is there for."""
    out = []
    for n in (0, 1, 2, 17, 18, 19, mtu - 28):
        out.append(("echo_data_%s" % ("mtu-28" if n == mtu - 28 else n), echo(pattern(n, n))))
    out.append(("echo_pad60", echo(b"", trailing=bytes([0xA5]) * 18)))
    out.append(("echo_ihl6", echo(pattern(5, 1), ihl=6)))
    out.append(("echo_ihl15", echo(pattern(33, 2), ihl=15)))
    out.append(("echo_code", echo(pattern(9, 3), code=5)))
    out.append(("echo_rest_0", echo(pattern(11, 4), rest=bytes(4))))
    out.append(("echo_rest_ones", echo(pattern(12, 5), rest=bytes([0xFF]) * 4)))
    out.append(("echo_zero_class_all_zero", echo(bytes(8), rest=bytes(4))))
    out.append(("echo_zero_class_all_zero_odd", echo(bytes(7), rest=bytes(4))))
    out.append(("echo_zero_class_nonzero", echo(bytes([0xED, 0xCB]), rest=bytes([0x12, 0x34, 0, 0]))))
    out.append(("echo_zero_class_nonzero_rest_0", echo(bytes([0, 1, 0xFF, 0xFE, 0, 0, 0]), rest=bytes(4))))
    out.append(("echo_zero_class_nonzero_tail", echo(bytes(4) + bytes([0xFF, 0xFF, 0]), rest=bytes(4))))
    out.append(("echo_bad_chksum", ip_packet(1, icmp(8, 0, REST, pattern(20, 6), bad=True))))
    out.append(("icmp_type0", ip_packet(1, icmp(0, 0, REST, pattern(20, 7)))))
    out.append(("icmp_type3", ip_packet(1, icmp(3, 3, bytes(4), pattern(28, 8)))))
    out.append(("echo_src_all_ones", echo(pattern(4, 9), src=ALL_ONES)))
    out.append(("echo_src_multicast", echo(pattern(4, 10), src=0xE0000001)))
    out.append(("echo_src_bcast", echo(pattern(4, 11), src=BCAST)))
    out.append(("echo_dst_not_local", echo(pattern(4, 12), dst=LOCAL + 1)))
    out.append(("echo_dst_bcast_%s" % ("set" if allow else "clear"), echo(pattern(4, 13), dst=BCAST)))
    out.append(("echo_dst_all_ones_%s" % ("set" if allow else "clear"), echo(pattern(4, 14), dst=ALL_ONES)))
    out.append(("echo_fragment", echo(pattern(16, 15), flags_off=0x2000)))
    out.append(("echo_after_fragment", echo(pattern(3, 16))))
    if mtu < 1500:
        out.append(("echo_too_large", echo(pattern(mtu - 27, 17))))
        out.append(("echo_after_too_large", echo(pattern(6, 18))))
    for ihl in (5, 7):
        for n in (0, 100):
            for with_chksum in (True, False):
                out.append(("udp_closed_ihl%d_data%d_%s" % (ihl, n, "chksum" if with_chksum else "nochksum"),
                            ip_packet(17, udp(pattern(n, n + ihl), with_chksum=with_chksum), ihl=ihl)))
    out.append(("udp_bad_chksum", ip_packet(17, udp(pattern(10, 19), bad=True))))
    out.append(("udp_dst_not_local", ip_packet(17, udp(pattern(10, 20), dst=LOCAL + 1), dst=LOCAL + 1)))
    out.append(("udp_dst_bcast", ip_packet(17, udp(pattern(10, 21), dst=BCAST), dst=BCAST)))
    out.append(("udp_src_multicast", ip_packet(17, udp(pattern(10, 22), src=0xE0000001), src=0xE0000001)))
    out.append(("udp_src_bcast", ip_packet(17, udp(pattern(10, 23), src=BCAST), src=BCAST)))
    out.append(("udp_src_all_ones", ip_packet(17, udp(pattern(10, 24), src=ALL_ONES), src=ALL_ONES)))
    out.append(("echo_last", echo(pattern(40, 25))))
    for k in range(8):                                  # carries the Ident past 0xFFFF where warm is high
        out.append(("echo_run_%d" % k, echo(pattern(k, 26 + k))))
    return out


def build_generator(reference):
    os.makedirs(os.path.dirname(GEN_BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(reference, "src"), "-o", GEN_BIN,
                    GEN_SRC], check=True)
    return GEN_BIN


def generate(reference):
    """The fixture's text, from the reference's code run on the cases above."""
    gen = build_generator(reference)
    req, plan = [], []
    for allow, mtu, warm in STACKS:
        req.append("S %d %d %d %d %d %d" % (allow, mtu, LOCAL, PREFIX, GATEWAY, warm))
        cs = cases(mtu, allow)
        plan.append((allow, mtu, warm, cs))
        req += ["I " + p.hex() for _, p in cs]
    ans = subprocess.run([gen], input="\n".join(req) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert ans[-1] == ""
    at, stacks = 0, []
    for allow, mtu, warm, cs in plan:
        rows = []
        for name, pkt in cs:
            got = []
            while ans[at] != ".":
                assert ans[at].startswith("P ")
                got.append(ans[at][2:])
                at += 1
            at += 1
            rows.append({"name": name, "in": pkt.hex(), "out": got})
        stacks.append({"allow": allow, "mtu": mtu, "addr": LOCAL, "prefix": PREFIX, "gateway": GATEWAY,
                       "warm": warm, "cases": rows})
    assert at == len(ans) - 1
    return json.dumps({"stacks": stacks}, indent=0, separators=(",", ":")) + "\n"


def load():
    with open(FIXTURE) as f:
        return json.load(f)["stacks"]


if __name__ == "__main__":
    text = generate(sys.argv[1])
    with open(FIXTURE, "w") as f:
        f.write(text)
    print("%s: %d bytes" % (FIXTURE, len(text)))
