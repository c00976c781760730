"""TEST INFRASTRUCTURE -- what the reference hands its protocol handlers for received ICMP
Destination Unreachable messages: the reference's own EthIpIface over its IpStack with two
recording protocol handlers for the protocol numbers 6 and 17 (icmp_du_ref_gen.cpp only includes
reference headers; the platform, the capture driver and the handlers are stubs of this project's),
compiled from the reference tree and fed the Ethernet frames below. The calls are recorded in
icmp_du_ref_cases.json:

  {"stacks": [{"addr": .., "prefix": .., "gateway": .., "mac": "<hex>",
               "cases": [{"name": .., "in": "<hex frame>", "out": [<event>, ...]}]}]}

An event is "D <handler> <code> <rest hex> <src_addr> <dst_addr> <ttl> <proto> <header_len>
<dgram_initial hex, or ->" (a handleIp4DestUnreach call) or "R <handler>" (a recvIp4Dgram call).
Every case runs on a fresh stack.

    python3 tests/golden/icmp_du_ref.py <reference tree>      # rewrites the fixture
"""
import json
import os
import struct
import subprocess
import sys

import frame_cases as F
import icmp_ref as I
import tcp_rsp_ref as TR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "icmp_du_ref_cases.json")
GEN_SRC = os.path.join(HERE, "icmp_du_ref_gen.cpp")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "icmp_du_ref_gen")

LOCAL_MAC = F.LOCAL_MAC
PEER_MAC = F.peer_mac(0)
ALL_ONES = 0xFFFFFFFF
STACKS = TR.STACKS                 # (address, prefix, a peer in the subnet, gateway): /24 and /30
netmask = TR.netmask
FAR = 0xC0A80105                   # 192.168.1.5: the far end of the quoted datagrams
FRAG_NEEDED = 4
CODES = (0, 1, 2, 3, 4, 5, 13)
RESTS = (0, 0x000005DC, 0xFFFF0100, 0x12340000)


def tcp_head(n, *, sport=5000, dport=80, seq=0x11223344):
    """The first n bytes of a TCP header."""
    return struct.pack(">HHIIHHHH", sport, dport, seq, 0x55667788, 0x5010, 4096, 0xABCD, 0)[:n] + \
        I.pattern(max(n - 20, 0), 3)


def udp_head(n, *, sport=5000, dport=53):
    return (struct.pack(">HHHH", sport, dport, 520, 0x1357) + I.pattern(max(n - 8, 0), 5))[:n]


def quoted(proto, l4, *, src, dst=FAR, ihl=5, hdr_bytes=None, total=1500, version=4, flags_off=0x4000,
           ttl=57):
    """The datagram quoted in a Destination Unreachable: an IPv4 header that says `version`, `ihl`
    and `total`, of which `hdr_bytes` are present (4 * ihl by default, at least 20; options: Nops),
    then the L4 bytes `l4`."""
    if hdr_bytes is None:
        hdr_bytes = max(4 * ihl, 20)
    h = bytearray(struct.pack(">BBHHHBBHII", version << 4 | ihl, 0, total, 0x7788, flags_off, ttl, proto, 0,
                              src, dst) + bytes([1]) * 40)
    struct.pack_into(">H", h, 10, I.chksum(bytes(h[:max(4 * ihl, 20)])))
    return bytes(h[:hdr_bytes]) + l4


def frame(data, *, src, dst, code=FRAG_NEEDED, rest=0x000005DC, type_=3, ihl=5, flags_off=0, bad=False,
          pad=0, pad60=False):
    """The Ethernet frame, from PEER_MAC, of an ICMP message with `data` behind its 8-byte header,
    then `pad` bytes of padding (pad60: up to 60 bytes)."""
    m = I.icmp(type_, code, struct.pack(">I", rest), data, bad=bad)
    f = LOCAL_MAC + PEER_MAC + b"\x08\x00" + I.ip_packet(1, m, src=src, dst=dst, ihl=ihl, flags_off=flags_off)
    f += bytes([0x5A]) * pad
    if pad60 and len(f) < 60:
        f += bytes([0x5A]) * (60 - len(f))
    return f


def cut(f, keep, *, fix_icmp):
    """The frame cut to `keep` bytes with the IPv4 total length (and header checksum) cut to match;
    fix_icmp: the ICMP checksum recomputed over what is left."""
    f = bytearray(f[:keep])
    hl = (f[14] & 0xF) * 4
    struct.pack_into(">H", f, 16, keep - 14)
    f[24:26] = b"\0\0"
    struct.pack_into(">H", f, 24, I.chksum(bytes(f[14:14 + hl])))
    if fix_icmp:
        t = 14 + hl
        f[t + 2:t + 4] = b"\0\0"
        struct.pack_into(">H", f, t + 2, I.chksum(bytes(f[t:])))
    return bytes(f)


def cases(local, prefix, peer, gateway):
    """[(name, frame)] for one stack."""
    bcast = (local & netmask(prefix)) | (~netmask(prefix) & ALL_ONES)
    other = peer if prefix == 30 else local + 1
    out = []

    def add(name, data, **kw):
        kw.setdefault("src", peer)
        kw.setdefault("dst", local)
        out.append((name, frame(data, **kw)))

    def q(proto, l4, **kw):
        kw.setdefault("src", local)
        return quoted(proto, l4, **kw)

    tcp20, udp8 = tcp_head(20), udp_head(8)
    for code in CODES:
        add("tcp_code_%d" % code, q(6, tcp_head(8)), code=code)
        add("udp_code_%d" % code, q(17, udp8), code=code)
    for rest in RESTS:
        add("tcp_rest_%08x" % rest, q(6, tcp_head(8)), rest=rest)
        add("udp_rest_%08x" % rest, q(17, udp8), rest=rest, code=3)
    for ihl in (5, 6, 15):
        add("outer_ihl_%d" % ihl, q(6, tcp_head(8)), ihl=ihl)
        add("quoted_ihl_%d" % ihl, q(6, tcp_head(8), ihl=ihl))
        add("both_ihl_%d" % ihl, q(6, tcp20, ihl=ihl), ihl=ihl)
    add("quoted_ihl_4", q(6, tcp_head(8), ihl=4))
    add("quoted_ihl_0", q(6, tcp_head(8), ihl=0))
    add("quoted_version_6", q(6, tcp_head(8), version=6))
    add("quoted_version_5", q(6, tcp_head(8), version=5))
    add("quoted_ihl_6_only_20_bytes", q(6, b"", ihl=6, hdr_bytes=20))
    add("quoted_ihl_6_only_23_bytes", q(6, b"", ihl=6, hdr_bytes=23))
    add("quoted_ihl_15_only_59_bytes", q(6, b"", ihl=15, hdr_bytes=59))
    add("quoted_total_below_header", q(6, tcp_head(8), total=19))
    add("quoted_total_equals_header", q(6, tcp_head(8), total=20))
    add("quoted_total_below_header_ihl_6", q(6, tcp_head(8), ihl=6, total=23))
    add("quoted_total_equals_header_ihl_6", q(6, tcp_head(8), ihl=6, total=24))
    add("quoted_total_cuts_l4_to_12", q(6, tcp_head(28), total=32))
    add("quoted_total_cuts_l4_to_8", q(6, tcp_head(28), total=28))
    add("quoted_total_cuts_l4_to_7", q(6, tcp_head(28), total=27))
    add("quoted_total_cuts_l4_to_5_udp", q(17, udp_head(28), total=25), code=3)
    for n in (0, 3, 4, 7, 8, 9, 28):
        add("tcp_l4_%d" % n, q(6, tcp_head(n)))
        add("udp_l4_%d" % n, q(17, udp_head(n)), code=3)
    add("icmp_data_19", q(6, b"")[:19])
    add("icmp_data_20", q(6, b""))
    add("icmp_data_0", b"")
    for proto in (1, 47):
        add("quoted_proto_%d" % proto, q(proto, tcp_head(8)))
        add("quoted_proto_%d_no_l4" % proto, q(proto, b""))
    add("quoted_src_not_ours", q(6, tcp_head(8), src=0xC0A80909))
    add("quoted_src_not_ours_udp", q(17, udp8, src=0xC0A80909), code=3)
    add("quoted_fragment_offset", q(6, tcp_head(8), flags_off=0x00B9))
    add("quoted_more_fragments", q(6, tcp_head(8), flags_off=0x2000))
    for name, src in (("all_ones", ALL_ONES), ("224_0_0_1", 0xE0000001), ("240_0_0_1", 0xF0000001),
                      ("subnet_bcast", bcast), ("zero", 0), ("outside", 0xC0A80101)):
        add("src_%s" % name, q(6, tcp_head(8)), src=src)
    for name, dst in (("subnet_bcast", bcast), ("all_ones", ALL_ONES), ("other_host", other)):
        add("dst_%s" % name, q(6, tcp_head(8)), dst=dst)
        add("dst_%s_udp" % name, q(17, udp8), dst=dst, code=3)
    add("bad_icmp_checksum", q(6, tcp_head(8)), bad=True)
    add("type_3_in_a_fragment", q(6, tcp_head(8)), flags_off=0x2000)
    add("type_3_in_a_later_fragment", q(6, tcp_head(8)), flags_off=0x0010)
    add("type_11_good_quote", q(6, tcp_head(8)), type_=11, code=0)
    add("type_8", q(6, tcp_head(8)), type_=8, code=0)
    add("type_0", q(6, tcp_head(8)), type_=0, code=0)
    add("padded_to_60", q(6, b"")[:12], pad60=True)
    add("padded_to_60_no_data", b"", pad60=True)
    add("icmp_data_19_padded_by_5", q(6, b"")[:19], pad=5)
    add("tcp_l4_4_padded_by_5", q(6, tcp_head(4)), pad=5)
    add("padded_by_5", q(6, tcp_head(8)), pad=5)
    add("padded_by_5_tcp_7", q(6, tcp_head(7)), pad=5)
    whole = frame(q(6, tcp_head(28), ihl=6), src=peer, dst=local)
    for keep in (14 + 20 + 8 + 22, 14 + 20 + 8 + 24 + 5, 14 + 20 + 8 + 24 + 8):
        out.append(("cut_to_%d_bytes" % keep, cut(whole, keep, fix_icmp=True)))
    out.append(("cut_to_%d_bytes_stale_icmp_checksum" % (14 + 20 + 8 + 24 + 8),
                cut(whole, 14 + 20 + 8 + 24 + 8, fix_icmp=False)))
    out.append(("cut_without_the_total_length", whole[:14 + 20 + 8 + 24 + 8]))
    out.append(("tcp_segment", TR.frame(TR.SYN, src=peer, dst=local)))
    out.append(("udp_datagram", LOCAL_MAC + PEER_MAC + b"\x08\x00" +
                I.ip_packet(17, I.udp(b"abc", src=peer, dst=local), src=peer, dst=local)))
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
    for local, prefix, peer, gateway in STACKS:
        cs = cases(local, prefix, peer, gateway)
        for name, f in cs:
            req.append("S %d %d %d %s" % (local, prefix, gateway, LOCAL_MAC.hex()))
            req.append("F " + (f.hex() or "-"))
        plan.append((local, prefix, gateway, cs))
    ans = subprocess.run([gen], input="\n".join(req) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert ans[-1] == ""
    at, stacks = 0, []
    for local, prefix, gateway, cs in plan:
        rows = []
        for name, f in cs:
            got = []
            while ans[at] != ".":
                assert ans[at][:2] in ("D ", "R ")
                got.append(ans[at])
                at += 1
            at += 1
            rows.append({"name": name, "in": f.hex(), "out": got})
        stacks.append({"addr": local, "prefix": prefix, "gateway": gateway, "mac": LOCAL_MAC.hex(),
                       "cases": rows})
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
