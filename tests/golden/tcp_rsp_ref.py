"""TEST INFRASTRUCTURE -- reference-produced answers to TCP segments of no connection: the
reference's own EthIpIface over its IpStack with IpTcpProto (tcp_rsp_ref_gen.cpp only includes
reference headers; the platform and the capture driver are stubs of this project's), compiled from
the reference tree and fed the Ethernet frames below. The answers are recorded in
tcp_rsp_ref_cases.json:

  {"stacks": [{"addr": .., "prefix": .., "gateway": .., "mac": "<hex>",
               "listeners": [[addr, port], ...],          in the order they were opened
               "cases": [{"name": .., "in": "<hex frame>", "out": [<event>, ...]}],
               "session": {"in": ["<hex frame>", ...], "out": [[<event>, ...], ...]}}]}

An event is "T <hex frame>" (a frame the stack sent, in full) or "SYNACK" (one frame left and it
is a SYN-ACK, not an RST: the reference went on into listen_input's PCB allocation). Every case
runs on a fresh stack, so the Ident is 0; the session keeps one stack, for the Ident sequence.
Before each frame an ARP reply makes its next hop's MAC known (the source inside the subnet, the
gateway otherwise), so that the answer is not held back by ARP resolution.

    python3 tests/golden/tcp_rsp_ref.py <reference tree>      # rewrites the fixture
"""
import json
import os
import struct
import subprocess
import sys

import arp_ref as AR
import frame_cases as F
import icmp_ref as I

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "tcp_rsp_ref_cases.json")
GEN_SRC = os.path.join(HERE, "tcp_rsp_ref_gen.cpp")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "tcp_rsp_ref_gen")

LOCAL_MAC = F.LOCAL_MAC
PEER_MAC = F.peer_mac(0)
ALL_ONES = 0xFFFFFFFF
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10
CLOSED, SPECIFIC, WILDCARD, WILD_FRONT, SPECIFIC_FRONT = 81, 80, 8080, 443, 444

# (address, prefix, a peer in the subnet, gateway)
STACKS = ((0x0A141E28, 24, 0x0A141E64, 0x0A141E01),      # 10.20.30.40/24, peer .100, gateway .1
          (0x0A141E29, 30, 0x0A141E2A, 0x0A141E2A))      # 10.20.30.41/30, peer = gateway .42


def netmask(prefix):
    return (ALL_ONES << (32 - prefix)) & ALL_ONES


def listeners(local):
    """[(addr, port)] in the order they are opened; a later one stands in front."""
    return [(local, SPECIFIC), (0, WILDCARD), (local, WILD_FRONT), (0, WILD_FRONT),
            (0, SPECIFIC_FRONT), (local, SPECIFIC_FRONT)]


def tcp(flags, *, src, dst, sport=40000, dport=CLOSED, seq=0x11223344, ack=0x55667788,
        window=4096, opts=b"", data=b"", doff=None, bad=False):
    """A TCP segment with a good checksum (bad: one bit off). `doff` overrides the data offset
    that 20 + len(opts) gives."""
    if doff is None:
        assert len(opts) % 4 == 0
        doff = 5 + len(opts) // 4
    s = bytearray(struct.pack(">HHIIHHHH", sport, dport, seq, ack, doff << 12 | flags, window, 0, 0) +
                  opts + data)
    c = I.chksum(struct.pack(">IIHH", src, dst, 6, len(s)) + bytes(s))
    struct.pack_into(">H", s, 16, c ^ (0x0100 if bad else 0))
    return bytes(s)


def frame(flags, *, src, dst, ihl=5, pad=0, pad60=False, **kw):
    """The Ethernet frame of a TCP segment from PEER_MAC, then `pad` bytes of padding (pad60: up
    to 60 bytes)."""
    f = LOCAL_MAC + PEER_MAC + b"\x08\x00" + I.ip_packet(6, tcp(flags, src=src, dst=dst, **kw), src=src,
                                                        dst=dst, ihl=ihl, flags_off=0x4000)
    f += bytes([0x5A]) * pad
    if pad60 and len(f) < 60:
        f += bytes([0x5A]) * (60 - len(f))
    return f


def mss_opt(v):
    return bytes([2, 4, v >> 8, v & 0xFF])


def _model():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tcp_rsp_cases
    return tcp_rsp_cases


def ack_for_rst_checksum(want, *, src, dst, sport, dport):
    """The ack_num of an ACK segment whose RST (seq = that ack_num) carries the TCP checksum
    `want`: a search in the model."""
    C = _model()
    for lo in range(0x10000):
        ack = 0x12340000 | lo
        if C.rst_tcp_checksum(local=dst, remote=src, lport=dport, rport=sport, seq=ack, ack=0,
                              flags=0x5004) == want:
            return ack
    raise AssertionError("no ack_num gives checksum 0x%04x" % want)


def cases(local, prefix, peer, gateway):
    """[(name, frame)] for one stack."""
    bcast = (local & netmask(prefix)) | (~netmask(prefix) & ALL_ONES)
    other = peer if prefix == 30 else local + 1
    out = []

    def add(name, flags, **kw):
        kw.setdefault("src", peer)
        kw.setdefault("dst", local)
        out.append((name, frame(flags, **kw)))

    for fl in range(16):
        flags = (SYN if fl & 1 else 0) | (ACK if fl & 2 else 0) | (FIN if fl & 4 else 0) | (RST if fl & 8 else 0)
        for port in (CLOSED, SPECIFIC, WILDCARD):
            add("flags_%02x_port_%d" % (flags, port), flags, dport=port, pad60=True)
    for port in (SPECIFIC, CLOSED):
        add("syn_psh_port_%d" % port, SYN | PSH, dport=port)
        add("syn_ece_cwr_port_%d" % port, SYN | 0xC0, dport=port)
        add("syn_urg_port_%d" % port, SYN | 0x20, dport=port)
    for port in (WILD_FRONT, SPECIFIC_FRONT):
        add("syn_port_%d" % port, SYN, dport=port)
        add("ack_port_%d" % port, ACK, dport=port)
        add("rst_port_%d" % port, RST, dport=port)
    for n, pad in ((0, 6), (1, 5), (1460, 4)):
        data = I.pattern(n, 11)
        for name, flags in (("psh", PSH), ("syn", SYN), ("fin", FIN), ("syn_fin", SYN | FIN), ("ack", ACK)):
            if n == 1460 and name in ("syn_fin", "ack"):
                continue
            add("data_%d_%s_padded" % (n, name), flags, data=data, pad=pad)
        add("data_%d_psh_listening" % n, PSH, data=data, pad=pad, dport=SPECIFIC)
    for ihl in (6, 15):
        add("ihl_%d_syn" % ihl, SYN, ihl=ihl)
        add("ihl_%d_ack_data" % ihl, ACK | PSH, ihl=ihl, data=I.pattern(7, 3))
        add("ihl_%d_syn_listening" % ihl, SYN, ihl=ihl, dport=SPECIFIC)
    for doff in (5, 6, 15):
        add("doff_%d_syn" % doff, SYN, opts=bytes([1]) * (4 * (doff - 5)), data=I.pattern(3, 5))
        add("doff_%d_syn_listening" % doff, SYN, opts=bytes([1]) * (4 * (doff - 5)), dport=SPECIFIC)
    add("doff_4", SYN, doff=4)
    add("doff_4_data", SYN, doff=4, data=I.pattern(24, 1))
    add("doff_above_datagram", SYN, doff=15, data=I.pattern(8, 1))
    add("doff_6_no_room", ACK, doff=6)
    for v in (215, 216, 536, 1460):
        add("mss_%d_listening" % v, SYN, opts=mss_opt(v), dport=SPECIFIC)
        add("mss_%d_wildcard" % v, SYN, opts=mss_opt(v), dport=WILDCARD)
        add("mss_%d_closed" % v, SYN, opts=mss_opt(v))
    add("mss_0_listening", SYN, opts=mss_opt(0), dport=SPECIFIC)
    add("mss_215_ack_listening", ACK, opts=mss_opt(215), dport=SPECIFIC)
    add("mss_215_syn_ack_listening", SYN | ACK, opts=mss_opt(215), dport=SPECIFIC)
    add("mss_wrong_length_listening", SYN, opts=bytes([2, 3, 0, 1]), dport=SPECIFIC)
    add("mss_215_behind_end_listening", SYN, opts=bytes([0, 0, 0, 0]) + mss_opt(215), dport=SPECIFIC)
    add("mss_twice_listening", SYN, opts=mss_opt(1460) + mss_opt(100), dport=SPECIFIC)
    add("wnd_scale_listening", SYN, opts=mss_opt(1460) + bytes([1, 3, 3, 7]), dport=SPECIFIC)
    add("wnd_scale_alone_listening", SYN, opts=bytes([3, 3, 7, 1]), dport=SPECIFIC)
    add("wnd_scale_closed", SYN, opts=mss_opt(1460) + bytes([1, 3, 3, 7]))
    add("seq_ffffffff_syn", SYN, seq=0xFFFFFFFF)
    add("seq_fffffff0_32_bytes", PSH, seq=0xFFFFFFF0, data=I.pattern(32, 9))
    add("seq_ffffffff_fin_1_byte", FIN, seq=0xFFFFFFFF, data=b"\x42")
    add("ack_ffffffff", ACK, ack=0xFFFFFFFF)
    add("ack_0", ACK, ack=0)
    for name, src in (("all_ones", ALL_ONES), ("224_0_0_1", 0xE0000001), ("239_255_255_255", 0xEFFFFFFF),
                      ("240_0_0_1", 0xF0000001), ("subnet_bcast", bcast), ("zero", 0),
                      ("outside", 0xC0A80101), ("223_255_255_255", 0xDFFFFFFF)):
        add("src_%s_syn_closed" % name, SYN, src=src)
        add("src_%s_syn_listening" % name, SYN, src=src, dport=SPECIFIC)
        add("src_%s_ack_listening" % name, ACK, src=src, dport=SPECIFIC)
    for name, dst in (("subnet_bcast", bcast), ("all_ones", ALL_ONES), ("other_host", other)):
        add("dst_%s_syn_closed" % name, SYN, dst=dst)
        add("dst_%s_syn_listening" % name, SYN, dst=dst, dport=SPECIFIC)
        add("dst_%s_syn_wildcard" % name, SYN, dst=dst, dport=WILDCARD)
    add("bad_tcp_checksum", SYN, bad=True)
    add("bad_tcp_checksum_listening", SYN, bad=True, dport=SPECIFIC)
    for want in (0x0000, 0x0001, 0xFFFE, 0x8000):
        a = ack_for_rst_checksum(want, src=peer, dst=local, sport=40000, dport=CLOSED)
        add("rst_checksum_%04x" % want, ACK, ack=a)
    out.append(("udp_closed_port", LOCAL_MAC + PEER_MAC + b"\x08\x00" +
                I.ip_packet(17, I.udp(b"abc", src=peer, dst=local), src=peer, dst=local)))
    out.append(("short_tcp", LOCAL_MAC + PEER_MAC + b"\x08\x00" +
                I.ip_packet(6, tcp(SYN, src=peer, dst=local)[:19], src=peer, dst=local)))
    return out


def session(local, prefix, peer, gateway, count=50):
    """Frames for one stack that keeps its state: RSTs and drops only (no SYN reaches a listener,
    so no PCB arises and no SYN-ACK takes an Ident)."""
    bcast = (local & netmask(prefix)) | (~netmask(prefix) & ALL_ONES)
    out = []
    for k in range(count):
        kw = dict(src=peer, dst=local, sport=41000 + k, seq=0x01000000 * k + 17 * k, ack=0x9000 + 257 * k)
        kind = k % 10
        if kind in (0, 5):
            out.append(frame(SYN, **kw))
        elif kind == 1:
            out.append(frame(ACK, dport=SPECIFIC, **kw))
        elif kind == 2:
            out.append(frame(RST, **kw))
        elif kind == 3:
            out.append(frame(PSH, data=I.pattern(k, k), pad60=True, **kw))
        elif kind == 4:
            out.append(frame(SYN, **dict(kw, src=bcast)))
        elif kind == 6:
            out.append(frame(FIN | ACK, dport=WILDCARD, **kw))
        elif kind == 7:
            out.append(frame(SYN, bad=True, **kw))
        elif kind == 8:
            out.append(frame(SYN, **dict(kw, src=0xC0A80100 + k)))
        else:
            out.append(frame(SYN | FIN, dport=SPECIFIC, **kw))
    return out


def next_hop_arp(f, local, prefix, gateway):
    """The ARP reply that tells the stack the MAC of the next hop of an answer to `f`."""
    src = int.from_bytes(f[26:30], "big") if len(f) >= 34 else 0
    mask = netmask(prefix)
    bcast = (local & mask) | (~mask & ALL_ONES)
    inside = (src & mask) == (local & mask) and src not in (bcast, local & mask, local)
    hop = src if inside else gateway
    return AR.arp(2, hop, local, sha=f[6:12] if len(f) >= 12 else PEER_MAC, tha=LOCAL_MAC,
                  eth_src=PEER_MAC, eth_dst=LOCAL_MAC)


def build_generator(reference):
    os.makedirs(os.path.dirname(GEN_BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(reference, "src"), "-o", GEN_BIN,
                    GEN_SRC], check=True)
    return GEN_BIN


def _event(e):
    """A sent frame as the fixture records it."""
    f = bytes.fromhex(e[2:])
    if len(f) >= 54 and f[12:14] == b"\x08\x00" and f[23] == 6:
        t = 14 + (f[14] & 0xF) * 4
        if f[t + 13] & SYN:
            return "SYNACK"
    return e


def generate(reference):
    """The fixture's text, from the reference's code run on the cases above."""
    gen = build_generator(reference)
    req, plan = [], []

    def start(local, prefix, gateway):
        req.append("S %d %d %d %s" % (local, prefix, gateway, LOCAL_MAC.hex()))
        for addr, port in listeners(local):
            req.append("L %d %d" % (addr, port))

    def feed(f, local, prefix, gateway):
        req.append("Q " + next_hop_arp(f, local, prefix, gateway).hex())
        req.append("F " + (f.hex() or "-"))

    for local, prefix, peer, gateway in STACKS:
        cs = cases(local, prefix, peer, gateway)
        for name, f in cs:
            start(local, prefix, gateway)
            feed(f, local, prefix, gateway)
        ss = session(local, prefix, peer, gateway)
        start(local, prefix, gateway)
        for f in ss:
            feed(f, local, prefix, gateway)
        plan.append((local, prefix, gateway, cs, ss))
    ans = subprocess.run([gen], input="\n".join(req) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert ans[-1] == ""
    at = 0

    def events():
        nonlocal at
        got = []
        while ans[at] != ".":
            assert ans[at][:2] == "T "
            got.append(_event(ans[at]))
            at += 1
        at += 1
        return got

    stacks = []
    for local, prefix, gateway, cs, ss in plan:
        s = {"addr": local, "prefix": prefix, "gateway": gateway, "mac": LOCAL_MAC.hex(),
             "listeners": [list(l) for l in listeners(local)], "cases": []}
        for name, f in cs:
            s["cases"].append({"name": name, "in": f.hex(), "out": events()})
        s["session"] = {"in": [f.hex() for f in ss], "out": [events() for _ in ss]}
        stacks.append(s)
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
