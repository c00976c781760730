"""TEST INFRASTRUCTURE -- reference-produced answers for the UDP Rx demux: the reference's own
IpStack with IpUdpProto, UdpListeners and UdpAssociations (udp_rx_ref_gen.cpp only includes
reference headers; the platform, the capture driver and the recording handlers are this
project's), compiled from the reference tree and fed the IP packets below. Every packet is
injected twice, into two stacks set up alike: one whose handlers all return AcceptContinue, one
whose handlers all return Reject (so the j-th message a stack sends carries the Ident j). The answers are recorded in udp_rx_ref_cases.json:

  {"stacks": [{"name": .., "addr": .., "prefix": .., "gateway": ..,
               "listeners": [[iface_addr, port, accept_broadcast, accept_nonlocal_dst], ...],
               "assocs": [[local_addr, remote_addr, local_port, remote_port, accept_nonlocal_dst], ...],
               "cases": [{"name": .., "in": "<hex IP packet>",
                          "calls": ["<L|A><creation number> <data length> <FNV-1a 64> <has_checksum>", ...],
                          "out": ["<hex IP packet>", ...],          (handlers accept)
                          "reject_out": ["<hex IP packet>", ...],   (handlers reject)
                          "src_rejected": 0|1}]}]}

"listeners" and "assocs" are in creation order; the reference walks its listener list newest
first (startListening prepends), which is the order of the device table (listener_table()).
"calls" is the same under both answers (a Reject does not end the walk) and is recorded once; the
generator run asserts that. "src_rejected": the source is one checkSendIp4Allowed refuses, so the
reference sends no unreach where IpUdpProto asks for one.

    python3 tests/golden/udp_rx_ref.py <reference tree>      # rewrites the fixture
"""
import json
import os
import struct
import subprocess
import sys

import icmp_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "udp_rx_ref_cases.json")
GEN_SRC = os.path.join(HERE, "udp_rx_ref_gen.cpp")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "udp_rx_ref_gen")

LOCAL, PREFIX, BCAST, GATEWAY, PEER, ALL_ONES = R.LOCAL, R.PREFIX, R.BCAST, R.GATEWAY, R.PEER, R.ALL_ONES
NONLOCAL = LOCAL + 1          # a unicast address of the subnet that is not the interface's
NONLOCAL2 = LOCAL + 2
SPORT = 40000
pattern = R.pattern


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def udp(data, *, src=PEER, dst=LOCAL, sport=SPORT, dport=5000, chk="good", udp_len=None, extra=b""):
    """A UDP datagram whose Length field is `udp_len` (default: 8 + the data), followed by `extra`
    bytes; the checksum ("good", "bad", "zero") covers the Length field's bytes, as the reference
    sums them after its truncation."""
    ln = 8 + len(data) if udp_len is None else udp_len
    u = bytearray(struct.pack(">HHHH", sport, dport, ln, 0) + data + extra)
    if chk != "zero":
        covered = bytes(u[:ln]) if 8 <= ln <= len(u) else bytes(u)
        c = R.chksum(struct.pack(">IIHH", src, dst, 17, ln) + covered) or 0xFFFF
        struct.pack_into(">H", u, 6, c ^ (0x0100 if chk == "bad" else 0))
    return bytes(u)


def packet(data=b"\x01\x02\x03", *, src=PEER, dst=LOCAL, ihl=5, ttl=61, **kw):
    return R.ip_packet(17, udp(data, src=src, dst=dst, **kw), src=src, dst=dst, ihl=ihl, ttl=ttl)


DSTS = (("local", LOCAL), ("bcast", BCAST), ("allones", ALL_ONES), ("nonlocal", NONLOCAL))

# The listeners of stack "ports": [iface_addr, port, accept_broadcast, accept_nonlocal_dst]
PORT_LISTENERS = [
    [0, 5000, 0, 0],
    [0, 5001, 1, 0],
    [0, 5002, 0, 1],
    [0, 5003, 1, 1],
    [0, 5000, 0, 0],              # a second and a third listener of one port
    [LOCAL, 5004, 0, 0],          # iface_addr equal to the interface's
    [NONLOCAL, 5005, 1, 1],       # iface_addr different: never matches
    [LOCAL, 5000, 1, 0],
]
PORT_ASSOCS = [
    [LOCAL, PEER, 6000, SPORT, 0],
    [NONLOCAL, PEER, 6000, SPORT, 1],      # non-local destination, accepted
    [NONLOCAL2, PEER, 6000, SPORT, 0],     # non-local destination, not accepted
    [LOCAL, PEER, 5000, SPORT, 0],         # an association and listeners for one packet
    [BCAST, PEER, 6000, SPORT, 1],
    [LOCAL, PEER, 6002, SPORT, 1],         # accept_nonlocal_dst with a local destination
]


def port_cases():
    out = []
    for port in (5000, 5001, 5002, 5003, 5004, 5005, 7):
        for dn, dst in DSTS:
            out.append(("lis_port%d_dst_%s" % (port, dn), packet(dst=dst, dport=port)))
    # associations: present, absent, keys that differ in exactly one field
    out.append(("assoc_hit", packet(dport=6000)))
    out.append(("assoc_hit_nonlocal_flag_local_dst", packet(dport=6002)))
    out.append(("assoc_nonlocal_accepted", packet(dst=NONLOCAL, dport=6000)))
    out.append(("assoc_nonlocal_refused", packet(dst=NONLOCAL2, dport=6000)))
    out.append(("assoc_bcast_dst", packet(dst=BCAST, dport=6000)))
    out.append(("assoc_and_listeners", packet(dport=5000)))
    out.append(("assoc_miss_remote_addr", packet(src=PEER + 1, dport=6000)))
    out.append(("assoc_miss_remote_port", packet(sport=SPORT + 1, dport=6000)))
    out.append(("assoc_miss_local_port", packet(dport=6001)))
    out.append(("assoc_miss_local_addr", packet(dst=LOCAL + 3, dport=6000)))
    out.append(("assoc_and_listeners_miss_remote_port", packet(sport=SPORT - 1, dport=5000)))
    # the UDP length, at an open and at a closed port
    for pn, port in (("open", 5000), ("closed", 7), ("assoc", 6000)):
        out.append(("len_8_%s" % pn, packet(b"", dport=port)))
        out.append(("len_equal_%s" % pn, packet(R.pattern(20, 3), dport=port)))
        out.append(("len_truncates_%s" % pn, packet(R.pattern(6, 4), dport=port, extra=R.pattern(9, 5))))
        out.append(("len_truncates_to_8_%s" % pn, packet(b"", dport=port, extra=R.pattern(4, 6))))
        out.append(("len_above_ip_%s" % pn, packet(R.pattern(6, 7), dport=port, udp_len=15)))
        out.append(("len_7_%s" % pn, packet(R.pattern(6, 8), dport=port, udp_len=7)))
        out.append(("len_0_%s" % pn, packet(R.pattern(6, 9), dport=port, udp_len=0)))
        for chk in ("zero", "good", "bad"):
            out.append(("chksum_%s_%s" % (chk, pn), packet(R.pattern(11, 10), dport=port, chk=chk)))
        out.append(("chksum_zero_truncated_%s" % pn,
                    packet(R.pattern(5, 11), dport=port, chk="zero", extra=R.pattern(3, 12))))
        for ihl in (5, 15):
            out.append(("ihl%d_%s" % (ihl, pn), packet(R.pattern(13, ihl), dport=port, ihl=ihl, ttl=7 + ihl)))
    out.append(("chksum_bad_nonlocal", packet(dst=NONLOCAL, dport=7, chk="bad")))
    # sources the reference sends no unreach to
    out.append(("src_all_ones_closed", packet(src=ALL_ONES, dport=7)))
    out.append(("src_bcast_closed", packet(src=BCAST, dport=7)))
    out.append(("src_multicast_closed", packet(src=0xE0000001, dport=7)))
    out.append(("src_all_ones_open", packet(src=ALL_ONES, dport=5000)))
    return out


# Stack "any": listeners of port 0.
ANY_LISTENERS = [
    [0, 0, 0, 0],
    [0, 0, 1, 1],
    [LOCAL, 0, 1, 0],
    [NONLOCAL, 0, 1, 1],
]


def any_cases():
    out = []
    for port in (1, 5000, 65535):
        for dn, dst in DSTS:
            out.append(("any_port%d_dst_%s" % (port, dn), packet(dst=dst, dport=port)))
    return out


# Stack "none": no listener, no association.
def none_cases():
    return [("none_dst_%s" % dn, packet(dst=dst, dport=5000)) for dn, dst in DSTS]


STACKS = (("ports", PORT_LISTENERS, PORT_ASSOCS, port_cases),
          ("any", ANY_LISTENERS, [], any_cases),
          ("none", [], [], none_cases))


def listener_table(stack):
    """The stack's listeners in the order the reference walks them (newest first):
    [(creation number, [iface_addr, port, accept_broadcast, accept_nonlocal_dst])]."""
    return [(k, stack["listeners"][k]) for k in reversed(range(len(stack["listeners"])))]


def build_generator(reference):
    os.makedirs(os.path.dirname(GEN_BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(reference, "src"), "-o", GEN_BIN,
                    GEN_SRC], check=True)
    return GEN_BIN


def generate(reference):
    """The fixture's text, from the reference's code run on the cases above."""
    gen = build_generator(reference)
    req, plan = [], []
    for name, listeners, assocs, cases in STACKS:
        cs = cases()
        plan.append((name, listeners, assocs, cs))
        for mode in (0, 1):                              # a fresh stack per answer: the Ident of
            req.append("S %d %d %d" % (LOCAL, PREFIX, GATEWAY))   # its j-th message is j
            req += ["L %d %d %d %d" % tuple(l) for l in listeners]
            req += ["A %d %d %d %d %d" % tuple(a) for a in assocs]
            req += ["I %d %s" % (mode, p.hex()) for _, p in cs]
    ans = subprocess.run([gen], input="\n".join(req) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert ans[-1] == ""
    at = 0

    def answer():
        nonlocal at
        calls, out = [], []
        while ans[at] != ".":
            kind, rest = ans[at].split(" ", 1)
            if kind == "C":
                k, number, ln, h, hc = rest.split()
                calls.append("%s%s %s %s %s" % (k, number, ln, h, hc))
            else:
                assert kind == "P"
                out.append(rest)
            at += 1
        at += 1
        return calls, out

    stacks = []
    for name, listeners, assocs, cs in plan:
        rows = []
        accepting = [answer() for _ in cs]
        rejecting = [answer() for _ in cs]
        for (cname, pkt), (calls, out), (calls_r, out_r) in zip(cs, accepting, rejecting):
            assert calls == calls_r, cname               # a Reject does not end the walk
            src, = struct.unpack_from(">I", pkt, 12)
            rows.append({"name": cname, "in": pkt.hex(), "calls": calls, "out": out, "reject_out": out_r,
                         "src_rejected": int(src in (ALL_ONES, BCAST))})
        stacks.append({"name": name, "addr": LOCAL, "prefix": PREFIX, "gateway": GATEWAY,
                       "listeners": listeners, "assocs": assocs, "cases": rows})
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
