"""TEST INFRASTRUCTURE -- reference-produced answers for the send path's route, permission tests,
ARP lookup and Ethernet header: the reference's own IpStack with one to three EthIpIface
(tx_resolve_ref_gen.cpp only includes reference headers; the platform and the capture drivers are
stubs of this project's), compiled from the reference tree and driven through the command
sequences below. The answers are recorded in tx_resolve_ref_cases.json:

  {"stacks": [{"name": .., "ifaces": [{"have", "addr", "prefix", "have_gw", "gateway", "mac"}, ...],
               "steps": [{"op": "F", "iface": k, "in": "<hex frame>", "out": [<event>, ...]},
                         {"op": "D", "name": .., "src": .., "dst": .., "flags": .., "iface": k or -1,
                          "err": <IpErr>, "out": [<event>, ...]}, ...]}]}

The interfaces are listed in the order they were constructed; the stack's list iterates them
last-constructed first (ip/IpIface.h:97). An event is "T <k> <hex>" (interface k's driver was
handed an IPv4 frame: its first 14 bytes) or "Q <k> <hex>" (any other frame, in full: the ARP
requests the stack sent, and its replies to injected requests). A stack's steps run in order on one
stack, so the ARP tables carry over: "F" injects a frame (an ARP reply or request that fills a
table), "D" is sendIp4Dgram(src, dst, flags, interface or none) with 8 payload bytes.

    python3 tests/golden/tx_resolve_ref.py <reference tree>      # rewrites the fixture
"""
import json
import os
import subprocess
import sys

import arp_ref as A
import frame_cases as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "tx_resolve_ref_cases.json")
GEN_SRC = os.path.join(HERE, "tx_resolve_ref_gen.cpp")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "tx_resolve_ref_gen")

ALL_ONES = 0xFFFFFFFF
ALLOW_BROADCAST, ALLOW_NONLOCAL_SRC = 1, 2      # IpSendFlags::AllowBroadcastFlag, ::AllowNonLocalSrc
OUTSIDE = 0xC0A84D07                            # 192.168.77.7
MULTICAST = 0xE0000001                          # 224.0.0.1
NUM_ARP_ENTRIES = 16                            # the generator's EthIpIfaceOptions::NumArpEntries


def ip(a, b, c, d):
    return a << 24 | b << 16 | c << 8 | d


def mac_of(k):
    return bytes([0x02, 0x00, 0x5E, 0x10, 0x20, 0x30 + k])


def peer_mac(addr, gen=0):
    """The MAC a peer with this address answers with (gen: after it changed its adapter)."""
    return bytes([0x02, 0x77 + gen, addr >> 24, addr >> 16 & 0xFF, addr >> 8 & 0xFF, addr & 0xFF])


def iface(k, addr=None, prefix=0, gateway=None):
    return {"have": int(addr is not None), "addr": addr or 0, "prefix": prefix,
            "have_gw": int(gateway is not None), "gateway": gateway or 0, "mac": mac_of(k).hex()}


# (name, interfaces in construction order)
STACKS = (
    ("one_24_gw", [iface(0, ip(10, 20, 30, 40), 24, ip(10, 20, 30, 1))]),
    ("one_30", [iface(0, ip(10, 20, 30, 41), 30)]),
    ("one_no_addr", [iface(0)]),
    ("one_no_addr_gw", [iface(0, gateway=ip(10, 20, 30, 1))]),
    # overlapping prefixes: the /30 inside the /24 inside the /16; the list iterates 2, 1, 0
    ("three_nested", [iface(0, ip(10, 20, 0, 5), 16), iface(1, ip(10, 20, 30, 40), 24, ip(10, 20, 30, 1)),
                      iface(2, ip(10, 20, 30, 41), 30)]),
    # one subnet twice: the list order decides, for the subnet and for the gateway
    ("two_same_24", [iface(0, ip(10, 20, 30, 40), 24, ip(10, 20, 30, 1)),
                     iface(1, ip(10, 20, 30, 50), 24, ip(10, 20, 30, 2))]),
    # a gateway interface met first in the list, a local one behind it; one without an address
    ("three_mixed", [iface(0, ip(10, 20, 30, 40), 24), iface(1, gateway=ip(10, 9, 9, 9)),
                     iface(2, ip(192, 168, 1, 10), 24, ip(192, 168, 1, 1))]),
)


def netmask(prefix):
    return (ALL_ONES << (32 - prefix)) & ALL_ONES if prefix else 0


def subnet(f):
    net = f["addr"] & netmask(f["prefix"])
    return net, net | (~netmask(f["prefix"]) & ALL_ONES)


def sends(ifaces):
    """[(name, src, dst, flags, iface or -1)]: one round of datagrams over a stack."""
    out = []
    first = next((f for f in ifaces if f["have"]), None)
    own = first["addr"] if first else ip(10, 20, 30, 40)
    for k, f in enumerate(ifaces):
        if not f["have"]:
            continue
        net, bcast = subnet(f)
        peer = net | ((f["addr"] + 1) & ~netmask(f["prefix"]) & ALL_ONES or 1)
        if peer == bcast:
            peer = net | 1
        tag = "if%d_" % k
        out += [(tag + "peer", f["addr"], peer, 0, -1),
                (tag + "peer_src_of_first", own, peer, 0, -1),
                (tag + "peer_nonlocal_allowed", OUTSIDE, peer, ALLOW_NONLOCAL_SRC, -1),
                (tag + "subnet_bcast", f["addr"], bcast, 0, -1),
                (tag + "subnet_bcast_allowed", f["addr"], bcast, ALLOW_BROADCAST, -1),
                (tag + "subnet_bcast_nonlocal_src", OUTSIDE, bcast, 0, -1),
                (tag + "subnet_bcast_allowed_nonlocal_src", OUTSIDE, bcast, ALLOW_BROADCAST, -1),
                (tag + "network_addr", f["addr"], net, 0, -1),
                (tag + "own_addr", f["addr"], f["addr"], 0, -1)]
        if f["have_gw"]:
            out.append((tag + "gateway_itself", f["addr"], f["gateway"], 0, -1))
    for name, dst in (("outside", OUTSIDE), ("zero", 0), ("multicast", MULTICAST), ("all_ones", ALL_ONES)):
        out += [(name, own, dst, 0, -1), (name + "_both_flags", OUTSIDE, dst, 3, -1),
                (name + "_allow_broadcast", own, dst, ALLOW_BROADCAST, -1)]
    # a named interface: each one with its own peer's address, another's, and the far ones
    peers = [o for o in out if o[0].endswith("_peer")]
    for k, f in enumerate(ifaces):
        src = f["addr"] if f["have"] else own
        tag = "force%d_" % k
        for name, _, dst, _, _ in peers[:2]:
            out += [(tag + name, src, dst, 0, k), (tag + name + "_nonlocal_allowed", own, dst, 2, k)]
        out += [(tag + "outside", src, OUTSIDE, 0, k), (tag + "outside_both_flags", OUTSIDE, OUTSIDE, 3, k),
                (tag + "all_ones", src, ALL_ONES, 0, k), (tag + "all_ones_allowed", src, ALL_ONES, 1, k),
                (tag + "all_ones_both_flags", OUTSIDE, ALL_ONES, 3, k), (tag + "zero_both_flags", src, 0, 3, k)]
    return out


def next_hops(ifaces):
    """Every (interface, address) an ARP answer is injected for: the unicast destinations of a
    round and the gateways, on every interface that has the address in its subnet."""
    want = []
    dsts = {s[2] for s in sends(ifaces)} | {f["gateway"] for f in ifaces if f["have_gw"]}
    for k, f in enumerate(ifaces):
        if not f["have"]:
            continue
        net, bcast = subnet(f)
        for d in sorted(dsts):
            if d not in (0, ALL_ONES, bcast, f["addr"]) and (d & netmask(f["prefix"])) == net:
                want.append((k, d))
    return want


def answers(ifaces, gen):
    """ARP frames that fill the tables: a reply to the interface for every other hop, a broadcast
    request (for some third address) from the rest."""
    out = []
    for n, (k, addr) in enumerate(next_hops(ifaces)):
        f = ifaces[k]
        if n % 3 != 2:
            fr = A.arp(2, addr, f["addr"], sha=peer_mac(addr, gen), tha=bytes.fromhex(f["mac"]),
                       eth_src=peer_mac(addr, gen), eth_dst=bytes.fromhex(f["mac"]))
        else:
            fr = A.arp(1, addr, f["addr"] ^ 0x80, sha=peer_mac(addr, gen), eth_src=F.peer_mac(1))
        out.append((k, fr))
    # an interface without an address hears an answer too: nothing is learned from it
    for k, f in enumerate(ifaces):
        if not f["have"]:
            out.append((k, A.arp(2, ip(10, 20, 30, 1), ip(10, 20, 30, 40), sha=peer_mac(ip(10, 20, 30, 1), gen))))
    return out


def plan(ifaces):
    """The steps of one stack: a round on empty tables (queries start), the same round again
    (queries in progress), the answers, the round resolved, changed answers, the round again."""
    steps = []
    for rnd, gen in (("empty", None), ("query", None), ("valid", 0), ("changed", 1)):
        if gen is not None:
            steps += [("F", k, fr) for k, fr in answers(ifaces, gen)]
        steps += [("D", "%s_%s" % (rnd, s[0])) + s[1:] for s in sends(ifaces)]
    return steps


def build_generator(reference):
    os.makedirs(os.path.dirname(GEN_BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(reference, "src"), "-o", GEN_BIN,
                    GEN_SRC], check=True)
    return GEN_BIN


def generate(reference):
    """The fixture's text, from the reference's code run on the plans above."""
    gen = build_generator(reference)
    req = []
    for name, ifaces in STACKS:
        assert all(sum(1 for k, _ in next_hops(ifaces) if k == j) + 2 < NUM_ARP_ENTRIES
                   for j in range(len(ifaces))), name     # no table ever recycles an entry
        req.append("S %d " % len(ifaces) + " ".join(
            "%d %d %d %d %d %s" % (f["have"], f["addr"], f["prefix"], f["have_gw"], f["gateway"], f["mac"])
            for f in ifaces))
        for st in plan(ifaces):
            req.append("F %d %s" % (st[1], st[2].hex()) if st[0] == "F" else "D %d %d %d %d" % st[2:])
    ans = subprocess.run([gen], input="\n".join(req) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert ans[-1] == ""
    at = 0

    def events():
        nonlocal at
        got = []
        while ans[at] != ".":
            assert ans[at][:2] in ("T ", "Q ")
            got.append(ans[at])
            at += 1
        at += 1
        return got

    stacks = []
    for name, ifaces in STACKS:
        steps = []
        for st in plan(ifaces):
            if st[0] == "F":
                steps.append({"op": "F", "iface": st[1], "in": st[2].hex(), "out": events()})
            else:
                assert ans[at][:2] == "E "
                err = int(ans[at][2:])
                at += 1
                steps.append({"op": "D", "name": st[1], "src": st[2], "dst": st[3], "flags": st[4],
                              "iface": st[5], "err": err, "out": events()})
        stacks.append({"name": name, "ifaces": ifaces, "steps": steps})
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
