"""TEST INFRASTRUCTURE -- reference-produced answers for ARP on receive: the reference's own
EthIpIface over its IpStack (arp_ref_gen.cpp only includes reference headers; the platform and the
capture driver are stubs of this project's), compiled from the reference tree and fed the Ethernet
frames below. The answers are recorded in arp_ref_cases.json:

  {"stacks": [{"have": 0|1, "addr": .., "prefix": .., "mac": "<hex>",
               "cases": [{"name": .., "in": "<hex frame>", "out": [<event>, ...],
                          "probe": "<hex frame>", "probe_out": [<event>, ...]}]}]}

An event is "T <hex frame>" (a frame the stack sent, in full) or "O <ip> <hex mac>" (an
EthArpObserver notification), in the order they happened. Every case runs on a fresh stack: the
frame "in" is injected, then the probe, an ICMP echo request whose IPv4 source is the case's ARP
sender address: its echo reply leaves for the MAC the stack learned from "in", or an ARP query is
broadcast because it learned none, or nothing leaves.

    python3 tests/golden/arp_ref.py <reference tree>      # rewrites the fixture
"""
import json
import os
import struct
import subprocess
import sys

import frame_cases as F
import icmp_ref as I

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "arp_ref_cases.json")
GEN_SRC = os.path.join(HERE, "arp_ref_gen.cpp")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "arp_ref_gen")

LOCAL_MAC = F.LOCAL_MAC
SENDER_MAC = F.peer_mac(0)      # the ARP sender hardware address
ETH_SRC = F.peer_mac(1)         # the Ethernet source of the ARP frames: another MAC
PROBE_MAC = F.peer_mac(2)       # the Ethernet source of the probes: a third
BCAST_MAC = b"\xff" * 6
ALL_ONES = 0xFFFFFFFF
OUTSIDE = 0xC0A80101            # 192.168.1.1

# (has an address, address, prefix, a peer in the subnet)
STACKS = ((1, 0x0A141E28, 24, 0x0A141E64),      # 10.20.30.40/24, peer .100
          (1, 0x0A141E29, 30, 0x0A141E2A),      # 10.20.30.41/30, peer .42 (broadcast .43)
          (0, 0x0A141E28, 24, 0x0A141E64))      # no address


def netmask(prefix):
    return (ALL_ONES << (32 - prefix)) & ALL_ONES


def arp(op, spa, tpa, *, sha=SENDER_MAC, tha=bytes(6), eth_src=ETH_SRC, eth_dst=BCAST_MAC,
        ethertype=0x0806, hwtype=1, ptype=0x0800, hlen=6, plen=4, pad=0):
    """An Ethernet frame with an ARP packet, then `pad` bytes of padding."""
    return (eth_dst + eth_src + struct.pack(">H", ethertype) +
            struct.pack(">HHBBH", hwtype, ptype, hlen, plen, op) + sha + struct.pack(">I", spa) +
            tha + struct.pack(">I", tpa) + bytes([0x5A]) * pad)


def probe(src, dst, *, eth_src=PROBE_MAC):
    """The echo request that asks the stack what it learned about `src`."""
    return LOCAL_MAC + eth_src + b"\x08\x00" + I.echo(I.pattern(5, 3), src=src, dst=dst)


def cases(have, local, prefix, peer):
    """[(name, frame, ARP sender address, Ethernet source of the probe)] for one stack."""
    bcast = (local & netmask(prefix)) | (~netmask(prefix) & ALL_ONES)
    other = peer if prefix == 30 else local + 1
    out = []

    def add(name, frame, sender=peer, probe_mac=PROBE_MAC):
        out.append((name, frame, sender, probe_mac))

    add("request_for_us", arp(1, peer, local))
    add("request_for_us_eth_src_is_sender", arp(1, peer, local, eth_src=SENDER_MAC))
    add("request_unicast", arp(1, peer, local, eth_dst=LOCAL_MAC))
    add("request_for_other", arp(1, peer, other))
    add("reply_to_us", arp(2, peer, local, tha=LOCAL_MAC, eth_dst=LOCAL_MAC))
    add("reply_to_other", arp(2, peer, other, tha=F.peer_mac(3)))
    add("op0", arp(0, peer, local))
    add("op3", arp(3, peer, local))
    add("op_0x0100", arp(0x0100, peer, local))
    for field, good in (("hwtype", 1), ("ptype", 0x0800), ("hlen", 6), ("plen", 4)):
        add("%s_minus_1" % field, arp(1, peer, local, **{field: good - 1}))
        add("%s_plus_1" % field, arp(1, peer, local, **{field: good + 1}))
    add("hwtype_swapped", arp(1, peer, local, hwtype=0x0100))
    add("len41", arp(1, peer, local)[:41])
    add("len42", arp(1, peer, local))
    add("len60", arp(1, peer, local, pad=18))
    add("len60_for_other", arp(1, peer, other, pad=18))
    add("len14_arp", arp(1, peer, local)[:14])
    add("len13", arp(1, peer, local)[:13])
    add("len0", b"")
    add("ethertype_ip4", arp(1, peer, local, ethertype=0x0800))
    add("ethertype_ip6", arp(1, peer, local, ethertype=0x86DD))
    add("ethertype_0x0608", arp(1, peer, local, ethertype=0x0608))
    add("sender_mac_bcast_request", arp(1, peer, local, sha=BCAST_MAC))
    add("sender_mac_bcast_reply", arp(2, peer, local, sha=BCAST_MAC))
    add("sender_mac_almost_bcast", arp(1, peer, other, sha=b"\xff" * 5 + b"\xfe"))
    add("sender_zero_request", arp(1, 0, local), sender=0)                    # an ARP probe
    add("sender_zero_for_other", arp(1, 0, other), sender=0)
    add("sender_zero_mac_bcast_request", arp(1, 0, local, sha=BCAST_MAC), sender=0)
    add("sender_zero_mac_bcast_reply", arp(2, 0, local, sha=BCAST_MAC), sender=0)
    add("sender_all_ones_request", arp(1, ALL_ONES, local), sender=ALL_ONES)
    add("sender_all_ones_reply", arp(2, ALL_ONES, local), sender=ALL_ONES)
    add("sender_subnet_bcast_request", arp(1, bcast, local), sender=bcast)
    add("sender_subnet_bcast_reply", arp(2, bcast, local), sender=bcast)
    add("sender_outside_request", arp(1, OUTSIDE, local), sender=OUTSIDE)
    add("sender_outside_reply", arp(2, OUTSIDE, local), sender=OUTSIDE)
    add("sender_network_addr", arp(2, local & netmask(prefix), local), sender=local & netmask(prefix))
    add("gratuitous_request_peer", arp(1, peer, peer))
    add("gratuitous_reply_peer", arp(2, peer, peer, tha=BCAST_MAC))
    add("gratuitous_request_own_addr", arp(1, local, local), sender=local)
    add("target_mac_garbage", arp(1, peer, local, tha=bytes([0xDE, 0xAD, 0xBE, 0xEF, 0x01, 0x02])))
    add("arp_then_echo_one_peer", arp(1, peer, local, eth_src=SENDER_MAC), probe_mac=SENDER_MAC)
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
    for have, local, prefix, peer in STACKS:
        for name, frame, sender, probe_mac in cases(have, local, prefix, peer):
            p = probe(sender, local, eth_src=probe_mac)
            req.append("S %d %d %d %s" % (have, local, prefix, LOCAL_MAC.hex()))
            req.append("F " + (frame.hex() or "-"))
            req.append("F " + p.hex())
            plan.append((have, local, prefix, name, frame, p))
    ans = subprocess.run([gen], input="\n".join(req) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert ans[-1] == ""
    at, stacks = 0, []

    def events():
        nonlocal at
        got = []
        while ans[at] != ".":
            assert ans[at][:2] in ("T ", "O ")
            got.append(ans[at])
            at += 1
        at += 1
        return got

    for have, local, prefix, name, frame, p in plan:
        if not stacks or (stacks[-1]["have"], stacks[-1]["addr"], stacks[-1]["prefix"]) != (have, local, prefix):
            stacks.append({"have": have, "addr": local, "prefix": prefix, "mac": LOCAL_MAC.hex(),
                           "cases": []})
        out = events()
        stacks[-1]["cases"].append({"name": name, "in": frame.hex(), "out": out, "probe": p.hex(),
                                    "probe_out": events()})
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
