"""TEST INFRASTRUCTURE -- reference-produced answers for the whole receive loop: the reference's own
EthIpIface over its IpStack with IpUdpProto (rx_loop_ref_gen.cpp only includes reference headers;
the platform, the capture driver and the recording handlers are this project's), compiled from the
reference tree and fed SESSIONS: sequences of Ethernet frames injected into ONE stack that keeps
its state (its ARP table, its next Ident). The answers are recorded in rx_loop_ref_cases.json:

  {"sessions": [{"allow": 0|1, "addr": .., "prefix": .., "mac": "<hex>", "seed": ..,
                 "listeners": [[iface_addr, port, accept_broadcast, accept_nonlocal_dst], ...],
                 "assocs": [[local_addr, remote_addr, local_port, remote_port, accept_nonlocal_dst], ...],
                 "frames": [["<hex frame in>", ["<hex frame the stack sent>", ...],
                             ["<L|A><creation number> <data length>", ...]], ...]}]}

"listeners" and "assocs" are in creation order (udp_rx_ref.listener_table gives the order the
reference walks them in); every handler accepts (AcceptContinue).

A session holds four peers. A peer's first frame is an ARP request for the interface's address
whose Ethernet source is its sender hardware address, so the reference knows every peer's MAC
before that peer's first IP frame and every response leaves for the received frame's source MAC.
Then, mixed by a seeded generator: echo requests, UDP for an association, for listeners and for
closed ports, broadcast UDP and broadcast pings (with AllowBroadcastPing off and on), more ARP, and
frames that every stage drops. No TCP (the reference would send resets), no fragments, no response
above the MTU, no protocol other than ICMP and UDP.

    python3 tests/golden/rx_loop_ref.py <reference tree>      # rewrites the fixture
"""
import json
import os
import random
import struct
import subprocess
import sys

import arp_ref as AR
import frame_cases as F
import icmp_ref as I
import udp_rx_ref as U

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "rx_loop_ref_cases.json")
GEN_SRC = os.path.join(HERE, "rx_loop_ref_gen.cpp")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "rx_loop_ref_gen")

LOCAL, ALL_ONES = I.LOCAL, I.ALL_ONES
LOCAL_MAC = F.LOCAL_MAC
PEERS = tuple((I.PEER + p, F.peer_mac(p)) for p in range(4))
OTHER_HOST = LOCAL + 1

# (AllowBroadcastPing, prefix, frames, seed)
SESSIONS = ((0, 24, 330, 1), (1, 24, 360, 2), (1, 16, 390, 3))
LISTENERS = [[0, 5000, 0, 0], [0, 5001, 1, 0], [0, 5001, 1, 1], [LOCAL, 5002, 0, 0], [OTHER_HOST, 5003, 1, 1]]
ASSOCS = [[LOCAL, PEERS[0][0], 6000, 30000, 0], [LOCAL, PEERS[1][0], 6001, 30001, 0]]
CLOSED = (7, 9, 5003, 6000, 40000)

KINDS = (("echo", 24), ("echo_opts", 3), ("udp_assoc", 9), ("udp_lis", 14), ("udp_closed", 14), ("udp_zero", 3),
         ("udp_bcast", 8), ("ping_bcast", 5), ("arp_req", 4), ("arp_other", 3), ("arp_bad", 2), ("bad_ip", 3),
         ("runt", 2), ("not_ip", 1), ("echo_bad", 2), ("icmp_other", 2), ("udp_bad", 2), ("udp_other_host", 2),
         ("echo_other_host", 1))


def eth(pkt, mac, pad60=False):
    f = LOCAL_MAC + mac + b"\x08\x00" + pkt
    return f + bytes([0x5A]) * (60 - len(f)) if pad60 and len(f) < 60 else f


def join(peer):
    """The peer's first frame: an ARP request for the interface's address from its own MAC."""
    ip, mac = peer
    return AR.arp(1, ip, LOCAL, sha=mac, tha=bytes(6), eth_src=mac, eth_dst=AR.BCAST_MAC, pad=0)


def frame(rng, kind, k, peer, bcast):
    ip, mac = peer
    data = I.pattern(rng.choice((0, 1, 2, 7, 18, 19, 40)), k & 0xFF)
    rest = struct.pack(">HH", rng.getrandbits(16), k)
    if kind in ("echo", "echo_opts", "ping_bcast", "echo_bad", "echo_other_host"):
        dst = {"ping_bcast": (bcast, ALL_ONES)[k & 1], "echo_other_host": OTHER_HOST}.get(kind, LOCAL)
        msg = I.icmp(8, 0, rest, data, bad=kind == "echo_bad")
        return eth(I.ip_packet(1, msg, src=ip, dst=dst, ihl=5 + (kind == "echo_opts") * (1 + k % 10), flags_off=0,
                               ident=k, ttl=61), mac, bool(k & 1))
    if kind == "icmp_other":
        return eth(I.ip_packet(1, I.icmp((0, 13)[k & 1], 0, rest, data), src=ip, dst=LOCAL, ihl=5, flags_off=0,
                               ident=k, ttl=61), mac, True)
    if kind.startswith("udp_"):
        src, sport, dst, chk = ip, U.SPORT, LOCAL, "good"
        if kind == "udp_assoc":
            dst, src, dport, sport = ASSOCS[k % 2][:4]
            mac = dict(PEERS)[src]
        elif kind == "udp_lis":
            dport = (5000, 5001, 5002)[k % 3]
        elif kind == "udp_bcast":
            dport, dst = (5000, 5001, 7)[k % 3], (bcast, ALL_ONES)[(k >> 2) & 1]
        elif kind == "udp_other_host":
            dport, dst = (5001, 7)[k & 1], OTHER_HOST
        else:
            dport = CLOSED[k % len(CLOSED)] if kind != "udp_bad" else 5000
            chk = {"udp_zero": "zero", "udp_bad": "bad"}.get(kind, "good")
        return eth(U.packet(data, src=src, dst=dst, ihl=5 + (k % 9 == 0), ttl=61, sport=sport, dport=dport,
                            chk=chk), mac, bool(k & 2))
    if kind == "arp_req":
        return join(peer) + bytes([0x5A]) * (18 * (k & 1))
    if kind == "arp_other":
        if k & 1:
            return AR.arp(2, ip, LOCAL, sha=mac, tha=LOCAL_MAC, eth_src=mac, eth_dst=LOCAL_MAC, pad=k % 19)
        return AR.arp(1, ip, OTHER_HOST, sha=mac, tha=bytes(6), eth_src=mac, eth_dst=AR.BCAST_MAC, pad=k % 19)
    if kind == "arp_bad":
        full = AR.arp(1, ip, LOCAL, sha=mac, eth_src=mac, hlen=6 + (k % 3 == 1), plen=4 + (k % 3 == 2))
        return full[:41] if k % 3 == 0 else full
    if kind == "bad_ip":
        f = bytearray(eth(I.ip_packet(1, I.icmp(8, 0, rest, data), src=ip, dst=LOCAL, ihl=5, flags_off=0, ident=k,
                                      ttl=61), mac))
        f[24] ^= 0x40
        return bytes(f)
    if kind == "runt":
        return (LOCAL_MAC + mac + b"\x08\x00")[:k % 14]
    assert kind == "not_ip"
    return LOCAL_MAC + mac + b"\x86\xdd" + data + bytes(40)


def session_frames(allow, prefix, count, seed):
    """The session's frames: peers 0 and 1 join at once, peers 2 and 3 a quarter and a half of the
    way in; every other frame is drawn among the peers that have joined."""
    rng = random.Random(41000 + seed)
    bcast = LOCAL | (ALL_ONES >> prefix)
    names = [k for k, w in KINDS for _ in range(w)]
    joins = {0: 0, 1: 1, count // 4: 2, count // 2: 3}
    out, joined = [], []
    for k in range(count):
        if k in joins:
            joined.append(PEERS[joins[k]])
            out.append(join(joined[-1]))
            continue
        kind = names[rng.getrandbits(16) % len(names)]
        peer = joined[rng.getrandbits(8) % len(joined)]
        if kind == "udp_assoc" and PEERS[1] not in joined:
            kind = "udp_lis"
        out.append(frame(rng, kind, k, peer, bcast))
    return out


def build_generator(reference):
    os.makedirs(os.path.dirname(GEN_BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(reference, "src"), "-o", GEN_BIN,
                    GEN_SRC], check=True)
    return GEN_BIN


def generate(reference):
    """The fixture's text, from the reference's code run on the sessions above."""
    gen = build_generator(reference)
    req, plan = [], []
    for allow, prefix, count, seed in SESSIONS:
        frames = session_frames(allow, prefix, count, seed)
        plan.append((allow, prefix, seed, frames))
        req.append("S %d %d %d %s" % (allow, LOCAL, prefix, LOCAL_MAC.hex()))
        req += ["L %d %d %d %d" % tuple(l) for l in LISTENERS]
        req += ["A %d %d %d %d %d" % tuple(a) for a in ASSOCS]
        req += ["F " + (f.hex() or "-") for f in frames]
    ans = subprocess.run([gen], input="\n".join(req) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert ans[-1] == ""
    at, sessions = 0, []
    for allow, prefix, seed, frames in plan:
        rows = []
        for f in frames:
            sent, calls = [], []
            while ans[at] != ".":
                assert ans[at][:2] in ("T ", "C ")
                (sent if ans[at][0] == "T" else calls).append(ans[at][2:])
                at += 1
            at += 1
            rows.append([f.hex(), sent, calls])
        sessions.append({"allow": allow, "addr": LOCAL, "prefix": prefix, "mac": LOCAL_MAC.hex(), "seed": seed,
                         "listeners": LISTENERS, "assocs": ASSOCS, "frames": rows})
    assert at == len(ans) - 1
    return json.dumps({"sessions": sessions}, indent=0, separators=(",", ":")) + "\n"


def load():
    with open(FIXTURE) as f:
        return json.load(f)["sessions"]


if __name__ == "__main__":
    text = generate(sys.argv[1])
    with open(FIXTURE, "w") as f:
        f.write(text)
    print("%s: %d bytes" % (FIXTURE, len(text)))
