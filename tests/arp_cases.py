"""TEST INFRASTRUCTURE -- shared by test_arp_host.py, test_gpu_arp.py and
test_gpu_large_span_arp.py: the model of ARP on receive and the frame builders.

The model is a plain Python restatement, over the frame's bytes with struct, of what the
reference does with a received Ethernet frame that is not IPv4:
  1. EthIpIface::recvFrame (eth/EthIpIface.h:367-390) and recvArpPacket (:474-508);
  2. the address tests of save_hw_addr (:587-627) and get_arp_entry (:664-698);
  3. send_arp_packet (:774-803).
All three are pinned against the reference's own EthIpIface by tests/golden/arp_ref_cases.json
(test_arp_host.py).
"""
import struct

import numpy as np

import arp_ref as R

NONE, MALFORMED, SEEN, REPLY = 27, 28, 29, 30
LEARN, NEW_OK, NOTIFY, REC_REPLY = 1, 2, 4, 8
HEADER = 42
NO_FRAME = 0xFFFFFFFFFFFFFFFF
ALL_ONES = 0xFFFFFFFF

RECORD = np.dtype({"names": ["sender_addr", "sender_mac", "op", "flags", "status", "reserved"],
                   "formats": ["<u4", ("u1", (6,)), "<u2", "u1", "u1", "<u2"],
                   "offsets": [0, 4, 10, 12, 13, 14], "itemsize": 16})


def iface(*, local=R.STACKS[0][1], prefix=24, have=True, mac=R.LOCAL_MAC):
    return dict(local=local, netmask=R.netmask(prefix), have=bool(have), mac=bytes(mac))


def stack_iface(stack):
    return iface(local=stack["addr"], prefix=stack["prefix"], have=stack["have"],
                 mac=bytes.fromhex(stack["mac"]))


# ---- steps 1 and 2: the record -------------------------------------------------------------------

def new_ok(ip, ifc):
    """get_arp_entry would create an entry for `ip` (:675-698)."""
    if ip == ALL_ONES or ip == 0 or not ifc["have"]:
        return False
    netaddr = ifc["local"] & ifc["netmask"]
    bcast = netaddr | (~ifc["netmask"] & ALL_ONES)
    return (ip & ifc["netmask"]) == netaddr and ip != bcast


def record(frame, ifc):
    """(status, sender address, sender MAC, op, flags) of one frame."""
    if len(frame) < 14 or frame[12:14] != b"\x08\x06":
        return NONE, 0, bytes(6), 0, 0
    if len(frame) < 42:
        return MALFORMED, 0, bytes(6), 0, 0
    hwtype, ptype, hlen, plen, op = struct.unpack_from(">HHBBH", frame, 14)
    if (hwtype, ptype, hlen, plen) != (1, 0x0800, 6, 4):
        return MALFORMED, 0, bytes(6), 0, 0
    mac = frame[22:28]
    ip, = struct.unpack_from(">I", frame, 28)
    target, = struct.unpack_from(">I", frame, 38)
    flags = 0
    if mac != b"\xff" * 6:
        flags |= LEARN
    if new_ok(ip, ifc):
        flags |= NEW_OK
    if flags & LEARN and ip not in (ALL_ONES, 0):
        flags |= NOTIFY
    reply = op == 1 and ifc["have"] and target == ifc["local"]
    if reply:
        flags |= REC_REPLY
    return (REPLY if reply else SEEN), ip, mac, op, flags


# ---- step 3: the bytes ---------------------------------------------------------------------------

def reply_frame(ip, mac, ifc):
    """The 42 bytes of send_arp_packet(Reply, mac, ip)."""
    return (mac + ifc["mac"] + b"\x08\x06" + struct.pack(">HHBBH", 1, 0x0800, 6, 4, 2) + ifc["mac"] +
            struct.pack(">I", ifc["local"]) + mac + struct.pack(">I", ip))


class Expected:
    """status (uint8), records (RECORD array), hdr_len (uint32), headers ({frame: 42 bytes}),
    chunk_index (uint64, n + 1, zero), reply_frame / seen_frame (uint64, n), counts."""


def respond(frames, ifc):
    """What arp_rx_respond must leave for `frames` (list of bytes)."""
    n = len(frames)
    e = Expected()
    e.status = np.zeros(n, dtype=np.uint8)
    e.records = np.zeros(n, dtype=RECORD)
    e.hdr_len = np.zeros(n, dtype=np.uint32)
    e.chunk_index = np.zeros(n + 1, dtype=np.uint64)
    e.reply_frame = np.full(n, NO_FRAME, dtype=np.uint64)
    e.seen_frame = np.full(n, NO_FRAME, dtype=np.uint64)
    e.headers = {}
    cache = {}
    j = k = 0
    for i, f in enumerate(frames):
        key = f[:42]
        if key not in cache:
            cache[key] = record(f, ifc)
        st, ip, mac, op, flags = cache[key]
        e.status[i] = st
        e.records[i] = (ip, np.frombuffer(mac, dtype=np.uint8), op, flags, st, 0)
        if st in (SEEN, REPLY):
            e.seen_frame[k] = i
            k += 1
        if st == REPLY:
            e.hdr_len[i] = HEADER
            e.headers[i] = reply_frame(ip, mac, ifc)
            e.reply_frame[j] = i
            j += 1
    e.counts = np.array([j, k], dtype=np.uint64)
    return e


# ---- the fixture's events ------------------------------------------------------------------------

def sent(events):
    return [bytes.fromhex(e[2:]) for e in events if e.startswith("T ")]


def observed(events):
    return [(int(e.split()[1]), bytes.fromhex(e.split()[2])) for e in events if e.startswith("O ")]


def probe_outcome(events, ifc):
    """What the probe showed: ("learned", the MAC the echo reply left for), ("query", None) for a
    broadcast ARP request, ("none", None)."""
    frames = sent(events)
    if not frames:
        return "none", None
    assert len(frames) == 1
    f = frames[0]
    if f[12:14] == b"\x08\x00":
        assert f[6:12] == ifc["mac"] and f[23] == 1 and f[34] == 0          # an echo reply
        return "learned", f[:6]
    assert f[12:14] == b"\x08\x06" and f[:6] == b"\xff" * 6 and f[20:22] == b"\x00\x01"
    return "query", None


# ---- crafted frames beyond the fixture -----------------------------------------------------------

def stack_frames(stack):
    return [bytes.fromhex(c["in"]) for c in stack["cases"]]


def request(k, ifc, *, pad=18):
    """A request for the interface's address from sender k (MAC and address vary with k)."""
    sha = bytes([0x02, 0xAA, (k >> 16) & 0xFF, (k >> 8) & 0xFF, k & 0xFF, 0x01])
    peer = (ifc["local"] & ifc["netmask"]) | (1 + k % 200)
    return R.arp(1, peer, ifc["local"], sha=sha, eth_src=R.ETH_SRC, pad=pad)


def other(k, ifc):
    """Valid ARP that gets no reply: a reply packet, a request for another address."""
    peer = (ifc["local"] & ifc["netmask"]) | (1 + k % 200)
    if k & 1:
        return R.arp(2, peer, ifc["local"], tha=ifc["mac"], pad=k % 19)
    return R.arp(1, peer, ifc["local"] ^ 0x80, pad=k % 19)


def not_arp(k):
    """Frames that are not ARP at all, short ones included."""
    kinds = (R.LOCAL_MAC + R.ETH_SRC + b"\x08\x00" + R.I.echo(R.I.pattern(k % 23, k)),
             R.arp(1, 1, 2, ethertype=0x86DD), R.LOCAL_MAC + R.ETH_SRC[:k % 7], b"",
             R.arp(1, 1, 2, ethertype=0x0800)[:14 + k % 28])
    return kinds[k % len(kinds)]


def sized_batch(n, kind):
    """n frames: "all" reply, "none" replies (valid ARP, malformed ARP), "no_arp", or "mixed"
    with replies at lanes 0 and 63 of a wave, at a block's first and last frame, in a block where
    every frame replies (the third) and between blocks without one."""
    ifc = iface()
    if kind == "all":
        return [request(k, ifc, pad=k % 19) for k in range(n)]
    if kind == "none":
        return [other(k, ifc) if k % 3 else R.arp(1, 5, ifc["local"], hlen=6 + k % 2, plen=5 - k % 2)
                for k in range(n)]
    if kind == "no_arp":
        return [not_arp(k) for k in range(n)]
    places = {i for i in (0, 63, 64, 127, 255, 256, n - 1) if 0 <= i < n} | set(range(512, min(n, 768)))
    return [request(k, ifc) if k in places else (other(k, ifc), not_arp(k), R.arp(1, 5, 6)[:41])[k % 3]
            for k in range(n)]
