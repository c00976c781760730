"""TEST INFRASTRUCTURE -- shared by test_tx_resolve_host.py, test_gpu_tx_resolve.py and
test_gpu_large_span_tx_resolve.py: the model of Tx resolve, the table keeper that plays the host
over the fixture's command sequences, and the batch builders.

The model is a plain Python restatement of what the reference does between "an IPv4 header is
ready" and "the frame is handed to the driver":
  1. routeIp4 / routeIp4ForceIface (ip/IpStack.h:713-780);
  2. checkSendIp4Allowed (:666-690);
  3. resolve_hw_addr with get_arp_entry(weak=false) (eth/EthIpIface.h:511-585, :635-698);
  4. the Ethernet header (:420-430).
All four are pinned against the reference's own IpStack and EthIpIface by
tests/golden/tx_resolve_ref_cases.json (test_tx_resolve_host.py).
"""
import struct

import numpy as np

import arp_cases as AC
import tx_resolve_ref as R

NONE, SENT, NO_ROUTE, BCAST_REJECTED, NONLOCAL_SRC, NO_HW_ROUTE, ARP_QUERY = range(41, 48)
FAILED = (NO_ROUTE, BCAST_REJECTED, NONLOCAL_SRC, NO_HW_ROUTE)
ALLOW_BROADCAST, ALLOW_NONLOCAL_SRC = 1, 2
ROUTE_ANY, NO_ENTRY, NO_SEG = 0xFFFF, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
GATEWAY, BROADCAST, NEW_ENTRY, FORCED = 1, 2, 4, 8
QUERY, VALID, REFRESHING = 1, 2, 3
ALL_ONES = 0xFFFFFFFF
BURST_INVALID, DGRAM_INVALID = 10, 13
# IpErr of the reference (infra/Err.h) for each status
IP_ERR = {SENT: 0, ARP_QUERY: 1, NO_HW_ROUTE: 4, NO_ROUTE: 5, BCAST_REJECTED: 13, NONLOCAL_SRC: 14}

IFACE = np.dtype({"names": ["addr", "netmask", "gateway", "prefix", "flags", "mac", "reserved"],
                  "formats": ["<u4", "<u4", "<u4", "u1", "u1", ("u1", (6,)), ("u1", (12,))],
                  "offsets": [0, 4, 8, 12, 13, 14, 20], "itemsize": 32})
ENTRY = np.dtype({"names": ["addr", "iface", "state", "mac", "reserved"],
                  "formats": ["<u4", "<u2", "u1", ("u1", (6,)), ("u1", (3,))],
                  "offsets": [0, 4, 6, 7, 13], "itemsize": 16})
ROUTE = np.dtype({"names": ["next_hop", "arp_index", "iface", "status", "flags", "reserved"],
                  "formats": ["<u4", "<u4", "<u2", "u1", "u1", "<u4"],
                  "offsets": [0, 4, 8, 10, 11, 12], "itemsize": 16})


# ---- the interfaces ------------------------------------------------------------------------------

def iface(addr=None, prefix=0, gateway=None, mac=R.mac_of(0)):
    """One interface of the model: what IpIface holds."""
    mask = R.netmask(prefix) if addr is not None else 0
    return dict(have=addr is not None, addr=addr or 0, prefix=prefix if addr is not None else 0,
                netmask=mask, have_gw=gateway is not None, gateway=gateway or 0, mac=bytes(mac))


def stack_ifaces(stack):
    """The fixture stack's interfaces in the order the stack's list iterates them: the reverse
    of their construction (ip/IpIface.h:97). Table index t is constructed interface n - 1 - t."""
    return [iface(f["addr"] if f["have"] else None, f["prefix"], f["gateway"] if f["have_gw"] else None,
                  bytes.fromhex(f["mac"])) for f in reversed(stack["ifaces"])]


def iface_table(ifaces):
    t = np.zeros(len(ifaces), dtype=IFACE)
    for k, f in enumerate(ifaces):
        t[k] = (f["addr"], f["netmask"], f["gateway"], f["prefix"], int(f["have"]) | 2 * int(f["have_gw"]),
                np.frombuffer(f["mac"], dtype=np.uint8), np.zeros(12, dtype=np.uint8))
    return t


def is_local(f, a):
    return f["have"] and (a & f["netmask"]) == (f["addr"] & f["netmask"])


def bcast_of(f):
    return (f["addr"] & f["netmask"]) | (~f["netmask"] & ALL_ONES)


# ---- the decision --------------------------------------------------------------------------------

def decide(src, dst, send_flags, force, ifaces, lookup):
    """(status, next_hop, arp_index, iface, route flags, the 14 header bytes or None, the entry
    used or None). lookup(iface, addr) -> (index, state, mac) or None."""
    flags, hop, k, f = 0, 0, force, None
    if force == ROUTE_ANY:
        best = -1
        for q, g in enumerate(ifaces):
            if is_local(g, dst):
                if g["prefix"] > best:
                    best, f, k = g["prefix"], g, q
            elif g["have_gw"] and f is None:
                f, k = g, q
        if f is not None:
            hop = dst if best >= 0 else f["gateway"]
            flags |= 0 if best >= 0 else GATEWAY
    else:
        flags |= FORCED
        if force < len(ifaces):
            g = ifaces[force]
            if dst == ALL_ONES or is_local(g, dst):
                f, hop = g, dst
            elif g["have_gw"]:
                f, hop = g, g["gateway"]
                flags |= GATEWAY
    if f is None:
        return NO_ROUTE, 0, NO_ENTRY, k & 0xFFFF, flags, None, None
    if not send_flags & ALLOW_BROADCAST and (dst == ALL_ONES or (f["have"] and dst == bcast_of(f))):
        return BCAST_REJECTED, hop, NO_ENTRY, k, flags, None, None
    if not send_flags & ALLOW_NONLOCAL_SRC and (not f["have"] or src != f["addr"]):
        return NONLOCAL_SRC, hop, NO_ENTRY, k, flags, None, None
    found = lookup(k, hop)
    mac, used, index = b"\xff" * 6, None, NO_ENTRY
    if found is not None:
        index, state, emac = found
        if state >= VALID:
            status, mac, used = SENT, emac, index
        else:
            status = ARP_QUERY
    elif hop == ALL_ONES:
        status, flags = SENT, flags | BROADCAST
    elif hop == 0 or not f["have"] or (hop & f["netmask"]) != (f["addr"] & f["netmask"]):
        status = NO_HW_ROUTE
    elif hop == bcast_of(f):
        status, flags = SENT, flags | BROADCAST
    else:
        status, flags = ARP_QUERY, flags | NEW_ENTRY
    header = mac + f["mac"] + b"\x08\x00" if status == SENT else None
    return status, hop, index, k, flags, header, used


def table_lookup(table):
    """lookup() over an ENTRY array with unique keys (sorted or not: the model does not search)."""
    by = {(int(e["iface"]), int(e["addr"])): (j, int(e["state"]), e["mac"].tobytes())
          for j, e in enumerate(table)}
    return lambda k, a: by.get((k, a))


class Expected:
    """status (uint8), routes (ROUTE), send_len (uint32), arp_used (uint8), held / failed (uint64,
    n), counts (uint64, 2), ring (uint8: the header ring after the call)."""


def expected(ring, stride, hdr_len, ifaces, table, *, seg_status=None, send_flags=None, force=None):
    """What tx_resolve must leave for the n slots of `ring` (uint8 array; slot i at i * stride)."""
    n = len(hdr_len)
    e = Expected()
    e.status = np.full(n, NONE, dtype=np.uint8)
    e.routes = np.zeros(n, dtype=ROUTE)
    e.send_len = np.zeros(n, dtype=np.uint32)
    e.arp_used = np.zeros(len(table), dtype=np.uint8)
    e.held = np.full(n, NO_SEG, dtype=np.uint64)
    e.failed = np.full(n, NO_SEG, dtype=np.uint64)
    e.ring = ring.copy()
    lookup = table_lookup(table)
    cache = {}
    h = f = 0
    for i in range(n):
        ln = int(hdr_len[i])
        at = i * stride
        ss = int(seg_status[i]) if seg_status is not None else 0
        if ln < 34 or ln > stride or ss in (BURST_INVALID, DGRAM_INVALID) or \
                ring[at + 12] != 8 or ring[at + 13] != 0:
            e.send_len[i] = ln
            continue
        src, dst = struct.unpack_from(">II", ring, at + 26)
        key = (src, dst, int(send_flags[i]) if send_flags is not None else 0,
               int(force[i]) if force is not None else ROUTE_ANY)
        if key not in cache:
            cache[key] = decide(*key, ifaces, lookup)
        st, hop, index, k, flags, header, used = cache[key]
        e.status[i] = st
        e.routes[i] = (hop, index, k, st, flags, 0)
        if st == SENT:
            e.send_len[i] = ln
            e.ring[at:at + 14] = np.frombuffer(header, dtype=np.uint8)
            if used is not None:
                e.arp_used[used] = 1
        elif st == ARP_QUERY:
            e.held[h] = i
            h += 1
        else:
            e.failed[f] = i
            f += 1
    e.counts = np.array([h, f], dtype=np.uint64)
    return e


# ---- the host's table keeper ---------------------------------------------------------------------

class Keeper:
    """The ARP tables of a stack as the host keeps them between batches (one dict per stack,
    keyed by (interface in table order, address)): starts empty, gains a Query entry where a
    datagram was held without one, makes an entry Valid on a learned ARP sender."""

    def __init__(self, ifaces):
        self.ifaces, self.entries = ifaces, {}

    def table(self):
        t = np.zeros(len(self.entries), dtype=ENTRY)
        for j, ((k, a), (state, mac)) in enumerate(sorted(self.entries.items())):
            t[j] = (a, k, state, np.frombuffer(mac, dtype=np.uint8), np.zeros(3, dtype=np.uint8))
        return t

    def held(self, k, hop, flags):
        """A datagram left as _ARP_QUERY: with _NEW_ENTRY the host makes the entry and
        broadcasts the first request. Returns whether a request leaves."""
        if flags & NEW_ENTRY:
            assert (k, hop) not in self.entries
            self.entries[(k, hop)] = (QUERY, bytes(6))
            return True
        assert self.entries[(k, hop)][0] == QUERY
        return False

    def arp_iface(self, k):
        """Interface k as arp_cases takes it."""
        f = self.ifaces[k]
        return dict(local=f["addr"], netmask=f["netmask"], have=f["have"], mac=f["mac"])

    def learned(self, k, rec):
        """save_hw_addr for one aipstack_arp_record of interface k, rec = (status, sender
        address, sender MAC, flags): wherever the record comes from, the model or the device."""
        st, ip, mac, flags = rec
        if st in (AC.SEEN, AC.REPLY) and flags & AC.LEARN and \
                ((k, ip) in self.entries or flags & AC.NEW_OK):
            self.entries[(k, ip)] = (VALID, bytes(mac))

    def heard(self, k, frame):
        """An ARP frame arrived on interface k: the model's record (arp_cases.record), then
        what the host does with it."""
        st, ip, mac, op, flags = AC.record(frame, self.arp_iface(k))
        self.learned(k, (st, ip, mac, flags))


# ---- header slots --------------------------------------------------------------------------------

def header(src, dst, *, length=54, eth=b"\xee" * 12, ethertype=b"\x08\x00", fill=0xA5):
    """A header slot's first `length` bytes: a stale Ethernet header, an IPv4 header with the
    addresses, then filler."""
    ip4 = struct.pack(">BBHHHBBHII", 0x45, 0, max(length - 14, 20), 7, 0, 64, 6, 0, src, dst)
    return (eth + ethertype + ip4 + bytes([fill]) * 64)[:length]


def ring_of(headers, stride, *, slack=0xC3):
    """(ring, hdr_len): each header at the start of its slot, the slot's slack filled."""
    ring = np.full(len(headers) * stride, slack, dtype=np.uint8)
    for i, h in enumerate(headers):
        ring[i * stride:i * stride + min(len(h), stride)] = np.frombuffer(h[:stride], dtype=np.uint8)
    return ring, np.array([len(h) for h in headers], dtype=np.uint32)


LAN = [iface(R.ip(10, 20, 30, 40), 24, R.ip(10, 20, 30, 1), R.mac_of(0))]
PEER_SENT, PEER_QUERY, PEER_NEW = R.ip(10, 20, 30, 100), R.ip(10, 20, 30, 101), R.ip(10, 20, 30, 102)


def lan_table(extra=0):
    """A sorted table for LAN: PEER_SENT Valid, PEER_QUERY in Query state, the gateway Refreshing,
    and `extra` further Valid entries around them."""
    t = np.zeros(3 + extra, dtype=ENTRY)
    t[0] = (PEER_SENT, 0, VALID, np.frombuffer(R.peer_mac(PEER_SENT), dtype=np.uint8), np.zeros(3, np.uint8))
    t[1] = (PEER_QUERY, 0, QUERY, np.zeros(6, np.uint8), np.zeros(3, np.uint8))
    t[2] = (R.ip(10, 20, 30, 1), 0, REFRESHING, np.frombuffer(R.peer_mac(1), dtype=np.uint8), np.zeros(3, np.uint8))
    for j in range(extra):
        a = R.ip(10, 20 + j % 3, 30 + j // 200 % 50, 110 + j % 100) + (j // 10000 << 16)
        t[3 + j] = (a, j % 2, VALID, np.frombuffer(R.peer_mac(a), dtype=np.uint8), np.zeros(3, np.uint8))
    order = np.lexsort((t["addr"], t["iface"]))
    t = t[order]
    keys = list(zip(t["iface"].tolist(), t["addr"].tolist()))
    assert len(set(keys)) == len(keys)
    return t


PLACES = (0, 63, 64, 255)


def placed_batch(n, kind="sent"):
    """n slots over LAN with a segment of `kind` ("sent", "query" or "error") at lanes 0, 63, 64,
    255 and the last index (as far as n goes); every other slot rotates through the other
    outcomes, nothing-to-resolve slots included."""
    own = LAN[0]["addr"]
    places = {i for i in PLACES + (n - 1,) if 0 <= i < n}
    others = [k for k in ("sent", "query", "error", "none", "new", "gateway") if k != kind]
    out = []
    for i in range(n):
        k = kind if i in places else others[i % len(others)]
        if k == "sent":
            out.append(header(own, PEER_SENT, length=34 + i % 31))
        elif k == "query":
            out.append(header(own, PEER_QUERY))
        elif k == "new":
            out.append(header(own, PEER_NEW))
        elif k == "error":
            out.append(header((own, own + 1, own, own)[i % 4],
                              (ALL_ONES, PEER_SENT, R.ip(10, 20, 30, 255), ALL_ONES)[i % 4]))
        elif k == "none":
            out.append((header(own, PEER_SENT)[:33], b"", header(own, PEER_SENT, ethertype=b"\x08\x06"),
                        header(own, PEER_SENT, ethertype=b"\x00\x08"))[i % 4])
        else:
            out.append(header(own, R.OUTSIDE + i % 5))
    return out


def random_case(seed, n, *, n_ifaces=4, n_arp=300):
    """(ifaces, table, headers, send_flags, force, seg_status): seeded random interfaces with
    overlapping subnets, a table over them, and segments whose addresses hit subnets, broadcast
    addresses, entries in every state, near misses and far addresses."""
    rng = np.random.default_rng(seed)
    ifaces = []
    for k in range(n_ifaces):
        kind = int(rng.integers(0, 6))
        prefix = int(rng.choice([8, 16, 24, 24, 28, 30]))
        addr = (R.ip(10, 20, int(rng.integers(30, 33)), int(rng.integers(1, 250))) if kind else None)
        gw = R.ip(10, 20, 30, int(rng.integers(1, 250))) if kind in (0, 2, 3) else None
        ifaces.append(iface(addr, prefix, gw, R.mac_of(k)))
    pool = sorted({R.ip(10, 20, int(rng.integers(29, 34)), int(rng.integers(0, 256))) for _ in range(n_arp)} |
                  {f["gateway"] for f in ifaces if f["have_gw"]})
    entries = {}
    for a in pool:
        k = int(rng.integers(0, n_ifaces))
        entries[(k, a)] = int(rng.choice([QUERY, VALID, VALID, REFRESHING]))
    table = np.zeros(len(entries), dtype=ENTRY)
    for j, ((k, a), state) in enumerate(sorted(entries.items())):
        table[j] = (a, k, state, np.frombuffer(R.peer_mac(a, k), dtype=np.uint8), np.zeros(3, np.uint8))
    addrs = [f["addr"] for f in ifaces if f["have"]] or [R.ip(10, 20, 30, 40)]
    special = [ALL_ONES, 0, R.OUTSIDE, R.MULTICAST] + [bcast_of(f) for f in ifaces if f["have"]] + \
        [f["addr"] & f["netmask"] for f in ifaces if f["have"]]
    headers = []
    for i in range(n):
        r = int(rng.integers(0, 20))
        dst = (pool[int(rng.integers(0, len(pool)))] if r < 11 else
               special[int(rng.integers(0, len(special)))] if r < 15 else
               R.ip(10, 20, int(rng.integers(29, 34)), int(rng.integers(0, 256))))
        src = addrs[int(rng.integers(0, len(addrs)))] if r % 5 else R.OUTSIDE
        length = int(rng.choice([34, 42, 54, 54, 54, 64, 33, 0, 20]))
        et = b"\x08\x00" if rng.integers(0, 16) else b"\x08\x06"
        headers.append(header(src, dst, length=length, ethertype=et, eth=bytes(rng.integers(0, 256, 12, dtype=np.uint8))))
    send_flags = rng.choice(np.array([0, 0, 0, 1, 2, 3, 0x80, 0xFF], dtype=np.uint8), n)
    force = rng.choice(np.array([ROUTE_ANY] * 5 + list(range(n_ifaces)) + [n_ifaces, 0xFFFE], dtype=np.uint16), n)
    seg_status = rng.choice(np.array([0, 0, 0, 0, 9, 10, 13, 17], dtype=np.uint8), n)
    return ifaces, table, headers, send_flags, force, seg_status
