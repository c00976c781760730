"""TEST INFRASTRUCTURE -- shared by test_udprx_host.py and test_gpu_udprx.py: the model of the UDP
Rx demux, the tables and the frame builders.

The model is a plain Python restatement, written independently of the kernel, of what the
reference does with a UDP datagram that passed its checks (udp/IpUdpProto.h:470-621):
  1. the ports, the truncation to the UDP length (:480-492), dst_is_iface_addr (:504);
  2. the association lookup and its accept_nonlocal_dst rule (:527-537);
  3. incomingPacketMatches for every listener, in list order (:255-289);
  4. the port unreachable of a datagram for the interface's address that nobody took (:611-619).
All four are pinned against the reference's own stack by tests/golden/udp_rx_ref_cases.json
(test_udprx_host.py); the verdicts rest on the frame oracle.
"""
import struct

import numpy as np

import frame_cases as F
import icmp_cases as IC
import udp_rx_ref as R

ACCEPT, ACCEPT_NO_CHKSUM = 6, 7
NO_ASSOC = 0xFFFFFFFF
ASSOC_NONLOCAL = 0x80000000
LIS_BROADCAST, LIS_NONLOCAL = 1, 2
VALID, HAS_CHKSUM, DST_LOCAL, DST_BCAST = 0x80, 1, 2, 4
NO_UNREACH, PORT_UNREACH = 0xFF, 3
NO_FRAME = 0xFFFFFFFFFFFFFFFF

LOCAL, BCAST, PEER = R.LOCAL, R.BCAST, R.PEER
eth = IC.eth
iface = IC.iface


# ---- the tables ---------------------------------------------------------------------------------

def listeners(rows, dtype, *, dirty=False):
    """[(iface_addr, port, accept_broadcast, accept_nonlocal_dst, cookie)] in list order -> the
    device table. `dirty`: every bit the contract calls undefined is set."""
    t = np.zeros(len(rows), dtype=dtype)
    for k, (addr, port, bc, nl, cookie) in enumerate(rows):
        t[k] = (addr, port, (LIS_BROADCAST if bc else 0) | (LIS_NONLOCAL if nl else 0), 0, cookie, 0)
    if dirty:
        t["flags"] |= 0xFC
        t["reserved0"] = 0xA5
        t["reserved1"] = 0xDEADBEEF
    return t


def assocs(rows, dtype):
    """[(local_addr, remote_addr, local_port, remote_port, accept_nonlocal_dst, handle)] -> the
    table in the order of CompareKeys (remote_port, remote_addr, local_port, local_addr)."""
    rows = sorted(rows, key=lambda r: (r[3], r[1], r[2], r[0]))
    t = np.zeros(len(rows), dtype=dtype)
    for k, (la, ra, lp, rp, nl, handle) in enumerate(rows):
        t[k] = (la, ra, lp, rp, handle | (ASSOC_NONLOCAL if nl else 0))
    return t


# ---- the model ----------------------------------------------------------------------------------

def listener_matches(lis, dport, is_bcast, dst_local, ifc):
    """incomingPacketMatches (:262-288) of one table entry (a listener of this interface)."""
    if lis["port"] != 0 and dport != lis["port"]:
        return False
    if not lis["flags"] & LIS_BROADCAST and is_bcast:
        return False
    if not lis["flags"] & LIS_NONLOCAL and not is_bcast and not dst_local:
        return False
    if lis["iface_addr"] != 0 and lis["iface_addr"] != ifc["local"]:
        return False
    return True


def model_frame(frame, verdict, ifc, lookup, lis):
    """(record as a dict or None, unreach code, delivered) of one frame with Rx verify's verdict;
    lookup: {(local_addr, remote_addr, local_port, remote_port): cookie}."""
    if verdict not in (ACCEPT, ACCEPT_NO_CHKSUM) or frame[23] != 17:
        return None, NO_UNREACH, False
    hl = (frame[14] & 0xF) * 4
    T = 14 + hl
    sport, dport, udp_len, field = struct.unpack_from(">HHHH", frame, T)
    src, dst = struct.unpack_from(">II", frame, 26)
    dst_local = dst == ifc["local"]
    is_bcast = dst == 0xFFFFFFFF or dst == ifc["bcast"]
    cookie = lookup.get((dst, src, dport, sport))
    assoc = NO_ASSOC
    if cookie is not None and (cookie & ASSOC_NONLOCAL or dst_local):
        assoc = cookie & 0x7FFFFFFF
    mask = 0
    for k in range(len(lis)):
        if listener_matches(lis[k], dport, is_bcast, dst_local, ifc):
            mask |= 1 << k
    rec = dict(remote_addr=src, local_addr=dst, remote_port=sport, local_port=dport, data_off=T + 8,
               data_len=udp_len - 8, listeners=mask, assoc=assoc,
               flags=VALID | (HAS_CHKSUM if field else 0) | (DST_LOCAL if dst_local else 0) |
               (DST_BCAST if is_bcast else 0), ttl=frame[22], reserved=0)
    deliver = assoc != NO_ASSOC or mask != 0
    return rec, (PORT_UNREACH if dst_local and not deliver else NO_UNREACH), deliver


class Expected:
    """verdict (uint8), dgrams (dgram dtype), unreach (uint8), deliver_frame (uint64, n), counts
    (uint64, 2)."""


def expected(frames, verdicts, ifc, assoc_table, lis_table, dgram_dtype):
    """What udp_rx_demux must leave for `frames` (list of bytes) with Rx verify's `verdicts`."""
    lookup = {}
    if assoc_table is not None:
        for a in assoc_table:
            lookup[(int(a["local_addr"]), int(a["remote_addr"]), int(a["local_port"]),
                    int(a["remote_port"]))] = int(a["cookie"])
    lis = [] if lis_table is None else [dict(port=int(l["port"]), flags=int(l["flags"]),
                                             iface_addr=int(l["iface_addr"])) for l in lis_table]
    n = len(frames)
    e = Expected()
    e.verdict = np.array(verdicts, dtype=np.uint8).copy()
    e.dgrams = np.zeros(n, dtype=dgram_dtype)
    e.unreach = np.full(n, NO_UNREACH, dtype=np.uint8)
    e.deliver_frame = np.full(n, NO_FRAME, dtype=np.uint64)
    j = u = 0
    for i, f in enumerate(frames):
        rec, code, deliver = model_frame(f, int(verdicts[i]), ifc, lookup, lis)
        if rec is not None:
            for k, val in rec.items():
                e.dgrams[k][i] = val
        e.unreach[i] = code
        u += code != NO_UNREACH
        if deliver:
            e.deliver_frame[j] = i
            j += 1
    e.counts = np.array([j, u], dtype=np.uint64)
    return e


# ---- a stack of the fixture ---------------------------------------------------------------------

def stack_iface(stack):
    return iface(local=stack["addr"], bcast=stack["addr"] | (0xFFFFFFFF >> stack["prefix"]))


def stack_tables(stack, key_dtype, lis_dtype):
    """(association table, listener table) of a fixture stack: handles and cookies are the
    creation numbers; the listeners in the order the reference walks them."""
    a = assocs([tuple(r) + (k,) for k, r in enumerate(stack["assocs"])], key_dtype)
    l = listeners([tuple(r) + (k,) for k, r in R.listener_table(stack)], lis_dtype)
    return a, l


def stack_frames(stack):
    return [eth(bytes.fromhex(c["in"])) for c in stack["cases"]]


def calls_of(e, i, frame, lis_table):
    """The handler calls the record of frame i stands for, as the fixture writes them: the
    association first, then the listeners in table order."""
    r = e.dgrams[i]
    if not r["flags"] & VALID:
        return []
    data = frame[int(r["data_off"]):int(r["data_off"]) + int(r["data_len"])]
    tail = " %d %016x %d" % (len(data), R.fnv1a(data), 1 if r["flags"] & HAS_CHKSUM else 0)
    out = []
    if r["assoc"] != NO_ASSOC:
        out.append("A%d" % int(r["assoc"]) + tail)
    for k in range(len(lis_table)):
        if (int(r["listeners"]) >> k) & 1:
            out.append("L%d" % int(lis_table["cookie"][k]) + tail)
    return out


# ---- frame sets beyond the fixture --------------------------------------------------------------

def dgram(dport, *, dst=LOCAL, src=PEER, sport=R.SPORT, n=3, pad60=False, **kw):
    return eth(R.packet(R.pattern(n, dport & 0xFF), src=src, dst=dst, sport=sport, dport=dport, **kw),
               pad60=pad60)


def bit_listeners(dtype, count=64, *, dirty=False):
    """`count` listeners, entry k on port 7000 + k: a datagram to that port sets bit k alone."""
    return listeners([(0, 7000 + k, 0, 0, 100 + k) for k in range(count)], dtype, dirty=dirty)


def bit_frames(count=64):
    """One datagram per listener of bit_listeners, and some to ports nobody listens on."""
    out = [dgram(7000 + k, n=k % 9) for k in range(count)]
    out += [dgram(6999), dgram(7000 + count), dgram(7031, dst=R.NONLOCAL), dgram(7063, dst=BCAST)]
    return out


def many_assocs(dtype, count):
    """`count` associations of distinct peers; every third accepts a non-local destination and is
    bound to one (R.NONLOCAL)."""
    return assocs([(R.NONLOCAL if j % 3 == 2 else LOCAL, PEER + 1 + j, 6000 + j % 7, 30000 + j % 11,
                    j % 3 == 2, j) for j in range(count)], dtype)


def assoc_frames(count, step=1):
    """A datagram for association j of many_assocs (every `step`-th), one that differs from it in
    the remote port, and for the non-local ones one to another non-local destination."""
    out = []
    for j in range(0, count, step):
        dst = R.NONLOCAL if j % 3 == 2 else LOCAL
        out.append(dgram(6000 + j % 7, dst=dst, src=PEER + 1 + j, sport=30000 + j % 11))
        out.append(dgram(6000 + j % 7, dst=dst, src=PEER + 1 + j, sport=30011))
    return out


def flood(n, *, open_port=None, seed=1):
    """n datagrams for the interface's address: to `open_port`, or each to another closed port."""
    return [dgram(open_port if open_port is not None else 20000 + (i * 7 + seed) % 30000, n=i % 23,
                  ihl=5 + (i % 11 == 0) * (i % 10), chk=("good", "zero")[i % 5 == 0],
                  pad60=bool(i & 1)) for i in range(n)]


def mixed(n, seed=20261020):
    """frame_cases.frames (TCP, UDP, ICMP, bad checksums, non-IP) with fixture-style datagrams to
    open and closed ports of the interface at every fifth index."""
    fr = F.frames(seed=seed, n=n)
    for i in range(0, n, 5):
        fr[i] = dgram(5000 if i % 10 else 7, n=i % 17)
    return fr


def without_udp(n, seed=20261021):
    """frame_cases.frames with every IPv4 UDP frame replaced by an ARP frame."""
    fr = F.frames(seed=seed, n=n)
    for i, f in enumerate(fr):
        if len(f) >= 34 and f[12:14] == b"\x08\x00" and f[23] == 17:
            fr[i] = F.LOCAL_MAC + F.peer_mac(1) + b"\x08\x06" + bytes(46)
    return fr
