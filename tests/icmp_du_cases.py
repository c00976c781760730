"""TEST INFRASTRUCTURE -- shared by test_icmp_du_host.py and the GPU tests of icmp_rx_unreach: the
model of what the call leaves, and the frame builders.

The model is a plain Python restatement of what the reference does with a received ICMP
Destination Unreachable up to and including the TCP handler's find_pcb:
  1. the source and destination tests of recvIcmp4Dgram (ip/IpStack.h:1093-1148);
  2. the parse of the quoted IPv4 header in handleIcmp4DestUnreach (:1192-1249);
  3. the code, length and key of IpTcpProto's handleIp4DestUnreach (tcp/IpTcpProto_input.h:154-182).
1 and 2 are pinned against the reference's own stack by tests/golden/icmp_du_ref_cases.json
(test_icmp_du_host.py); 3 is four lines, checked by reading them, over a table whose key order
tests/cpp/tcprx_table_test.cpp pins.
"""
import numpy as np

import frame_cases as F
import icmp_du_ref as R

NONE, PARSED, TCP_NO_PCB, TCP_PCB = 37, 38, 39, 40
NO_PCB = 0xFFFFFFFF
NO_FRAME = 0xFFFFFFFFFFFFFFFF
ALL_ONES = 0xFFFFFFFF

RECORD = np.dtype({"names": ["local_addr", "remote_addr", "local_port", "remote_port", "seq", "rest", "pcb",
                             "ip_off", "l4_len", "code", "proto", "ttl", "hl"],
                   "formats": ["<u4", "<u4", "<u2", "<u2", "<u4", "<u4", "<u4", "<u2", "<u2", "u1", "u1", "u1",
                               "u1"],
                   "offsets": [0, 4, 8, 10, 12, 16, 20, 24, 26, 28, 29, 30, 31], "itemsize": 32})
KEY = np.dtype({"names": ["local_addr", "remote_addr", "local_port", "remote_port", "cookie"],
                "formats": ["<u4", "<u4", "<u2", "<u2", "<u4"], "offsets": [0, 4, 8, 10, 12],
                "itemsize": 16})

LOCAL, PREFIX, PEER, GATEWAY = R.STACKS[0]


def iface(*, local=LOCAL, prefix=PREFIX, mac=R.LOCAL_MAC):
    mask = R.netmask(prefix)
    return dict(local=local, bcast=(local & mask) | (~mask & ALL_ONES), mac=bytes(mac))


def stack_iface(stack):
    return iface(local=stack["addr"], prefix=stack["prefix"], mac=bytes.fromhex(stack["mac"]))


def stack_frames(stack):
    return [bytes.fromhex(c["in"]) for c in stack["cases"]]


# ---- the model -----------------------------------------------------------------------------------

def be16(f, at):
    return int.from_bytes(f[at:at + 2], "big")


def be32(f, at):
    return int.from_bytes(f[at:at + 4], "big")


def record(f, verdict, ifc):
    """The record of frame `f` with Rx verify's `verdict` as a dict (pcb = NO_PCB), or None."""
    if verdict != 6 or len(f) < 42:                               # AIPSTACK_RX_ACCEPT
        return None
    hl, total = (f[14] & 0xF) * 4, be16(f, 16)
    if f[23] != 1 or be16(f, 20) & 0x3FFF:
        return None
    assert hl >= 20 and total >= hl + 8 and 14 + total <= len(f)  # what an accepted frame has
    src, dst = be32(f, 26), be32(f, 30)
    if src == ALL_ONES or (src & 0xF0000000) == 0xE0000000 or src == ifc["bcast"]:
        return None
    if dst not in (ifc["local"], ifc["bcast"], ALL_ONES):
        return None
    t = 14 + hl
    if f[t] != 3:
        return None
    data = f[t + 8:14 + total]                                    # Ethernet padding is not data
    if len(data) < 20 or data[0] >> 4 != 4:
        return None
    qhl, qtotal = (data[0] & 0xF) * 4, be16(data, 2)
    if qhl < 20 or qhl > len(data) or qtotal < qhl:
        return None
    l4_len = min(len(data), qtotal) - qhl
    l4 = data[qhl:qhl + l4_len]
    r = dict(local_addr=be32(data, 12), remote_addr=be32(data, 16), local_port=0, remote_port=0, seq=0,
             rest=be32(f, t + 4), pcb=NO_PCB, ip_off=t + 8, l4_len=l4_len, code=f[t + 1], proto=data[9],
             ttl=data[8], hl=qhl)
    if l4_len >= 8:
        r.update(local_port=be16(l4, 0), remote_port=be16(l4, 2), seq=be32(l4, 4))
    return r


def looks_up(r):
    """IpTcpProto's handler goes on to find_pcb (the stack calls it for protocol 6 only)."""
    return r["proto"] == 6 and r["code"] == 4 and r["l4_len"] >= 8


class Expected:
    """verdict (uint8), status (uint8), records (RECORD), pcb_frame (uint64, n), counts (uint64, 2)."""


def expected(frames, verdicts, ifc, pcbs=None):
    """What icmp_rx_unreach must leave for `frames` (list of bytes) whose Rx verify verdicts are
    `verdicts`, with the PCB table `pcbs` (a KEY array with unique keys, in any order, or None)."""
    n = len(frames)
    table = {}
    if pcbs is not None:
        for k in pcbs:
            table[(int(k["local_addr"]), int(k["remote_addr"]), int(k["local_port"]),
                   int(k["remote_port"]))] = int(k["cookie"])
        assert len(table) == len(pcbs)
    e = Expected()
    e.verdict = np.asarray(verdicts, dtype=np.uint8).copy()
    e.status = np.full(n, NONE, dtype=np.uint8)
    e.records = np.zeros(n, dtype=RECORD)
    e.pcb_frame = np.full(n, NO_FRAME, dtype=np.uint64)
    j = valid = 0
    for i, f in enumerate(frames):
        r = record(f, int(verdicts[i]), ifc)
        if r is None:
            continue
        valid += 1
        st = PARSED
        if looks_up(r):
            cookie = table.get((r["local_addr"], r["remote_addr"], r["local_port"], r["remote_port"]))
            st = TCP_NO_PCB if cookie is None else TCP_PCB
            if cookie is not None:
                r["pcb"] = cookie
                e.pcb_frame[j] = i
                j += 1
        e.status[i] = st
        e.records[i] = tuple(r[name] for name in RECORD.names)
    e.counts = np.array([j, valid], dtype=np.uint64)
    return e


def verdicts_of(oracle, frames):
    buf, off = F.pack(frames)
    return oracle.rx_verify_batch(buf, off)


# ---- the fixture's events ------------------------------------------------------------------------

def handler_calls(events):
    """[(handler, code, rest, src_addr, dst_addr, ttl, proto, header_len, dgram_initial)] of the
    handleIp4DestUnreach calls among a case's events."""
    out = []
    for e in events:
        p = e.split(" ")
        if p[0] == "D":
            out.append((int(p[1]), int(p[2]), int(p[3], 16), int(p[4]), int(p[5]), int(p[6]), int(p[7]),
                        int(p[8]), b"" if p[9] == "-" else bytes.fromhex(p[9])))
    return out


# ---- crafted frames beyond the fixture -----------------------------------------------------------

def frag_needed(key, *, mtu=1400, seq=0x01020304, l4=20, src=PEER, dst=LOCAL, **kw):
    """A frag-needed message about a segment of the connection `key` = (local_addr, remote_addr,
    local_port, remote_port), quoting `l4` bytes of its TCP header."""
    la, ra, lp, rp = key
    q = R.quoted(6, R.tcp_head(l4, sport=lp, dport=rp, seq=seq), src=la, dst=ra)
    return R.frame(q, src=src, dst=dst, code=4, rest=mtu, **kw)


def pcb_table(count, *, local=LOCAL):
    """`count` connections (unsorted; cookie = 1000 + index), a multiple of 8: entry i differs from
    entry i ^ 1 only in remote_port, from i ^ 2 only in local_port and from i ^ 4 only in
    remote_addr."""
    t = np.zeros(count, dtype=KEY)
    for i in range(count):
        g = i // 8
        t[i] = (local, 0xC0A80000 + 2 * g + (i >> 2 & 1), 5000 + 2 * (g % 3000) + (i >> 1 & 1),
                20000 + 2 * (g % 20000) + (i & 1), 1000 + i)
    return t


def key_of(t, i):
    return (int(t["local_addr"][i]), int(t["remote_addr"][i]), int(t["local_port"][i]),
            int(t["remote_port"][i]))


def near_miss(t, i, k):
    """A key that is not in the table and differs from entry i in one field."""
    la, ra, lp, rp = key_of(t, i)
    return ((la, ra, lp, rp ^ 0x4000), (la, ra, lp ^ 0x4000, rp), (la, ra ^ 0x01000000, lp, rp),
            (la ^ 0x00010000, ra, lp, rp))[k % 4]


def other_frames(k):
    """Frames that are no Destination Unreachable: the UDP, TCP, ARP and echo frames of the other
    case modules."""
    import tcp_rsp_cases as TC
    import udp_rx_cases as UC
    kinds = (lambda: TC.rst_due(k), lambda: TC.no_rst(k), lambda: TC.not_tcp(k),
             lambda: UC.dgram(5000 + k % 7, n=k % 19, pad60=bool(k & 1)),
             lambda: R.LOCAL_MAC + R.PEER_MAC + b"\x08\x00" + R.I.echo(R.I.pattern(k % 31, k)),
             lambda: R.TR.AR.arp(1, PEER, LOCAL))
    return kinds[k % len(kinds)]()


def random_unreach(rng, table):
    """A Destination Unreachable with random quoted fields: every code, protocol, header length
    and quoted length the parse distinguishes; every second one a well-formed frag-needed message
    about a TCP segment, of a connection of `table` now and then."""
    plain = bool(rng.integers(0, 2))
    code = 4 if plain else int(rng.choice([0, 1, 2, 3, 4, 5, 13]))
    proto = 6 if plain else int(rng.choice([6, 17, 1, 47]))
    ihl = int(rng.choice([5, 5, 6, 15] if plain else [5, 6, 15, 4]))
    n = int(rng.choice([8, 9, 20, 28] if plain else [0, 3, 7, 8, 9, 20, 28]))
    if len(table) and rng.integers(0, 2):
        i = int(rng.integers(0, len(table)))
        la, ra, lp, rp = key_of(table, i) if rng.integers(0, 3) else near_miss(table, i, int(rng.integers(0, 4)))
    else:
        la, ra = (int(x) for x in rng.integers(0, 1 << 32, 2))
        lp, rp = (int(x) for x in rng.integers(0, 1 << 16, 2))
    total = 1500 if plain else int(rng.choice([1500, 4 * ihl + n, 4 * ihl + max(n - 3, 0), 4 * ihl - 1, 40]))
    q = R.quoted(proto, R.tcp_head(n, sport=lp, dport=rp, seq=int(rng.integers(0, 1 << 32))), src=la, dst=ra,
                 ihl=ihl, total=total, version=4 if plain else int(rng.choice([4, 4, 4, 6])),
                 ttl=int(rng.integers(0, 256)), flags_off=int(rng.choice([0x4000, 0, 0x2000, 0x0007])))
    bcast = iface()["bcast"]
    return R.frame(q, src=int(rng.choice([PEER, PEER, PEER, 0xC0A80101, bcast, 0xE0000001, ALL_ONES])),
                   dst=int(rng.choice([LOCAL, LOCAL, LOCAL, bcast, ALL_ONES, LOCAL + 1])), code=code,
                   rest=int(rng.integers(0, 1 << 32)), ihl=int(rng.choice([5, 5, 6, 15])),
                   bad=not rng.integers(0, 12), pad=int(rng.choice([0, 0, 5])), pad60=bool(rng.integers(0, 2)))


def random_batch(seed, n, table):
    """n frames, one in four a Destination Unreachable with random quoted fields."""
    rng = np.random.default_rng(seed)
    return [random_unreach(rng, table) if rng.integers(0, 4) == 0 else other_frames(int(rng.integers(0, 1 << 20)))
            for _ in range(n)]


def sized_batch(n, table, hits):
    """n frames with a frag-needed message of a connection of `table` at every index of `hits`
    (inside n), a near miss behind each where there is room, and every third other frame a
    Destination Unreachable of another kind."""
    hits = sorted({i for i in hits if 0 <= i < n})
    out = []
    for k in range(n):
        if k in hits:
            out.append(frag_needed(key_of(table, (7 * k) % len(table)), mtu=576 + k % 900, seq=k))
        elif k - 1 in hits:
            out.append(frag_needed(near_miss(table, (7 * (k - 1)) % len(table), k)))
        elif k % 3 == 0:
            out.append(R.frame(R.quoted((6, 17, 1)[k // 3 % 3], R.tcp_head((8, 4, 28)[k % 3]), src=LOCAL),
                               src=PEER, dst=LOCAL, code=(4, 3, 1, 0)[k // 3 % 4], pad60=bool(k & 1)))
        else:
            out.append(other_frames(k))
    return out
