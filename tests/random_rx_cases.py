"""TEST INFRASTRUCTURE -- the seeded scenario generators of test_gpu_random_rx.py (the UDP Rx demux
and the ICMP responder). They need no GPU: test_random_rx_cases.py runs every one of them over the
full seed range with the CPU oracle, checks that the scenarios cover what they are meant to cover,
and runs the first seeds through the stand-alone builds of the shared C++ (udprx_common.h,
icmp_common.h).

One ``np.random.default_rng(base + seed)`` per scenario; every expectation comes from the models
of udp_rx_cases.py and icmp_cases.py and from the CPU oracle, none from the library under test. A
scenario never drops a frame after drawing it; what a generator does not draw is listed in its
docstring.
"""
import struct

import numpy as np

import aipstack_amd as A

import frame_cases as F
import icmp_cases as IC
import icmp_ref as IR
import random_tcp_cases as T
import udp_rx_cases as UC
import udp_rx_ref as UR

SEEDS = 40
MAX_ELEMENTS = T.MAX_ELEMENTS
KEY, LIS, DGRAM = A.TCP_PCB_KEY_DTYPE, A.UDP_LISTENER_DTYPE, A.UDP_RX_DGRAM_DTYPE
ALL_ONES = 0xFFFFFFFF
AUX_BLOCKS = (-1, 1, 2)
SPECIAL_PORTS = (0, 1, 0x00FF, 0x0100, 0xFF00, 65535)


def bswap16(x):
    return (x & 0xFF) << 8 | x >> 8


def bswap32(x):
    return struct.unpack("<I", struct.pack(">I", x))[0]


def _addresses(rng):
    """(local, prefix, broadcast, a unicast address of the subnet that is not the interface's).
    Six times in ten the local address is frame_cases.LOCAL_IP, so that the frames of
    frame_cases.frames are for the interface; else they are for a non-local address."""
    local = IR.LOCAL if rng.random() < 0.6 else int(rng.integers(0x01000000, 0xE0000000))
    prefix = int(rng.integers(8, 31))
    host = ALL_ONES >> prefix
    if local & host == host:
        local -= 1
    if local & host == 0:
        local += 1
    other = next(a for a in (local ^ 1, local ^ 2, local ^ 3) if a & host not in (0, host))
    return local, prefix, local | host, other


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _flags_off(rng):
    """Not a fragment (DF or nothing) but one time in twenty: MF, MF and an offset, an offset."""
    if rng.random() >= 0.05:
        return int(rng.choice([0, 0x4000]))
    return int(rng.choice([0x2000, 0x2000 | int(rng.integers(1, 100)), int(rng.integers(1, 0x2000))]))


def _finish(rng, pkt, peer, *, cut=True):
    """The Ethernet frame of an IP packet: padding to 60 bytes (three in ten), bytes beyond the
    IPv4 total length (one in ten), cut to fewer than 42 bytes (one in twenty-five)."""
    f = IC.eth(pkt, src_mac=F.peer_mac(peer % 4), pad60=rng.random() < 0.3)
    if rng.random() < 0.1:
        f += _bytes(rng, int(rng.integers(1, 18)))
    if cut and rng.random() < 0.04:
        f = f[:int(rng.integers(0, 42))]
    return f


# ---- UDP Rx demux -----------------------------------------------------------------------------

UDP_STRIDES = (2048, 2049, 1536, 0)          # 0: the smallest that holds the longest frame
KEY_FIELDS = ("local_addr", "remote_addr", "local_port", "remote_port")


def sort_key(k):
    """CompareKeys' order of a (local_addr, remote_addr, local_port, remote_port) tuple."""
    return (k[3], k[1], k[2], k[0])


def neighbours(k, field):
    """The keys that differ from k in `field` alone: +1, -1 and the byte-swapped value."""
    bits, swap = (32, bswap32) if field < 2 else (16, bswap16)
    out = []
    for v in ((k[field] + 1) % (1 << bits), (k[field] - 1) % (1 << bits), swap(k[field])):
        if v != k[field]:
            q = list(k)
            q[field] = v
            out.append(tuple(q))
    return out


class UdpScenario:
    """frames / verdicts (the oracle's Rx verify), ifc, assocs / listeners (device tables or None),
    e (udp_rx_cases.expected), slotted, lead, slot, dgram_shift, aux_blocks, dirty; pool: the
    tuples the frames draw from; edge: (first, last, below, above) keys or None."""


def _udp_frame(rng, tup, peer, *, clean=False):
    la, ra, lp, rp = tup
    ihl = 5 if clean or rng.random() < 0.6 else int(rng.integers(5, 16))
    extra = b"" if clean or rng.random() >= 0.15 else _bytes(rng, int(rng.integers(1, 21)))
    room = 1500 - 4 * ihl - 8 - len(extra)
    r = rng.random()
    n = 0 if r < 0.1 else 1 if r < 0.2 else 2 * int(rng.integers(1, 33)) + 1 if r < 0.45 \
        else int(rng.integers(2, 65)) if r < 0.8 else int(rng.integers(0, room + 1))
    r = rng.random()
    chk = "good" if clean or r >= 0.23 else "zero" if r < 0.15 else "bad"
    pkt = IR.ip_packet(17, UR.udp(_bytes(rng, n), src=ra, dst=la, sport=rp, dport=lp, chk=chk, extra=extra),
                       src=ra, dst=la, ihl=ihl, ttl=int(rng.integers(0, 256)),
                       flags_off=0 if clean else _flags_off(rng), ident=int(rng.integers(0, 65536)))
    return _finish(rng, pkt, peer, cut=not clean)


def _udp_listeners(rng, local, other, ports, pool, n_lis, any_port, dirty):
    rows = []
    for k in range(n_lis):
        r = rng.random()
        addr = 0 if r < 0.6 else local if r < 0.85 else other
        port = 0 if any_port and rng.random() < 0.1 else int(ports[int(rng.integers(0, len(ports)))])
        bc, nl = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        if n_lis == 64 and k in (31, 32, 63):         # bits 31, 32 and 63 match whatever reaches the port
            addr, bc, nl = (0, local)[k & 1], True, True
            port = pool[k % len(pool)][2]
        rows.append((addr, port, bc, nl, int(rng.integers(0, 1 << 32))))
    return UC.listeners(rows, LIS, dirty=dirty) if rows else None


def _assoc_count(rng):
    r = rng.random()
    if r < 0.3:
        return int(rng.integers(0, 4))
    if r < 0.75:
        return (1 << int(rng.integers(2, 11))) + int(rng.integers(-1, 2))
    return int(rng.integers(4, 2001))


def _udp_assocs(rng, pool, edge, want, dsts, ports):
    """`want` distinct keys: for a pool tuple its exact key (one in two) and, per field, a key that
    differs in that field alone by +-1 or by its byte order (35 in a hundred each); then keys made
    of the pool's field values, then random ones. With `edge`, its first and last key are in, and
    every other key sorts between them."""
    rows = {}

    def add(k):
        if len(rows) < want and k not in rows and (
                edge is None or sort_key(edge[0]) < sort_key(k) < sort_key(edge[1])):
            handle = int(rng.choice([0, 0x7FFFFFFF, int(rng.integers(0, 1 << 31))], p=[0.05, 0.1, 0.85]))
            rows[k] = (rng.random() < 0.4, handle)

    if edge is not None:
        for k in edge[:2]:
            rows[k] = (rng.random() < 0.4, int(rng.integers(0, 1 << 31)))
    for j in rng.permutation(len(pool)):
        k = pool[int(j)]
        if rng.random() < 0.5:
            add(k)
        for f in range(4):
            if rng.random() < 0.35:
                nb = neighbours(k, f)
                add(nb[int(rng.integers(0, len(nb)))])
    tries = 0
    while len(rows) < want:
        tries += 1
        if tries < 4 * want and rng.random() < 0.5:
            k = tuple(pool[int(rng.integers(0, len(pool)))][f] for f in range(4))
        else:
            k = (int(dsts[int(rng.integers(0, len(dsts)))]), int(rng.integers(0x01000002, 0xDF000000)),
                 int(rng.integers(0, 65536)), int(rng.integers(1, 65535)))
        add(k)
    return UC.assocs([k + v for k, v in rows.items()], KEY) if rows else None


def udp_scenario(oracle, seed):
    """1-1500 frames of frame_cases.frames (every verdict; for the interface where its address is
    frame_cases', else for a non-local one), six in ten of them overwritten by UDP datagrams: to
    the interface's address, the subnet broadcast, 255.255.255.255 and a non-local address of the
    subnet; IHL 5-15; 0, 1, an odd number, 2-64 or up to what an MTU of 1500 holds of data bytes;
    a UDP length that cuts 1-20 bytes off the IP payload; padding to 60 bytes and bytes beyond the
    IPv4 total length; the checksum field zero, good or bad; any TTL; fragments; frames cut to
    fewer than 42 bytes. Their (destination, source, ports) come from a pool of 4-40 tuples over
    a few peers (addresses whose numeric order differs from their order in memory among them) and
    a dozen ports (0, 1, 0x00FF, 0x0100, 0xFF00, 65535, 0x0102, 0x0201 among them), one in ten
    from a pool tuple changed in one field, fifteen in a hundred at random.
    Listeners: 0-64 (64 for every seed that is 1 mod 4), port from the same ports (port 0 only in a quarter of the scenarios, or
    nothing would be left unclaimed), iface_addr 0, the interface's or another, both flags drawn;
    with 64 entries bits 31, 32 and 63 match what reaches their port; three scenarios in ten set
    every reserved byte and undefined flag bit. Associations: 0-3, 2^k - 1, 2^k, 2^k + 1
    (k = 2-10) or up to 2000 keys by _udp_assocs; six scenarios in ten with two keys or more pin
    the table's first and last key and send clean datagrams with exactly those keys, with one
    that sorts below the first and one above the last. Cookie bit 31 four times in ten, handles
    up to 0x7FFFFFFF.
    Layout: CSR with lead 0-3, or ring slots of 2048, 2049, 1536 bytes (where every frame fits)
    or of the longest frame's length; d_dgrams 0 or 8 bytes off a 16-byte boundary; aux_blocks
    -1, 1 or 2.
    Not drawn: frames above 1594 bytes, slot lengths above the stride, more than 64 listeners
    (rejected), unsorted tables (test_gpu_udprx.py), IPv4 options other than Nops, VLAN tags."""
    rng = np.random.default_rng(8000 + seed)
    n = T._count(rng)
    local, prefix, bcast, other = _addresses(rng)
    ports = list(SPECIAL_PORTS) + [0x0102, 0x0201] + [int(p) for p in rng.integers(1, 65536, 4)]
    peers = [IR.PEER, IR.PEER + 1, bswap32(IR.PEER), 0x01000002, 0x02000001,
             int(rng.integers(0x01000002, 0xDF000000))]
    dsts = [local] * 5 + [bcast, ALL_ONES, other, other]
    pool = [(int(dsts[int(rng.integers(0, len(dsts)))]), int(peers[int(rng.integers(0, len(peers)))]),
             int(ports[int(rng.integers(0, len(ports)))]), int(ports[int(rng.integers(0, len(ports)))]))
            for _ in range(int(rng.integers(4, 41)))]
    pool = list(dict.fromkeys(pool))
    want = _assoc_count(rng)
    edge = None
    if want >= 2 and rng.random() < 0.6:
        lp = int(ports[int(rng.integers(0, len(ports)))])
        edge = ((local, 0x01000001, lp, 0), (local, 0xDF000001, lp, 65535),
                (local, 0x01000000, lp, 0), (local, 0xDF000002, lp, 65535))
    frames = F.frames(seed=8000 + seed, n=n)
    forced = list(edge) if edge is not None else []
    for i in np.nonzero(rng.random(n) < 0.6)[0]:
        if forced:
            frames[i] = _udp_frame(rng, forced.pop(0), int(i), clean=True)
            continue
        r = rng.random()
        tup = pool[int(rng.integers(0, len(pool)))]
        if r >= 0.85:
            tup = (int(dsts[int(rng.integers(0, len(dsts)))]), int(rng.integers(1, 1 << 32)),
                   int(rng.integers(0, 65536)), int(rng.integers(0, 65536)))
        elif r >= 0.75:
            nb = neighbours(tup, int(rng.integers(0, 4)))
            tup = nb[int(rng.integers(0, len(nb)))]
        frames[i] = _udp_frame(rng, tup, int(i))
    sc = UdpScenario()
    sc.seed, sc.n, sc.frames, sc.pool = seed, n, frames, pool
    sc.edge = edge if not forced else None             # (fewer than four datagrams: no pinned ends)
    sc.prefix = prefix
    sc.ifc = IC.iface(local=local, bcast=bcast, ttl=int(rng.integers(0, 256)),
                      ip_id=int(rng.integers(0, 65536)))
    sc.assocs = _udp_assocs(rng, pool, edge, want, dsts, ports)
    r = rng.random()
    n_lis = 64 if seed % 4 == 1 else 0 if r < 0.12 else int(rng.integers(1, 9)) if r < 0.6 else int(rng.integers(9, 65))
    sc.dirty = rng.random() < 0.3
    sc.listeners = _udp_listeners(rng, local, other, ports, pool, n_lis, rng.random() < 0.25, sc.dirty)
    buf, off = F.pack(frames)
    sc.verdicts = oracle.rx_verify_batch(buf, off)
    sc.e = UC.expected(frames, sc.verdicts, sc.ifc, sc.assocs, sc.listeners, DGRAM)
    sc.slotted = bool(rng.integers(0, 2))
    sc.lead = int(rng.integers(0, 4))
    longest = max(max(len(f) for f in frames), 1)
    slot = int(rng.choice(UDP_STRIDES))
    sc.slot = slot if slot >= longest else longest
    sc.dgram_shift = 8 * int(rng.integers(0, 2))
    sc.aux_blocks = int(rng.choice(AUX_BLOCKS))
    return sc


def udp_key(frame):
    T0 = 14 + (frame[14] & 0xF) * 4
    src, dst = struct.unpack_from(">II", frame, 26)
    sport, dport = struct.unpack_from(">HH", frame, T0)
    return dst, src, dport, sport


def udp_table_keys(sc):
    """The association table's keys in table order."""
    if sc.assocs is None:
        return []
    return [tuple(int(a[f]) for f in KEY_FIELDS) for a in sc.assocs]


# ---- ICMP responder ---------------------------------------------------------------------------

HDR_STRIDES = (42, 64, 72, 96, 128)
MTUS = (256, 576, 1006, 1500)
ECHO_CLASSES = ("carry", "carry_to_one", "zero_class", "field_zero", "field_ones")


class IcmpScenario:
    """frames / verdicts / codes (a list or None) of the whole scenario, ifc (its first batch's
    interface), batches [(first frame, end, interface with the batch's first Ident, Expected)],
    slotted, hdr_stride, shift, aux_blocks."""


def _echo(rng, mtu, dst, src, peer, p_big):
    """An echo request. Half of them get a checksum field of one of ECHO_CLASSES, forced through
    the identifier word so that the request still verifies: with w0 the type/code word, the reply's
    incremental update (icmp_common.h) carries end-around where w0 + field >= 2^16
    ("carry"; == 2^16 gives 0x0001, "carry_to_one"; field 0xFFFF, the other zero of a sum whose
    checksum is 0x0000, "field_ones"), and where w0 + field == 0xFFFF the kernel has to read the
    data ("zero_class": the reply's field is 0xFFFF if every byte is zero, else 0x0000)."""
    ihl = 5 if rng.random() < 0.6 else int(rng.integers(5, 16))
    code = 0 if rng.random() < 0.9 else int(rng.integers(0, 256))
    room = mtu - 28
    r = rng.random()
    n = 0 if r < 0.1 else 1 if r < 0.18 else 2 * int(rng.integers(1, 32)) + 1 if r < 0.4 \
        else 2 * int(rng.integers(1, 33)) if r < 0.6 else room if r < 0.67 \
        else room + 1 if r < 0.67 + p_big else int(rng.integers(0, room + 1))
    r = rng.random()
    data = bytes(n) if r < 0.15 else b"\xff" * n if r < 0.25 else _bytes(rng, n)
    ident, seq = int(rng.integers(0, 65536)), int(rng.integers(0, 65536))
    cls = ECHO_CLASSES[int(rng.integers(0, len(ECHO_CLASSES)))] if rng.random() < 0.5 else None
    bad = cls is None and rng.random() < 0.12
    w0 = 0x0800 | code
    if cls is not None:
        if cls == "zero_class" and rng.random() < 0.4:
            data, seq = bytes(n), 0                     # every byte zero: the identifier comes out 0
        field = {"carry": int(rng.integers(0x10000 - w0, 0xFFFF)), "carry_to_one": 0x10000 - w0,
                 "zero_class": 0xFFFF - w0, "field_zero": 0, "field_ones": 0}[cls]
        ident = ((~field & 0xFFFF) - w0 - seq - IR.be_sum(data)) % 0xFFFF
    msg = bytearray(IR.icmp(8, code, struct.pack(">HH", ident, seq), data, bad=bad))
    if cls is not None:
        assert struct.unpack_from(">H", msg, 2)[0] == field, cls
        if cls == "field_ones":
            msg[2:4] = b"\xff\xff"
    pkt = IR.ip_packet(1, bytes(msg), src=src, dst=dst, ihl=ihl, ttl=int(rng.integers(0, 256)),
                       flags_off=_flags_off(rng), ident=int(rng.integers(0, 65536)))
    return _finish(rng, pkt, peer)


def echo_class(frame):
    """Which of ECHO_CLASSES (or "plain") an echo request's checksum field falls in."""
    t = 14 + (frame[14] & 0xF) * 4
    w0, field = struct.unpack_from(">HH", frame, t)
    if field == 0xFFFF:
        return "field_ones"
    if field == 0:
        return "field_zero"
    if w0 + field == 0xFFFF:
        return "zero_class"
    if w0 + field == 0x10000:
        return "carry_to_one"
    return "carry" if w0 + field > 0x10000 else "plain"


def icmp_batches(frames, verdicts, codes, ifc):
    """The scenario as the batches of a host that takes the slow path for a TOO_LARGE frame, cut
    as icmp_cases.stack_batches cuts a stack's cases: a batch ends behind such a frame, and the
    next one starts one Ident later."""
    status = [IC.plan(f, int(v), IC.NO_UNREACH if codes is None else int(codes[i]), ifc)[0]
              for i, (f, v) in enumerate(zip(frames, verdicts))]
    out, start, ip_id = [], 0, ifc["ip_id"]
    while start < len(frames):
        big = next((i for i in range(start, len(frames)) if status[i] == IC.TOO_LARGE), None)
        end = len(frames) if big is None else big + 1
        f = dict(ifc, ip_id=ip_id & 0xFFFF)
        e = IC.respond(frames[start:end], verdicts[start:end],
                       None if codes is None else codes[start:end], f)
        assert e.status.tolist() == status[start:end]
        out.append((start, end, f, e))
        ip_id += int(e.counts[0]) + (0 if big is None else 1)
        start = end
    return out


def icmp_scenario(oracle, seed):
    """1-1500 frames of frame_cases.frames (every verdict; its echo requests and UDP datagrams are
    for the interface where its address is frame_cases'), 55 in a hundred of them overwritten: by
    echo requests (two in three; _echo) to the interface's address, the subnet broadcast,
    255.255.255.255 and a non-local address, IHL 5-15, data of 0, 1, an odd or an even number of
    bytes, exactly what the MTU holds, one byte more (TOO_LARGE; about 2.5 per scenario) or any
    length below, all zero, all 0xFF or random, a bad checksum, fragments; by other ICMP types;
    by UDP datagrams and by frames of another protocol with 0-12 payload bytes (what an unreach
    quotes). Sources: four peers, and 15 in a hundred the subnet broadcast, 255.255.255.255, a
    multicast address or 0.0.0.0. Interface: any MAC and TTL, MTU 256, 576, 1006, 1500 or
    between, ip_id anywhere, 35 in a hundred within 100 below 0x10000; allow_broadcast_ping drawn.
    Unreach codes: None (one in five), else 0xFF but for a drawn share (a tenth to a half) of ALL
    frames, whatever their verdict, which get a code 0-15. Layout: CSR from an odd address or ring
    slots of 2048 bytes, hdr_stride 42, 64, 72, 96 or 128, the ring 0 or 8 bytes off its 64-byte
    boundary, aux_blocks -1, 1 or 2. A TOO_LARGE frame ends a batch (icmp_batches).
    Not drawn: frames above 1594 bytes, an MTU above 1500 or below 256 (rejected), unreach codes
    above 15, IPv4 options other than Nops, slot strides other than 2048."""
    rng = np.random.default_rng(9000 + seed)
    n = T._count(rng)
    local, prefix, bcast, other = _addresses(rng)
    mtu = int(rng.choice(MTUS)) if rng.random() < 0.75 else int(rng.integers(257, 1500))
    ip_id = 0x10000 - int(rng.integers(1, 101)) if rng.random() < 0.35 else int(rng.integers(0, 65536))
    mac = bytes([int(rng.integers(0, 128)) * 2]) + _bytes(rng, 5)
    ifc = IC.iface(local=local, bcast=bcast, mtu=mtu, ip_id=ip_id, ttl=int(rng.integers(0, 256)),
                   allow=bool(rng.integers(0, 2)), mac=mac)
    frames = F.frames(seed=9000 + seed, n=n)
    p_big = min(0.04, 2.5 / n)
    for i in np.nonzero(rng.random(n) < 0.55)[0]:
        peer = int(rng.integers(0, 4))
        r = rng.random()
        src = IR.PEER + peer if r < 0.85 else bcast if r < 0.89 else ALL_ONES if r < 0.92 \
            else 0xE0000000 + int(rng.integers(0, 1 << 28)) if r < 0.96 else 0
        r = rng.random()
        dst = local if r < 0.6 else bcast if r < 0.72 else ALL_ONES if r < 0.82 else other
        r = rng.random()
        if r < 0.66:
            frames[i] = _echo(rng, mtu, dst, src, peer, p_big)
            continue
        ihl = 5 if rng.random() < 0.6 else int(rng.integers(5, 16))
        kw = dict(src=src, dst=dst, ihl=ihl, ttl=int(rng.integers(0, 256)), flags_off=_flags_off(rng))
        if r < 0.76:
            pkt = IR.ip_packet(1, IR.icmp(int(rng.choice([0, 3, 13, int(rng.integers(0, 256))])),
                                          int(rng.integers(0, 16)), _bytes(rng, 4),
                                          _bytes(rng, int(rng.integers(0, 60)))), **kw)
        elif r < 0.92:
            pkt = IR.ip_packet(17, IR.udp(_bytes(rng, int(rng.integers(0, 40))), src=src, dst=dst,
                                          dport=int(rng.integers(0, 65536)),
                                          with_chksum=rng.random() < 0.8, bad=rng.random() < 0.1), **kw)
        else:
            pkt = IR.ip_packet(int(rng.choice([47, 50, 132])), _bytes(rng, int(rng.integers(0, 13))), **kw)
        frames[i] = _finish(rng, pkt, peer)
    codes = None
    if rng.random() >= 0.2:
        codes = np.where(rng.random(n) < rng.uniform(0.1, 0.5), rng.integers(0, 16, n), IC.NO_UNREACH)
        codes = [int(c) for c in codes]
    sc = IcmpScenario()
    sc.seed, sc.n, sc.frames, sc.codes, sc.ifc = seed, n, frames, codes, ifc
    buf, off = F.pack(frames)
    sc.verdicts = oracle.rx_verify_batch(buf, off)
    sc.batches = icmp_batches(frames, sc.verdicts, codes, ifc)
    sc.slotted = bool(rng.integers(0, 2))
    sc.hdr_stride = int(rng.choice(HDR_STRIDES))
    sc.shift = 8 * int(rng.integers(0, 2))
    sc.aux_blocks = int(rng.choice(AUX_BLOCKS))
    return sc
