"""TEST INFRASTRUCTURE -- shared by test_ipfrag_host.py, test_gpu_ipfrag.py and the random
scenarios: the model of the UDP send with IPv4 fragmentation and the case generators.

The model is a plain Python restatement of the reference's UDP send for one datagram,
UdpApi::sendUdpIp4Packet (udp/IpUdpProto.h:152-184) + IpStack::sendIp4Dgram (ip/IpStack.h:373-464)
+ send_fragmented (:467-539), written independently of the kernels: send_fragmented's loop as a
loop (a remaining length that shrinks, not the closed form of the library), the checksums from the
CPU oracle over the bytes (pseudo-header + UDP header + payload; each 20-byte IPv4 header).
test_ipfrag_host.py pins its leaf functions (Ip4RoundFragLen, two checksums) against code compiled
from the reference; test_stack_tx_ref_host.py holds the whole model to the packets the reference
stack emits (tests/golden/stack_tx_ref_cases.json).

A datagram case is a dict: ``pieces`` ((offset, length) x 2 into the batch's payload buffer),
``mtu``, ``ip_id``, ``reserved``, ``hdr`` (48 template bytes); for a datagram that breaks the
contract, or whose counts are made to disagree, also ``give`` = (fragments, chunks) the caller's
index hands it.
"""
import struct

import numpy as np

ACCEPT = 6
FRAG_NEEDED = 12
DGRAM_INVALID = 13
HDR0, HDRK = 42, 34
MIN_MTU = 256
MTUS = (256, 576, 1006, 1500, 9000)

LOCAL_MAC = bytes([0x02, 0, 0, 0, 0, 0x01])
PEER_MAC = bytes([0x02, 0, 0, 0, 0, 0x02])


def template(src=0x0A000001, dst=0x0A000002, sport=40000, dport=53, ttl=64, dscp=0, df=False,
             junk=0xA5):
    """48 template bytes as Ip4CommonSendParams and UdpTxInfo fill the header; the overwritten
    fields (and the six pad bytes) hold `junk`."""
    j2 = bytes([junk]) * 2
    eth = PEER_MAC + LOCAL_MAC + b"\x08\x00"
    ip = (struct.pack(">BB", 0x45, dscp) + j2 + j2 + struct.pack(">HBB", 0x4000 if df else 0, ttl, 17) +
          j2 + struct.pack(">II", src, dst))
    udp = struct.pack(">HH", sport, dport) + j2 + j2
    t = eth + ip + udp + j2 * 3
    assert len(t) == 48
    return t


def dgram(p0, p1=(0, 0), *, mtu=1500, ip_id=0x1234, reserved=0, hdr=None, give=None, **tmpl):
    c = dict(pieces=(tuple(p0), tuple(p1)), mtu=mtu, ip_id=ip_id, reserved=reserved,
             hdr=hdr if hdr is not None else template(**tmpl))
    if give is not None:
        c["give"] = tuple(give)
    return c


class Batch:
    def __init__(self, cases, payload):
        self.cases, self.payload = cases, payload


def payload_bytes(n=1 << 17, seed=13):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


# ---- the model ----------------------------------------------------------------------------

def round_frag_len(header_length, mtu):
    """Ip4RoundFragLen (proto/Ip4Proto.h:71-73)."""
    return header_length + ((mtu - header_length) // 8) * 8


def descriptor_ok(c):
    """The datagram contract, the part a descriptor alone decides (chksum.h)."""
    h = c["hdr"]
    D = c["pieces"][0][1] + c["pieces"][1][1]
    return (c["mtu"] >= MIN_MTU and 8 + D <= 65535 and c["reserved"] == 0
            and h[12:14] == b"\x08\x00" and h[14] == 0x45 and h[23] == 17
            and (h[20] & ~0x40) == 0 and h[21] == 0)


def ip_packets_of(c):
    """[(IP payload offset, IP payload length, MF)] of the datagram, or None for
    IpErr::FragmentationNeeded: sendIp4Dgram's decision (:404-421) and send_fragmented's loop
    (:470-538) over the P = 8 + D bytes of UDP header and payload."""
    P = 8 + c["pieces"][0][1] + c["pieces"][1][1]
    mtu = c["mtu"]
    if 20 + P <= mtu:
        return [(0, P, False)]
    if c["hdr"][20] & 0x40:
        return None
    pkt_send_len = round_frag_len(20, mtu)
    out = [(0, pkt_send_len - 20, True)]
    fragment_offset = pkt_send_len - 20
    remaining = P - fragment_offset
    more = True
    while more:
        assert fragment_offset % 8 == 0
        if 20 + remaining <= mtu:
            pkt_send_len = 20 + remaining
            more = False
        out.append((fragment_offset, pkt_send_len - 20, more))
        fragment_offset += pkt_send_len - 20
        remaining -= pkt_send_len - 20
    return out


def fragments_of(c):
    """[(offset, length, MF, [(payload offset, length) chunks])]: each packet's bytes of the UDP
    payload (fragment 0 starts with the 8 UDP header bytes, which lie in its header slot) as
    chunks of the two pieces; [] for FragmentationNeeded."""
    (o0, l0), (o1, l1) = c["pieces"]
    out = []
    for off, ln, mf in ip_packets_of(c) or []:
        a, b = max(off - 8, 0), off + ln - 8
        chunks = []
        if a < min(b, l0):
            chunks.append((o0 + a, min(b, l0) - a))
        if b > max(a, l0):
            s1 = max(a, l0)
            chunks.append((o1 + s1 - l0, b - s1))
        out.append((off, ln, mf, chunks))
    return out


def counts_of(c):
    fr = fragments_of(c)
    return len(fr), sum(len(ch) for *_, ch in fr)


def udp_checksum(oracle, c, payload):
    """udp/IpUdpProto.h:163-179 over the whole datagram."""
    h = c["hdr"]
    (o0, l0), (o1, l1) = c["pieces"]
    data = payload[o0:o0 + l0].tobytes() + payload[o1:o1 + l1].tobytes()
    P = 8 + len(data)
    cover = h[26:34] + struct.pack(">HH", 17, P) + h[34:38] + struct.pack(">HH", P, 0) + data
    arr = np.frombuffer(cover, dtype=np.uint8).copy()
    chk = oracle.final(arr, 0, arr.size)
    return chk if chk else 0xFFFF


def fragment_header(oracle, c, off, ln, mf, udp_chk):
    """The header bytes of the fragment at IP-payload offset `off`: 42 for the first (with the
    UDP header), 34 for the others."""
    h = bytearray(c["hdr"][:HDR0 if off == 0 else HDRK])
    tfo, = struct.unpack_from(">H", h, 20)
    struct.pack_into(">H", h, 16, 20 + ln)
    struct.pack_into(">H", h, 18, c["ip_id"])
    struct.pack_into(">H", h, 20, tfo | (0x2000 if mf else 0) | off // 8)
    struct.pack_into(">H", h, 24, 0)
    ip = np.frombuffer(bytes(h[14:34]), dtype=np.uint8).copy()
    struct.pack_into(">H", h, 24, oracle.final(ip, 0, 20))
    if off == 0:
        P = 8 + c["pieces"][0][1] + c["pieces"][1][1]
        struct.pack_into(">HH", h, 38, P, udp_chk)
    return bytes(h)


def model_layout(cases):
    """(frag_index, chunk_base, status) as aipstack_udp_dgram_layout must give them, or None if a
    datagram breaks the contract."""
    fi, cb, st = [0], [0], []
    for c in cases:
        if not descriptor_ok(c):
            return None
        ns, nc = counts_of(c)
        fi.append(fi[-1] + ns)
        cb.append(cb[-1] + nc)
        st.append(FRAG_NEEDED if ip_packets_of(c) is None else ACCEPT)
    return (np.array(fi, dtype=np.uint64), np.array(cb, dtype=np.uint64), np.array(st, dtype=np.uint8))


def caller_index(cases):
    """The index a caller hands over: the model's counts, and for a datagram with ``give`` those
    counts."""
    fi, cb = [0], [0]
    for c in cases:
        ns, nc = c["give"] if "give" in c else counts_of(c)
        fi.append(fi[-1] + ns)
        cb.append(cb[-1] + nc)
    return np.array(fi, dtype=np.uint64), np.array(cb, dtype=np.uint64)


class Expected:
    """What aipstack_udp_tx_fragment must leave: ``headers`` ((n, 42) bytes, the first hdr_len of
    each row; rows of invalid fragments unused), ``hdr_len``, ``status``, ``dgram_status``,
    ``chunk_off`` (payload offsets; -1 = address 0), ``chunk_len``, ``chunk_index``, ``frag_case``
    (datagram of each fragment), ``frag_k``, ``frag_off``, ``frag_len``, ``frag_chunks``."""


def expected(oracle, batch, frag_index=None, chunk_base=None):
    cases, payload = batch.cases, batch.payload
    if frag_index is None:
        frag_index, chunk_base = caller_index(cases)
    n, nc = int(frag_index[-1]), int(chunk_base[-1])
    e = Expected()
    e.headers = np.zeros((n, HDR0), dtype=np.uint8)
    e.hdr_len = np.zeros(n, dtype=np.uint32)
    e.status = np.full(n, DGRAM_INVALID, dtype=np.uint8)
    e.dgram_status = np.full(len(cases), DGRAM_INVALID, dtype=np.uint8)
    e.chunk_off = np.full(nc, -1, dtype=np.int64)
    e.chunk_len = np.zeros(nc, dtype=np.uint32)
    e.chunk_index = np.zeros(n + 1, dtype=np.uint64)
    e.chunk_index[n] = nc
    e.frag_case = np.zeros(n, dtype=np.int64)
    e.frag_k = np.zeros(n, dtype=np.int64)
    e.frag_off = np.zeros(n, dtype=np.int64)
    e.frag_len = np.zeros(n, dtype=np.int64)
    e.frag_chunks = [[] for _ in range(n)]
    for d, c in enumerate(cases):
        f0, ns = int(frag_index[d]), int(frag_index[d + 1] - frag_index[d])
        c0, ncd = int(chunk_base[d]), int(chunk_base[d + 1] - chunk_base[d])
        e.frag_case[f0:f0 + ns] = d
        e.frag_k[f0:f0 + ns] = np.arange(ns)
        frs = fragments_of(c) if descriptor_ok(c) else None
        if frs is None or len(frs) != ns or sum(len(ch) for *_, ch in frs) != ncd:
            # status 13, slots untouched, chunk entries empty; the fragments share the entries
            # out in order (chksum.h)
            for k in range(ns):
                e.chunk_index[f0 + k] = c0 + min(k, ncd)
            continue
        e.dgram_status[d] = FRAG_NEEDED if ip_packets_of(c) is None else ACCEPT
        if not frs:
            continue
        chk = udp_checksum(oracle, c, payload)
        at = c0
        for k, (off, ln, mf, chunks) in enumerate(frs):
            i = f0 + k
            e.status[i] = ACCEPT
            e.chunk_index[i] = at
            for o, l in chunks:
                assert l > 0
                e.chunk_off[at], e.chunk_len[at] = o, l
                at += 1
            e.frag_chunks[i] = chunks
            e.frag_off[i], e.frag_len[i] = off, ln
            h = fragment_header(oracle, c, off, ln, mf, chk)
            e.hdr_len[i] = len(h)
            e.headers[i, :len(h)] = np.frombuffer(h, dtype=np.uint8)
        assert at == c0 + ncd
    return e


def descriptors(batch, base_addr, dtype):
    """The aipstack_udp_dgram array of the batch with its payload buffer at `base_addr`."""
    g = np.zeros(len(batch.cases), dtype=dtype)
    for d, c in enumerate(batch.cases):
        for p in (0, 1):
            g["data_addr"][d, p] = base_addr + c["pieces"][p][0]
            g["data_len"][d, p] = c["pieces"][p][1]
        g["mtu"][d], g["ip_id"][d], g["reserved"][d] = c["mtu"], c["ip_id"], c["reserved"]
        g["hdr"][d] = np.frombuffer(c["hdr"], dtype=np.uint8)
    return g


def frame_of(e, payload, i, headers=None):
    """Fragment i as a linear frame (from the model's headers, or from `headers` rows)."""
    h = (e.headers if headers is None else headers)[i, :int(e.hdr_len[i])].tobytes()
    return h + b"".join(payload[o:o + l].tobytes() for o, l in e.frag_chunks[i])


def linearise(e, payload, headers=None):
    """The emitted fragments as linear frames: (buffer, offsets, their fragment numbers)."""
    parts, offs, ids = [], [0], []
    for i in np.nonzero(e.status == ACCEPT)[0]:
        f = frame_of(e, payload, int(i), headers)
        parts.append(np.frombuffer(f, dtype=np.uint8))
        offs.append(offs[-1] + len(f))
        ids.append(int(i))
    buf = np.concatenate(parts) if parts else np.zeros(1, dtype=np.uint8)
    return buf, np.array(offs, dtype=np.uint64), ids


def reassemble(e, payload, d, headers=None):
    """Datagram d put together again from its fragments, by their offset fields: one frame with
    the first fragment's Ethernet and IPv4 header (total length and flags / offset rewritten, the
    header checksum made anew) followed by the IP payload: what the receiver's reassembly hands on."""
    ids = [int(i) for i in np.nonzero((e.frag_case == d) & (e.status == ACCEPT))[0]]
    parts = {}
    for i in ids:
        f = frame_of(e, payload, i, headers)
        fo, = struct.unpack_from(">H", f, 20)
        parts[(fo & 0x1FFF) * 8] = f[34:]
    body = b""
    for off in sorted(parts):
        assert off == len(body)
        body += parts[off]
    first = bytearray(frame_of(e, payload, ids[0], headers)[:34])
    struct.pack_into(">H", first, 16, 20 + len(body))
    struct.pack_into(">H", first, 20, struct.unpack_from(">H", first, 20)[0] & 0x4000)
    struct.pack_into(">H", first, 24, 0)      # the rebuilt header's own checksum, in plain Python
    total = sum(struct.unpack_from(">10H", first, 14))
    while total >> 16:
        total = (total & 0xFFFF) + (total >> 16)
    struct.pack_into(">H", first, 24, ~total & 0xFFFF)
    return bytes(first) + body


# ---- properties of a batch, from the model alone (no vacuous tests) -----------------------

def count_straddle_odd_first(e):
    """Fragments of two chunks whose first has an odd length (as tcpseg_cases counts segments)."""
    return sum(1 for ch in e.frag_chunks if len(ch) == 2 and ch[0][1] & 1)


def branches(batch, e=None):
    """Which branches of the loop the batch's valid datagrams take, from the model alone."""
    got = set()
    for c in batch.cases:
        if not descriptor_ok(c) or "give" in c:
            continue
        pk = ip_packets_of(c)
        (o0, l0), (o1, l1) = c["pieces"]
        if pk is None:
            got.add("S=0")
            continue
        S = len(pk)
        F = round_frag_len(20, c["mtu"]) - 20
        got.add("S=1" if S == 1 else "S>1")
        if S > 64:
            got.add("S>64")
        if S > 1 and pk[-1][1] > F:
            got.add("last>F")
        two = [k for k, (*_, ch) in enumerate(fragments_of(c)) if len(ch) == 2]
        if two:
            got.add("straddle")
            if S > 1 and (l0 + 8) // F > S - 1:
                assert two == [S - 1]
                got.add("clamped")
        elif l0 and l1:
            got.add("edge")          # both pieces, the boundary between two fragments
        else:
            got.add("no_straddle")
    if e is not None:
        first = e.hdr_len == HDR0
        udp = e.headers[:, 40].astype(int) << 8 | e.headers[:, 41]
        if (udp[first] == 0xFFFF).any():
            got.add("0xFFFF")
    return got


# ---- case generators ------------------------------------------------------------------------

def _mf(mtu):
    M = mtu - 20
    return M, (M // 8) * 8


def clamp_case(mtu=256, S=3, back=2, **kw):
    """A datagram of S fragments on an mtu with M % 8 != 0 whose last fragment is longer than F
    and whose piece boundary lies in that fragment's bytes past (S - 1) * F + F: the arithmetic
    chunk number (len0 + 8) // F names fragment S, which does not exist."""
    M, F = _mf(mtu)
    assert M % 8 >= 2
    P = (S - 1) * F + F + M % 8 - 1
    D = P - 8
    l0 = D - back
    assert (l0 + 8) // F == S
    return dgram((3, l0), (70001, D - l0), mtu=mtu, **kw)


def boundary_batch():
    """About 300 datagrams: for each mtu P = M, M + 1, M + F, M + F + 1, the piece boundary at
    len0 in {F - 9, F - 8, F - 7} and either piece empty, the clamped straddle, D = 0 and
    D = 65527 at mtu 256 (283 fragments), DF with and without need, then random sizes with odd
    piece lengths and odd addresses."""
    pay = payload_bytes()
    rng = np.random.default_rng(77)
    cs = []
    for mtu in MTUS:
        M, F = _mf(mtu)
        for P in (M, M + 1, M + F, M + F + 1):
            cs.append(dgram((5, P - 8), mtu=mtu, ip_id=P & 0xFFFF))
        D = M + F + 3 - 8
        for l0 in (F - 9, F - 8, F - 7):
            cs.append(dgram((1001, l0), (70002, D - l0), mtu=mtu, ip_id=l0))
        cs.append(dgram((0, 0), (70003, D), mtu=mtu))
        cs.append(dgram((1003, D), (0, 0), mtu=mtu))
        cs.append(dgram((7, M - 8), mtu=mtu, df=True))               # DF, fits
        cs.append(dgram((7, M - 7), mtu=mtu, df=True))               # DF, does not: S = 0
    cs.append(clamp_case(256))
    cs.append(clamp_case(1006, S=2, back=1))
    cs.append(dgram((0, 0), mtu=256))                                # D = 0
    cs.append(dgram((0, 0), mtu=1500, src=0, dst=0, sport=0, dport=0))
    cs.append(dgram((1, 65527), mtu=256, ip_id=0xFFFF))              # 283 fragments
    cs.append(dgram((9, 30000), (60001, 35527), mtu=9000))           # D = 65527, two pieces
    while len(cs) < 300:
        mtu = MTUS[int(rng.integers(0, 4))]                          # 9000 only above
        M, F = _mf(mtu)
        D = int(rng.integers(0, 5 * M))
        l0 = int(rng.integers(0, D + 1)) if rng.integers(0, 3) else D
        cs.append(dgram((int(rng.integers(0, 30000)) | 1, l0),
                        (int(rng.integers(40000, 60000)) | int(rng.integers(0, 2)), D - l0), mtu=mtu,
                        ip_id=int(rng.integers(0, 65536)), ttl=int(rng.integers(1, 256)),
                        src=int(rng.integers(0, 1 << 32)), dst=int(rng.integers(0, 1 << 32)),
                        sport=int(rng.integers(0, 65536)), dport=int(rng.integers(0, 65536)),
                        dscp=int(rng.integers(0, 256)) if rng.integers(0, 4) == 0 else 0))
    return Batch(cs, pay)


def spanning_batch():
    """One datagram of 87 fragments (mtu 256, D = 20,000) that begins and ends inside a wave,
    between datagrams of one to three fragments and runs of datagrams of no fragment."""
    pay = payload_bytes()
    z = lambda: dgram((7, 300), mtu=256, df=True)                     # noqa: E731  S = 0
    small = lambda j: dgram((11 * j + 1, 100 + 150 * (j % 4)), mtu=256, ip_id=j)   # noqa: E731
    cs = [z(), z()] + [small(j) for j in range(25)] + [z(), z(), z()]
    cs.append(dgram((3, 9000), (50001, 11000), mtu=256, ip_id=0xBEEF))
    cs += [z()] + [small(j) for j in range(25, 50)] + [z(), z()]
    return Batch(cs, pay)


def zero_udp_checksum_batch(oracle):
    """Datagrams whose UDP sum comes out 0, so that the field is sent as 0xFFFF: the last two
    payload bytes of each (an even length) are patched to the value that completes the sum. One
    fits its MTU, one is fragmented, one has two pieces."""
    pay = payload_bytes().copy()
    cs = []
    for j, (ln, l0, mtu) in enumerate(((2, 2, 1500), (100, 100, 576), (3000, 3000, 1500),
                                       (2000, 999, 576))):
        o = 5000 * (j + 1) + (j & 1)
        c = dgram((o, l0), (o + l0, ln - l0), mtu=mtu, ip_id=j, sport=1000 + j)
        pay[o + ln - 2:o + ln] = 0
        chk = udp_checksum(oracle, c, pay)
        pay[o + ln - 2], pay[o + ln - 1] = chk >> 8, chk & 0xFF
        cs.append(c)
    cs.insert(1, dgram((1, 500)))
    return Batch(cs, pay)


INVALID_CLASSES = ["mtu_small", "d_big", "reserved", "ethertype", "vihl", "proto", "mf", "offset",
                   "evil_bit"]


def invalid_case(cls):
    """A datagram of the given invalid class; the caller's index gives it 2 fragments, 3 chunks."""
    kw, hdr = {}, bytearray(template())
    p0, p1 = (40, 500), (0, 0)
    if cls == "mtu_small":
        kw["mtu"] = 255
    elif cls == "d_big":
        p0, p1 = (0, 65000), (0, 528)
    elif cls == "reserved":
        kw["reserved"] = 1 << 24
    elif cls == "ethertype":
        hdr[12:14] = b"\x86\xdd"
    elif cls == "vihl":
        hdr[14] = 0x46
    elif cls == "proto":
        hdr[23] = 6
    elif cls == "mf":
        hdr[20] = 0x20
    elif cls == "offset":
        hdr[21] = 1
    elif cls == "evil_bit":
        hdr[20] = 0x80
    return dgram(p0, p1, hdr=bytes(hdr), give=(2, 3), **kw)


def invalid_batch():
    """An invalid datagram of each class between valid ones (fragmented, one of them straddling)."""
    pay = payload_bytes()
    cs = [dgram((1, 2000), (4001, 999), mtu=576)]
    for j, cls in enumerate(INVALID_CLASSES):
        cs.append(invalid_case(cls))
        cs.append(dgram((50 * j + 1, 900 + j), (9000 + j, 300), mtu=576, ip_id=j))
    return Batch(cs, pay)


def mismatch_batch():
    """Valid descriptors whose caller-given counts disagree: too few / too many fragments, too
    few / too many chunks, no fragment but chunks, a DF datagram above its MTU that is given a
    fragment; valid neighbours."""
    pay = payload_bytes()
    good = lambda j: dgram((10 * j + 1, 1000), (7001, 200), mtu=576, ip_id=j)   # noqa: E731
    three = dict(mtu=576)                                                      # 3 frags, 3 chunks
    assert counts_of(dgram((1, 1500), **three)) == (3, 3)
    cs = [good(0), dgram((1, 1500), give=(2, 3), **three), good(1),
          dgram((1, 1500), give=(5, 3), **three), good(2),
          dgram((1, 1500), give=(3, 2), **three), good(3),
          dgram((1, 1500), give=(3, 6), **three), good(4),
          dgram((1, 1500), give=(0, 2), **three), good(5),
          dgram((1, 1500), give=(1, 0), df=True, **three), good(6)]
    return Batch(cs, pay)


def multipass_batch(n):
    """Exactly n fragments from the ingredients of boundary_batch (its 283-fragment datagram
    left out) with spanning_batch in their middle, then invalid_batch and mismatch_batch, each
    datagram taken if it still fits; one-fragment datagrams make up the rest."""
    pay = payload_bytes()
    cs, total = [], 0
    pool = [c for c in boundary_batch().cases if counts_of(c)[0] < 200]
    for c in pool[:60] + spanning_batch().cases + pool[60:] + invalid_batch().cases + mismatch_batch().cases:
        ns = c["give"][0] if "give" in c else counts_of(c)[0]
        if total + ns <= n:
            cs.append(c)
            total += ns
    cs += [dgram((3 * j + (j & 1), 1 + (j * 37) % 700), mtu=1006, ip_id=j) for j in range(n - total)]
    return Batch(cs, pay)


def lying_indices(batch):
    """(name, frag_index, chunk_base) triples that lie about a batch of valid datagrams: the
    running sums shifted, cut short, running past the totals, decreasing, and not starting at 0.
    The totals n_frags and n_chunks stay the honest ones."""
    fi, cb = caller_index(batch.cases)
    n, nc = int(fi[-1]), int(cb[-1])
    m = len(batch.cases)
    out = []
    a = fi.copy(); a[m // 2:] += 3                                   # too many from the middle on
    out.append(("frags_past_the_total", a, cb.copy()))
    a = fi.copy(); a[m // 2:] -= np.minimum(a[m // 2:], 2)
    out.append(("frags_too_few", a, cb.copy()))
    a = fi.copy(); a[1:m] = a[1:m][::-1]                             # decreasing
    out.append(("frags_decreasing", a, cb.copy()))
    b = cb.copy(); b[1:m] = b[1:m][::-1]
    out.append(("chunks_decreasing", fi.copy(), b))
    b = cb.copy(); b[m // 3:] += nc + 1000                           # far past the table
    out.append(("chunks_past_the_table", fi.copy(), b))
    a = fi.copy(); a[0] = 5
    b = cb.copy(); b[0] = 4
    out.append(("not_from_zero", a, b))
    a = np.full_like(fi, np.uint64(1) << np.uint64(63))
    out.append(("huge", a, a.copy()))
    assert n > 0 and nc > 0
    return out
