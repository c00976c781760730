"""TEST INFRASTRUCTURE -- shared by test_tcpseg_host.py and test_gpu_tcpseg.py: the model of TCP
burst segmentation and the case generators.

The model is a plain Python restatement of the reference's send loop for one burst,
pcb_output_segment (tcp/IpTcpProto_output.h:1069-1102) + PcbOutputHelper::sendSegment (:1236-1284)
+ IpStack::sendIp4DgramFast (ip/IpStack.h:632-663), written independently of the kernels: the
per-segment fields by the reference's rules, the checksums from the CPU oracle over the bytes
(pseudo-header + TCP header + data; the IPv4 header). test_tcpseg_host.py pins its checksum call
sequences against code compiled from the reference; test_stack_tx_ref_host.py holds the whole
model to the segments the reference stack emits (tests/golden/stack_tx_ref_cases.json).

A burst case is a dict: ``pieces`` ((offset, length) x 2 into the batch's payload buffer),
``seq``, ``psh_offset``, ``mss``, ``ip_id``, ``flags``, ``reserved`` (3 bytes), ``hdr`` (56
template bytes); for a burst that breaks the contract also ``give`` = (segments, chunks) the
caller's index hands it.
"""
import struct

import numpy as np

ACCEPT = 6
BURST_INVALID = 10
FIN = 1
HDR = 54

LOCAL_MAC = bytes([0x02, 0, 0, 0, 0, 0x01])
PEER_MAC = bytes([0x02, 0, 0, 0, 0, 0x02])


def template(src=0x0A000001, dst=0x0A000002, sport=40000, dport=80, ack=0x0A0B0C0D,
             window=0x2000, ttl=64, dscp=0, frag=0x4000, urgent=0, junk=0xA5):
    """56 template bytes as prepareCommon / prepareSendIp4Dgram leave the header; the six
    overwritten fields (and the two pad bytes) hold `junk`."""
    j2, j4 = bytes([junk]) * 2, bytes([junk]) * 4
    eth = PEER_MAC + LOCAL_MAC + b"\x08\x00"
    ip = (struct.pack(">BB", 0x45, dscp) + j2 + j2 + struct.pack(">HBB", frag, ttl, 6) + j2 +
          struct.pack(">II", src, dst))
    tcp = (struct.pack(">HH", sport, dport) + j4 + struct.pack(">I", ack) + j2 +
           struct.pack(">H", window) + j2 + struct.pack(">H", urgent))
    t = eth + ip + tcp + j2
    assert len(t) == 56
    return t


def burst(p0, p1=(0, 0), *, mss=1460, seq=0x01020304, psh_offset=0, ip_id=0x1234, flags=0,
          reserved=(0, 0, 0), hdr=None, give=None):
    c = dict(pieces=(tuple(p0), tuple(p1)), mss=mss, seq=seq, psh_offset=psh_offset, ip_id=ip_id,
             flags=flags, reserved=tuple(reserved), hdr=hdr if hdr is not None else template())
    if give is not None:
        c["give"] = tuple(give)
    return c


class Batch:
    def __init__(self, cases, payload):
        self.cases, self.payload = cases, payload


def payload_bytes(n=1 << 16, seed=11):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


# ---- the model ----------------------------------------------------------------------------

def descriptor_ok(c):
    """The burst contract, the part a descriptor alone decides (chksum.h)."""
    h = c["hdr"]
    D = c["pieces"][0][1] + c["pieces"][1][1]
    return (1 <= c["mss"] <= 65535 - 40 and D < 2 ** 32 and tuple(c["reserved"]) == (0, 0, 0)
            and (c["flags"] & ~FIN) == 0 and h[12:14] == b"\x08\x00" and h[14] == 0x45
            and h[23] == 6)


def segments_of(c):
    """[(start, len, [(payload offset, length) chunks])] of a burst (:1069-1090): the data in mss
    steps; a FIN alone is one segment without data; nothing otherwise."""
    (o0, l0), (o1, l1) = c["pieces"]
    D, mss = l0 + l1, c["mss"]
    if D == 0:
        return [(0, 0, [])] if c["flags"] & FIN else []
    out = []
    start = 0
    while start < D:
        ln = min(mss, D - start)
        chunks = []
        if start < l0:                                   # bytes of piece 0
            chunks.append((o0 + start, min(ln, l0 - start)))
        if start + ln > l0:                              # bytes of piece 1
            s1 = max(start, l0)
            chunks.append((o1 + s1 - l0, start + ln - s1))
        out.append((start, ln, chunks))
        start += ln
    return out


def be_words(b):
    b = bytes(b)
    if len(b) & 1:
        b += b"\x00"
    return sum((b[i] << 8) | b[i + 1] for i in range(0, len(b), 2))


def fold_not(s):
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def segment_fields(c, k, start, ln, last):
    """(seq_num, offset_flags, ident, IPv4 total length) of segment k (:1079-1102, IpStack.h:653)."""
    fl = 0x5000 | 0x10                                   # Tcp4EncodeOffset(5) | Ack
    if (c["flags"] & FIN) and last:
        fl |= 0x01 | 0x08                                # Fin|Psh
    psh = c["psh_offset"]
    if start < psh <= start + ln:                        # InOpenClosedIntervalStartLen
        fl |= 0x08
    return (c["seq"] + start) & 0xFFFFFFFF, fl, (c["ip_id"] + k) & 0xFFFF, 40 + ln


def segment_header(oracle, c, payload, k, start, ln, chunks, last):
    """The 54 header bytes of segment k: the template with the six fields written; checksums by
    the CPU oracle over the bytes they cover."""
    seq, fl, ident, tot = segment_fields(c, k, start, ln, last)
    h = bytearray(c["hdr"][:HDR])
    struct.pack_into(">H", h, 16, tot)
    struct.pack_into(">H", h, 18, ident)
    struct.pack_into(">H", h, 24, 0)
    struct.pack_into(">I", h, 38, seq)
    struct.pack_into(">H", h, 46, fl)
    struct.pack_into(">H", h, 50, 0)
    ip = np.frombuffer(bytes(h[14:34]), dtype=np.uint8).copy()
    struct.pack_into(">H", h, 24, oracle.final(ip, 0, 20))
    data = b"".join(payload[o:o + l].tobytes() for o, l in chunks)
    pseudo = bytes(h[26:34]) + struct.pack(">HH", 6, 20 + ln)
    cover = np.frombuffer(pseudo + bytes(h[34:54]) + data, dtype=np.uint8).copy()
    struct.pack_into(">H", h, 50, oracle.final(cover, 0, cover.size))   # 0 stays 0 (TCP)
    return bytes(h)


def model_layout(cases):
    """(seg_index, chunk_base) as aipstack_tcp_burst_layout must give them, or None if a burst
    breaks the contract."""
    si, cb = [0], [0]
    for c in cases:
        if not descriptor_ok(c):
            return None
        segs = segments_of(c)
        si.append(si[-1] + len(segs))
        cb.append(cb[-1] + sum(len(ch) for _, _, ch in segs))
    return np.array(si, dtype=np.uint64), np.array(cb, dtype=np.uint64)


def caller_index(cases):
    """The index a caller hands over: the model's counts, and for a burst with ``give`` (one
    that breaks the contract, or whose counts are made to disagree) those counts."""
    si, cb = [0], [0]
    for c in cases:
        if "give" in c:
            ns, nc = c["give"]
        else:
            segs = segments_of(c)
            ns, nc = len(segs), sum(len(ch) for _, _, ch in segs)
        si.append(si[-1] + ns)
        cb.append(cb[-1] + nc)
    return np.array(si, dtype=np.uint64), np.array(cb, dtype=np.uint64)


class Expected:
    """What aipstack_tcp_tx_segment must leave: ``headers`` ((n, 54) bytes, rows of invalid
    segments unused), ``status``, ``chunk_off`` (payload offsets; -1 = address 0),
    ``chunk_len``, ``chunk_index``, ``seg_case`` (burst of each segment), ``seg_k``,
    ``seg_flags`` (offset_flags), ``seg_chunks``."""


def expected(oracle, batch, seg_index=None, chunk_base=None):
    cases, payload = batch.cases, batch.payload
    if seg_index is None:
        seg_index, chunk_base = caller_index(cases)
    n, nc = int(seg_index[-1]), int(chunk_base[-1])
    e = Expected()
    e.headers = np.zeros((n, HDR), dtype=np.uint8)
    e.status = np.full(n, BURST_INVALID, dtype=np.uint8)
    e.chunk_off = np.full(nc, -1, dtype=np.int64)
    e.chunk_len = np.zeros(nc, dtype=np.uint32)
    e.chunk_index = np.zeros(n + 1, dtype=np.uint64)
    e.chunk_index[n] = nc
    e.seg_case = np.zeros(n, dtype=np.int64)
    e.seg_k = np.zeros(n, dtype=np.int64)
    e.seg_flags = np.zeros(n, dtype=np.int64)
    e.seg_chunks = [[] for _ in range(n)]
    for b, c in enumerate(cases):
        s0, ns = int(seg_index[b]), int(seg_index[b + 1] - seg_index[b])
        c0, ncb = int(chunk_base[b]), int(chunk_base[b + 1] - chunk_base[b])
        e.seg_case[s0:s0 + ns] = b
        e.seg_k[s0:s0 + ns] = np.arange(ns)
        segs = segments_of(c) if descriptor_ok(c) else None
        if segs is None or len(segs) != ns or sum(len(ch) for _, _, ch in segs) != ncb:
            # status 10, slots untouched, chunk entries empty; the segments share the entries
            # out in order (chksum.h)
            for k in range(ns):
                e.chunk_index[s0 + k] = c0 + min(k, ncb)
            continue
        at = c0
        for k, (start, ln, chunks) in enumerate(segs):
            i = s0 + k
            e.status[i] = ACCEPT
            e.chunk_index[i] = at
            for o, l in chunks:
                assert l > 0
                e.chunk_off[at], e.chunk_len[at] = o, l
                at += 1
            e.seg_chunks[i] = chunks
            e.seg_flags[i] = segment_fields(c, k, start, ln, k == ns - 1)[1]
            e.headers[i] = np.frombuffer(
                segment_header(oracle, c, payload, k, start, ln, chunks, k == ns - 1), dtype=np.uint8)
        assert at == c0 + ncb
    return e


def descriptors(batch, base_addr, dtype):
    """The aipstack_tcp_burst array of the batch with its payload buffer at `base_addr`."""
    d = np.zeros(len(batch.cases), dtype=dtype)
    for b, c in enumerate(batch.cases):
        for p in (0, 1):
            d["data_addr"][b, p] = base_addr + c["pieces"][p][0]
            d["data_len"][b, p] = c["pieces"][p][1]
        d["seq"][b], d["psh_offset"][b] = c["seq"], c["psh_offset"]
        d["mss"][b], d["ip_id"][b], d["flags"][b] = c["mss"], c["ip_id"], c["flags"]
        d["reserved"][b] = c["reserved"]
        d["hdr"][b] = np.frombuffer(c["hdr"], dtype=np.uint8)
    return d


def linearise(e, payload):
    """The accepted segments as linear frames: (buffer, offsets, their segment numbers)."""
    parts, offs, ids = [], [0], []
    for i in np.nonzero(e.status == ACCEPT)[0]:
        f = e.headers[i].tobytes() + b"".join(payload[o:o + l].tobytes() for o, l in e.seg_chunks[i])
        parts.append(np.frombuffer(f, dtype=np.uint8))
        offs.append(offs[-1] + len(f))
        ids.append(int(i))
    buf = np.concatenate(parts) if parts else np.zeros(1, dtype=np.uint8)
    return buf, np.array(offs, dtype=np.uint64), ids


# ---- properties of a batch, from the model alone (no vacuous tests) -----------------------

def count_straddle_odd_first(e):
    return sum(1 for ch in e.seg_chunks if len(ch) == 2 and ch[0][1] & 1)


def count_flags(e):
    ok = e.status == ACCEPT
    f = e.seg_flags[ok] & 0x3F
    return {"psh_only": int((f == 0x18).sum()), "fin_psh": int((f == 0x19).sum()),
            "neither": int((f == 0x10).sum())}


# ---- case generators ------------------------------------------------------------------------

def sizes_batch():
    """Small mss and data sizes; one burst of 200 segments; FIN shapes; wraps."""
    pay = payload_bytes()
    cs = []
    for D in (1, 2, 3):
        cs.append(burst((100 + D, D), mss=1, ip_id=D))
    at = 1
    for mss in (536, 1460):
        for k in (1, 2, 3):
            for D in (mss * k - 1, mss * k, mss * k + 1):
                cs.append(burst((at, D), mss=mss, seq=0x10000000 + at, ip_id=at & 0xFFFF))
                at += 3
    cs.append(burst((7, 200 * 97 - 5), mss=97, psh_offset=200 * 97 - 5))   # 200 segments
    cs.append(burst((0, 0), flags=FIN))                                   # FIN only
    cs.append(burst((33, 1000), mss=400, flags=FIN))                      # FIN with data
    cs.append(burst((35, 1200), mss=400, flags=FIN))                      # FIN, last segment full
    cs.append(burst((9, 3 * 1460), ip_id=0xFFFE))                         # ident wraps
    cs.append(burst((11, 2 * 1460), seq=0xFFFFFF00))                      # seq wraps
    return Batch(cs, pay)


def one_segment_bursts(n):
    pay = payload_bytes()
    return Batch([burst((3 * b + (b & 1), 1 + (b * 37) % 700), mss=700, seq=b * 1000, ip_id=b,
                        psh_offset=(b % 3) * 5) for b in range(n)], pay)


def zero_segment_batch():
    """Bursts of no segment first, last and in runs between others."""
    pay = payload_bytes()
    z = lambda: burst((0, 0))                                             # noqa: E731
    cs = [z(), z(), burst((1, 3000)), z(), z(), z(), burst((5, 100), mss=50), z(),
          burst((0, 0), flags=FIN), z(), z()]
    cs += [burst((2 * b, 600), mss=256) for b in range(40)]
    cs += [z() for _ in range(70)]
    cs += [burst((9, 64 * 40), mss=40), z(), z()]
    return Batch(cs, pay)


def boundary_batch(mss=100):
    """The piece boundary at every offset of a 3-segment burst (D = 3*mss - 7), pieces at odd
    addresses and far apart; data_len[0] == 0 and data_len[1] == 0 included."""
    pay = payload_bytes()
    D = 3 * mss - 7
    cs = []
    for l0 in range(0, D + 1):
        cs.append(burst((1001 + (l0 % 3), l0), (30001 + (l0 % 2), D - l0), mss=mss, seq=l0 * 7919,
                        ip_id=l0, psh_offset=l0))
    return Batch(cs, pay)


def psh_batch():
    """psh_offset at 0, start, start + 1, start + len, start + len + 1, D and beyond D, for every
    segment of a burst with a short last segment; with and without FIN."""
    pay = payload_bytes()
    mss, D = 300, 3 * 300 - 120
    offs = {0, D, D + 1, D + 1000}
    for k in range(3):
        start, ln = k * mss, min(mss, D - k * mss)
        offs |= {start, start + 1, start + ln, start + ln + 1}
    cs = []
    for fl in (0, FIN):
        for p in sorted(offs):
            cs.append(burst((17, D), mss=mss, psh_offset=p, flags=fl, ip_id=p))
    return Batch(cs, pay)


def zero_tcp_checksum_batch(oracle):
    """Segments whose TCP checksum comes out 0x0000: the last two payload bytes of each (an even
    length, at its own place in the buffer) are patched to the value that completes the sum."""
    pay = payload_bytes().copy()
    cs = []
    for j, (ln, odd_addr) in enumerate(((2, 0), (100, 1), (1460, 0))):
        o = 5000 * (j + 1) + odd_addr
        c = burst((o, ln), mss=1460, seq=0x777 * (j + 1), ip_id=j)
        pay[o + ln - 2:o + ln] = 0
        h = segment_header(oracle, c, pay, 0, 0, ln, [(o, ln)], True)
        chk = struct.unpack_from(">H", h, 50)[0]
        pay[o + ln - 2], pay[o + ln - 1] = chk >> 8, chk & 0xFF
        cs.append(c)
    cs.insert(1, burst((1, 500)))
    return Batch(cs, pay)


def zero_ip_checksum_batch(oracle):
    """Segments whose IPv4 header checksum comes out 0x0000 (the header's sum is 0xFFFF), by the
    choice of ip_id. A sum of 0 (checksum 0xFFFF) cannot occur: the version/IHL byte is not 0."""
    pay = payload_bytes()
    cs = []
    for j, ln in enumerate((1, 700, 1460)):
        c = burst((300 * j, ln), ip_id=0, hdr=template(src=0x0A000001 + 77 * j))
        h = segment_header(oracle, c, pay, 0, 0, ln, [(300 * j, ln)], True)
        c["ip_id"] = struct.unpack_from(">H", h, 24)[0]   # ident 0 -> c; ident c -> sum 0xFFFF
        cs.append(c)
    cs.append(burst((2, 2000)))
    return Batch(cs, pay)


INVALID_CLASSES = ["mss0", "mss_big", "reserved", "flags", "ethertype", "vihl", "proto", "d_2_32"]


def invalid_case(cls):
    """A burst of the given invalid class; the caller's index gives it 2 segments, 3 chunks."""
    kw, hdr = {}, bytearray(template())
    p0, p1 = (40, 500), (0, 0)
    if cls == "mss0":
        kw["mss"] = 0
    elif cls == "mss_big":
        kw["mss"] = 65535 - 39
    elif cls == "reserved":
        kw["reserved"] = (0, 1, 0)
    elif cls == "flags":
        kw["flags"] = 2 | FIN
    elif cls == "ethertype":
        hdr[12:14] = b"\x86\xdd"
    elif cls == "vihl":
        hdr[14] = 0x46
    elif cls == "proto":
        hdr[23] = 17
    elif cls == "d_2_32":
        p0, p1 = (0, 0xFFFFFFFF), (0, 1)
        kw["mss"] = 65000
    return burst(p0, p1, hdr=bytes(hdr), give=(2, 3), **kw)


def invalid_batch():
    """An invalid burst of each class between valid ones (one of them straddling)."""
    pay = payload_bytes()
    cs = [burst((1, 2000), (4001, 999), mss=700, flags=FIN)]
    for j, cls in enumerate(INVALID_CLASSES):
        cs.append(invalid_case(cls))
        cs.append(burst((50 * j + 1, 900 + j), (9000 + j, 300), mss=512, ip_id=j, psh_offset=600))
    return Batch(cs, pay)


def mismatch_batch():
    """Valid descriptors whose caller-given counts disagree: too few / too many segments, too few
    / too many chunks, no segment but chunks; valid neighbours."""
    pay = payload_bytes()
    good = lambda j: burst((10 * j + 1, 1000), (7001, 200), mss=300, ip_id=j)   # noqa: E731
    three = dict(mss=500)                                                      # 3 segs, 3 chunks
    cs = [good(0), burst((1, 1500), give=(2, 3), **three), good(1),
          burst((1, 1500), give=(5, 3), **three), good(2),
          burst((1, 1500), give=(3, 2), **three), good(3),
          burst((1, 1500), give=(3, 6), **three), good(4),
          burst((1, 1500), give=(0, 2), **three), good(5)]
    return Batch(cs, pay)


def multipass_batch(n):
    """Exactly n segments from the ingredients of boundary_batch (three bursts and more per
    wave), invalid_batch (bursts that break the contract), three bursts of 100 segments (waves
    of two bursts) and sizes_batch (one burst of 200 segments: waves of one burst), in that
    order, each burst taken if it still fits; one-segment bursts make up the rest."""
    pay = payload_bytes()
    cs, total = [], 0
    hundred = [burst((3 + j, 100 * 97 - j), mss=97, seq=0xFFFFF000, ip_id=0xFFC0 + j) for j in range(3)]
    for c in boundary_batch().cases + invalid_batch().cases + hundred + sizes_batch().cases:
        ns = c["give"][0] if "give" in c else len(segments_of(c))
        if total + ns <= n:
            cs.append(c)
            total += ns
    cs += one_segment_bursts(n - total).cases
    return Batch(cs, pay)


def burst_loop_batch(n_bad=700):
    """One valid one-segment burst, then `n_bad` bursts that break the contract while owning
    chunk entries but no segment: invalid_case of every class (3 entries each) in turn with
    valid descriptors whose index gives them no segment and 2 entries."""
    cs = [burst((5, 700), mss=1460, ip_id=77)]
    for j in range(n_bad):
        if j & 1:
            cs.append(burst((10 * j + 1, 1500), mss=500, ip_id=j, give=(0, 2)))
        else:
            c = invalid_case(INVALID_CLASSES[(j // 2) % len(INVALID_CLASSES)])
            c["give"] = (0, 3)
            cs.append(c)
    return Batch(cs, payload_bytes())
