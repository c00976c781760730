"""TEST INFRASTRUCTURE -- shared by test_ipreass_host.py, test_gpu_ipreass.py and the random
scenarios: two models of IPv4 reassembly on receive and the case generators.

1. ``model``: the declarative semantics of aipstack_ip4_rx_reassemble (chksum.h), written
   independently of the kernels: the frame oracle's Rx verify per frame, then group the
   fragments by key, sort by offset, test completeness, judge the linearised payload.
2. ``HoleReassembler``: a plain Python restatement of IpReassembly::reassembleIp4
   (ip/IpReassembly.h:181-386), the RFC 815 hole list, with ample entries and holes and no expiry.
   test_ipreass_host.py feeds it every batch in batch order: every group ``model`` completes, it
   completes too, with the same bytes; it is pinned against answers recorded from code compiled
   from the reference (tests/golden/ip_reass_ref_cases.json).

A batch is a list of frames (bytes). Fragment trains of the project's own sender come from
ipfrag_cases (``train``): what the project sends is what it receives.
"""
import struct

import numpy as np

import ipfrag_cases as F

NOT_IP4, IP_MALFORMED, IP_CHKSUM, FRAGMENT, L4_MALFORMED, L4_CHKSUM = 0, 1, 2, 3, 4, 5
ACCEPT, NO_CHKSUM, OTHER = 6, 7, 8
MEMBER, DROP_FRAG, TRUNCATED = 14, 15, 16
NONE = 0xFFFFFFFF
MAX_REASS = 65531
MAX_STEPS = 8192

DGRAM_DTYPE = np.dtype({
    "names": ["n_frags", "last_frame", "data_len", "proto", "verdict", "reserved"],
    "formats": ["<u4", "<u4", "<u2", "u1", "u1", "<u4"],
    "offsets": [0, 4, 8, 10, 11, 12], "itemsize": 16})

ETH = F.PEER_MAC + F.LOCAL_MAC + b"\x08\x00"


# ---- checksums in plain Python ------------------------------------------------------------

def wsum(data, init=0):
    """Ones'-complement sum (folded to 16 bits) of big-endian words; an odd tail is zero-padded."""
    if len(data) & 1:
        data = data + b"\0"
    s = init + int(np.frombuffer(data, dtype=">u2").astype(np.uint64).sum())
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def pseudo(src, dst, proto, length):
    return wsum(struct.pack(">IIHH", src, dst, proto, length))


# ---- frames ---------------------------------------------------------------------------------

def ip_frame(src, dst, ident, proto, flags_off, payload, *, ihl=5, ttl=64, pad=0, total=None):
    """An Ethernet frame with a good IPv4 header (ihl > 5: NOP options) around `payload`."""
    hl = 4 * ihl
    total = hl + len(payload) if total is None else total
    h = bytearray(struct.pack(">BBHHHBBHII", 0x40 | ihl, 0, total, ident, flags_off, ttl, proto, 0,
                              src, dst) + b"\x01" * (hl - 20))
    struct.pack_into(">H", h, 10, ~wsum(bytes(h)) & 0xFFFF)
    return ETH + bytes(h) + payload + b"\xEE" * pad


def udp_body(src, dst, sport, dport, data, *, ulen=None, chk=None):
    ulen = 8 + len(data) if ulen is None else ulen
    body = bytearray(struct.pack(">HHHH", sport, dport, ulen, 0) + data)
    if chk is None:
        chk = ~wsum(bytes(body[:ulen]), pseudo(src, dst, 17, ulen)) & 0xFFFF or 0xFFFF
    struct.pack_into(">H", body, 6, chk)
    return bytes(body)


def tcp_body(src, dst, sport, dport, data, *, doff=5):
    body = bytearray(struct.pack(">HHIIHHHH", sport, dport, 1000, 2000, doff << 12 | 0x10, 4096, 0, 0)
                     + b"\x01" * (4 * doff - 20) + data)
    struct.pack_into(">H", body, 16, ~wsum(bytes(body), pseudo(src, dst, 6, len(body))) & 0xFFFF)
    return bytes(body)


def icmp_body(data):
    body = bytearray(struct.pack(">BBHHH", 8, 0, 0, 7, 9) + data)
    struct.pack_into(">H", body, 2, ~wsum(bytes(body)) & 0xFFFF)
    return bytes(body)


def cut(body, cuts):
    """[(offset, bytes, MF)] of `body` cut at the byte positions `cuts` (multiples of 8)."""
    edges = [0] + list(cuts) + [len(body)]
    return [(a, body[a:b], b != len(body)) for a, b in zip(edges, edges[1:])]


def frag_frames(src, dst, ident, proto, pieces, **kw):
    """One frame per (offset, bytes, MF) piece."""
    return [ip_frame(src, dst, ident, proto, (0x2000 if mf else 0) | off // 8, data, **kw)
            for off, data, mf in pieces]


def train(oracle, cases, payload=None):
    """The frames the project's own UDP send emits for the ipfrag_cases datagrams `cases`
    (the model of ipfrag_cases: headers and payload chunks joined)."""
    payload = F.payload_bytes() if payload is None else payload
    e = F.expected(oracle, F.Batch(cases, payload))
    return [[F.frame_of(e, payload, int(i)) for i in np.nonzero((e.frag_case == d) & (e.status == F.ACCEPT))[0]]
            for d in range(len(cases))]


def whole_frames(rng, n):
    """n unfragmented frames: accepted TCP / UDP / ICMP, UDP without checksum, another protocol,
    and rejected ones (bad IPv4 checksum, bad TCP checksum, ARP, a runt)."""
    out = []
    for j in range(n):
        src, dst = int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 32))
        data = rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8).tobytes()
        k = j % 11
        if k == 0:
            f = ip_frame(src, dst, j, 6, 0, tcp_body(src, dst, 80, 1024 + j, data))
        elif k == 1:
            f = ip_frame(src, dst, j, 17, 0x4000, udp_body(src, dst, 53, j, data))
        elif k == 2:
            f = ip_frame(src, dst, j, 1, 0, icmp_body(data))
        elif k == 3:
            f = ip_frame(src, dst, j, 17, 0, udp_body(src, dst, 53, j, data, chk=0))
        elif k == 4:
            f = ip_frame(src, dst, j, 47, 0, data)
        elif k == 5:
            f = bytearray(ip_frame(src, dst, j, 6, 0, tcp_body(src, dst, 80, j, data)))
            f[24] ^= 0x40
            f = bytes(f)
        elif k == 6:
            f = bytearray(ip_frame(src, dst, j, 6, 0, tcp_body(src, dst, 80, j, data + b"x")))
            f[-1] ^= 1
            f = bytes(f)
        elif k == 9:
            f = ETH + b"\x45" * 10
        elif k == 10:
            f = ip_frame(src, dst, j, 6, 0, data[:10])
        elif k == 7:
            f = F.PEER_MAC + F.LOCAL_MAC + b"\x08\x06" + data[:28].ljust(28, b"\0")
        else:
            f = ETH[:int(rng.integers(0, 14))]
        out.append(f)
    return out


class Batch:
    """Frames back to back in a buffer that ends at the last frame's last byte."""

    def __init__(self, frames):
        self.frames = list(frames)
        self.offsets = np.zeros(len(self.frames) + 1, dtype=np.uint64)
        self.offsets[1:] = np.cumsum([len(f) for f in self.frames])
        self.buf = np.frombuffer(b"".join(self.frames), dtype=np.uint8).copy()
        if self.buf.size == 0:
            self.buf = np.zeros(0, dtype=np.uint8)

    @property
    def n(self):
        return len(self.frames)

    def permuted(self, perm):
        return Batch([self.frames[int(p)] for p in perm])


# ---- 1. the declarative model ---------------------------------------------------------------

def parse_fragment(f):
    """The fields ip/IpStack.h:1021-1034 takes from a frame Rx verify called a fragment."""
    hl = (f[14] & 0xF) * 4
    total, ident, fo, ttl, proto = struct.unpack_from(">HHHBB", f, 16)
    src, dst = struct.unpack_from(">II", f, 26)
    return dict(key=(src, dst, ident, proto), src=src, dst=dst, ident=ident, proto=proto, ttl=ttl,
                off=8 * (fo & 0x1FFF), mf=bool(fo & 0x2000), poff=14 + hl,
                data=f[14 + hl:14 + total], header=f[14:34])


def dgram_verdict(proto, src, dst, body):
    L = len(body)
    if proto == 6:
        if L < 20:
            return L4_MALFORMED
        return ACCEPT if wsum(body, pseudo(src, dst, 6, L)) == 0xFFFF else L4_CHKSUM
    if proto == 17:
        if L < 8:
            return L4_MALFORMED
        ulen, chk = struct.unpack_from(">HH", body, 4)
        if ulen < 8 or ulen > L:
            return L4_MALFORMED
        if chk == 0:
            return NO_CHKSUM
        if ulen < L:
            return TRUNCATED
        return ACCEPT if wsum(body, pseudo(src, dst, 17, ulen)) == 0xFFFF else L4_CHKSUM
    if proto == 1:
        if L < 8:
            return L4_MALFORMED
        return ACCEPT if wsum(body) == 0xFFFF else L4_CHKSUM
    return OTHER


class Expected:
    """``verdict``, ``chunk_off`` (payload offset in its frame; -1 = address 0), ``chunk_len``,
    ``next``, ``head``, ``dgram`` (DGRAM_DTYPE) per frame; ``groups``: key -> frame indices in
    batch order; ``complete``: key -> frame indices in offset order; ``body``: key -> the
    reassembled bytes; ``frags``: frame index -> parsed fields."""


def model(oracle, batch, max_reass=MAX_REASS):
    n = batch.n
    e = Expected()
    e.verdict = (oracle.rx_verify_batch(batch.buf if batch.buf.size else np.zeros(1, np.uint8),
                                        batch.offsets) if n else np.zeros(0, np.uint8)).copy()
    e.chunk_off = np.full(n, -1, dtype=np.int64)
    e.chunk_len = np.zeros(n, dtype=np.uint32)
    e.next = np.full(n, NONE, dtype=np.uint32)
    e.head = np.full(n, NONE, dtype=np.uint32)
    e.dgram = np.zeros(n, dtype=DGRAM_DTYPE)
    e.groups, e.complete, e.body, e.frags = {}, {}, {}, {}
    for i in np.nonzero(e.verdict == FRAGMENT)[0]:
        i = int(i)
        p = parse_fragment(batch.frames[i])
        e.frags[i] = p
        if not p["data"]:
            e.verdict[i] = DROP_FRAG
            continue
        e.groups.setdefault(p["key"], []).append(i)
    for key, members in e.groups.items():
        fr = e.frags
        over = [i for i in members
                if not (fr[i]["off"] <= max_reass and len(fr[i]["data"]) <= max_reass - fr[i]["off"])]
        order = sorted(members, key=lambda i: fr[i]["off"])
        ok = not over and fr[order[0]]["off"] == 0
        for a, b in zip(order, order[1:]):
            ok = ok and fr[b]["off"] == fr[a]["off"] + len(fr[a]["data"]) and fr[a]["mf"]
        ok = ok and not fr[order[-1]]["mf"]
        for i in members:
            if i in over:
                e.verdict[i] = DROP_FRAG
            else:
                e.chunk_off[i], e.chunk_len[i] = fr[i]["poff"], len(fr[i]["data"])
        if not ok:
            continue
        assert len(order) >= 2
        body = b"".join(fr[i]["data"] for i in order)
        e.complete[key], e.body[key] = order, body
        for a, b in zip(order, order[1:] + [NONE]):
            e.verdict[a], e.head[a], e.next[a] = MEMBER, order[0], b
        src, dst, _, proto = key
        e.dgram[order[0]] = (len(order), order[-1], len(body), proto,
                             dgram_verdict(proto, src, dst, body), 0)
    return e


def linearised(batch, e, key):
    """The complete group `key` as one frame: the head's Ethernet and base IPv4 header with the
    total length, flags / offset and checksum rewritten, then the reassembled payload; None if it
    does not fit 16 bits of total length."""
    body = e.body[key]
    if 20 + len(body) > 65535:
        return None
    src, dst, ident, proto = key
    return ip_frame(src, dst, ident, proto, 0, body)


# ---- 2. the hole algorithm, restated ----------------------------------------------------------

class HoleReassembler:
    """IpReassembly::reassembleIp4 (ip/IpReassembly.h:181-386) with one entry per key, any number
    of holes, no expiry. ``feed`` returns the reassembled bytes when the call returns true."""
    NULL = 0xFFFF
    HOLE = 4                                            # HoleDescriptor::Size

    def __init__(self, max_reass=MAX_REASS, max_holes=None):
        self.max, self.size = max_reass, max_reass + self.HOLE
        self.max_holes = max_holes
        self.entries = {}

    def feed(self, key, mf, off, data):
        assert mf or off > 0
        if len(data) == 0:                                                  # :189-191
            return None
        r = self.entries.get(key)
        if r is None:                                                       # :197-215
            r = dict(first=0, length=0, data=bytearray(self.size), holes={0: [self.size, self.NULL]})
            self.entries[key] = r
        done = self._update(r, mf, off, data)
        if done is not True:
            if done is False:                                               # invalidate_reass
                del self.entries[key]
            return None
        del self.entries[key]                                               # :373
        return bytes(r["data"][:r["length"]])

    def _update(self, r, mf, off, data):
        """True: complete; None: stored, incomplete; False: invalidate."""
        if off > self.max or len(data) > self.max - off:                   # :219-223
            return False
        end = off + len(data)
        if not mf:                                                          # :237-250
            if r["length"] != 0 and end != r["length"]:
                return False
            r["length"] = end
        elif r["length"] != 0 and end > r["length"]:
            return False
        holes = r["holes"]

        def link(prev, to):                                                 # reass_link_prev
            if prev == self.NULL:
                r["first"] = to
            else:
                holes[prev][1] = to

        prev, h, num = self.NULL, r["first"], 0
        while True:                                                         # :256-337
            size, nxt = holes[h]
            hend = h + size
            if not mf and h > end:                                          # :274
                return False
            if off >= hend or end <= h:                                     # :279
                prev, h = h, nxt
                num += 1
            else:
                del holes[h]
                if off > h:                                                 # :290-309
                    if off - h < self.HOLE:
                        return False
                    holes[h] = [off - h, nxt]
                    prev = h
                    num += 1
                if end < hend:                                              # :312-330
                    if hend - end < self.HOLE:
                        return False
                    holes[end] = [hend - end, self.NULL]
                    link(prev, end)
                    prev = end
                    num += 1
                link(prev, nxt)                                             # :333
                h = nxt
            if h == self.NULL:
                break
        r["data"][off:end] = data                                           # :343-346
        if r["length"] == 0 or r["first"] < r["length"]:                    # :350-356
            if self.max_holes is not None and num > self.max_holes:
                return False
            return None
        assert r["first"] == r["length"]
        return True


def feed_batch(batch, e, max_reass=MAX_REASS):
    """Every fragment of the batch (by the verify verdict, whatever the call made of it) fed to a
    HoleReassembler in batch order: {key: [(frame index of the completing call, bytes)]}."""
    h = HoleReassembler(max_reass)
    out = {}
    for i in sorted(e.frags):
        p = e.frags[i]
        got = h.feed(p["key"], p["mf"], p["off"], p["data"])
        if got is not None:
            out.setdefault(p["key"], []).append((i, got))
    return out


# ---- the hash of ipreass_common.h, restated (for crafted collisions) --------------------------

M32 = 0xFFFFFFFF


def _mix(h):
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ h >> 16


def _rotl13(h):
    return (h << 13 | h >> 19) & M32


def hash_key(src, dst, ident, proto):
    h = src * 0x9E3779B1 & M32
    h = _rotl13(h) ^ (dst * 0x85EBCA77 & M32)
    h = _rotl13(h) ^ ((ident | proto << 16) * 0xC2B2AE3D & M32)
    return _mix(h)


def hash_key_off(src, dst, ident, proto, off):
    return _mix((hash_key(src, dst, ident, proto) + off * 0x27D4EB2F + 1) & M32)


def table_slots(n):
    s = 64
    while s < 4 * n:
        s <<= 1
    return s


def colliding_batch(n_keys=64, frags=3):
    """n_keys complete datagrams (protocols without an L4 checksum) whose keys share one home slot
    of the key table this very batch gets: among them keys that differ only in ident and two that
    differ only in proto; and one more datagram cut at two offsets whose (key, offset) entries
    share a home slot of the other table (entries that differ only in offset)."""
    src, dst = 0x0A010203, 0x0A040506
    n = n_keys * frags + 3
    mask = table_slots(n) - 1
    protos = (47, 253, 254, 99)
    base = None
    for x in range(1, 65536):                                   # two keys that differ only in proto
        for q in range(100, 250):
            if hash_key(src, dst, x, q) & mask == hash_key(src, dst, x, 47) & mask:
                base = (x, q)
                break
        if base:
            break
    want = hash_key(src, dst, base[0], 47) & mask
    keys = [(base[0], 47), base]
    for idn in range(1, 65536):
        for q in protos:
            if len(keys) < n_keys and (idn, q) not in keys and hash_key(src, dst, idn, q) & mask == want:
                keys.append((idn, q))
    assert len(keys) == n_keys == len(set(keys))
    assert len({q for _, q in keys}) >= 2 and sum(q == 47 for _, q in keys) >= 2
    frames = []
    for j, (idn, proto) in enumerate(keys):
        body = bytes([(j + k) & 0xFF for k in range(8 * frags - 3)])
        frames += frag_frames(src, dst, idn, proto, cut(body, range(8, 8 * frags, 8)))
    seen, pair = {}, None
    for off in range(8, 4096, 8):                               # entries that differ only in offset
        h = hash_key_off(src, dst, 7, 47, off) & mask
        if h in seen:
            pair = (seen[h], off)
            break
        seen[h] = off
    body = bytes(k * 7 & 0xFF for k in range(pair[1] + 5))
    frames += frag_frames(src, dst, 7, 47, cut(body, pair))
    assert len(frames) == n
    return frames, keys, want


# ---- crafted groups: one per branch -----------------------------------------------------------

A_, B_ = 0xC0A80001, 0xC0A80002


def crafted(max_reass=MAX_REASS):
    """[(name, frames, what)]: `what` = the datagram verdict the model must give the group, or
    None for a group that must stay incomplete. Every group has its own ident."""
    rng = np.random.default_rng(5)
    data = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()   # noqa: E731
    out = []
    ident = [100]

    def add(name, proto, body, cuts, what, edit=None, **kw):
        ident[0] += 1
        pieces = cut(body, cuts)
        if edit:
            pieces = edit(pieces)
        out.append((name, frag_frames(A_, B_, ident[0], proto, pieces, **kw), what))

    u = lambda k, **kw: udp_body(A_, B_, 7, 9, data(k), **kw)           # noqa: E731
    add("udp_ok", 17, u(100), [40, 80], ACCEPT)
    add("udp_reversed", 17, u(100), [40, 80], ACCEPT, edit=lambda p: p[::-1])
    add("missing_first", 17, u(100), [40, 80], None, edit=lambda p: p[1:])
    add("missing_middle", 17, u(100), [40, 80], None, edit=lambda p: [p[0], p[2]])
    add("missing_last", 17, u(100), [40, 80], None, edit=lambda p: p[:2])
    add("duplicate", 17, u(100), [40, 80], None, edit=lambda p: p + [p[1]])
    add("overlap", 17, u(100), [40, 80], None,
        edit=lambda p: p + [(32, b"\x55" * 16, True)])
    add("extra_past_end", 17, u(100), [40, 80], None,
        edit=lambda p: p + [(200, b"\x55" * 8, False)])
    add("two_dgrams_one_key", 17, u(100), [40, 80], None, edit=lambda p: p + p)
    add("empty_fragment", 17, u(100), [40, 80], ACCEPT,
        edit=lambda p: p + [(16, b"", True)])
    add("lone_mf", 17, u(100), [], None, edit=lambda p: [(0, p[0][1], True)])
    add("lone_tail", 17, u(100), [], None, edit=lambda p: [(48, p[0][1], False)])
    add("corrupt_middle", 17, u(100), [40, 80], L4_CHKSUM,
        edit=lambda p: [p[0], (p[1][0], bytes([p[1][1][0] ^ 1]) + p[1][1][1:], True), p[2]])
    add("udp_chk0", 17, u(100, chk=0), [40], NO_CHKSUM)
    b = bytearray(u(98))
    b[-2:] = b"\0\0"
    b[6:8] = b"\0\0"
    fix = 0xFFFF - wsum(bytes(b), pseudo(A_, B_, 17, len(b)))          # the data makes the sum 0xFFFF
    b[-2:] = struct.pack(">H", fix)
    b[6:8] = b"\xFF\xFF"                                                # ... so the field is 0 -> 0xFFFF
    add("udp_ffff", 17, bytes(b), [40], ACCEPT)
    add("udp_len_short", 17, u(100, ulen=60), [40], TRUNCATED)
    add("udp_len_long", 17, u(100, ulen=109), [40], L4_MALFORMED)
    add("udp_len_below_8", 17, u(100, ulen=7), [40], L4_MALFORMED)
    add("tcp_ok", 6, tcp_body(A_, B_, 80, 5000, data(300)), [160], ACCEPT)
    flip = lambda b: b[:-1] + bytes([b[-1] ^ 1])                        # noqa: E731
    add("tcp_bad", 6, flip(tcp_body(A_, B_, 80, 5000, data(300))), [160], L4_CHKSUM)
    add("tcp_below_20", 6, b"\x11" * 19, [8, 16], L4_MALFORMED)
    add("tcp_header_8", 6, tcp_body(A_, B_, 80, 5001, data(50), doff=7), [8, 16, 24, 32], ACCEPT)
    add("tcp_header_16", 6, tcp_body(A_, B_, 80, 5002, data(51)), [16, 32], ACCEPT)
    add("icmp_ok", 1, icmp_body(data(77)), [24, 48], ACCEPT)
    add("icmp_bad", 1, flip(icmp_body(data(77))), [24, 48], L4_CHKSUM)
    add("proto_47", 47, data(99), [32], OTHER)
    add("ihl_6", 17, u(100), [40, 80], ACCEPT, ihl=6)
    add("ihl_15", 17, u(100), [40, 80], ACCEPT, ihl=15)
    add("padded", 17, u(20), [8], ACCEPT, pad=18)
    # both sides of max_reass_size (the default, 65531): a last fragment that ends exactly at it,
    # one byte past it, and an offset past it
    big = data(MAX_REASS)
    cuts = sorted(set(range(8000, max_reass - 8, 8000)) | {max_reass - 3 & ~7})
    add("ends_at_max", 47, big[:max_reass], cuts, OTHER)
    add("ends_past_max", 47, big[:max_reass] + b"\x01", cuts, None)
    if max_reass + 8 <= 65528:
        add("offset_past_max", 47, data(40), [16], None,
            edit=lambda p: p + [((max_reass + 8) & ~7, b"\x01" * 8, False)])
    return out


SMALL_MAX = 104


def crafted_small_max():
    """Groups against max_reass_size = SMALL_MAX: offset and length on both sides of it."""
    rng = np.random.default_rng(6)
    d = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()     # noqa: E731
    mk = lambda idn, pieces: frag_frames(A_, B_, idn, 47, pieces)       # noqa: E731
    return [("len_at_max", mk(1, cut(d(104), [96])), OTHER),
            ("len_past_max", mk(2, cut(d(105), [96])), None),
            ("off_at_max", mk(3, [(0, d(104), True), (104, d(1), False)]), None),
            ("off_past_max", mk(4, [(0, d(96), True), (112, d(1), False)]), None),
            ("off_below_max", mk(5, [(0, d(96), True), (96, d(1), False)]), OTHER)]


def alignment_batch():
    """Sixteen complete UDP datagrams whose fragments start at every byte alignment 0-15: runt
    frames of 0..15 bytes shift what follows."""
    rng = np.random.default_rng(8)
    frames, at = [], 0
    for a in range(16):
        data = rng.integers(0, 256, 61 + a, dtype=np.uint8).tobytes()
        frames.append(b"\0" * ((a - (at + 34)) % 16))           # the next payload starts at a mod 16
        frames += frag_frames(A_ + a, B_, a, 17, cut(udp_body(A_ + a, B_, 1, 2, data), [24, 48]))
        at = sum(len(f) for f in frames)
    return frames


# ---- round trips: what the project sends ---------------------------------------------------

def round_trip_batch(oracle, seed=3, small=True):
    """Trains from ipfrag_cases at mtu 256, 257-263, 576 and 1500, D from 0 up, both payload pieces,
    shuffled within and across datagrams, interleaved with whole frames."""
    rng = np.random.default_rng(seed)
    cases = []
    for j, mtu in enumerate((256, 257, 258, 259, 260, 261, 262, 263, 576, 1500)):
        M = mtu - 20
        for D in (0, 1, M - 8, M - 7, 2 * M, 3 * M + 5, 5 * M + 1, 9 * M):
            l0 = int(rng.integers(0, D + 1))
            cases.append(F.dgram((1 + j, l0), (70000 + j, D - l0), mtu=mtu, ip_id=len(cases),
                                 src=0x0A000000 + j, sport=1000 + len(cases)))
    trains = train(oracle, cases)
    frames = [f for t in trains for f in t] + whole_frames(rng, 60)
    perm = rng.permutation(len(frames))
    return [frames[int(p)] for p in perm], cases


def big_datagrams(oracle):
    """One 65,515-byte datagram of 45 fragments (mtu 1500), one datagram of 1,000 eight-byte
    fragments, and D = 65,527 (P = 65,535: past max_reass_size, its tail is oversize)."""
    pay = F.payload_bytes()
    t = train(oracle, [F.dgram((3, 65507), mtu=1500, ip_id=1), F.dgram((1, 65527), mtu=1500, ip_id=2)], pay)
    assert len(t[0]) == 45
    body = udp_body(A_, B_, 5, 6, pay[:7990].tobytes())
    tiny = frag_frames(A_, B_, 3, 17, cut(body, range(8, 8000 - 2, 8)))
    assert len(tiny) == 1000
    return t[0], t[1], tiny


# ---- seeded scenarios --------------------------------------------------------------------------

CAUSES = ("missing_first", "missing_middle", "missing_last", "duplicate", "overlap", "extra",
          "two_dgrams", "oversize", "lone")


class Scenario:
    pass


def scenario(oracle, seed):
    """A mixture: complete groups of every protocol and verdict, incomplete groups of every cause,
    empty fragments, whole frames; shuffled. ``causes``: key -> the cause injected."""
    rng = np.random.default_rng(1000 + seed)
    max_reass = MAX_REASS if seed % 4 else 2000
    groups, causes = [], {}
    n_groups = int(rng.integers(18, 30))
    for g in range(n_groups):
        src, dst = 0x0A000000 + int(rng.integers(1, 50)), 0x0B000000 + int(rng.integers(1, 50))
        ident = g * 7 + seed
        kind = int(rng.integers(0, 8))
        size = int(rng.integers(9, 1200))
        d = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        if kind in (0, 1, 2):
            k2 = int(rng.integers(0, 5))
            kw = ({}, {"chk": 0}, {"ulen": 8 + size // 2}, {"ulen": size + 20}, {"ulen": 3})[k2]
            proto, body = 17, udp_body(src, dst, g, 53, d, **kw)
        elif kind in (3, 4):
            proto, body = 6, tcp_body(src, dst, 80, g, d) if rng.integers(0, 4) else b"\x22" * 17
        elif kind == 5:
            proto, body = 1, icmp_body(d)
        else:
            proto, body = int(rng.choice([47, 50, 253])), d
        if rng.integers(0, 6) == 0 and len(body) > 30:                      # a corrupted byte
            pos = int(rng.integers(8, len(body)))
            body = body[:pos] + bytes([body[pos] ^ 0x10]) + body[pos + 1:]
        ncut = int(rng.integers(1, min(6, max(2, len(body) // 8))))
        cuts = sorted(set(int(c) * 8 for c in rng.integers(1, max(2, (len(body) - 1) // 8 + 1), ncut)
                          if 0 < int(c) * 8 < len(body)))
        if not cuts:
            cuts = [8]
        pieces = cut(body, cuts)
        key = (src, dst, ident, proto)
        if g % 2 == 1 or (max_reass < 3000 and len(body) > max_reass):
            cause = CAUSES[(g // 2 + seed) % len(CAUSES)]
            if len(body) > max_reass:
                cause = "oversize"
            if cause == "missing_first":
                pieces = pieces[1:]
            elif cause == "missing_middle" and len(pieces) >= 3:
                pieces = [pieces[0]] + pieces[2:]
            elif cause == "missing_last" or cause == "missing_middle":
                cause, pieces = "missing_last", pieces[:-1]
            elif cause == "duplicate":
                pieces = pieces + [pieces[int(rng.integers(0, len(pieces)))]]
            elif cause == "overlap":
                pieces = pieces + [(pieces[1][0] - 8, b"\x77" * 16, True)]
            elif cause == "extra":
                pieces = pieces + [(pieces[-1][0] + 64 + (len(pieces[-1][1]) + 7 & ~7), b"\x78" * 5, False)]
            elif cause == "two_dgrams":
                pieces = pieces + cut(body[:-1] + b"\x00", cuts)
            elif cause == "oversize":
                if len(body) <= max_reass:
                    pieces = pieces + [((max_reass + 8) & ~7 if max_reass + 16 < 65528 else 65528,
                                        b"\x79" * 8, False)]
            elif cause == "lone":
                pieces = [(0, pieces[0][1], True)]
            causes[key] = cause
        if rng.integers(0, 5) == 0:                                         # an empty fragment
            pieces = pieces + [(8 * int(rng.integers(0, 50)), b"", True)]
        ihl = 5 if rng.integers(0, 5) else int(rng.integers(6, 16))
        groups.append(frag_frames(src, dst, ident, proto, pieces, ihl=ihl, pad=int(rng.integers(0, 3))))
    if seed % 5 == 0:
        groups += train(oracle, [F.dgram((seed, 700), (70000, 900), mtu=256, ip_id=0xF000 + seed)])
    frames = [f for g in groups for f in g] + whole_frames(rng, int(rng.integers(10, 40)))
    perm = rng.permutation(len(frames))
    s = Scenario()
    s.batch = Batch([frames[int(p)] for p in perm])
    s.max_reass, s.causes = max_reass, causes
    return s


SEEDS = tuple(range(40))
