"""TEST INFRASTRUCTURE -- a Python model of aipstack_tcp_tx_control (send_tcp_nodata with
WriteTcpOptions under sendIp4Dgram, built from plain byte strings and a generic Internet
checksum, independently of the library's word arithmetic) and the builders of its test cases: the
descriptor of a recorded reference frame, the edge set of the options, flags, sequence numbers,
Ident wrap and checksum values, and the invalid descriptors."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import tcp_ctl_ref as R  # noqa: E402

EMITTED, INVALID, MAX_HEADER = 48, 49, 62
OPT_MSS, OPT_WS = 1, 2
FLAGS = (0x02, 0x12, 0x10, 0x19, 0x04, 0x14, 0x00, 0x3F)

# aipstack_tcp_ctl (chksum.h)
CTL = np.dtype({
    "names": ["local_addr", "remote_addr", "local_port", "remote_port", "seq", "ack", "window", "mss",
              "flags", "options", "wnd_scale", "reserved0", "reserved1"],
    "formats": ["<u4", "<u4", "<u2", "<u2", "<u4", "<u4", "<u2", "<u2", "u1", "u1", "u1", "u1", "<u4"],
    "offsets": [0, 4, 8, 10, 12, 16, 20, 22, 24, 25, 26, 27, 28],
    "itemsize": 32,
})

LOCAL, REMOTE = 0x0A141E28, 0x0A141E64
MAC = bytes.fromhex("0200c0a80001")


def chksum(b):
    """The Internet checksum of `b` (an even number of bytes) as the field holds it."""
    s = sum(struct.unpack(">%dH" % (len(b) // 2), b))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def ctl(**kw):
    d = dict(local_addr=LOCAL, remote_addr=REMOTE, local_port=80, remote_port=40000, seq=0x01020304,
             ack=0x0A0B0C0D, window=4096, mss=0, flags=0x10, options=0, wnd_scale=0, reserved0=0,
             reserved1=0)
    d.update(kw)
    return d


def valid(c):
    return c["reserved0"] == 0 and c["reserved1"] == 0 and (c["options"] & ~3) == 0


def options_of(c):
    o = b""
    if c["options"] & OPT_MSS:
        o += bytes([2, 4]) + struct.pack(">H", c["mss"])
    if c["options"] & OPT_WS:
        o += bytes([1, 3, 3, c["wnd_scale"]])
    return o


def build(c, iface, ttl, ident):
    """The header of the valid descriptor `c` (a mapping) sent from `iface` (a mapping with
    "mac") with the TTL and the Ident: 54, 58 or 62 bytes, the destination MAC zero."""
    opts = options_of(c)
    src, dst = struct.pack(">I", c["local_addr"]), struct.pack(">I", c["remote_addr"])
    tcp = struct.pack(">HHIIHHHH", c["local_port"], c["remote_port"], c["seq"], c["ack"],
                      (5 + len(opts) // 4) << 12 | c["flags"], c["window"], 0, 0) + opts
    ck = chksum(src + dst + struct.pack(">HH", 6, len(tcp)) + tcp)
    tcp = tcp[:16] + struct.pack(">H", ck) + tcp[18:]
    ip = struct.pack(">HHHHBBH", 0x4500, 20 + len(tcp), ident & 0xFFFF, 0x4000, ttl, 6, 0) + src + dst
    ip = ip[:10] + struct.pack(">H", chksum(ip)) + ip[12:]
    return bytes(6) + bytes(iface["mac"]) + b"\x08\x00" + ip + tcp


def to_array(cs):
    t = np.zeros(len(cs), dtype=CTL)
    for k, c in enumerate(cs):
        for name, v in c.items():
            t[k][name] = v
    return t


class Expected:
    """What the call leaves for the descriptors `cs`: headers {i: bytes}, hdr_len, status, counts."""

    def __init__(self, cs, iface, ttl):
        n = len(cs)
        self.headers, self.hdr_len = {}, np.zeros(n, dtype=np.int32)
        self.status = np.full(n, INVALID, dtype=np.uint8)
        j = 0
        for i, c in enumerate(cs):
            if valid(c):
                h = build(c, iface, ttl, iface["ip_id"] + j)
                self.headers[i], self.hdr_len[i], self.status[i] = h, len(h), EMITTED
                j += 1
        self.counts = np.array([j, n - j], dtype=np.int64)


def from_frame(f):
    """The descriptor send_tcp_nodata was given for the recorded frame `f`, and (iface, ttl,
    ident) it was sent with."""
    assert R.is_tcp(f) and f[14] == 0x45
    hl = 14 + 20 + (f[46] >> 4) * 4
    assert len(f) == hl                                    # no data
    lport, rport, seq, ack, of, wnd = struct.unpack(">HHIIHH", f[34:50])
    c = ctl(local_addr=int.from_bytes(f[26:30], "big"), remote_addr=int.from_bytes(f[30:34], "big"),
            local_port=lport, remote_port=rport, seq=seq, ack=ack, window=wnd, flags=of & 0xFF)
    o = f[54:hl]
    while o:
        if o[:2] == bytes([2, 4]):
            assert not c["options"]
            c["options"] |= OPT_MSS
            c["mss"] = int.from_bytes(o[2:4], "big")
        else:
            assert o[:3] == bytes([1, 3, 3])
            c["options"] |= OPT_WS
            c["wnd_scale"] = o[3]
        o = o[4:]
    return c, dict(mac=f[6:12], ip_id=int.from_bytes(f[18:20], "big")), f[22], int.from_bytes(f[18:20], "big")


def seq_for_tcp_checksum(want, **kw):
    """A descriptor whose TCP checksum is `want`: a search over the low half of seq."""
    ifc = dict(mac=MAC, ip_id=0)
    for lo in range(0x10000):
        c = ctl(seq=0x43210000 | lo, **kw)
        if build(c, ifc, 64, 0)[50:52] == struct.pack(">H", want):
            return c
    raise AssertionError("no seq gives the TCP checksum 0x%04x" % want)


def ident_for_ip_checksum(want, c, ttl=64):
    """The Ident with which `c`'s IPv4 header checksum is `want`, or None if there is none."""
    for ident in range(0x10000):
        if build(c, dict(mac=MAC, ip_id=0), ttl, ident)[24:26] == struct.pack(">H", want):
            return ident
    return None


def invalid_set():
    return [ctl(reserved0=1), ctl(reserved0=0x80), ctl(reserved1=1), ctl(reserved1=0x80000000),
            ctl(options=4), ctl(options=4 | 3, mss=1460, wnd_scale=6)]


def edge_set():
    """Valid descriptors: every option subset x the flag set, the ends of seq and ack, window and
    option values at their ends, and the three TCP checksum values."""
    out = []
    for opts in range(4):
        for fl in FLAGS:
            out.append(ctl(options=opts, flags=fl, mss=1460, wnd_scale=6, seq=0x1000 * fl + opts,
                           remote_port=40000 + opts))
    for seq in (0, 0xFFFFFFFF):
        for ack in (0, 0xFFFFFFFF):
            out.append(ctl(seq=seq, ack=ack, flags=0x12, options=3, mss=536, wnd_scale=14))
    out += [ctl(window=0), ctl(window=0xFFFF), ctl(options=1, mss=0), ctl(options=1, mss=0xFFFF),
            ctl(options=2, wnd_scale=0), ctl(options=2, wnd_scale=0xFF), ctl(mss=1460, wnd_scale=7),
            ctl(local_addr=0xFFFFFFFF, remote_addr=0, local_port=0xFFFF, remote_port=0),
            ctl(local_addr=0, remote_addr=0xFFFFFFFF, local_port=0, remote_port=0xFFFF)]
    for want in (0x0000, 0x0001, 0xFFFE):
        out.append(seq_for_tcp_checksum(want))
        out.append(seq_for_tcp_checksum(want, flags=0x12, options=3, mss=1460, wnd_scale=6))
    return out


def pinned(c):
    """True for an edge descriptor whose fields must stay as they are: a sequence or
    acknowledgement number at an end of its range, or a TCP checksum found by search."""
    ck = build(c, dict(mac=MAC, ip_id=0), 64, 0)[50:52]
    return c["seq"] in (0, 0xFFFFFFFF) or c["ack"] in (0, 0xFFFFFFFF) or \
        ck in (b"\x00\x00", b"\x00\x01", b"\xff\xfe")


def batch(n, invalid_at=()):
    """n descriptors cycling through the edge set, an invalid one at each place of `invalid_at`.
    The first pass through the edge set is the set as it is; later passes vary the
    acknowledgement number of every descriptor that is not `pinned`."""
    edge, bad = edge_set(), invalid_set()
    keep = [pinned(c) for c in edge]
    cs = [dict(edge[k % len(edge)]) if k < len(edge) or keep[k % len(edge)]
          else dict(edge[k % len(edge)], ack=0x40000000 + k) for k in range(n)]
    for m, i in enumerate(sorted(set(invalid_at))):
        cs[i] = dict(bad[m % len(bad)], ack=i)
    return cs


def covers_the_ends(cs):
    """True if the valid descriptors of `cs` hold the TCP checksums 0x0000, 0x0001 and 0xFFFE
    and every combination of seq and ack in {0, 0xFFFFFFFF}."""
    ok = [c for c in cs if valid(c)]
    cks = {build(c, dict(mac=MAC, ip_id=0), 64, 0)[50:52].hex() for c in ok}
    ends = {(c["seq"], c["ack"]) for c in ok}
    return {"0000", "0001", "fffe"} <= cks and \
        {(a, b) for a in (0, 0xFFFFFFFF) for b in (0, 0xFFFFFFFF)} <= ends
