"""TEST INFRASTRUCTURE -- the case generators of test_gpu_large_span_rx.py, on the arena, windows,
filler and SHIFTS of large_span_cases.py: the frames of aipstack_udp_rx_demux / _slotted and of
aipstack_icmp_rx_respond / _slotted on both sides of a 2^31 and a 2^32 byte offset from the base
and of a device address that is a multiple of 2^32, and the responder's header ring across the two
offsets. They need no GPU: test_large_span_rx_cases.py runs them for fake base pointers.

A case is a pure function of (P, shift, kind). The expectations are the models of udp_rx_cases.py
and icmp_cases.py on the windows' frames alone, their frame indices mapped to the batch's; a filler
frame (zero bytes) gives a zero record, 0xFF and NONE, and the verdict the oracle gives it.

Out of reach: d_dgrams past 4 GiB needs 2^27 frames, and a 64-byte header ring past 4 GiB -- the
whole-line store path of the responder -- needs 2^26; the ring case here has 65,536-byte slots, so
it takes the plain-store path.
"""
import numpy as np

import aipstack_amd as A

import frame_cases as F
import icmp_cases as IC
import icmp_ref as IR
import large_span_cases as L
import large_span_ipreass_cases as LI
import udp_rx_cases as UC
import udp_rx_ref as UR

KEY, LIS, DGRAM = A.TCP_PCB_KEY_DTYPE, A.UDP_LISTENER_DTYPE, A.UDP_RX_DGRAM_DTYPE
DISTANCES = (1, 17, 40, "len-1")      # the Ethernet, the IPv4, the UDP/ICMP header, the data straddle
STRADDLERS = ("udp_hit", "udp_closed", "echo", "udp_code3")
IFACE = IC.iface(ip_id=0xFFF0)
ARP = F.LOCAL_MAC + F.peer_mac(1) + b"\x08\x06" + bytes(46)


def tables():
    """(associations, listeners): "udp_hit" has one of each."""
    tbl = UC.assocs([(UR.LOCAL, UR.PEER, 5000, UR.SPORT, False, 3),
                     (UR.LOCAL, UR.PEER + 1, 6000, UR.SPORT, False, 0x7FFFFFFF)], KEY)
    return tbl, UC.listeners([(0, 5000, 0, 0, 7), (0, 5001, 1, 1, 8)], LIS)


def pool():
    """({straddler name: frame}, side frames): a datagram that an association and a listener
    take, one to a closed port, an echo request with data, a datagram with IPv4 options to a
    closed port (the host passes code 3 for it); the sides: non-responders (ARP, a datagram for
    another host, a bad echo checksum, a short TCP frame) and more responders."""
    st = {"udp_hit": UC.dgram(5000, n=33), "udp_closed": UC.dgram(9, n=21),
          "echo": IC.eth(IR.echo(IR.pattern(50, 3))), "udp_code3": UC.dgram(10, n=8, ihl=7)}
    sides = [ARP, UC.dgram(9, dst=UR.NONLOCAL, n=5),
             IC.eth(IR.ip_packet(1, IR.icmp(8, 0, IR.REST, IR.pattern(18, 3), bad=True))),
             IC.eth(IR.echo(b"")), IC.eth(IR.echo(IR.pattern(9, 1)), pad60=True),
             UC.dgram(6000, src=UR.PEER + 1, n=2), UC.dgram(11, n=0), IC.eth(IR.ip_packet(6, IR.pattern(10, 2))),
             UC.dgram(5001, dst=UR.BCAST, n=1)]
    return st, sides


def host_codes(frames):
    """Code 3 for every IPv4 UDP frame, as a host without listeners asks (icmp_cases.host_codes)."""
    return IC.host_codes(frames)


# ---- (a) CSR frames across the edges ----------------------------------------------------------

class CsrCase:
    """offsets (uint64, n + 1, from the base P + shift), lens, windows, frames {frame index:
    bytes} of the windows' frames, across [(frame that holds each edge byte, straddler name)],
    edges, n, shift."""


def csr_case(P, shift, kind):
    """One window round each edge of large_span_ipreass_cases.edges_of: the side frames, the
    straddler -- it starts `kind` bytes before the edge -- and the sides again with the other three
    straddler types among them. Which straddler lies across which edge rotates with the edge, the
    distance and the shift, so that every type meets every distance."""
    edges = LI.edges_of(P, shift)
    st, sides = pool()
    turn = DISTANCES.index(kind) + L.SHIFTS.index(shift)
    c = CsrCase()
    lens, c.windows, c.across, c.frames = [], [], [], {}
    at = 0
    for w, e in enumerate(edges):
        name = STRADDLERS[(w + turn) % 4]
        mid = st[name]
        pre = sides[w:] + sides[:w]
        post = [st[s] for s in STRADDLERS if s != name] + sides[::-1]
        d = len(mid) - 1 if kind == "len-1" else kind
        assert 0 < d < len(mid)
        items = pre + [mid] + post
        ws = e - d - sum(len(f) for f in pre)
        assert ws >= at
        q, r = divmod(ws - at, L.FILL)
        lens += [L.FILL] * q + ([r] if r else [])
        c.across.append((len(lens) + len(pre), name))
        for j, f in enumerate(items):
            c.frames[len(lens) + j] = f
        data = np.frombuffer(b"".join(items), dtype=np.uint8).copy()
        c.windows.append(L.Window(shift + ws, data))
        lens += [len(f) for f in items]
        at = ws + data.size
    lens += [L.FILL] * 3
    c.lens = np.array(lens, dtype=np.int64)
    c.offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(c.lens.astype(np.uint64), out=c.offsets[1:])
    c.n, c.edges, c.shift, c.kind = len(lens), edges, shift, kind
    assert shift + int(c.offsets[-1]) <= L.ARENA_BYTES
    return c


def filler_verdicts(oracle, lens):
    """The oracle's verdict for a frame of zero bytes, per length in `lens`."""
    out = {}
    for ln in sorted(set(int(x) for x in lens)):
        out[ln] = int(oracle.rx_verify_batch(np.zeros(max(ln, 1), dtype=np.uint8), [0, ln])[0])
    return out


def _window_frames(oracle, frames):
    idx = sorted(frames)
    fr = [frames[i] for i in idx]
    buf, off = F.pack(fr)
    return np.array(idx, dtype=np.int64), fr, oracle.rx_verify_batch(buf, off)


def _verdicts(oracle, n, lens, g, v):
    fv = filler_verdicts(oracle, np.delete(lens, g))
    out = np.zeros(n, dtype=np.uint8)
    for ln, val in fv.items():
        out[lens == ln] = val
    out[g] = v
    return out


def expected_udp(oracle, n, lens, frames):
    """udp_rx_cases.Expected of a batch of n frames whose `frames` {index: bytes} are the only
    ones with bytes other than zero."""
    g, fr, v = _window_frames(oracle, frames)
    tbl, lis = tables()
    local = UC.expected(fr, v, IFACE, tbl, lis, DGRAM)
    e = UC.Expected()
    e.verdict = _verdicts(oracle, n, lens, g, v)
    e.dgrams = np.zeros(n, dtype=DGRAM)
    e.dgrams[g] = local.dgrams
    e.unreach = np.full(n, UC.NO_UNREACH, dtype=np.uint8)
    e.unreach[g] = local.unreach
    k = int(local.counts[0])
    e.deliver_frame = np.full(n, UC.NO_FRAME, dtype=np.uint64)
    e.deliver_frame[:k] = g[local.deliver_frame[:k].astype(np.int64)]
    e.counts = local.counts.copy()
    e.local, e.rows = local, g
    return e


def expected_icmp(oracle, n, lens, frames, codes):
    """icmp_cases.Expected of such a batch; `codes`: {frame index: code} (None: no requests).
    headers: {batch index: 42 bytes}; chunks: [(batch index, offset in the frame, length)]."""
    g, fr, v = _window_frames(oracle, frames)
    local = IC.respond(fr, v, None if codes is None else [codes.get(int(i), IC.NO_UNREACH) for i in g], IFACE)
    e = IC.Expected()
    e.verdict = _verdicts(oracle, n, lens, g, v)
    e.status = np.full(n, IC.NONE, dtype=np.uint8)
    e.status[g] = local.status
    e.hdr_len = np.zeros(n, dtype=np.uint32)
    e.hdr_len[g] = local.hdr_len
    has = np.zeros(n + 1, dtype=np.uint64)
    has[g[np.array([fi for fi, _, _ in local.chunks], dtype=np.int64)] + 1] = 1
    e.chunk_index = np.cumsum(has).astype(np.uint64)
    k = int(local.counts[0])
    e.response_frame = np.full(n, IC.NO_FRAME, dtype=np.uint64)
    e.response_frame[:k] = g[local.response_frame[:k].astype(np.int64)]
    e.counts = local.counts.copy()
    e.headers = {int(g[i]): h for i, h in local.headers.items()}
    e.chunks = [(int(g[fi]), off, ln) for fi, off, ln in local.chunks]
    e.local, e.rows, e.local_frames = local, g, fr
    return e


# ---- (b) ring slots -----------------------------------------------------------------------------

SLOTTED = [(stride, 65600) for stride, _ in L.SLOTTED]      # 257 tiles: the scan's second step


class SlottedCase:
    """Slot i = lens[i] bytes at base + i * stride, base = P + shift: frames {slot: bytes} in the
    first and the last slot and in the slots round the two edges, length 0 everywhere else;
    windows: one per frame."""


def slotted_case(stride, n, shift):
    st, sides = pool()
    every = [st[s] for s in STRADDLERS] + sides
    c = SlottedCase()
    c.stride, c.n, c.shift, c.edges = stride, n, shift, L.EDGES
    slots = [0, n - 1]
    for e in L.EDGES:
        slots += list(range(e // stride - 6, e // stride + 7))
    c.frames = {s: every[(j + shift) % len(every)] for j, s in enumerate(sorted(set(slots)))}
    c.lens = np.zeros(n, dtype=np.int64)
    for s, f in c.frames.items():
        c.lens[s] = len(f)
    c.windows = [L.Window(shift + s * stride, np.frombuffer(f, dtype=np.uint8).copy()) for s, f in c.frames.items()]
    assert shift + (n - 1) * stride + 65535 <= L.ARENA_BYTES
    return c


# ---- (c) the responder's header ring ----------------------------------------------------------

RING_STRIDE, RING_SLOTS, FRAME_SLOT = L.RING_STRIDE, 65600, 64


class RingCase:
    """n frames in slots of FRAME_SLOT bytes of a small buffer of their own (`buf`, `lens`); the
    responders (echo requests of 0-18 data bytes) at `rows`, every other slot empty; e: the model's
    Expected for the whole batch."""


def ring_case(oracle):
    """Responders at large_span_cases.ring_rows: every row within 256 of slots 32768 and 65536
    (whose headers start at offsets 2^31 and 2^32 of the ring) and every 61st row."""
    c = RingCase()
    c.n = n = RING_SLOTS
    _, c.rows = L.ring_rows(n)
    echo = [IC.eth(IR.echo(IR.pattern(k % 19, k), ident=k)) for k in range(64)]
    frames = {int(r): echo[j % 64] for j, r in enumerate(c.rows)}
    assert max(len(f) for f in echo) <= FRAME_SLOT
    c.lens = np.zeros(n, dtype=np.int64)
    c.buf = np.zeros(n * FRAME_SLOT, dtype=np.uint8)
    for r, f in frames.items():
        c.lens[r] = len(f)
        c.buf[r * FRAME_SLOT:r * FRAME_SLOT + len(f)] = np.frombuffer(f, dtype=np.uint8)
    c.frames = frames
    c.e = expected_icmp(oracle, n, c.lens, frames, None)
    return c
