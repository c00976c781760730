"""TEST INFRASTRUCTURE -- shared by test_tx_cut_cases.py and test_gpu_tx_cut.py: the send-side
sweep over every payload length, cut and alignment. Host arrays only; every expectation comes from
the existing models (tcpseg_cases, ipfrag_cases, hsplit_cases, linearise_cases, tx_resolve_cases)
and the CPU oracle.

Every send call reads its payload as aligned 16-byte segments under byte masks, so a chunk's code
path is chosen by its address mod 16, its length mod 16 and the parity of the offset at which it
joins the one's-complement sum. A *spec* names those for a payload of two chunks:
(D, l0, a0, a1, x) = D payload bytes behind the header, cut after l0 of them, the two chunks at
addresses a0 and a1 mod 16, x bytes of the payload in front of the first chunk (in the header slot;
0 for the producers and the chained batch, whose first chunk starts the sum).

  family A  short_specs: the full cross D 0..17 x every cut x a0 x a1 (one batch per a0);
            long_specs: D 18..130 x every cut, the addresses dealt out so that for either chunk
            every (address mod 16, length mod 16, start parity) occurs (triples() computes the set);
            for UDP also frag_specs, payloads round the fragment boundaries of two MTUs with
            (mtu - 20) % 8 != 0; for the header-split fill also the split point at every position
            and one to three chunks at every cut; for the chained batch chains of one to three
            chunks of 0..33 bytes, empty chunks included.
  family B  the seed that folds: the two bytes that complete a sum of 0 at every address mod 16 and
            with the cut at each of the last four positions (so they straddle the cut, or a 16-byte
            boundary); hsplit_cases.tcp_inslot_ffff behind two chunks in the same way.
  family C  about 500 segments of family A at gaps of 0..17 bytes, to be run twice: alt() of a
            buffer inverts every byte that no chunk describes.

A device allocation starts on a 16-byte boundary (the GPU test asserts it), so an offset into a
payload buffer mod 16 is the address mod 16."""
import struct

import numpy as np

import aipstack_amd as A

import hsplit_cases as H
import ipfrag_cases as U
import linearise_cases as LC
import tcpseg_cases as T
import tx_resolve_cases as RC
import tx_resolve_ref as R

GUARD = 64                              # undescribed bytes in front of and behind a payload buffer
SHORT, LONG = 17, 130
MSS = (1, 7, 16, 33, 1460)              # the last: one segment whatever D
MSS_LONG = MSS[1:]                      # D up to 130 at mss 1 would be 160,000 segments
MTUS = (1500, 262, 271)                 # whole; (mtu - 20) % 8 = 2 and 3
C_SEGMENTS = 513
POISON = 0xC3
FRAGMENT = 3                            # Rx verify's verdict for a fragment (AIPSTACK_RX_FRAGMENT)


# ---- payload buffers -----------------------------------------------------------------------------

class Ring:
    """A payload buffer as it is laid out: place() gives the next chunk's offset, build() the random
    bytes and the mask of the bytes some chunk describes."""

    def __init__(self, seed):
        self.at, self.off, self.len, self.seed = GUARD, [], [], seed

    def place(self, ln, align=None, gap=0):
        at = self.at + gap
        if align is not None:
            at += (align - at) % 16
        self.off.append(at)
        self.len.append(ln)
        self.at = at + ln
        return at

    def build(self):
        size = self.at + GUARD
        data = np.random.default_rng(self.seed).integers(0, 256, size, dtype=np.uint8)
        d = np.zeros(size + 1, dtype=np.int64)
        off, ln = np.array(self.off, dtype=np.int64), np.array(self.len, dtype=np.int64)
        np.add.at(d, off, 1)
        np.add.at(d, off + ln, -1)
        return data, np.cumsum(d)[:-1] > 0


def alt(data, described):
    """The buffer with every byte that no chunk describes inverted."""
    out = data.copy()
    out[~described] ^= 0xFF
    return out


def end_alignments(chunks, described):
    """({e}, {e}): the end alignments e = (offset + length) % 16 of the chunks behind which an
    undescribed byte lies (i) in the chunk's own last 16-byte segment, (ii) in the segment after."""
    same, after = set(), set()
    for o, l in chunks:
        end = o + l
        if l == 0 or end % 16 == 0:
            continue
        nxt = end + (-end) % 16
        if not described[end:nxt].all():
            same.add(end % 16)
        if not described[nxt:nxt + 16].all():
            after.add(end % 16)
    return same, after


# ---- specs ---------------------------------------------------------------------------------------

def short_specs(a0):
    return [(D, l0, a0, a1, 0) for D in range(SHORT + 1) for l0 in range(D + 1) for a1 in range(16)]


def long_specs(lo=SHORT + 1, hi=LONG, xs=(0,)):
    """Every D in lo..hi at every cut; the addresses are dealt out in turn within each class of
    (length mod 16, start parity), separately for the first and the second chunk."""
    out, c0, c1 = [], {}, {}
    for D in range(lo, hi + 1):
        for l0 in range(D + 1):
            x = xs[(D + l0 // 2) % len(xs)]
            k0, k1 = (l0 % 16, x & 1), ((D - l0) % 16, (x + l0) & 1)
            c0[k0] = a0 = (c0.get(k0, -1) + 1) % 16
            c1[k1] = a1 = (c1.get(k1, 4) + 1) % 16
            out.append((D, l0, a0, a1, x))
    return out


def triples(specs):
    """({(a, len % 16, start parity)} of the non-empty first chunks, the same of the second)."""
    first = {(a0, l0 % 16, x & 1) for D, l0, a0, a1, x in specs if l0}
    second = {(a1, (D - l0) % 16, (x + l0) & 1) for D, l0, a0, a1, x in specs if D - l0}
    return first, second


def frag_specs():
    """(D, l0, a0, a1, mtu): UDP payloads round the first and the second fragment boundary of the
    two MTUs that leave M % 8 bytes over, the cut round 0, either boundary and D."""
    out, j = [], 0
    for mtu in MTUS[1:]:
        F = (mtu - 20) // 8 * 8
        for D in list(range(F - 14, F + 6)) + list(range(2 * F - 12, 2 * F + 12)):
            cuts = set(range(4)) | set(range(D - 3, D + 1))
            for b in (F - 8, 2 * F - 8):
                cuts |= set(range(b - 9, b + 10))
            for l0 in sorted(c for c in cuts if 0 <= c <= D):
                out.append((D, l0, j % 16, (j // 16 + 3 * j) % 16, mtu))
                j += 1
    return out


# ---- the two producers ---------------------------------------------------------------------------

class Batch:
    """cases and payload as tcpseg_cases.Batch / ipfrag_cases.Batch hold them; described: the mask
    of the payload bytes that a piece describes; specs: one per case."""

    def __init__(self, kind, cases, payload, described, specs):
        self.kind, self.cases, self.payload, self.described, self.specs = kind, cases, payload, described, specs

    def pieces(self):
        return [p for c in self.cases for p in c["pieces"]]


RESOLVE_DST = (RC.PEER_SENT, RC.PEER_QUERY, RC.PEER_NEW, R.OUTSIDE, RC.ALL_ONES, R.ip(10, 20, 30, 255))


def tcp_batch(specs, seed, mss_of=None, gaps=False, resolve=False):
    """One burst per spec: FIN on every third, psh_offset walking over 0..D + 1, the mss in turn."""
    ring, cs = Ring(seed), []
    for j, (D, l0, a0, a1, _) in enumerate(specs):
        al = (None, None) if gaps else (a0, a1)
        o0 = ring.place(l0, al[0], j % 18 if gaps else 0)
        o1 = ring.place(D - l0, al[1], (j // 18 + j) % 18 if gaps else 0)
        mss = mss_of(j, D, l0, a0, a1) if mss_of else MSS[(j + j // 5) % 5]
        addr = dict(src=RC.LAN[0]["addr"] + (j % 7 == 3), dst=RESOLVE_DST[j % 6]) if resolve else \
            dict(src=0x0A000001 + j % 251, dst=0x0A000002 + j % 13)
        cs.append(T.burst((o0, l0), (o1, D - l0), mss=mss, seq=(0x01020304 + 7919 * j) & 0xFFFFFFFF,
                          psh_offset=j % (D + 2), ip_id=(31 * j) & 0xFFFF, flags=T.FIN if j % 3 == 0 else 0,
                          hdr=T.template(sport=40000 + j % 997, window=0x2000 + j % 4099, **addr)))
    payload, described = ring.build()
    return Batch("tcp", cs, payload, described, specs)


def short_mss(j, D, l0, a0, a1):
    """Every mss at every (D, cut) and, over the 16 batches, with every a0 and every a1."""
    return MSS[(a0 + a1 + l0 + D) % 5]


def udp_batch(specs, seed, gaps=False, resolve=False):
    """One datagram per spec; a spec's fifth entry above 255 is its MTU, otherwise the MTUs in turn."""
    ring, cs = Ring(seed), []
    for j, (D, l0, a0, a1, m) in enumerate(specs):
        al = (None, None) if gaps else (a0, a1)
        o0 = ring.place(l0, al[0], j % 18 if gaps else 0)
        o1 = ring.place(D - l0, al[1], (j // 18 + j) % 18 if gaps else 0)
        addr = dict(src=RC.LAN[0]["addr"] + (j % 7 == 3), dst=RESOLVE_DST[j % 6]) if resolve else \
            dict(src=0x0A000001 + j % 251, dst=0x0A000002 + j % 13)
        cs.append(U.dgram((o0, l0), (o1, D - l0), mtu=m if m > 255 else MTUS[j % 3], ip_id=(31 * j) & 0xFFFF,
                          sport=40000 + j % 997, dport=53 + j % 11, **addr))
    payload, described = ring.build()
    return Batch("udp", cs, payload, described, specs)


def expect(oracle, b):
    return (T if b.kind == "tcp" else U).expected(oracle, b)


HDR_STRIDE = 64
RING_BYTE = 0xEE


def hdr_lens_of(b, e):
    return np.where(e.status == T.ACCEPT, T.HDR, 0).astype(np.uint32) if b.kind == "tcp" else e.hdr_len


def want_ring(b, e, stride=HDR_STRIDE):
    """The header ring a producer must leave over RING_BYTE: the header, zeros up to
    min(stride, 64) (chksum.h)."""
    n = len(e.status)
    want = np.full((n, stride), RING_BYTE, dtype=np.uint8)
    ok = e.status == T.ACCEPT
    want[ok, :min(stride, 64)] = 0
    w = e.headers.shape[1]
    want[ok, :w] = e.headers[ok]
    return want.reshape(-1)


SLOT_STRIDE = 320                       # of the linearised frames; the longest here has 285 bytes


def _scenario(form, headers, stride, hdr_lens, status, index, chunk_off, chunk_len, payload):
    hl = hdr_lens.astype(np.int64)
    idx = index.astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(chunk_len.astype(np.int64))])
    total = hl + csum[idx[1:]] - csum[idx[:-1]]
    off = np.concatenate([[0], np.cumsum(total)]).astype(np.uint64)
    assert (chunk_off >= 0).all() and total.max() <= SLOT_STRIDE
    return LC.Scenario(form=form, frame_max=SLOT_STRIDE, slot_stride=SLOT_STRIDE, hdr_stride=stride,
                       headers=headers, hdr_lens=hl.astype(np.uint32), seg_status=status.copy(),
                       index=index.astype(np.uint64), chunk_buf=np.zeros(chunk_off.size, dtype=np.int64),
                       chunk_off=chunk_off.astype(np.int64), chunk_len=chunk_len.astype(np.uint32),
                       bufs=[payload], offsets=off if form == "csr" else None, tags=[""] * len(hl))


def scenario(b, e, form):
    """What a producer leaves, as the linearise model takes it: the Scenario of its header ring,
    chunk table and statuses over the batch's payload, the CSR rooms exact."""
    return _scenario(form, want_ring(b, e), HDR_STRIDE, hdr_lens_of(b, e), e.status, e.chunk_index,
                     e.chunk_off, e.chunk_len, b.payload)


def split_scenario(sp, want_h, want_st, form):
    """The same for a header-split layout after the fill: `want_h`, `want_st` of
    hsplit_cases.expected, the layout's own chunk table (offsets into its payload)."""
    off, ln, index = sp.chunk_table(0)
    return _scenario(form, want_h, sp.hdr_stride, sp.hdr_lens, want_st, index, off.astype(np.int64), ln,
                     sp.payload)


def alt_slack(ring, stride, hdr_lens):
    """A header ring with every slot byte from hdr_len on inverted."""
    r = ring.reshape(-1, stride).copy()
    r[np.arange(stride)[None, :] >= np.asarray(hdr_lens)[:, None]] ^= 0xFF
    return r.reshape(-1)


TEMPLATE_OVERWRITTEN = {"tcp": (16, 17, 18, 19, 24, 25, 38, 39, 40, 41, 46, 47, 50, 51, 54, 55),
                        "udp": (16, 17, 18, 19, 24, 25, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47)}


def alt_templates(b):
    """The cases with every template byte inverted that chksum.h documents as ignored and
    overwritten, and the pad bytes behind the header. (UDP's MF and fragment offset share their
    two bytes with the copied DF bit and the contract wants them 0: they stay.)"""
    out = []
    for c in b.cases:
        h = bytearray(c["hdr"])
        for k in TEMPLATE_OVERWRITTEN[b.kind]:
            h[k] ^= 0xFF
        out.append(dict(c, hdr=bytes(h)))
    return Batch(b.kind, out, alt(b.payload, b.described), b.described, b.specs)


def mixed_specs(kind):
    """Specs of family A for the mixed batch: (UDP) fragmenting ones, then long and short ones in
    turn."""
    long_, short = long_specs(), short_specs(5)[3::29]
    pool = [s for pair in zip(long_[::41 if kind == "tcp" else 49], short * 3) for s in pair]
    if kind == "udp":
        fr = frag_specs()
        pool = fr[::max(1, len(fr) // 60)] + pool
    return pool


def mixed_batch(kind):
    """About C_SEGMENTS segments: the specs of mixed_specs in order, each taken if it still fits."""
    out, mss_at, total = [], [], 0
    for j, s in enumerate(mixed_specs(kind)):
        if kind == "udp":
            k = U.counts_of(U.dgram((0, s[1]), (0, s[0] - s[1]), mtu=s[4] if s[4] > 255 else 1500))[0]
        else:
            mss_at.append(MSS[j % 5] if s[0] <= SHORT else MSS_LONG[j % 4])
            k = -(-s[0] // mss_at[-1]) if s[0] else int(len(out) % 3 == 0)      # FIN alone
        if total + k <= C_SEGMENTS:
            out.append(s)
            total += k
        elif kind == "tcp":
            mss_at.pop()
    if kind == "udp":
        return udp_batch(out, 92, gaps=True, resolve=True)
    return tcp_batch(out, 91, mss_of=lambda j, *_: mss_at[j], gaps=True, resolve=True)


# ---- family B for the producers: the sum that comes out 0 ----------------------------------------

FOLD_D = (2, 4, 18, 34, 100)


def fold_specs():
    """(D, l0, a0, a1): the cut at each of the last four positions; the piece that holds byte D - 2
    (the first of the two completing bytes) placed so that this byte lies at every address mod 16:
    at 15 the two bytes straddle a 16-byte boundary, with the cut at D - 1 the piece boundary."""
    out = []
    for D in FOLD_D:
        for l0 in range(max(D - 3, 0), D + 1):
            for r in range(16):
                if l0 > D - 2:                      # byte D - 2 lies in piece 0, at a0 + D - 2
                    a0, a1 = (r - (D - 2)) % 16, (7 * r + l0) % 16
                else:                               # in piece 1, at a1 + D - 2 - l0
                    a0, a1 = (7 * r + l0) % 16, (r - (D - 2 - l0)) % 16
                out.append((D, l0, a0, a1, 0))
    return out


def _at(c, k):
    """Payload offset of byte k of a case's data."""
    (o0, l0), (o1, _) = c["pieces"]
    return o0 + k if k < l0 else o1 + k - l0


def fold_batch(oracle, kind):
    specs = fold_specs()
    if kind == "tcp":
        b = tcp_batch(specs, 71, mss_of=lambda *_: 1460)
    else:
        b = udp_batch([s[:4] + (1500,) for s in specs], 72)
    pay = b.payload
    for c, (D, *_rest) in zip(b.cases, specs):
        p, q = _at(c, D - 2), _at(c, D - 1)
        pay[p] = pay[q] = 0
        if kind == "tcp":
            (start, ln, chunks), = T.segments_of(c)
            h = T.segment_header(oracle, c, pay, 0, 0, ln, chunks, True)
            chk = struct.unpack_from(">H", h, 50)[0]
        else:
            chk = U.udp_checksum(oracle, c, pay)
        pay[p], pay[q] = chk >> 8, chk & 0xFF
    return b


def completing_bytes(b):
    """[(address mod 16 of byte D - 2, the two bytes lie in different pieces)] per case."""
    return [(_at(c, s[0] - 2) % 16, s[1] == s[0] - 1) for c, s in zip(b.cases, b.specs)]


# ---- the header-split fill -------------------------------------------------------------------------

SPLIT_STRIDE = 256
VARIANTS = [("tcp", 5, 5), ("tcp", 5, 15), ("udp", 5, 0), ("tcp", 6, 5), ("tcp", 6, 15), ("udp", 6, 0)]


class Split:
    """sp: the aipstack_amd.SplitFrames layout; described: the mask over sp.payload; seg: the
    segments as split_layout took them."""

    def __init__(self, sp, described, seg):
        self.sp, self.described, self.seg = sp, described, seg

    def alt(self):
        """The layout with every payload byte outside the chunks and every slot byte from hdr_len
        on inverted."""
        sp = self.sp
        h = sp.headers.reshape(-1, sp.hdr_stride).copy()
        cols = np.arange(sp.hdr_stride)[None, :] >= sp.hdr_lens[:, None]
        h[cols] ^= 0xFF
        return A.SplitFrames(h.reshape(-1), sp.hdr_stride, sp.hdr_lens, alt(sp.payload, self.described), sp.chunks)


def _frame(variant, data):
    proto, ihl, doff = variant
    if proto == "tcp":
        f, fixed, _ = H.tcp_segment(data, ihl=ihl, doff=doff)
        return f, fixed
    return H.udp_segment(data, ihl=ihl)


def split_layout(segs, seed, gaps=False):
    """segs: (variant, x, [(chunk length, address mod 16)]). A variant of VARIANTS: the TCP options
    and x payload bytes lie in the slot behind the fixed L4 header; with a fourth entry the x bytes
    count from the end of the fixed header, options included (so the split can lie inside them).
    A (frame, split point) pair in the variant's place: that frame, split there."""
    ring, n = Ring(seed), len(segs)
    pool = np.random.default_rng(seed + 1000).integers(0, 256, 1 << 16, dtype=np.uint8)
    headers = np.full(n * SPLIT_STRIDE, RING_BYTE, dtype=np.uint8)
    hdr_lens = np.zeros(n, dtype=np.uint32)
    chunks, frames = [], []
    for i, (variant, x, parts) in enumerate(segs):
        parts = [(l, a) for l, a in parts if l]
        body = x + sum(l for l, _ in parts)
        if isinstance(variant[0], bytes):
            f, h = variant
        else:
            opts = 4 * (variant[2] - 5) if variant[0] == "tcp" else 0
            inside = len(variant) > 3
            s = (37 * i) % ((1 << 16) - 256)
            f, fixed = _frame(variant[:3], pool[s:s + body - (opts if inside else 0)].tobytes())
            h = fixed + x + (0 if inside else opts)
        assert h <= SPLIT_STRIDE and len(f) == h + body - x, (variant, x, parts)
        headers[i * SPLIT_STRIDE:i * SPLIT_STRIDE + h] = np.frombuffer(f[:h], dtype=np.uint8)
        hdr_lens[i] = h
        chunks.append([(ring.place(l, None if gaps else a, (i + 5 * k) % 18 if gaps else 0), l)
                       for k, (l, a) in enumerate(parts)])
        frames.append(f)
    payload, described = ring.build()
    for f, h, ch in zip(frames, hdr_lens, chunks):
        at = int(h)
        for o, l in ch:
            payload[o:o + l] = np.frombuffer(f[at:at + l], dtype=np.uint8)
            at += l
    return Split(A.SplitFrames(headers, SPLIT_STRIDE, hdr_lens, payload, chunks), described, segs)


def split_short(a0):
    """The full cross behind the fixed L4 header, TCP and UDP in turn."""
    return split_layout([(VARIANTS[(l0 + a1) % 3], 0, [(l0, a0), (D - l0, a1)])
                         for D, l0, a0, a1, _ in short_specs(a0)], 300 + a0)


def split_long_specs():
    return long_specs(xs=(0, 1))


def split_long():
    return split_layout([(VARIANTS[j % 6], x, [(l0, a0), (D - l0, a1)])
                         for j, (D, l0, a0, a1, x) in enumerate(split_long_specs())], 320)


SPLIT_P, PIECES_P = 48, 24


def split_points():
    """Payloads of 0..48 bytes with the split at every position from the end of the fixed L4 header
    to the frame's end, every variant; then payloads of 0..24 bytes behind the fixed header cut
    into up to three chunks at every pair of positions, the variants in turn."""
    segs, j = [], 0
    for v in VARIANTS:
        opts = 4 * (v[2] - 5) if v[0] == "tcp" else 0
        for P in range(SPLIT_P + 1):
            for x in range(opts + P + 1):
                segs.append((v + ("inside",), x, [(opts + P - x, (j + j // 16) % 16)]))
                j += 1
    for P in range(PIECES_P + 1):
        for c1 in range(P + 1):
            for c2 in range(c1, P + 1):
                segs.append((VARIANTS[j % 6], 0, [(c1, j % 16), (c2 - c1, (j // 16) % 16), (P - c2, (5 * j + 1) % 16)]))
                j += 1
    return split_layout(segs, 330)


def split_fold():
    """hsplit_cases.tcp_inslot_ffff (20 + x TCP bytes in the slot, x in 0..3) behind two chunks:
    the cut at each of the last four positions, the first chunk at every address, the second at
    both parities."""
    rng = np.random.default_rng(340)
    segs = []
    for x in range(4):
        for P in (3, 17, 18, 40):
            data = rng.integers(0, 256, P, dtype=np.uint8).tobytes()
            f, at = H.tcp_inslot_ffff(data, 20 + x)
            rest = P - x
            for l0 in range(max(rest - 3, 0), rest + 1):
                for a0 in range(16):
                    for par in (0, 1):
                        segs.append(((f, at), x, [(l0, a0), (rest - l0, (5 * a0 + l0) // 2 * 2 % 16 + par)]))
    return split_layout(segs, 341)


def split_mixed():
    specs = split_long_specs()
    specs = specs[::max(1, len(specs) // C_SEGMENTS)][:C_SEGMENTS]
    return split_layout([(VARIANTS[j % 6], x, [(l0, a0), (D - l0, a1)])
                         for j, (D, l0, a0, a1, x) in enumerate(specs)], 350, gaps=True)


# ---- the chained batch and the chain fill --------------------------------------------------------

CHAIN_MAX = 33


class Chains:
    """chains: per chain [(payload offset, length)], empty chunks included; states; payload,
    described."""

    def __init__(self, chains, states, payload, described):
        self.chains, self.states, self.payload, self.described = chains, states, payload, described

    def table(self, base):
        """(addr uint64, len uint32, index uint64) with the payload at address `base`."""
        addr = np.array([base + o for ch in self.chains for o, _ in ch], dtype=np.uint64)
        ln = np.array([l for ch in self.chains for _, l in ch], dtype=np.uint32)
        idx = np.zeros(len(self.chains) + 1, dtype=np.uint64)
        idx[1:] = np.cumsum([len(ch) for ch in self.chains])
        return addr, ln, idx

    def expected(self, oracle, payload=None):
        """The final checksums: the oracle's seeded sum over each chain's concatenated bytes."""
        p = self.payload if payload is None else payload
        flat = np.concatenate([p[o:o + l] for ch in self.chains for o, l in ch] + [np.zeros(1, np.uint8)])
        off = np.zeros(len(self.chains) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([sum(l for _, l in ch) for ch in self.chains])
        return oracle.batch_seeded_csr(flat, off, self.states)


def chain_specs():
    """[(under, [(length, address mod 16)])]: one chunk of 0..33 bytes at every address; two
    chunks of every pair of lengths with either of them at every address; three chunks of every
    triple of lengths, their addresses dealt out within each (position, length mod 16, start
    parity) class."""
    out = []
    R34 = range(CHAIN_MAX + 1)
    for l in R34:
        for a in range(16):
            out.append((0, [(l, a)]))
    for l0 in R34:
        for l1 in R34:
            for a in range(16):
                other = (5 * a + l0 + l1) % 16
                out.append((0, [(l0, a), (l1, other)]))
                out.append((1, [(l0, other), (l1, a)]))
    cnt = {}
    for l0 in R34:
        for l1 in R34:
            for l2 in R34:
                parts, at = [], 0
                for pos, l in enumerate((l0, l1, l2)):
                    k = (pos, l % 16, at & 1)
                    cnt[k] = a = (cnt.get(k, 3 * pos) + 1) % 16
                    parts.append((l, a))
                    at += l
                out.append((-1, parts))
    return out


def chain_triples(specs, n):
    """Per position the {(address mod 16, length mod 16, start parity)} of the non-empty chunks of
    the n-chunk chains."""
    got = [set() for _ in range(n)]
    for _, parts in specs:
        if len(parts) != n:
            continue
        at = 0
        for pos, (l, a) in enumerate(parts):
            if l:
                got[pos].add((a, l % 16, at & 1))
            at += l
    return got


def chain_batch(oracle, specs, seed, gaps=False):
    """Every 50th chain's state is raised by the chain's own checksum, so that its sum folds to
    0xFFFF and the final checksum is 0."""
    ring, chains = Ring(seed), []
    for j, (_, parts) in enumerate(specs):
        chains.append([(ring.place(l, None if gaps else a, (j + 7 * k) % 18 if gaps else 0), l)
                       for k, (l, a) in enumerate(parts)])
    payload, described = ring.build()
    states = ((np.arange(len(specs), dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 20)).astype(np.uint32)
    c = Chains(chains, states, payload, described)
    first = c.expected(oracle)
    states[::50] += first[::50]
    return c


def chain_mixed(oracle):
    specs = chain_specs()
    return chain_batch(oracle, specs[::max(1, len(specs) // C_SEGMENTS)][:C_SEGMENTS], 95, gaps=True)


def field_offsets(n):
    """Where the chain fill stores chain i's checksum in a buffer of 3 * n + 2 bytes: every
    address parity and every offset mod 16; every seventh chain has no field."""
    off = 1 + 3 * np.arange(n, dtype=np.int64)
    off[6::7] = -1
    return off


def filled_fields(n, sums, zero_as_ffff):
    """The field buffer after the fill, over POISON."""
    buf = np.full(3 * n + 2, POISON, dtype=np.uint8)
    v = np.where((sums == 0) & zero_as_ffff, 0xFFFF, sums).astype(np.uint16)
    off = field_offsets(n)
    m = off >= 0
    buf[off[m]], buf[off[m] + 1] = (v[m] >> 8).astype(np.uint8), (v[m] & 0xFF).astype(np.uint8)
    return buf, v


# ---- computed once per process ---------------------------------------------------------------------

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def producer(oracle, kind, name):
    """(batch, the model's Expected) of a named producer batch: "short<a0>", "long", "frag" (UDP),
    "fold", "mixed"."""
    def make():
        if name.startswith("short"):
            a0 = int(name[5:])
            b = tcp_batch(short_specs(a0), 10 + a0, short_mss) if kind == "tcp" else udp_batch(short_specs(a0), 30 + a0)
        elif name == "long":
            b = tcp_batch(long_specs(), 50, lambda j, *_: MSS_LONG[(j + j // 4) % 4]) if kind == "tcp" \
                else udp_batch(long_specs(), 51)
        elif name == "frag":
            b = udp_batch(frag_specs(), 52)
        elif name == "fold":
            b = fold_batch(oracle, kind)
        else:
            b = mixed_batch(kind)
        return b, expect(oracle, b)
    return cached((kind, name), make)


PRODUCER_BATCHES = {"tcp": ["short%d" % a for a in range(16)] + ["long", "fold"],
                    "udp": ["short%d" % a for a in range(16)] + ["long", "frag", "fold"]}
SPLIT_BATCHES = {**{"short%d" % a: (lambda a=a: split_short(a)) for a in range(16)}, "long": split_long,
                 "points": split_points, "fold": split_fold, "mixed": split_mixed}


def split(name):
    return cached(("split", name), SPLIT_BATCHES[name])
