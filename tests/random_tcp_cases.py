"""TEST INFRASTRUCTURE -- the seeded scenario generators of test_gpu_random_tcp.py (header-split
Tx fill, TCP burst segmentation, TCP Rx parse). They need no GPU: test_random_tcp_cases.py runs
every one of them over the full seed range with the CPU oracle and checks that the scenarios
cover what they are meant to cover.

One ``np.random.default_rng(base + seed)`` per scenario; every expectation comes from the models
of hsplit_cases.py, tcpseg_cases.py and tcprx_cases.py and from the CPU oracle, none from the
library under test. A scenario never drops an element after drawing it; what a generator does not
draw is listed in its docstring.
"""
import struct

import numpy as np

import aipstack_amd as A

import frame_cases as F
import hsplit_cases as H
import tcprx_cases as R
import tcpseg_cases as S

SEEDS = 40
MAX_ELEMENTS = 1500
GUARD_BYTE = 0xA7


def blob(rng, nbytes):
    """Random bytes with runs of 0x00 and 0xFF."""
    b = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
    for _ in range(int(rng.integers(4, 24))):
        s = int(rng.integers(0, nbytes))
        b[s:s + int(rng.integers(1, 4000))] = rng.choice([0x00, 0xFF])
    return b


def _count(rng, most=MAX_ELEMENTS):
    """Scenario sizes: a few elements, a few waves, or many blocks."""
    r = rng.random()
    if r < 0.15:
        return int(rng.integers(1, 8))
    if r < 0.5:
        return int(rng.integers(8, 300))
    return int(rng.integers(300, most + 1))


# ---- header-split Tx fill ---------------------------------------------------------------------

HS_STRIDES = (54, 64, 72, 100, 128, 256, 300)
HS_TAIL = 320        # bytes after the last slot that the model carries along (a header length
                     # above the stride reaches into them; they must come back untouched)


class HsplitScenario:
    """sp: a SplitFrames whose ``headers`` holds the n slots followed by HS_TAIL guard bytes;
    shift: bytes the ring start lies off its 64-byte boundary; want_h / want_st / ok: what the
    fill must leave (hsplit_cases.expected); swapped: per segment, the in-slot L4 length is odd."""


def _hs_payload(rng, src):
    r = rng.random()
    ln = 0 if r < 0.1 else int(rng.integers(1, 65)) if r < 0.3 else int(rng.integers(0, 3001))
    o = int(rng.integers(0, src.size - ln + 1))
    return src[o:o + ln].tobytes()


def _hs_segment(rng, src, golden):
    """(frame, forced split point or None)"""
    r = rng.random()
    if r < 0.38:
        return H.tcp_segment(_hs_payload(rng, src), ihl=int(rng.integers(5, 16)),
                             doff=int(rng.integers(5, 16)))[0], None
    if r < 0.58:
        return H.udp_segment(_hs_payload(rng, src), ihl=int(rng.integers(5, 16)),
                             sport=int(rng.integers(1, 65536)))[0], None
    if r < 0.63:
        return H.icmp_zero_segment(int(rng.choice([8, 9, 40, 41, 100])))[0], None
    if r < 0.70:
        pay = _hs_payload(rng, src)
        f, at = H.tcp_inslot_ffff(pay, 20 + int(rng.integers(0, min(len(pay), 3) + 1)))
        return f, (at if rng.random() < 0.7 else None)
    return golden[int(rng.integers(0, len(golden)))], None


def hsplit_scenario(oracle, seed):
    """Segments from hsplit_cases.tcp_segment / udp_segment (IHL and data offset 5-15, payloads
    of 0-3000 bytes with runs of 0x00 and 0xFF), icmp_zero_segment, tcp_inslot_ffff and the golden
    frames (malformed and non-IPv4 frames included). H is uniform in [0, min(len, stride, 256)]
    (seven in ten), uniform from the end of the fixed L4 header up (so that short strides keep
    filled segments), or up to 30 bytes above min(stride, 256) (three in a hundred). The rest of
    the segment is cut into 0-4 chunks at random points (odd points and empty chunks included; no
    chunk at all for a non-empty rest truncates the segment), laid in random order with gaps of
    0-5 bytes. Both checksum fields hold random bytes. The ring start's residue mod 16 is
    seed % 16, so that 40 seeds meet every residue; its 64-byte phase is drawn.
    Segment 0 is an exact-length TCP segment split inside its payload or at its end (filled);
    from 8 segments on, the last one has a 10-byte header (status 9).
    Not drawn: segments over 3 KiB + headers (the model is a Python loop over them)."""
    rng = np.random.default_rng(5000 + seed)
    golden = H.golden_frames()
    n = _count(rng)
    stride = int(rng.choice(HS_STRIDES))
    cap = min(stride, H.MAX_SPLIT_HEADER)
    shift = 16 * int(rng.integers(0, 4)) + seed % 16
    src = blob(rng, 1 << 16)
    headers = np.full(n * stride + HS_TAIL, GUARD_BYTE, dtype=np.uint8)
    headers[:n * stride] = 0xEE
    hdr_lens = np.zeros(n, dtype=np.uint32)
    pieces, per_seg = [], []
    for i in range(n):
        forced = None
        if i == 0:
            f = H.tcp_segment(_hs_payload(rng, src))[0]
        elif i == n - 1 and n >= 8:
            f, forced = H.tcp_segment(_hs_payload(rng, src))[0], 10
        else:
            f, forced = _hs_segment(rng, src, golden)
        f = bytearray(f)
        a, hl, proto = H._l4_fixed_end(f)
        if len(f) >= 26:
            f[24:26] = rng.integers(0, 256, 2, dtype=np.uint8).tobytes()
        fo = {6: 16, 17: 6, 1: 2}.get(proto)
        if fo is not None and len(f) >= 14 + hl + fo + 2:
            f[14 + hl + fo:14 + hl + fo + 2] = rng.integers(0, 256, 2, dtype=np.uint8).tobytes()
        top = min(len(f), cap)
        r = rng.random()
        if forced is not None and forced <= top:
            h = forced
        elif i == 0 or (r >= 0.70 and r < 0.97 and a <= top):
            h = int(rng.integers(a, top + 1))
        elif r >= 0.97 and i > 0:
            h = cap + int(rng.integers(1, 31))
        else:
            h = int(rng.integers(0, top + 1))
        hdr_lens[i] = h
        inslot = min(h, len(f), stride)
        headers[i * stride:i * stride + inslot] = np.frombuffer(bytes(f[:inslot]), dtype=np.uint8)
        rest = np.frombuffer(bytes(f[min(h, len(f)):]), dtype=np.uint8)
        k = int(rng.integers(0, 5))
        if k == 0 and rest.size and (i == 0 or rng.random() < 0.9):
            k = 1
        cuts = np.sort(rng.integers(0, rest.size + 1, size=max(k - 1, 0)))
        edges = [0] + cuts.tolist() + [rest.size] if k else []
        segs = [rest[edges[j]:edges[j + 1]] for j in range(k)]
        per_seg.append(len(segs))
        pieces += segs
    where = [0] * len(pieces)
    at = int(rng.integers(0, 6))
    for k in rng.permutation(len(pieces)):
        where[k] = at
        at += pieces[k].size + int(rng.integers(0, 6))
    payload = np.full(max(at, 1), 0xDD, dtype=np.uint8)
    for k, pc in enumerate(pieces):
        payload[where[k]:where[k] + pc.size] = pc
    chunks, k = [], 0
    for cnt in per_seg:
        chunks.append([(where[k + j], int(pieces[k + j].size)) for j in range(cnt)])
        k += cnt
    sc = HsplitScenario()
    sc.seed, sc.n, sc.stride, sc.shift = seed, n, stride, shift
    sc.just_written = bool(rng.integers(0, 2))
    sc.sp = A.SplitFrames(headers, stride, hdr_lens, payload, chunks)
    sc.want_h, sc.want_st, sc.st_lin, sc.ok = H.expected(oracle, sc.sp)
    lin, off = sc.sp.linearise()
    sc.swapped = np.zeros(n, dtype=bool)
    for i in np.nonzero(sc.want_st == H.ACCEPT)[0]:
        o = int(off[i])
        sc.swapped[i] = (int(hdr_lens[i]) - 14 - (int(lin[o + 14]) & 0xF) * 4) & 1
    return sc


# ---- TCP burst segmentation -------------------------------------------------------------------

TS_MSS = (1, 2, 3, 7, 100, 536, 1460, 8960, 65495)
TS_STRIDES = (54, 64, 72, 128)
TS_BURST_SEGMENTS = 25


class TcpsegScenario:
    """batch (tcpseg_cases.Batch), si / cb (the caller's index), e (tcpseg_cases.expected),
    stride, shift, just_written."""


def _ts_template(rng):
    return S.template(src=int(rng.integers(1, 1 << 32)), dst=int(rng.integers(1, 1 << 32)),
                      sport=int(rng.integers(0, 65536)), dport=int(rng.integers(0, 65536)),
                      ack=int(rng.integers(0, 1 << 32)), window=int(rng.integers(0, 65536)),
                      ttl=int(rng.integers(1, 256)), dscp=int(rng.integers(0, 256)),
                      urgent=int(rng.integers(0, 65536)), junk=int(rng.integers(0, 256)))


def _ts_burst(rng, nbytes, most_segments, nonzero=False):
    mss = int(rng.choice(TS_MSS))
    r = rng.random()
    D = 0 if r < 0.1 and not nonzero else int(rng.integers(1, 200)) if r < 0.35 \
        else int(rng.integers(1, 20001))
    D = min(D, mss * most_segments)
    r = rng.random()
    l0 = 0 if r < 0.1 else D if r < 0.2 else int(rng.integers(0, D + 1))
    o0 = int(rng.integers(0, nbytes - l0 + 1))
    o1 = int(rng.integers(0, nbytes - (D - l0) + 1))
    seq = int(rng.integers(0, 1 << 32))
    if rng.random() < 0.125:
        seq = 0xFFFFFFFF - int(rng.integers(0, 30000))
    ip_id = int(rng.integers(0, 65536))
    if rng.random() < 0.25:
        ip_id = 0xFFFF - int(rng.integers(0, 300))
    return S.burst((o0, l0), (o1, D - l0), mss=mss, seq=seq, ip_id=ip_id,
                   psh_offset=int(rng.integers(0, D + 3)), flags=S.FIN if rng.random() < 0.3 else 0,
                   hdr=_ts_template(rng))


def tcpseg_scenario(oracle, seed):
    """1-120 bursts: mss from TS_MSS, 0-20000 data bytes split between the two pieces at a random
    point (0 and D one time in ten each), pieces at any byte of the payload buffer, psh_offset in
    [0, D + 2], FIN three times in ten, seq uniform over 32 bits (one in eight within 30000 of the
    wrap), ip_id uniform (one in four in the top 300 values), the template's addresses, ports,
    ack, window, TTL, DSCP, urgent pointer and junk at random; the ring stride from TS_STRIDES, its
    start on a 64-byte boundary four times in ten, else 0-63 bytes off it. 8 % of the bursts are
    tcpseg_cases.invalid_case of a random class, 5 % valid descriptors whose caller-given counts
    disagree, 10 % zero-segment bursts. Burst 0 is valid with at least one segment; from two
    bursts on, the last one is an invalid_case.
    Not drawn: bursts of more than 25 segments (D is cut to 25 * mss) and batches over 1500
    segments (the Python model builds every header), so mss = 1, 2, 3, 7 carry at most 175 bytes."""
    rng = np.random.default_rng(6000 + seed)
    nb = int(rng.integers(1, 121))
    pay = blob(rng, 1 << 16)
    cases, total = [], 0
    for b in range(nb):
        room = max(0, min(TS_BURST_SEGMENTS, MAX_ELEMENTS - total))
        r = rng.random()
        if b == 0:
            c = _ts_burst(rng, pay.size, 7 if nb == 1 else TS_BURST_SEGMENTS, nonzero=True)
        elif b == nb - 1 or r < 0.08:
            c = S.invalid_case(S.INVALID_CLASSES[int(rng.integers(0, len(S.INVALID_CLASSES)))])
        elif room == 0:
            c = S.burst((0, 0), hdr=_ts_template(rng))
        else:
            c = _ts_burst(rng, pay.size, room)
            if r < 0.13:
                segs = S.segments_of(c)
                ns, nc = len(segs), sum(len(ch) for _, _, ch in segs)
                give = [(0, 2), (ns + 1, nc), (max(ns - 1, 0), nc + 1), (ns, nc + 2), (ns + 2, nc + 1)]
                give = [g for g in give if g != (ns, nc)]
                c["give"] = give[int(rng.integers(0, len(give)))]
        cases.append(c)
        total += c["give"][0] if "give" in c else len(S.segments_of(c))
    sc = TcpsegScenario()
    sc.seed = seed
    sc.batch = S.Batch(cases, pay)
    sc.si, sc.cb = S.caller_index(cases)
    sc.e = S.expected(oracle, sc.batch, sc.si, sc.cb)
    sc.stride = int(rng.choice(TS_STRIDES))
    sc.shift = 0 if rng.random() < 0.4 else int(rng.integers(0, 64))   # (0: the aligned emit form)
    sc.just_written = bool(rng.integers(0, 2))
    return sc


def tcpseg_wraps(sc):
    """(ident wraps, seq wraps) inside accepted bursts of 3 or more segments."""
    ident = seq = 0
    for b, c in enumerate(sc.batch.cases):
        s0, ns = int(sc.si[b]), int(sc.si[b + 1] - sc.si[b])
        if ns < 3 or sc.e.status[s0] != S.ACCEPT:
            continue
        segs = S.segments_of(c)
        ident += c["ip_id"] + ns - 1 > 0xFFFF
        seq += c["seq"] + segs[-1][0] > 0xFFFFFFFF
    return ident, seq


# ---- TCP Rx parse -----------------------------------------------------------------------------

RX_STRIDES = (192, 256, 1536, 2048)


class TcprxScenario:
    """frames / verdicts (the oracle's Rx verify), tbl (sorted), e (tcprx_cases.expected), lead,
    seg_shift; the slotted form: stride, ring, lens, slot_frames (what a slot shows), slot_e."""


def _rx_options(rng, nbytes):
    """`nbytes` option bytes: structured from kinds {0, 1, 2, 3, other} with right and wrong
    lengths (half of the time), or uniform."""
    if rng.random() < 0.5:
        return rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()
    out = bytearray()
    while len(out) < nbytes:
        r = rng.random()
        if r < 0.06:
            out.append(0)
        elif r < 0.35:
            out.append(1)
        elif r < 0.55:
            ln = 4 if rng.random() < 0.8 else int(rng.choice([0, 1, 2, 3, 5, 6, 40]))
            out += bytes([2, ln]) + rng.integers(0, 256, max(ln - 2, 0), dtype=np.uint8).tobytes()
        elif r < 0.75:
            ln = 3 if rng.random() < 0.8 else int(rng.choice([0, 1, 2, 4, 5, 200]))
            out += bytes([3, ln]) + rng.integers(0, 256, min(max(ln - 2, 0), 8), dtype=np.uint8).tobytes()
        else:
            ln = int(rng.integers(2, 9)) if rng.random() < 0.85 else int(rng.integers(0, 256))
            out += bytes([int(rng.integers(4, 256)), ln]) + \
                rng.integers(0, 256, min(max(ln - 2, 0), 8), dtype=np.uint8).tobytes()
    return bytes(out[:nbytes])


def _rx_tcp_frame(rng, src):
    ihl = 5 if rng.random() < 0.6 else int(rng.integers(5, 16))
    r = rng.random()
    doff = 5 if r < 0.3 else int(rng.integers(0, 5)) if r < 0.36 else int(rng.integers(5, 16))
    nopt = 4 * max(doff - 5, 0)
    if rng.random() < 0.06:                      # 4 * doff exceeds the datagram
        nopt = int(rng.integers(0, nopt + 1)) & ~3 if nopt else 0
        pay = b"" if nopt < 4 * max(doff - 5, 0) else src[:3].tobytes()
    else:
        r = rng.random()
        ln = 0 if r < 0.3 else int(rng.integers(1, 40)) if r < 0.6 else int(rng.integers(1, 1461))
        o = int(rng.integers(0, src.size - ln + 1))
        pay = src[o:o + ln].tobytes()
    opts = _rx_options(rng, nopt)
    kw = {}
    if rng.random() < 0.05:                      # the IPv4 total length announces less
        kw["dgram_len"] = max(0, 20 + len(opts) + len(pay) - int(rng.integers(1, 30)))
    return R.tcp_frame(src=R.PEER_IP + int(rng.integers(0, 4)), dst=R.LOCAL_IP + int(rng.integers(0, 2)),
                       sport=int(rng.integers(1024, 1064)), dport=int(rng.choice([80, 81, 443])),
                       seq=int(rng.integers(0, 1 << 32)), ack=int(rng.integers(0, 1 << 32)),
                       flags=int(rng.integers(0, 0x1000)), window=int(rng.integers(0, 65536)),
                       ihl=ihl, doff=doff, opts=opts, payload=pay,
                       trailing=rng.integers(0, 256, int(rng.integers(1, 18)), dtype=np.uint8).tobytes()
                       if rng.random() < 0.2 else b"", pad60=rng.random() < 0.3, **kw)


def _rx_table(rng, frames, e):
    """A random third of the accepted TCP tuples, near misses of others (one field +-1, local
    and remote swapped), 0-3000 random extra keys; sorted by the model's CompareKeys order."""
    keys = [R.key_of(frames[i]) for i in np.nonzero(e.segs["opts"] & R.SEG_VALID)[0]]
    keys = list(dict.fromkeys(keys))
    chosen, near = [], []
    for k in keys:
        r = rng.random()
        if r < 1 / 3:
            chosen.append(k)
        elif r < 0.6:
            q = list(k)
            if rng.random() < 0.3:
                q = [k[1], k[0], k[3], k[2]]
            else:
                f = int(rng.integers(0, 4))
                q[f] = (q[f] + int(rng.choice([-1, 1]))) % ((1 << 32) if f < 2 else (1 << 16))
            near.append(tuple(q))
    extra = int(rng.integers(0, 3001)) if rng.random() < 0.7 else 0
    rnd = [(R.LOCAL_IP + int(a), R.PEER_IP + int(b), int(c), int(d)) for a, b, c, d in zip(
        rng.integers(0, 3, extra), rng.integers(0, 6, extra), rng.integers(1, 65536, extra),
        rng.integers(1, 65536, extra))]
    allk = list(dict.fromkeys(chosen + near + rnd))
    if not allk:
        return None
    return R.model_sort(R.table([k + (7 + i,) for i, k in enumerate(allk)], A.TCP_PCB_KEY_DTYPE))


def tcprx_scenario(oracle, seed):
    """1-1500 frames, half from frame_cases.frames (all nine verdict classes, filled and mutated
    already) and half from tcprx_cases.tcp_frame with IHL 5-15, data offset 0-15, structured or
    uniform option bytes, option lengths that make 4 * doff exceed the datagram, trailing bytes,
    padding to 60 bytes and an IPv4 total length that announces less than there is; these get
    their checksums from the oracle's Tx fill. About one frame in ten is then corrupted by one
    bit. Frame 0 is a valid TCP frame and stays whole; from 8 frames on, the last one has data
    offset 3. The tuples of the tcp_frame frames come from a small pool (4 peers x 2 local
    addresses x 40 x 3 ports) so that tuples repeat and near misses are close.
    The slotted form takes the frames that fit its stride (the others cannot lie in a slot), a
    few TCP frames with a length above the stride."""
    rng = np.random.default_rng(7000 + seed)
    n = _count(rng)
    src = blob(rng, 1 << 14)
    own = rng.random(n) < 0.5
    own[0] = True
    if n >= 8:
        own[n - 1] = True
    made = []
    for i in np.nonzero(own)[0]:
        if i == 0:
            made.append(R.tcp_frame(sport=1024, opts=struct.pack(">BBH", 2, 4, 1460), doff=6,
                                    payload=src[:int(rng.integers(0, 100))].tobytes()))
        elif i == n - 1 and n >= 8:
            made.append(R.tcp_frame(doff=3, sport=1025, payload=src[:9].tobytes()))
        else:
            made.append(_rx_tcp_frame(rng, src))
    made, _ = R.fill(oracle, made)
    mixed = F.frames(seed=7000 + seed, n=int((~own).sum())) if (~own).any() else []
    frames, mi, oi = [], iter(mixed), iter(made)
    for i in range(n):
        frames.append(next(oi) if own[i] else next(mi))
    for i in np.nonzero(rng.random(n) < 0.1)[0]:
        if i and len(frames[i]) > 12:
            f = bytearray(frames[i])
            f[int(rng.integers(12, len(f)))] ^= 1 << int(rng.integers(0, 8))
            frames[i] = bytes(f)
    buf, off = F.pack(frames)
    sc = TcprxScenario()
    sc.seed, sc.n, sc.frames = seed, n, frames
    sc.verdicts = oracle.rx_verify_batch(buf, off)
    sc.tbl = _rx_table(rng, frames, R.expected(frames, sc.verdicts, None, A.TCP_RX_SEG_DTYPE))
    sc.e = R.expected(frames, sc.verdicts, sc.tbl, A.TCP_RX_SEG_DTYPE)
    sc.lead, sc.seg_shift = int(rng.integers(0, 16)), 8 * int(rng.integers(0, 2))
    # the slotted form
    stride = sc.stride = int(rng.choice(RX_STRIDES))
    fit = [f for f in frames if len(f) <= stride]
    sc.ring = rng.integers(0, 256, max(len(fit), 1) * stride, dtype=np.uint8)
    sc.lens = np.zeros(len(fit), dtype=np.uint32)
    for i, f in enumerate(fit):
        sc.ring[i * stride:i * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
        sc.lens[i] = len(f)
    for i in [i for i, f in enumerate(fit) if len(f) >= 54 and f[23] == 6][:int(rng.integers(0, 4))]:
        sc.lens[i] = stride + 1 + int(rng.integers(0, 3000))
    sc.slot_frames = [sc.ring[i * stride:i * stride + min(int(sc.lens[i]), stride)].tobytes()
                      for i in range(len(fit))]
    # (a length above the stride is clamped to it, as verify clamps it: the frame is the slot)
    sc.slot_verdicts = oracle.rx_verify_slotted(sc.ring, stride, np.minimum(sc.lens, stride)) \
        if fit else np.zeros(0, dtype=np.uint8)
    sc.slot_e = R.expected(sc.slot_frames, sc.slot_verdicts, sc.tbl, A.TCP_RX_SEG_DTYPE)
    return sc


def tcprx_option_branches(sc):
    """The branch names ParseTcpOptions takes over the scenario's parsed frames."""
    trace = []
    for i in np.nonzero(sc.e.segs["opts"] & R.SEG_VALID)[0]:
        f = sc.frames[i]
        T = 14 + (f[14] & 0xF) * 4
        R.parse_options(f[T + 20:T + (f[T + 12] >> 4) * 4], trace)
    return set(trace)


def tcprx_hit_and_miss_in_a_wave(sc):
    valid = (sc.e.segs["opts"] & R.SEG_VALID) != 0
    hit = valid & (sc.e.pcb != R.NO_PCB)
    miss = valid & (sc.e.pcb == R.NO_PCB)
    return any(hit[w:w + 64].any() and miss[w:w + 64].any() for w in range(0, sc.n, 64))
