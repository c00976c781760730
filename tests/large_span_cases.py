"""TEST INFRASTRUCTURE -- the case generators of test_gpu_large_span.py: where in the address space
the bytes of a batch lie. They need no GPU: test_large_span_cases.py runs them for fake base
pointers and checks that they cover what they are meant to cover.

The GPU tests work in one zero-filled device arena of ARENA_BYTES whose first byte has the device
address P. A case is a pure function of (P, its parameters): it names *windows* -- (arena offset,
bytes) pairs of a few hundred KiB at the most, the only places that hold non-zero bytes -- and
the elements of the batch (offsets, lengths, addresses). Every element lies either wholly inside
one window or wholly in the zero filler, so an expectation is the CPU oracle (or one of the
Python models) on a window with window-local offsets, or on one zero filler of the element's
length; no host buffer of gigabytes is ever made.

The edges: byte offsets 2^31 and 2^32 from the base handed to the entry point (the base is
P + shift, shift in SHIFTS), and A4, the smallest multiple of 2^32 strictly above P.

An element sequence that is contiguous by construction (CSR offsets) has exactly one element
across an edge, so those families take the straddle as a parameter (``kind`` in CSR_KINDS /
FRAME_KINDS) and the tests run every kind. The fixed-stride families cannot choose where a packet
lies relative to an edge; they cover what their stride gives (see strided_case, slotted_case).
"""

import numpy as np

import frame_cases as F
import hsplit_cases as H
import ipfrag_cases as I
import tcprx_cases as R
import tcpseg_cases as S

KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30
ARENA_BYTES = 5 * GiB + 64 * KiB
E31, E32 = 1 << 31, 1 << 32
EDGES = (E31, E32)
SHIFTS = (0, 1, 8, 15)
SIDE = 64 * KiB              # packets on each side of an edge: several 12 KiB wave chunks
FILL = 65535                 # the zero filler element
MAX_WINDOW = 1 * MiB
DISTANCES = (1, 15, 16, 17, "len-1")          # e - start of the element across an edge
CSR_KINDS = ("big", "ends_starts") + DISTANCES
FRAME_KINDS = ("ends_starts",) + DISTANCES


def a4_of(P):
    """The smallest multiple of 2^32 strictly above P."""
    return (P // E32 + 1) * E32


class Window:
    """`data` (uint8) at arena offset `start`."""

    def __init__(self, start, data):
        self.start, self.data = int(start), np.ascontiguousarray(data, dtype=np.uint8)

    @property
    def end(self):
        return self.start + self.data.size


def check_windows(windows):
    """Inside the arena, under 1 MiB each, disjoint."""
    ws = sorted(windows, key=lambda w: w.start)
    for w in ws:
        assert 0 <= w.start and w.end <= ARENA_BYTES and 0 < w.data.size < MAX_WINDOW
    for a, b in zip(ws, ws[1:]):
        assert a.end <= b.start, (a.start, a.end, b.start)


def _rand(rng, n):
    """Random bytes with a few runs of 0x00 and 0xFF."""
    b = rng.integers(0, 256, size=n, dtype=np.uint8)
    for _ in range(4):
        if n > 8:
            s = int(rng.integers(0, n - 4))
            b[s:s + int(rng.integers(1, 600))] = rng.choice([0x00, 0xFF])
    return b


# ---- families 1 and 2: chksum_batch_strided --------------------------------------------------

class StridedCase:
    """Packet i = `len` bytes at base + i * stride, base = P + shift. windows; `runs`: (first
    packet, count, window number) of the packets that lie in windows (the rest are filler)."""


def strided_dense(stride, plen, shift, seed=0):
    """Back to back (stride == len) or a dense gapped batch: n just large enough that the last
    packet ends >= 1 MiB past offset 2^32. One window per edge: the whole packets (gaps included,
    random too) from >= 64 KiB before the edge to >= 64 KiB after it; one more for the last 8
    packets, so that a truncated count shows. A fixed stride decides where packets lie relative
    to an edge: the one across it (or the two that meet at it) is in the window."""
    rng = np.random.default_rng(100 + seed + 7 * shift + stride)
    c = StridedCase()
    c.stride, c.len, c.shift = stride, plen, shift
    c.n = n = -(-(E32 + MiB - plen) // stride) + 1      # the last packet ends >= 1 MiB past 2^32
    c.windows, c.runs = [], []
    for e in EDGES:
        i0 = (e - SIDE) // stride - 1
        i1 = -(-(e + SIDE) // stride) + 1
        c.runs.append((i0, i1 - i0, len(c.windows)))
        c.windows.append(Window(shift + i0 * stride, _rand(rng, (i1 - i0) * stride)))
    c.runs.append((n - 8, 8, len(c.windows)))
    c.windows.append(Window(shift + (n - 8) * stride, _rand(rng, 7 * stride + plen)))
    c.edges = EDGES
    return c


SPARSE = [(8 * MiB - 16, 520), (8 * MiB, 520), (E31, 3), (E32 + 16, 2)]
GUARD = 16


def strided_sparse(stride, n, plen, shift, seed=0):
    """Strides at the host's dispatch threshold (8 MiB) and huge ones: every packet is a window
    of its own that also holds random bytes in the 16 bytes before and after it, so that a kernel
    that sums a neighbour's bytes fails."""
    rng = np.random.default_rng(200 + seed + 7 * shift + plen + stride % 1000)
    c = StridedCase()
    c.stride, c.len, c.shift, c.n = stride, plen, shift, n
    c.windows, c.runs = [], []
    for i in range(n):
        lo = min(GUARD, shift + i * stride)
        c.runs.append((i, 1, i))
        c.windows.append(Window(shift + i * stride - lo, _rand(rng, lo + plen + GUARD)))
    c.edges = EDGES
    return c


def strided_local(c, run):
    """(window, offset of the run's first packet inside it)"""
    i0, _, w = run
    return c.windows[w], c.shift + i0 * c.stride - c.windows[w].start


# ---- the contiguous layouts of families 3 and 5 ----------------------------------------------

class CsrCase:
    """offsets (uint64, n + 1, from the base P + shift); windows; runs: (first element, count,
    window number) -- the window's first byte is the first element's first byte; `across`: per
    edge the element that holds byte e (kind "ends_starts": the one that starts at it)."""


BIG_BACK = 30001    # the 65535-byte packet of kind "big" starts this far before the edge


def _csr_layout(rng, kind, shift, side, straddler, tail_fillers=17):
    lens, runs, windows, across = [], [], [], []
    at = 0
    for e in EDGES:
        pre, post = side(rng), side(rng)
        mid = None if kind == "ends_starts" else straddler(rng, kind)
        d = 0 if mid is None else BIG_BACK if kind == "big" else \
            len(mid) - 1 if kind == "len-1" else kind
        assert mid is None or 0 < d < len(mid)
        items = pre + ([mid] if mid is not None else []) + post
        ws = e - d - sum(len(p) for p in pre)
        q, r = divmod(ws - at, FILL)
        assert ws >= at
        lens += [FILL] * q + ([r] if r else [])
        runs.append((len(lens), len(items), len(windows)))
        across.append(len(lens) + len(pre))
        data = np.concatenate([np.frombuffer(bytes(p), dtype=np.uint8) for p in items])
        windows.append(Window(shift + ws, data))
        lens += [len(p) for p in items]
        at = ws + data.size
    lens += [FILL] * tail_fillers
    c = CsrCase()
    c.kind, c.shift = kind, shift
    c.offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(np.array(lens, dtype=np.uint64), out=c.offsets[1:])
    c.lens = np.array(lens, dtype=np.int64)
    c.n = len(lens)
    c.windows, c.runs, c.across, c.edges = windows, runs, across, EDGES
    c.in_window = np.zeros(c.n, dtype=bool)
    for i0, cnt, _ in runs:
        c.in_window[i0:i0 + cnt] = True
    return c


def csr_local(c, run):
    """(window, window-local uint64 offsets of the run's elements)"""
    i0, cnt, w = run
    return c.windows[w], c.offsets[i0:i0 + cnt + 1] - c.offsets[i0]


N_FILL_STATES = 8


def csr_case(kind, shift, seed=0):
    """Family 3. Filler packets are 65535 zero bytes (and at most one shorter one in front of
    each window). Each window: 150 packets of 0-1600 bytes on either side of the edge (>= 64 KiB
    each) and the one across it by `kind`: "big" = a 65535-byte packet, "ends_starts" = none (a
    packet ends at the edge and the next starts there), else a packet of 20-1600 bytes that
    starts that many bytes before it. `states` for the seeded form: random in the windows, one of
    N_FILL_STATES values on the filler (so that its expectation is a handful of oracle calls)."""
    rng = np.random.default_rng(300 + seed + 16 * CSR_KINDS.index(kind) + shift)

    def side(rng):
        while True:
            ln = rng.integers(0, 1601, 150)
            ln[rng.integers(0, 150, 6)] = 0
            if ln.sum() >= SIDE:
                return [_rand(rng, int(l)).tobytes() for l in ln]

    def straddler(rng, kind):
        return _rand(rng, FILL if kind == "big" else int(rng.integers(20, 1601))).tobytes()

    c = _csr_layout(rng, kind, shift, side, straddler)
    c.fill_states = rng.integers(0, 1 << 32, N_FILL_STATES, dtype=np.uint32)
    c.fill_states[0], c.fill_states[1] = 0, 0xFFFFFFFF
    c.states = c.fill_states[rng.integers(0, N_FILL_STATES, c.n)]
    c.states[c.in_window] = rng.integers(0, 1 << 32, int(c.in_window.sum()), dtype=np.uint32)
    return c


# ---- frames -------------------------------------------------------------------------------------

_pool = {}


def frame_pool(oracle):
    """Frames for the frame families, made once: frame_cases.frames (every verdict class, the
    ones the oracle rejects included) and tcprx_cases frames (geometry, padding, bad offsets)
    with checksums by the oracle's Tx fill; every frame at least 18 bytes (so that every straddle
    distance fits) -- the shorter ones of frame_cases are kept for the sides."""
    if "pool" not in _pool:
        made, _ = R.fill(oracle, R.geometry_frames()[::7] + R.padding_frames() +
                         [f for f, _ in R.bad_offset_frames()])
        _pool["pool"] = F.frames(seed=20261020, n=700) + made
    return _pool["pool"]


def jumbo_frames(oracle):
    """TCP and UDP frames of 40000, 65521 and 65535 bytes (filled by the oracle): the only ones
    that can reach an edge from the start of a 64 KiB slot."""
    if "jumbo" not in _pool:
        rng = np.random.default_rng(77)
        fr = []
        for total in (40000, 65521, 65535):
            fr.append(R.tcp_frame(payload=_rand(rng, total - 54).tobytes(), sport=5000 + len(fr)))
            fr.append(H.udp_segment(_rand(rng, total - 42).tobytes())[0])
        _pool["jumbo"] = R.fill(oracle, fr)[0]
    return _pool["jumbo"]


def frames_csr_case(oracle, kind, shift, seed=0):
    """Family 5. Filler frames are 65535 zero bytes: 64 of them span 4,194,240 bytes, inside the
    4 MiB contract of the frame batches. Each window: >= 100 frames and >= 64 KiB on either side
    of the edge (three 64-frame header windows and more) and the frame across it by `kind`:
    distances 1 (the Ethernet header straddles), 15, 16, 17 (the IPv4 header does), "len-1"."""
    rng = np.random.default_rng(500 + seed + 16 * FRAME_KINDS.index(kind) + shift)
    pool = frame_pool(oracle)

    def side(rng):
        out, total = [], 0
        while len(out) < 100 or total < SIDE:
            out.append(pool[int(rng.integers(0, len(pool)))])
            total += len(out[-1])
        return out

    def straddler(rng, kind):
        while True:
            f = pool[int(rng.integers(0, len(pool)))]
            if len(f) >= 60 and f[12:14] == b"\x08\x00":
                return f

    c = _csr_layout(rng, kind, shift, side, straddler)
    c.frames = {}
    for i0, cnt, w in c.runs:
        o = (c.offsets[i0:i0 + cnt + 1] - c.offsets[i0]).astype(np.int64)
        d = c.windows[w].data
        c.frames[w] = [d[o[k]:o[k + 1]].tobytes() for k in range(cnt)]
    return c


def span_of_64(offsets):
    """The largest span of 64 consecutive frames."""
    o = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    k = min(64, o.size - 1)
    return int((o[k:] - o[:-k]).max())


def pcb_table(frames, verdicts, dtype):
    """A small table (model order) with every second accepted TCP tuple of `frames`."""
    ks = [R.key_of(f) for f, v in zip(frames, verdicts) if v == R.ACCEPT and f[23] == 6][::2]
    ks = list(dict.fromkeys(ks))
    return R.model_sort(R.table([k + (11 + i,) for i, k in enumerate(ks)], dtype))


# ---- family 4: ring slots ---------------------------------------------------------------------

SLOTTED = [(65536, 65536 + 64), (65521, 65600)]


class SlottedCase:
    """Slot i = lens[i] bytes at base + i * stride. Every slot with a length is a window of its
    own (its bytes, then up to 16 random bytes more where the slot has room); `slots`: their
    numbers, in window order; `frames`: their bytes as a list."""


def _slot_windows(stride, n):
    """The 128 slots round each edge's slot (fewer where the ring ends first)."""
    return [list(range(e // stride - 64, min(e // stride + 64, n))) for e in EDGES]


def slotted_case(stride, n, shift, seed=0, frames=None, jumbo=None):
    """128 slots round slot 2^31 / stride and 128 round 2^32 / stride; lengths 0 elsewhere.
    Checksum form (frames None): lengths 0-1600, every 16th up to the stride, and the four slots
    round each edge full (min(stride, 65535) bytes): with stride 65536 one ends a byte before the
    edge and the next starts at it, with 65521 the edge lies inside one. Frame forms: `frames`
    drawn at random, with `jumbo` frames in the four slots round each edge (the two longest that
    fit the stride in the slot before the edge and the one at it)."""
    rng = np.random.default_rng(400 + seed + shift + stride)
    c = SlottedCase()
    c.stride, c.n, c.shift = stride, n, shift
    c.lens = np.zeros(n, dtype=np.uint32)
    c.windows, c.slots, c.frames = [], [], []
    full = min(stride, FILL)
    for e, idx in zip(EDGES, _slot_windows(stride, n)):
        mid = e // stride
        for j, i in enumerate(idx):
            near = mid - 2 <= i <= mid + 1
            if frames is None:
                ln = full if near else int(rng.integers(0, full + 1)) if j % 16 == 5 \
                    else int(rng.integers(0, 1601))
                body = _rand(rng, ln)
            else:
                fits = sorted((f for f in jumbo if len(f) <= stride), key=len)
                f = fits[-1 - (i - mid) % 2] if i in (mid - 1, mid) \
                    else fits[int(rng.integers(0, len(fits)))] if near \
                    else frames[int(rng.integers(0, len(frames)))]
                ln, body = len(f), np.frombuffer(f, dtype=np.uint8)
            c.lens[i] = ln
            if ln == 0:
                continue
            slack = _rand(rng, min(GUARD, stride - ln))
            c.slots.append(i)
            c.frames.append(body.tobytes())
            c.windows.append(Window(shift + i * stride, np.concatenate([body, slack])))
    c.edges = EDGES
    return c


# ---- family 6: absolute addresses ---------------------------------------------------------------

HALF = 128 * KiB
FAR_BYTES = 64 * KiB


class AbsCase:
    """P, a4 (arena offset of A4), windows: [0] round A4, [1] low, [2] more than 2^32 above it;
    `mirror` (the windows' bytes back to back, for the oracle) and `local(arena offset)`."""

    def local(self, off):
        at = 0
        for w in self.windows:
            if w.start <= off < w.end:
                return at + off - w.start
            at += w.data.size
        raise ValueError("offset outside every window")

    def has(self, off, ln):
        return any(w.start <= off and off + ln <= w.end for w in self.windows)


def abs_windows(P, seed=0):
    rng = np.random.default_rng(600 + seed)
    c = AbsCase()
    c.P, c.a4 = P, a4_of(P) - P
    lo = max(0, c.a4 - HALF)
    far = 512 * MiB + 10
    if abs(c.a4 - far) < 2 * MiB:
        far = 256 * MiB + 10
    c.far_low, c.far_high = far, far + E32 + 4099
    c.windows = [Window(lo, _rand(rng, c.a4 + HALF - lo)), Window(c.far_low, _rand(rng, FAR_BYTES)),
                 Window(c.far_high, _rand(rng, FAR_BYTES))]
    c.mirror = np.concatenate([w.data for w in c.windows])
    return c


def chain_case(P, seed=0):
    """Chains (lists of (arena offset, length) chunks) round A4: wholly below, wholly above,
    across it by every distance of DISTANCES, ending and starting at it, starting at every
    residue mod 16 across it, back to back across it (the column-run path of the JUST_WRITTEN
    hint) with a chunk boundary at, before and after A4, two chunks more than 2^32 bytes apart in
    both orders, and the chunk at A4 first with a low one second. `states` are random."""
    c = abs_windows(P, seed)
    rng = np.random.default_rng(650 + seed)
    a4, ch = c.a4, []
    below = min(a4, HALF)                      # bytes of window 0 below A4
    c.groups = {}

    def add(group, chunks):
        c.groups.setdefault(group, []).append(len(ch))
        ch.append([(int(o), int(l)) for o, l in chunks])

    for ln in (1, 2, 700, 1460):
        if below >= 3 * ln + 40:
            add("below", [(a4 - 3 * ln - 33, ln), (a4 - ln - 7, ln)])
        add("above", [(a4 + 5, ln), (a4 + 2 * ln + 40, ln)])
    add("ends_at", [(a4 - min(below, 1500), min(below, 1500))])
    add("starts_at", [(a4, 1500)])
    for ln in (100, 1460, 9000, FILL):
        for d in DISTANCES:
            dd = ln - 1 if d == "len-1" else d
            if dd <= below:
                add("across", [(a4 - dd, ln)])
    for r in range(16):
        start = (max(a4 - 64, 0) & ~15) + r
        if start >= a4 and a4 >= 16:
            start -= 16
        add("residue", [(start, 200)])
    if below >= 3000:
        add("back_to_back", [(a4 - 2920 + k * 1460, 1460) for k in range(5)])       # boundary at A4
        add("back_to_back", [(a4 - 2000 + k * 1460, 1460) for k in range(4)])       # A4 in a chunk
        add("back_to_back", [(a4 - 2921 + k * 1461, 1461) for k in range(5)])       # odd lengths
        add("back_to_back", [(a4 - 3000, 2999), (a4 - 1, 2), (a4 + 1, 3000)])
    add("back_to_back", [(a4 + k * 9000, 9000) for k in range(3)])
    add("far", [(c.far_low, 1460), (c.far_high, 1460)])
    add("far", [(c.far_high + 3, 1461), (c.far_low + 5, 777)])
    add("far", [(a4, 1460), (c.far_low + 4000, 1460)])                               # A4 first
    add("far", [(c.far_low + 9001, 33), (a4, 1)])
    c.chains = ch
    for chain in ch:
        for o, l in chain:
            assert c.has(o, l), (o, l)
    c.states = rng.integers(0, 1 << 32, len(ch), dtype=np.uint32)
    c.states[::5] = 0
    return c


def chain_table(c):
    """(addr uint64, len uint32, index uint64) with the arena at device address c.P."""
    addr = np.array([c.P + o for chn in c.chains for o, _ in chn], dtype=np.uint64)
    ln = np.array([l for chn in c.chains for _, l in chn], dtype=np.uint32)
    idx = np.zeros(len(c.chains) + 1, dtype=np.uint64)
    idx[1:] = np.cumsum([len(chn) for chn in c.chains])
    return addr, ln, idx


def chain_expected(oracle, c, mirror=None):
    """The final checksums of the chains by the oracle, on the windows' bytes."""
    m = c.mirror if mirror is None else mirror
    return np.array([oracle.chain(int(s), m, [(c.local(o), l) for o, l in chn])
                     for chn, s in zip(c.chains, c.states)], dtype=np.uint16)


FIELD_ZONE = 64        # bytes on either side of A4 that the chain-fill chains leave alone


def chain_fill_case(P, seed=0):
    """Chains that leave the FIELD_ZONE bytes on either side of A4 alone: below the zone, above
    it, back to back on either side, both sides in one chain in both orders, and the far ones.
    The zone reads zero, and chain i's checksum field is two bytes of it: below A4, above it, and
    (chain 1) the one byte on either side of it. The last two chains get field address 0."""
    c = abs_windows(P, seed)
    rng = np.random.default_rng(660 + seed)
    lo, hi = max(c.a4 - FIELD_ZONE, 0), c.a4 + FIELD_ZONE
    room = lo - c.windows[0].start
    ch = []
    for ln in (1, 2, 700, 1460):
        if room >= 3 * ln + 33:
            ch.append([(lo - 3 * ln - 33, ln), (lo - ln, ln)])
            ch.append([(hi + 7, ln), (lo - ln, ln)])
            ch.append([(lo - 2 * ln, 2 * ln), (hi, ln)])
        ch.append([(hi, ln), (hi + 2 * ln + 41, ln)])
        ch.append([(hi + 3 * ln, ln + 1)])
    if room >= 4380:
        ch.append([(lo - 4380 + k * 1460, 1460) for k in range(3)])
    ch.append([(hi + k * 1461, 1461) for k in range(3)])
    ch.append([(c.far_low, 1460), (c.far_high, 1460)])
    ch.append([(c.far_high + 3, 1461), (c.far_low + 5, 777)])
    ch.append([(hi, 1460), (c.far_low + 4000, 1460)])
    ch.append([(c.far_low + 9001, 33), (hi + 1, 1)])
    c.chains = [[(int(o), int(l)) for o, l in chn] for chn in ch]
    for chn in c.chains:
        for o, l in chn:
            assert c.has(o, l) and (o + l <= lo or o >= hi)
    c.states = rng.integers(0, 1 << 32, len(ch), dtype=np.uint32)
    c.states[::5] = 0
    w = c.windows[0]
    w.data[lo - w.start:hi - w.start] = 0
    c.mirror = np.concatenate([x.data for x in c.windows])
    slots = [o for o in range(lo + 1, hi - 2, 3)         # odd and even addresses, disjoint
             if o + 2 <= c.a4 - 1 or o >= c.a4 + 1]
    c.fields = np.zeros(len(c.chains), dtype=np.uint64)
    c.field_off = [None] * len(c.chains)
    order = [i for i in range(len(c.chains) - 2) if i != 1]
    assert len(slots) >= len(order)
    for k, i in enumerate(order):                        # spread over the zone, both sides of A4
        c.field_off[i] = slots[k * len(slots) // len(order)]
    c.field_off[1] = c.a4 - 1
    used = [o for o in c.field_off if o is not None]
    assert len(set(used)) == len(used)
    for i, o in enumerate(c.field_off):
        if o is not None:
            c.fields[i] = P + o
    return c


def _abs_pieces(c, rng, most):
    """Two-piece ranges (window-0-local offsets) for the Tx builders: across A4 by every distance,
    ending and starting at it, the boundary between the pieces at A4, wholly below and above."""
    w = c.windows[0]
    a = c.a4 - w.start                          # A4, window-local
    out = []
    for d in (1, 15, 16, 17):
        if a >= d:
            out.append(((a - d, most), (int(rng.integers(0, w.data.size - most)), 333)))
    if a >= most:
        out.append(((a - most + 1, most), (0, 0)))                   # len - 1 before A4
        out.append(((a - most, most), (a, most)))                    # pieces meet at A4
        out.append(((int(rng.integers(0, a - most + 1)), most // 2), (a - most // 3, most)))
    out.append(((a, most), (a + 2 * most, 17)))
    out.append(((a + 7, most), (0, 0)))
    return out


def tcpseg_abs_case(oracle, P, seed=0):
    """Bursts whose data pieces lie round A4 (tcpseg_cases model; payload = window 0)."""
    c = abs_windows(P, seed)
    rng = np.random.default_rng(700 + seed)
    cases = []
    for j, (p0, p1) in enumerate(_abs_pieces(c, rng, 5000)):
        cases.append(S.burst(p0, p1, mss=(1460, 536, 999, 4999)[j % 4], seq=0xFFFFF000 + j,
                             ip_id=0xFFFE + j & 0xFFFF, psh_offset=j * 500,
                             flags=S.FIN if j % 3 == 0 else 0))
    c.batch = S.Batch(cases, c.windows[0].data)
    c.si, c.cb = S.caller_index(cases)
    c.e = S.expected(oracle, c.batch, c.si, c.cb)
    c.base_addr = P + c.windows[0].start
    return c


def ipfrag_abs_case(oracle, P, seed=0):
    """Datagrams whose payload pieces lie round A4 (ipfrag_cases model; payload = window 0)."""
    c = abs_windows(P, seed)
    rng = np.random.default_rng(800 + seed)
    cases = []
    for j, (p0, p1) in enumerate(_abs_pieces(c, rng, 5000)):
        cases.append(I.dgram(p0, p1, mtu=I.MTUS[j % len(I.MTUS)], ip_id=0x4000 + j))
    c.batch = I.Batch(cases, c.windows[0].data)
    c.fi, c.cb = I.caller_index(cases)
    c.e = I.expected(oracle, c.batch, c.fi, c.cb)
    c.base_addr = P + c.windows[0].start
    return c


def hsplit_abs_case(oracle, P, split_frames, seed=0):
    """Header-split segments whose payload chunks lie round A4: exact-length TCP and UDP segments
    of hsplit_cases, headers in a small ring of their own, each segment's payload one or two
    chunks of window 0 at the places of _abs_pieces (the window's bytes are the payload, so the
    segments are built from them). `split_frames` = aipstack_amd.SplitFrames."""
    c = abs_windows(P, seed)
    rng = np.random.default_rng(900 + seed)
    d = c.windows[0].data
    stride = 64
    pieces = _abs_pieces(c, rng, 1460)
    headers = np.full(len(pieces) * stride, 0xEE, dtype=np.uint8)
    hdr_lens = np.zeros(len(pieces), dtype=np.uint32)
    chunks = []
    for j, ((o0, l0), (o1, l1)) in enumerate(pieces):
        pay = d[o0:o0 + l0].tobytes() + d[o1:o1 + l1].tobytes()
        f, h = (H.tcp_segment(pay)[0], 54) if j % 2 == 0 else (H.udp_segment(pay)[0], 42)
        headers[j * stride:j * stride + h] = np.frombuffer(f[:h], dtype=np.uint8)
        hdr_lens[j] = h
        chunks.append([(o, l) for o, l in ((o0, l0), (o1, l1)) if l])
    c.sp = split_frames(headers, stride, hdr_lens, d, chunks)
    c.want_h, c.want_st, _, c.ok = H.expected(oracle, c.sp)
    c.base_addr = P + c.windows[0].start
    return c


def pieces_cover(c, pieces):
    """Which of the distances 1, 15, 16, 17 before A4 some piece of `pieces` starts at, and
    whether one ends at it and one starts at it (window-0-local offsets)."""
    a = c.a4 - c.windows[0].start
    flat = [p for pp in pieces for p in pp if p[1]]
    return ({a - o for o, l in flat if o < a < o + l}, any(o + l == a for o, l in flat),
            any(o == a for o, l in flat))


# ---- family 6: the header ring of the Tx builders across offsets 2^31 and 2^32 ------------------

RING_STRIDE = 65536
RING_SLOTS = 65536 + 300
NEAR = 256


def ring_rows(n, every=61):
    """(rows within NEAR of slot 2^31 / 65536 and of slot 2^32 / 65536, clipped to the ring; those
    plus every `every`-th row: the rows compared with the model in full)."""
    near = np.concatenate([np.arange(e // RING_STRIDE - NEAR, min(e // RING_STRIDE + NEAR + 1, n))
                           for e in EDGES])
    return near, np.union1d(near, np.arange(0, n, every))


class RingCase:
    """n header slots of RING_STRIDE bytes from the base P + shift (the builders' d_hdr): slot
    32768 starts at offset 2^31, slot 65536 at 2^32. `near`, `rows` (ring_rows); `headers`: the
    model's header bytes of `rows` ((len(rows), 64), zero past each header); the payload lies in
    a small buffer of its own (`payload`), addressed by the offsets of the chunk table."""


def hsplit_ring_case(oracle, split_frames):
    """tx_fill_header_split: the rows of `near` hold exact-length TCP segments (54-byte headers,
    333 payload bytes each, one chunk), every other slot is a zero filler header of 54 bytes
    without chunks, whose status the model gives (it must stay untouched). in_h / want_h: the
    near rows' 64 slot bytes before and after the fill."""
    c = RingCase()
    c.n = n = RING_SLOTS
    c.near, _ = ring_rows(n)
    k = c.near.size
    slots, hdr_lens, payload, _ = H.ring_batch(k, seed=31, payload_len=333, stride=64)
    c.sp = split_frames(slots, 64, hdr_lens, payload, [[(j * 333, 333)] for j in range(k)])
    c.in_h = slots.reshape(k, 64).copy()
    want_h, c.want_near, _, ok = H.expected(oracle, c.sp)
    assert ok.all()
    c.want_h = want_h.reshape(k, 64)
    c.payload = payload
    filler = split_frames(np.zeros(64, dtype=np.uint8), 64, np.array([54], dtype=np.uint32),
                          payload, [[]])
    fh, fst, _, _ = H.expected(oracle, filler)
    assert not fh.any()                                       # the model leaves a filler as it is
    c.want_st = np.full(n, fst[0], dtype=np.uint8)
    c.want_st[c.near] = c.want_near
    c.hdr_lens = np.full(n, 54, dtype=np.uint32)
    c.chunk_off = np.arange(k, dtype=np.int64) * 333
    c.chunk_len = np.full(k, 333, dtype=np.uint32)
    has = np.zeros(n, dtype=np.int64)
    has[c.near] = 1
    c.chunk_index = np.zeros(n + 1, dtype=np.uint64)
    c.chunk_index[1:] = np.cumsum(has)
    return c


TS_RING_BURSTS = [(10000, 1), (22768, 3), (20000, 2), (12700, 7), (300, 5), (RING_SLOTS - 65768, 4)]


def tcpseg_ring_case(oracle):
    """tcp_tx_segment: six bursts with mss 1-7 give RING_SLOTS segments; one burst ends with slot
    32767 (the next starts in the slot at 2^31), one holds slot 65536. The chunk table is the
    model's for every segment; the headers for `rows`."""
    rng = np.random.default_rng(41)
    c = RingCase()
    c.payload = _rand(rng, 160 * KiB)
    cases = []
    for j, (segs, mss) in enumerate(TS_RING_BURSTS):
        D = segs * mss - (mss // 2)                           # a short last segment
        l0 = int(rng.integers(1, D))
        cases.append(S.burst((int(rng.integers(0, 50 * KiB)), l0),
                             (80 * KiB + int(rng.integers(0, 9)), D - l0), mss=mss,
                             seq=0xFFFF0000 + 977 * j, ip_id=0xF000 + 4001 * j & 0xFFFF,
                             psh_offset=D // 2, flags=S.FIN if j % 2 else 0))
    c.batch = S.Batch(cases, c.payload)
    c.si, c.cb = S.caller_index(cases)
    c.n = n = int(c.si[-1])
    c.near, c.rows = ring_rows(n)
    nc = int(c.cb[-1])
    c.chunk_off, c.chunk_len = np.zeros(nc, dtype=np.int64), np.zeros(nc, dtype=np.uint32)
    c.chunk_index = np.zeros(n + 1, dtype=np.uint64)
    c.chunk_index[n] = nc
    c.headers = np.zeros((c.rows.size, 64), dtype=np.uint8)
    c.row_chunks = []
    want = set(c.rows.tolist())
    at, r = 0, 0
    for b, cs in enumerate(cases):
        assert S.descriptor_ok(cs)
        segs = S.segments_of(cs)
        for k, (start, ln, chunks) in enumerate(segs):
            i = int(c.si[b]) + k
            c.chunk_index[i] = at
            for o, l in chunks:
                c.chunk_off[at], c.chunk_len[at] = o, l
                at += 1
            if i in want:
                c.headers[r, :S.HDR] = np.frombuffer(S.segment_header(
                    oracle, cs, c.payload, k, start, ln, chunks, k == len(segs) - 1), dtype=np.uint8)
                c.row_chunks.append(chunks)
                r += 1
    assert at == nc and r == c.rows.size
    return c


def ipfrag_ring_case(oracle):
    """udp_tx_fragment: 244 datagrams of 60000-65527 bytes with mtu 256 (232 data bytes per
    fragment) give just over 65536 fragments. The chunk table and the header lengths are the
    model's for every fragment; the headers for `rows`."""
    rng = np.random.default_rng(43)
    c = RingCase()
    c.payload = _rand(rng, 160 * KiB)
    cases = []
    for j in range(244):
        D = 65527 if j % 7 == 0 else int(rng.integers(60000, 65528))
        l0 = int(rng.integers(1, D))
        cases.append(I.dgram((int(rng.integers(0, 14 * KiB)), l0),
                             (80 * KiB + int(rng.integers(0, 14 * KiB)), D - l0), mtu=256,
                             ip_id=0xFF00 + 37 * j & 0xFFFF, sport=1000 + j))
    c.batch = I.Batch(cases, c.payload)
    c.fi, c.cb = I.caller_index(cases)
    c.n = n = int(c.fi[-1])
    c.near, c.rows = ring_rows(n)
    nc = int(c.cb[-1])
    c.chunk_off, c.chunk_len = np.zeros(nc, dtype=np.int64), np.zeros(nc, dtype=np.uint32)
    c.chunk_index = np.zeros(n + 1, dtype=np.uint64)
    c.chunk_index[n] = nc
    c.hdr_len = np.zeros(n, dtype=np.uint32)
    c.headers = np.zeros((c.rows.size, 64), dtype=np.uint8)
    c.row_chunks = []
    want = set(c.rows.tolist())
    at, r = 0, 0
    for d, cs in enumerate(cases):
        assert I.descriptor_ok(cs)
        chk = I.udp_checksum(oracle, cs, c.payload)
        for k, (off, ln, mf, chunks) in enumerate(I.fragments_of(cs)):
            i = int(c.fi[d]) + k
            c.chunk_index[i] = at
            c.hdr_len[i] = I.HDR0 if k == 0 else I.HDRK
            for o, l in chunks:
                c.chunk_off[at], c.chunk_len[at] = o, l
                at += 1
            if i in want:
                h = I.fragment_header(oracle, cs, off, ln, mf, chk)
                assert len(h) == c.hdr_len[i]
                c.headers[r, :len(h)] = np.frombuffer(h, dtype=np.uint8)
                c.row_chunks.append(chunks)
                r += 1
    assert at == nc and r == c.rows.size
    return c


def ring_frames(c, headers, hdr_len):
    """The rows of c.rows as linear frames: `headers` ((rows, 64), as the device left them), the
    first hdr_len[r] bytes of each, then the payload bytes of the model's chunks."""
    return [headers[r, :int(hdr_len[r])].tobytes() +
            b"".join(c.payload[o:o + l].tobytes() for o, l in c.row_chunks[r])
            for r in range(c.rows.size)]
