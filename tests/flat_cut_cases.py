"""TEST INFRASTRUCTURE -- the inputs of test_gpu_flat_cut.py: the four flat checksum batches
(strided, CSR, seeded CSR, ring slots) at every packet length and every start address mod 16, in
every kernel form the dispatch of chksum_kernels.hip can select. A length or alignment test that is
off by a few bytes gives a wrong sum, not a fault; only a sweep finds it.

Lengths. DENSE is 0..272 (the 64-byte short-run threshold, the 192-byte chunk halving, two 128-byte
lines, 17 segments). EDGE is [T - 17, T + 17] round every threshold of the dispatch, and
65502..65535. The thresholds as the code has them (launch_short_runs, launch_gapped,
chksum_batch_kernel): packets per chunk halve where cp * len crosses 12288 (384, 768, 1536, 3072,
6144; 192 lies in DENSE); 1024 (column runs); 8192 (SU 48 / 50); 12288 (a one-packet chunk's 12 KiB);
32768 (gapped columns: ns <= 2048 segments). The code has one more that the issue's list lacks: a
run of more than kSegTabMax = 1536 segments (24576 bytes: one packet at chunk_packets 1, two of 12288,
sixteen of 1536) leaves the segment-table and stream forms for the per-packet wave mode, so 24576 is
in THRESHOLDS too.

Layouts (LAYOUTS): "b2b" strided with stride == len; "gap16" strided at the next multiple of 16
above len + 1; "odd" strided at a stride = 1 mod 16 with n >= 67, so that one launch meets all 16
start alignments and ends in a partial chunk; "csr" and "seeded", one batch that holds every
(length, start mod 16) pair (a pad packet of 0..15 bytes in front of each brings it to its start;
empty packets at the front, in the middle and at the end; the first offset is odd); "slotted", the
pairs in slots of 2048 bytes (lengths up to 2048) and 65536 bytes (the rest), and DENSE again in
slots of 273 bytes (odd) and lengths up to 1584 in slots of 1584 bytes; in each the last slot's
length equals the stride. Start alignments of strided and slotted calls come from the base.

Forms (FORMS): name -> (tunables, just_written). A batch below 16 chunks of 64 packets per CU
(262,144 packets on 256 CUs) is "small": with chunk_packets 0 it bypasses short runs, column runs
and gapped columns for the generic kernel, so a small batch reaches those only with chunk_packets
forced; every form but "default" and the gather / stream forms without a chunk size forces it.
"large" is chunk_packets 0 on a batch above that size, the dispatch production batches get; it is
no entry of FORMS because its batches are built otherwise (large_strided, large_plan): a strided
batch repeats 67 packets of the random buffer on the device, CSR and ring slots repeat DENSE. The
default form gets every pair (full=True); every other form, "large" included, all of DENSE at all
16 starts and EDGE at starts 0, 1, 8, 15, except what LARGE_EXEMPT lists with its reason.

Exclusions (EXEMPT, by layout): none. Where a layout cannot place a pair in one call it places it
in another (a base shift), so every layout's default plan holds every pair. LARGE_EXEMPT: the
lengths the large form leaves out, by layout.

Families: A lengths over synth.random_bytes; B values (crafted packets whose sum is a non-zero
multiple of 0xFFFF beside all-zero twins, and three saturating patterns); C one mixed batch of 513
packets laid out twice, the second time with every byte outside every packet inverted.

Nothing here needs a GPU or torch; expectations come from the CPU oracle alone."""
import numpy as np

from aipstack_amd import synth

GUARD = 256                      # bytes in front of the first and behind the last packet of a buffer
OUT_GUARD = 64                   # uint16 elements on each side of the results
POISON16 = 0xC3C3
DENSE = list(range(273))
THRESHOLDS = (384, 768, 1024, 1536, 3072, 6144, 8192, 12288, 24576, 32768)
EDGE = sorted({t + d for t in THRESHOLDS for d in range(-17, 18)} | set(range(65502, 65536)))
LENGTHS = sorted(set(DENSE) | set(EDGE))
FEW = (0, 1, 8, 15)
LAYOUTS = ("b2b", "gap16", "odd", "csr", "seeded", "slotted")
FAMILIES = ("A", "B", "C")
EXEMPT = {name: {} for name in LAYOUTS}          # {layout: {(length, start): reason}}
C_PACKETS = 513
SAT_LENGTHS = (1500, 9000, 32767, 65535)
SEED_STATES = (0, 0xFFFF, 0xFFFF0000, 0xFFFFFFFF)
LARGE_N = 256 * 16 * 64                          # pick_shape: 16 chunks of 64 packets on each of 256 CUs
# (1..17: a packet inside one 16-byte segment, which gapped column runs must leave to the gathered stream)
LARGE_LENGTHS = sorted({t + d for t in (64, 192, 384, 768, 1024, 1536, 3072, 6144, 8192) for d in (-1, 0, 1)}
                       | {1, 8, 15, 16, 17})
_TOP = tuple(range(65502, 65536))
LARGE_EXEMPT = {                                 # {layout: {length: reason}}, all starts of the length
    "b2b": {l: "262,144 packets of 64 KiB are 17 GB; above 8192 bytes the dispatch has no further threshold, "
               "and 32751..32785 run the same SU 48 kernel at one packet per chunk" for l in _TOP},
    "gap16": {l: "262,144 packets of 64 KiB are 17 GB; above ns = 2048 segments (32768 bytes) the dispatch has no "
                 "further threshold, and 32769..32785 run the same gathered stream" for l in _TOP},
    "odd": {l: "an odd stride takes launch<GappedDesc> whatever the batch's size; a large batch differs only in "
               "chunk_packets 8, which the form cp8 forces on the whole subset" for l in LENGTHS},
    "csr": {},
    "seeded": {},
    "slotted": {l: "batch_slotted_from never looks at a length: a large batch differs only in chunk_packets 16, "
                   "which the form cp16 forces on the whole subset; a ring of 262,144 slots of 65536 bytes is 17 GB"
                for l in EDGE if l > DENSE[-1]},
}
DEFAULTS = {"gather": 1, "short_loads": -1, "stream": 0, "chunk_packets": 0}

# name -> (tunables, just_written); the comment: the branch a back-to-back strided / CSR batch takes
FORMS = {
    "default": ({}, False),                                        # small: the generic kernel, stream mode SU 8
    "default-jw": ({}, True),
    "cp1": ({"chunk_packets": 1}, False),                          # short runs: prefixes SU 16 below 1024, columns
    "cp2": ({"chunk_packets": 2}, False),                          # SU 64 from 1024, SU 48 over 8192 at cp 1
    "cp4": ({"chunk_packets": 4}, False),                          # 4, 8, 32: what the default dispatch picks at
    "cp8": ({"chunk_packets": 8}, False),                          # 1536..3071, 768..1535 and 192..383 bytes
    "cp16": ({"chunk_packets": 16}, False),
    "cp32": ({"chunk_packets": 32}, False),
    "cp64": ({"chunk_packets": 64}, False),                        # columns cap the chunk at 16 packets
    "cp1-jw": ({"chunk_packets": 1}, True),                        # SU 66, SU 50 over 8192
    "cp16-jw": ({"chunk_packets": 16}, True),
    "loads0-cp16": ({"short_loads": 0, "chunk_packets": 16}, False),   # stream prefixes at every length
    "loads1-cp16": ({"short_loads": 1, "chunk_packets": 16}, False),   # global loads SU 32
    "loads2-cp16": ({"short_loads": 2, "chunk_packets": 16}, False),   # column runs at every length
    "loads2-cp1-jw": ({"short_loads": 2, "chunk_packets": 1}, True),
    "loads3-cp16": ({"short_loads": 3, "chunk_packets": 16}, False),   # segment tables SU 96
    "loads3-cp64": ({"short_loads": 3, "chunk_packets": 64}, False),   # capped at 32 packets
    "loads0-cp2": ({"short_loads": 0, "chunk_packets": 2}, False),
    "gather0": ({"gather": 0}, False),                             # the round-4 gathered stream
    "gather0-cp16": ({"gather": 0, "chunk_packets": 16}, False),
    "gather-1": ({"gather": -1}, False),                           # stream mode, 64-packet chunks
    "gather-1-cp2": ({"gather": -1, "chunk_packets": 2}, False),
    "stream-1": ({"stream": -1}, False),                           # the per-packet wave mode
    "stream-1-cp16": ({"stream": -1, "chunk_packets": 16}, False),
    "stream2-cp16": ({"stream": 2, "chunk_packets": 16}, False),
    "stream4-cp16": ({"stream": 4, "chunk_packets": 16}, False),
    "stream8-cp16": ({"stream": 8, "chunk_packets": 16}, False),
    "stream2": ({"stream": 2}, False),
    "stream8-gather0-cp2": ({"stream": 8, "gather": 0, "chunk_packets": 2}, False),
}
assert all(set(t) <= set(DEFAULTS) for t, _ in FORMS.values())


class Call:
    """One call of an entry point. kind "strided": base (byte offset in the buffer `buf`), stride,
    length, n. "csr" / "seeded": offsets (n + 1, into buf), states. "slotted": base, stride, lens.
    final: the FINAL flag. start: per packet, its byte offset in buf; plen: per packet."""

    def __init__(self, kind, buf, n, final=False, **kw):
        self.kind, self.buf, self.n, self.final = kind, buf, n, final
        self.base = self.stride = self.length = 0
        self.offsets = self.states = self.lens = None
        self.__dict__.update(kw)
        if kind == "strided":
            self.start = self.base + np.arange(n, dtype=np.int64) * self.stride
            self.plen = np.full(n, self.length, dtype=np.int64)
        elif kind == "slotted":
            self.start = self.base + np.arange(n, dtype=np.int64) * self.stride
            self.plen = np.minimum(self.lens.astype(np.int64), min(self.stride, 65535))
        else:
            self.start = self.offsets[:-1]
            self.plen = np.diff(self.offsets)


class Plan:
    """bufs {name: uint8 array, GUARD bytes in front and behind}; calls; out_pos (per call, where
    its results start in the guarded uint16 output: cumulative, so even and odd)."""

    def __init__(self, bufs, calls):
        self.bufs, self.calls = bufs, calls
        self.out_pos = OUT_GUARD + np.concatenate([[0], np.cumsum([c.n for c in calls])]).astype(np.int64)
        self.out_size = int(self.out_pos[-1]) + OUT_GUARD

    def pairs(self):
        """{(length, start mod 16)} over every packet of every call."""
        out = set()
        for c in self.calls:
            out |= set(zip(c.plen.tolist(), (c.start % 16).tolist()))
        return out

    def inside(self, name):
        """A mask over bufs[name]: the bytes that belong to a packet of some call."""
        m = np.zeros(self.bufs[name].size + 1, dtype=np.int64)
        for c in self.calls:
            if c.buf == name:
                np.add.at(m, c.start, 1)
                np.add.at(m, c.start + c.plen, -1)
        return np.cumsum(m)[:-1] > 0


def expect(oracle, plan):
    """The guarded output as it must be afterwards (uint16: poison, and each call's results)."""
    want = np.full(plan.out_size, POISON16, dtype=np.uint16)
    for c, pos in zip(plan.calls, plan.out_pos):
        b = plan.bufs[c.buf]
        if c.kind == "strided":
            r = oracle.batch_strided(b, c.stride, c.length, c.n, final=c.final, base_off=c.base)
        elif c.kind == "csr":
            r = oracle.batch_csr(b, c.offsets, final=c.final)
        elif c.kind == "seeded":
            r = oracle.batch_seeded_csr(b, c.offsets, c.states)
        else:
            r = oracle.batch_slotted(b[c.base:], c.stride, c.plen, final=c.final)
        want[pos:pos + c.n] = r
    return want


# ---- placing packets -------------------------------------------------------------------------------

def _lengths(full, upto=None, above=None):
    return [l for l in LENGTHS if (upto is None or l <= upto) and (above is None or l > above)]


def _bases(length, full):
    return range(16) if full or length <= DENSE[-1] else FEW


def _gap_stride(length):
    return (length + 31) // 16 * 16


def _odd_stride(length):
    return length + ((1 - length) % 16 or 16)


_R = {}


def random_buffer(nbytes=GUARD + 16 + 246 * 65536 + GUARD, seed=20261201):
    """The shared buffer of families A and C: random bytes, no zero byte where a DENSE call of a
    strided layout can end a packet (67 packets at a stride of up to 289 bytes from the 16 lowest
    bases), so that a byte read past such a packet's end always counts."""
    if (nbytes, seed) not in _R:
        r = synth.random_bytes(seed, nbytes)
        head = r[:GUARD + 32 + 68 * 304]
        head[head == 0] = 0x5A
        _R[(nbytes, seed)] = r
    return _R[(nbytes, seed)]


def _csr_call(kind, packets, starts, lead, seed, states=None, front=3, middle=5, end=4):
    """Packets (byte arrays) back to back, each at its start mod 16 (None: wherever it falls)
    behind a pad packet of random bytes; empty packets at the front, in the middle and at the end.
    Returns (buffer, offsets, the index of each given packet in the batch)."""
    rnd = synth.random_bytes(seed, 16 * (len(packets) + 1) + 2 * GUARD)
    parts, lens, index = [rnd[:GUARD + lead]], [0] * front, []
    at = GUARD + lead
    for j, (p, s) in enumerate(zip(packets, starts)):
        if j == len(packets) // 2:
            lens += [0] * middle
        if s is not None:
            pad = (s - at) % 16
            parts.append(rnd[GUARD + 16 * j:GUARD + 16 * j + pad])
            lens.append(pad)
            at += pad
        index.append(len(lens))
        parts.append(p)
        lens.append(len(p))
        at += len(p)
    lens += [0] * end
    parts.append(rnd[-GUARD:])
    off = GUARD + lead + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.concatenate(parts), off, np.array(index)


def seed_states(n, seed):
    """States drawn in turn from SEED_STATES and random."""
    st = synth.words(seed, 0, n).astype(np.uint32)
    for k, v in enumerate(SEED_STATES):
        st[k::5] = v
    return st


# ---- family A ---------------------------------------------------------------------------------------

def _strided_calls(layout, buf, lengths, bases_of, final_of=lambda i: bool(i & 1)):
    calls = []
    for length in lengths:
        for b in ((0,) if layout == "odd" else bases_of(length)):
            k = len(calls)
            if layout == "odd":
                calls.append(Call("strided", buf, 67 + (length & 1), final_of(k), base=GUARD + (length % 16),
                                  stride=_odd_stride(length), length=length))
            else:
                stride = length if layout == "b2b" else _gap_stride(length)
                calls.append(Call("strided", buf, 17 + ((length + b) & 1), final_of(k), base=GUARD + b,
                                  stride=stride, length=length))
    return calls


def _slot_calls(buf, full):
    rng = np.random.default_rng(20261202)
    calls = []
    groups = [(2048, _lengths(full, upto=2048), range(16) if full else FEW),
              (65536, _lengths(full, above=2048), range(16) if full else FEW),
              (1584, _lengths(full, upto=1584), (0, 7))]
    for stride, lens, bases in groups:
        for b in bases:
            ln = np.array(list(rng.permutation(lens)) + [min(stride, 65535)], dtype=np.uint32)
            calls.append(Call("slotted", buf, ln.size, bool(b & 1), base=GUARD + b, stride=stride, lens=ln))
    for e in range(16):            # stride 273 is odd: length k lies in a slot that starts at e + k mod 16
        z = int(e % 3 == 1)            # an empty slot in front: 274 or 275 slots
        ln = np.array([0] * z + DENSE + [273], dtype=np.uint32)
        calls.append(Call("slotted", buf, ln.size, False, base=GUARD + (e - z) % 16, stride=273, lens=ln))
    return calls


def _csr_pairs(full):
    """(length, start) in a fixed shuffled order: long packets beside short ones in a chunk."""
    pairs = [(l, s) for l in LENGTHS for s in _bases(l, full)]
    rng = np.random.default_rng(20261203)
    return [pairs[i] for i in rng.permutation(len(pairs))]


def plan_a(layout, full):
    """Family A of a layout: full (the default form: every pair) or the other forms' subset."""
    if layout in ("b2b", "gap16", "odd"):
        return Plan({"R": random_buffer()}, _strided_calls(layout, "R", LENGTHS, lambda l: _bases(l, full)))
    if layout == "slotted":
        return Plan({"R": random_buffer()}, _slot_calls("R", full))
    pairs = _csr_pairs(full)
    total = sum(l for l, _ in pairs)
    data = synth.random_bytes(20261204 + full, total)
    data[data == 0] = 0xA5
    at = np.concatenate([[0], np.cumsum([l for l, _ in pairs])])
    buf, off, _ = _csr_call(layout, [data[at[i]:at[i + 1]] for i in range(len(pairs))], [s for _, s in pairs], 3,
                            20261205)
    n = off.size - 1
    # the whole batch and the batch without its last (empty) packet, twice in turn: odd and even
    # counts at even and odd output elements
    cuts = [(n, off), (n - 1, off[:-1]), (n, off), (n - 1, off[:-1])]
    if layout == "csr":
        return Plan({"csr": buf}, [Call("csr", "csr", m, f, offsets=o) for (m, o), f in zip(cuts, (False, True, True, False))])
    st = seed_states(n, 20261206)
    return Plan({"csr": buf}, [Call("seeded", "csr", m, True, offsets=o, states=st[:m]) for m, o in cuts])


def large_strided(layout):
    """The large form of the strided layouts b2b and gap16: [(band, [(length, bases)])], one GPU
    test case per band. A call is LARGE_N + 67 packets and more; packet i is packet i mod 67 of
    the random buffer (the GPU test repeats them on the device), at the start mod 16 its base and
    stride give."""
    keep = [l for l in LENGTHS if l not in LARGE_EXEMPT[layout]]
    bands = [("dense", [l for l in keep if l <= DENSE[-1]])]
    bands += [(str(t), [l for l in keep if abs(l - t) <= 17 and l > DENSE[-1]]) for t in THRESHOLDS]
    assert sorted(l for _, ls in bands for l in ls) == keep
    return [(name, [(l, tuple(_bases(l, False))) for l in ls]) for name, ls in bands]


def large_plan(layout):
    """chunk_packets 0 on a batch of LARGE_N packets and more. CSR and seeded CSR: the other
    forms' subset of pairs, then every DENSE pair over and over, each packet at its start behind a
    pad packet. Ring slots: slots of 273 bytes whose lengths run 0..273 and an empty slot, 275 in
    all, over and over: 275 = 3 mod 16, so each length meets all 16 starts."""
    if layout == "slotted":
        ln = np.resize(np.array(DENSE + [273, 0], dtype=np.uint32), LARGE_N + 275 * 16)
        buf = synth.random_bytes(20261208, 2 * GUARD + 16 + ln.size * 273)
        return Plan({"large": buf}, [Call("slotted", "large", ln.size, False, base=GUARD + 5, stride=273, lens=ln)])
    dense = [(l, s) for l in DENSE for s in range(16)]
    rng = np.random.default_rng(20261209)
    pairs = _csr_pairs(False)
    while 2 * len(pairs) < LARGE_N:
        pairs += [dense[i] for i in rng.permutation(len(dense))]
    at = np.concatenate([[0], np.cumsum([l for l, _ in pairs])])
    data = synth.random_bytes(20261210, int(at[-1]))
    buf, off, _ = _csr_call(layout, [data[at[i]:at[i + 1]] for i in range(len(pairs))], [s for _, s in pairs], 1,
                            20261220)
    n = off.size - 1
    assert n >= LARGE_N
    if layout == "csr":
        return Plan({"large": buf}, [Call("csr", "large", n, True, offsets=off)])
    return Plan({"large": buf}, [Call("seeded", "large", n, True, offsets=off, states=seed_states(n, 20261211))])


# ---- family B: values ----------------------------------------------------------------------------------

POSITIONS = ("inside", "across", "last2", "tail", "odd_start")
B_LENGTHS = (2, 3, 16, 17, 31, 33, 64, 65, 100, 255, 1023, 1024, 1500, 1501, 9000, 9001)


def word_sum(b):
    """The sum of the big-endian 16-bit words of b, an odd last byte as a high byte."""
    b = np.asarray(b, dtype=np.uint8)
    if b.size & 1:
        b = np.concatenate([b, np.zeros(1, dtype=np.uint8)])
    return int(b.reshape(-1, 2).astype(np.uint64).dot(np.array([256, 1], dtype=np.uint64)).sum())


def fold(s):
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def crafted(length, p, seed):
    """A packet of random bytes whose 16-bit word at the even offset p completes the sum to a
    non-zero multiple of 0xFFFF, both of its bytes non-zero. p == length - 1: the word's high byte
    is the odd tail byte, and its low byte goes into the (otherwise zero) word in front."""
    pkt = synth.random_bytes(seed, length)
    tail = p == length - 1
    assert p % 2 == 0 and p < length and (not tail or length >= 3)
    for bump in range(1, 256):
        pkt[p - 2 if tail else p:p + 2] = 0
        t = (0xFFFF - word_sum(pkt) % 0xFFFF) % 0xFFFF or 0xFFFF
        hi, lo = (p, p - 1) if tail else (p, p + 1)
        pkt[hi], pkt[lo] = t >> 8, t & 0xFF
        if t >> 8 and t & 0xFF:
            break
        pkt[(p + 8) % length] ^= bump            # another sum: another completing word
    assert word_sum(pkt) % 0xFFFF == 0 and word_sum(pkt) > 0 and pkt[p]
    return pkt


def crafted_offsets(length):
    """The even offsets of the completing word worth having in a packet of this length: near the
    front (inside a segment at an even start, across a boundary at an odd one: 14 + start 1 = 15),
    and at the end (the last two bytes, or the odd tail byte)."""
    ps = {0, length - 2 if length % 2 == 0 else length - 1}
    if length >= 16:
        ps |= {14}
    if length >= 40:
        ps |= {30, 20}
    return sorted(p for p in ps if 0 <= p < length and (p < length - 1 or length >= 3))


def position_tags(length, start, p):
    """Which of POSITIONS the completing word at p of a packet at `start` occupies."""
    tags = set()
    if p == length - 1:
        tags.add("tail")
    else:
        tags.add("across" if (start + p) % 16 == 15 else "inside")
        if p == length - 2:
            tags.add("last2")
    if start & 1:
        tags.add("odd_start")
    return tags


def saturating(pattern, nbytes):
    """all 0xFF; 0xFFFF alternating with 0x0001; 0xFF in column 5 of 16 only (by buffer address)."""
    a = np.zeros(nbytes, dtype=np.uint8)
    if pattern == "ff":
        a[:] = 0xFF
    elif pattern == "alt":
        a[0::4] = a[1::4] = 0xFF
        a[3::4] = 1
    else:
        a[5::16] = 0xFF
    return a


SAT_PATTERNS = ("ff", "alt", "col")


def _crafted_list():
    """[(packet, p or None: the zero twin)]"""
    out = []
    for length in B_LENGTHS:
        for p in crafted_offsets(length):
            out.append((crafted(length, p, 7000 + 10 * length + p), p))
            out.append((np.zeros(length, dtype=np.uint8), None))
    return out


def plan_b(layout):
    """Family B. Returns (plan, crafted): crafted = [(call, packet, p or None)] names the crafted
    packets and their twins, whose results must be 0xFFFF and 0 (unseeded, not final)."""
    cl = _crafted_list()
    sat_n = 68 * 65552
    bufs = {"sat-" + k: np.concatenate([np.zeros(GUARD, np.uint8), saturating(k, sat_n), np.zeros(GUARD, np.uint8)])
            for k in SAT_PATTERNS}
    calls, marks = [], []
    if layout in ("b2b", "gap16", "odd"):
        n = 68 if layout == "odd" else 18
        stride_of = {"b2b": lambda l: l, "gap16": _gap_stride, "odd": _odd_stride}[layout]
        parts, at = [np.full(GUARD, 0x5C, np.uint8)], GUARD
        for length in B_LENGTHS:
            mine = [(pk, p) for pk, p in cl if len(pk) == length]
            stride = stride_of(length)
            for b in ((0, 1) if layout == "odd" else (0, 1, 7, 8)):
                region = np.full(16 + n * stride + 16, 0x5C, dtype=np.uint8)
                for i in range(n):
                    pk, p = mine[i % len(mine)]
                    region[b + i * stride:b + i * stride + length] = pk
                    marks.append((len(calls), i, p))
                parts.append(region)
                calls.append(Call("strided", "crafted", n, False, base=at + b, stride=stride, length=length))
                at += region.size
        parts.append(np.full(GUARD, 0x5C, np.uint8))
        bufs["crafted"] = np.concatenate(parts)
        for k in SAT_PATTERNS:
            for length in SAT_LENGTHS:
                for b in ((3,) if layout == "odd" else (0, 1, 8, 15)):
                    nn = (4 + (b & 1) if length > 9000 else 17 + (b & 1)) if layout != "odd" else 67 + (length & 1)
                    calls.append(Call("strided", "sat-" + k, nn, bool(b & 1), base=GUARD + b,
                                      stride=stride_of(length), length=length))
        return Plan(bufs, calls), marks
    sat = [(saturating(k, length + 16)[s:s + length], s) for k in SAT_PATTERNS for length in SAT_LENGTHS for s in FEW]
    if layout == "slotted":
        for stride, pk in ((2048, [c for c in cl if len(c[0]) <= 2048]), (65536, [c for c in cl if len(c[0]) > 2048])):
            for b in (0, 1, 7, 8, 15):
                ring = synth.random_bytes(7 + b, GUARD + 16 + len(pk) * stride + GUARD)
                for i, (p, _) in enumerate(pk):
                    ring[GUARD + b + i * stride:GUARD + b + i * stride + len(p)] = p
                name = "ring%d-%d" % (stride, b)
                bufs[name] = ring
                marks += [(len(calls), i, p) for i, (_, p) in enumerate(pk)]
                calls.append(Call("slotted", name, len(pk), False, base=GUARD + b, stride=stride,
                                  lens=np.array([len(p) for p, _ in pk], dtype=np.uint32)))
        for k in SAT_PATTERNS:           # the saturating lengths in slots of 65536 bytes of the pattern itself
            for b in FEW:
                ln = np.array(SAT_LENGTHS, dtype=np.uint32)
                calls.append(Call("slotted", "sat-" + k, 4, bool(b & 1), base=GUARD + b, stride=65536, lens=ln))
        return Plan(bufs, calls), marks
    packets = [p for p, _ in cl] * 4 + [p for p, _ in sat]
    starts = [s for s in (0, 1, 8, 15) for _ in cl] + [s for _, s in sat]
    buf, off, index = _csr_call(layout, packets, starts, 1, 20261212)
    bufs = {"csr": buf}
    n = off.size - 1
    marks = [(0, int(index[j]), cl[j % len(cl)][1]) for j in range(4 * len(cl))]
    if layout == "csr":
        return Plan(bufs, [Call("csr", "csr", n, f, offsets=off) for f in (False, True)]), marks
    states = seed_states(n, 20261213)
    ones = states.copy()
    ones[index[4 * len(cl):]] = np.resize(np.array(SEED_STATES[1:], dtype=np.uint32), len(sat))
    zero = np.zeros(n, dtype=np.uint32)          # state 0, final: the twins give 0xFFFF, the crafted packets 0
    return Plan(bufs, [Call("seeded", "csr", n, True, offsets=off, states=s) for s in (zero, states, ones)]), marks


# ---- family C: surroundings ---------------------------------------------------------------------------

def plan_c(layout):
    """One mixed batch of C_PACKETS packets in a buffer of its own; alt(plan) is the same plan with
    every byte outside every packet inverted."""
    n = C_PACKETS
    rng = np.random.default_rng(20261214)
    lens = rng.integers(0, 1601, n)
    lens[[0, 100, 256, 511, 512]] = (1, 0, 2047, 63, 17)
    if layout in ("b2b", "gap16", "odd"):
        length = 1499
        stride = {"b2b": length, "gap16": 1520, "odd": 1505}[layout]
        buf = synth.random_bytes(20261215, GUARD + 3 + n * stride + GUARD)
        return Plan({"c": buf}, [Call("strided", "c", n, False, base=GUARD + 3, stride=stride, length=length)])
    if layout == "slotted":
        buf = synth.random_bytes(20261216, GUARD + 9 + n * 2048 + GUARD)
        return Plan({"c": buf}, [Call("slotted", "c", n, True, base=GUARD + 9, stride=2048, lens=lens.astype(np.uint32))])
    off = GUARD + 5 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    buf = synth.random_bytes(20261217, int(off[-1]) + GUARD)
    if layout == "csr":
        return Plan({"c": buf}, [Call("csr", "c", n, True, offsets=off)])
    return Plan({"c": buf}, [Call("seeded", "c", n, True, offsets=off, states=seed_states(n, 20261218))])


def alt(plan):
    """The plan over buffers whose bytes outside every packet are inverted."""
    return Plan({k: np.where(plan.inside(k), b, b ^ 0xFF).astype(np.uint8) for k, b in plan.bufs.items()}, plan.calls)


def clamp_case():
    """The one deliberate contract violation: a length over its slot, clamped to the slot and
    reported. Returns (buffer, base, stride, lens as given)."""
    stride, n = 512, 131
    buf = synth.random_bytes(20261219, GUARD + n * stride + GUARD)
    lens = np.full(n, 300, dtype=np.uint32)
    lens[77] = stride + 5
    return buf, GUARD, stride, lens


_cache = {}


def cached(key, make):
    """make(), computed once per process and left unchanged."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def plan(layout, family, full):
    if family == "A":
        return cached((layout, "A", full), lambda: plan_a(layout, full))
    if family == "B":
        return cached((layout, "B"), lambda: plan_b(layout))[0]
    return cached((layout, "C"), lambda: plan_c(layout))
