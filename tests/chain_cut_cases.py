"""TEST INFRASTRUCTURE -- shared by test_chain_cut_cases.py and test_gpu_chain_cut.py: the sweep of
the chained batch (chksum_chain_kernel, sum_gathered_chunks, the COLS column-run form,
sum_short_chunk_from, chain_field_scatter_kernel) over its table, stream and run geometry. Host
arrays only; every expectation comes from the CPU oracle (Chains.expected).

The kernel walks a group of `cpg` chains (p0 = c * cpg) 64 chunks at a time from the group's first
chunk K0, so what a chunk's lane sees depends on the chunk's position relative to K0 mod 64. The
families are built so that this position is the same under every `cpg`:

  T  table geometry: groups of 64 chains (a filler of s chunks, the target of L chunks, a trailer,
     empty chains up to 64), chunks of 0..3 bytes. Under cpg >= 4 a group of the kernel starts
     where one of these starts or inside its empty chains; under cpg 2 the filler still precedes
     the target; under cpg 1 every chain starts its own group (s = 0, see t_triples).
  S  stream geometry: one chain of exactly 64 chunks per case, so a case is one slice under every
     cpg; its segment count T takes every value 1..1344.
  L  chunk lengths and the short-first rule: three-chunk chains, the middle chunk swept.
  R  column runs: one chain of 64 chunks per case (one slice), nr run chunks back to back and
     ns_ lone short headers; broken runs in a second batch.
  B  sums that fold to 0xFFFF; chains of 128 chunks, so each starts a slice under every cpg.
  C  513 chains cropped out of T, S, L and R with their surroundings, run twice (alt).
  F  the field pass: T's batch with field_offsets, and f_big's cus * 64 * 256 + 513 chains.

FORMS names the kernel forms. The tunable "nontemporal" 0 needs an AIPSTACK_ALL_VARIANTS build and
is out of scope here."""
import numpy as np

from tx_cut_cases import GUARD, Chains, Ring, alt, cached, field_offsets, filled_fields  # noqa: F401

DEFAULTS = {"stream": 0, "chunk_packets": 0, "chunks_per_wave": 0, "chain_short": -1}
CPGS = (1, 2, 4, 8, 16, 32, 64)

# name -> (tunables, the JUST_WRITTEN hint)
FORMS = {
    "su4": ({}, False),
    "su2": ({"stream": 2}, False),
    "jw": ({}, True),
    "jw-su2": ({"stream": 2}, True),
    "jw-short0": ({"chain_short": 0}, True),
    "short0": ({"chain_short": 0}, False),
    "short1": ({"chain_short": 1}, False),
    "short65535": ({"chain_short": 65535}, False),
    **{"cpg%d" % c: ({"chunk_packets": c}, False) for c in CPGS},
    "cpw2": ({"chunks_per_wave": 2}, False),
    "cpw3": ({"chunks_per_wave": 3}, False),
    "cpw4096": ({"chunks_per_wave": 4096}, False),
    "jw-cpg64": ({"chunk_packets": 64}, True),
    "jw-cpg1": ({"chunk_packets": 1}, True),
    "su2-cpg64": ({"stream": 2, "chunk_packets": 64}, False),
    "short0-cpg1": ({"chain_short": 0, "chunk_packets": 1}, False),
}

FAMILY_FORMS = {
    "T": list(FORMS),
    "S": ["su4", "su2", "jw-su2", "jw-short0", "short0", "short65535"],
    "L": ["su4", "short0", "short1", "short65535", "jw", "jw-cpg1"],
    "R": ["jw", "jw-cpg64", "jw-cpg1", "su4"],
    "B": ["su4", "su2", "jw"],
    "C": list(FORMS),
}


def kernel_form(name):
    """(SU, COLS) of chksum_chain_kernel as chain_batch and launch_chain pick them."""
    t, jw = FORMS[name]
    su = 2 if t.get("stream", 0) == 2 else 4
    short = t.get("chain_short", -1)
    return su, bool(jw and su > 2 and short != 0)


PRODUCT_KERNELS = {(2, False), (4, False), (4, True)}   # what launch_chain instantiates (no COLS at SU 2)


class Case:
    """chains: a Chains; calls: the (lo, hi) chain ranges, one batch each; tags: per chain."""

    def __init__(self, chains, calls=None, tags=None, split=None):
        self.chains, self.tags, self.split = chains, tags, split
        self.calls = calls or [(0, len(chains.chains))]


def _states(n, seed):
    s = ((np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(2654435761)) % np.uint64(1 << 32)
    s = s.astype(np.uint32)
    s[3::11] = 0
    s[5::13] = 0xFFFF
    return s


def _finish(ring, chains, seed, tags=None, calls=None, split=None):
    payload, described = ring.build()
    return Case(Chains(chains, _states(len(chains), seed), payload, described), calls, tags, split)


# ---- family T: the table ---------------------------------------------------------------------------

T_COUNTS = tuple(range(7)) + tuple(range(62, 67)) + tuple(range(126, 131)) + tuple(range(190, 195))
T_BATCH_MAX = 130


def _tiny(ring, rng, count, force=None):
    """`count` chunks of 0..3 bytes with one or two undescribed bytes in front of each."""
    lens = rng.integers(0, 4, count)
    for k, v in (force or {}).items():
        if 0 <= k < count:
            lens[k] = v
    return [(ring.place(int(l), None, 1 + int(g)), int(l)) for l, g in zip(lens, rng.integers(0, 2, count))]


def t_case():
    """One group of 64 chains per (s, L); then the empty-chain edges; then, as batches of their own,
    every n in 1..T_BATCH_MAX. tags: (s, L) on each target chain."""
    rng = np.random.default_rng(7001)
    ring, chains, tags = Ring(7000), [], []

    def group(parts):
        """parts: chains of the group in order; padded with empty chains to 64."""
        assert len(parts) <= 64
        for tag, ch in parts:
            chains.append(ch)
            tags.append(tag)
        for _ in range(64 - len(parts)):
            chains.append([])
            tags.append(None)

    for s in range(64):
        for L in T_COUNTS:
            # kernel: `if (before) q ^= carry_par;`, `if (cid < 0) cid = carry_cid;`, `mark[cs - kr]`
            # -- the target's chunks at lanes 63 and 0 of a slice are empty in turn
            force = {}
            if (s + L) % 3 == 0:
                force[64 - s] = force[128 - s] = 0           # lane 0 of the second and third slice
            elif (s + L) % 3 == 1:
                force[63 - s] = force[127 - s] = 0           # lane 63
            parts = [(None, _tiny(ring, rng, s))] if s else []
            parts.append(((s, L), _tiny(ring, rng, L, force)))
            parts.append((None, _tiny(ring, rng, 1 + (s + L) % 3)))
            group(parts)
    # kernel: `chain_nonempty`, `K0`, `K1`, `for (kb = K0; kb < K1; ...)` with K0 == K1
    group([(None, []), ("first-empty", _tiny(ring, rng, 5)), (None, _tiny(ring, rng, 70))])
    group([("last-nonempty", _tiny(ring, rng, 3))] * 1 + [(None, _tiny(ring, rng, 1)) for _ in range(62)] + [(None, [])])
    group([])                                                # 64 empty chains between non-empty groups
    group([("crosses", _tiny(ring, rng, 70)), ("empty-between", []), ("crosses", _tiny(ring, rng, 70))])
    group([(None, _tiny(ring, rng, 64)), ("fresh-at-lane0", _tiny(ring, rng, 64)), (None, _tiny(ring, rng, 2))])
    calls = [(0, len(chains))]
    # kernel: `cnt = min(cpg, n - p0)`, `K1 = cnt < kWave ? offset_of(grp, cnt) : ...`, `lane < cnt`
    for n in range(1, T_BATCH_MAX + 1):
        lo = len(chains)
        for i in range(n):
            k = (0, 1, 2, 3, 5, 0, 1, 67)[(i + n) % 8] if (i * 7 + n) % 29 else 130
            chains.append(_tiny(ring, rng, k))
            tags.append(None)
        calls.append((lo, lo + n))
    return _finish(ring, chains, 7002, tags, calls)


def t_triples(c, cpg, lo=0, hi=None):
    """Regrouping chains [lo, hi) as launch_chain does (p0 = c * cpg): ({(s mod 64, crosses a
    slice boundary, parity carried over it)} of the non-empty chains -- the parity None where
    nothing is crossed --, {the carry_cid cases at lane 0 of a slice that is not a group's first:
    "continued", "fresh"})."""
    hi = len(c.chains) if hi is None else hi
    idx = np.zeros(len(c.chains) + 1, dtype=np.int64)
    idx[1:] = np.cumsum([len(ch) for ch in c.chains])
    triples, carry = set(), set()
    for i in range(lo, hi):
        ch = c.chains[i]
        if not ch:
            continue
        k0 = idx[lo + (i - lo) // cpg * cpg]
        s = int(idx[i] - k0)
        first, last = s // 64, (s + len(ch) - 1) // 64
        if first == last:
            triples.add((s % 64, False, None))
        for b in range(first + 1, last + 1):
            before = sum(l for _, l in ch[:64 * b - s])
            triples.add((s % 64, True, before & 1))
            carry.add("continued")
        if s % 64 == 0 and s > 0:
            carry.add("fresh")
    return triples, carry


# ---- family S: the gathered stream -----------------------------------------------------------------

S_MAX = 1344                            # five groups of U = 4 windows plus one window


def _seg_chunk(ns, j, T):
    """(address mod 16, length) of a chunk of `ns` 16-byte segments: starts of both parities, ends
    dealt over all of 1..16."""
    if ns == 0:
        return (3 * j + T) % 16, 0
    rs, e = (3 * j + T) % 16, (5 * j + 7 * T + T // 16) % 16 + 1
    if ns == 1 and e <= rs:
        rs = e - 1
    return rs, 16 * (ns - 1) + e - rs


def _spread(T, lanes):
    """T segments over the 64 lanes: only `lanes` get any, as evenly as it goes, the larger
    shares rotating with T."""
    ns = [0] * 64
    k = len(lanes)
    for i, j in enumerate(lanes):
        ns[j] = T // k + (1 if (i + T) % k < T % k else 0)
    assert sum(ns) == T
    return ns


def s_specs():
    """[(tag, [segments per lane])]."""
    # kernel (sum_gathered_chunks): `nwin`, `groups`, `for (; g + 2u < groups; g += 2u)`,
    # `if (g + 2u == groups)`, `c = min(c0, T - 1u)`, `s = c0 < T ? s : 0u`
    out = [(("T", T), _spread(T, list(range(64)))) for T in range(1, S_MAX + 1)]
    for T in range(64, S_MAX + 1, 64):
        # kernel: `if (bwin >= nwin) gsum = carry;` (cs == T on a multiple of 64)
        for e in (1, 2, 63):
            out.append((("trail", T, e), _spread(T, list(range(64 - e)))))
        for p in (0, 31, 63):
            out.append((("own", T, p), _spread(T, [p])))
        # kernel: `bwin == wu`, `start_win`, `start_bit` -- a chunk starting on a window boundary
        # and one segment before it
        for first in (64, 63):
            out.append((("win", T, first), [first] + _spread(T - first, list(range(63)))[:63]))
    return out


def s_case():
    ring, chains, tags = Ring(7100), [], []
    for tag, ns in s_specs():
        T = sum(ns)
        ch = []
        for j, k in enumerate(ns):
            rs, l = _seg_chunk(k, j, T)
            ch.append((ring.place(l, rs, 1), l))
        chains.append(ch)
        tags.append(tag)
    return _finish(ring, chains, 7101, tags)


def s_geometry(T, U):
    """(groups, groups mod 2, nwin mod U) of sum_gathered_chunks for a stream of T segments."""
    nwin = (T + 63) >> 6
    groups = (nwin + U - 1) // U
    return groups, groups % 2, nwin % U


# ---- family L: lengths and the short-first rule ----------------------------------------------------

L_DENSE = 144
L_EDGE = sorted(set(range(145, 273)) | {1459, 1460, 1461, 4095, 4096, 4097} | set(range(65519, 65536)) |
                {128 * k + d for k in range(2, 5) for d in (-1, 1)})      # (127 and 129: dense)
B2B, ADJ, FAR = 0, 1, 2


def l_specs():
    """[(length, start mod 128, start parity in the chain, layout)], ordered by layout so that the
    slices of 64 chunks hold one layout each (lone short chunks alone take COLS' short path)."""
    out = []
    for l in range(1, L_DENSE + 1):
        for st in range(128):
            for par in (0, 1):
                out.append((l, st, par, (l // 3 + st + par) % 3))
    for i, l in enumerate(L_EDGE):
        for st in range(16):
            out.append((l, st + 16 * ((i + st) % 8), (i + st) & 1, (i + st // 2) % 3))
    out.sort(key=lambda x: (x[3], x[0] > 128))
    return out


def l_case():
    """The swept chunk in the middle of a three-chunk chain; then the two-chunk chains of 1-byte
    chunks side by side."""
    # kernel: `lv <= short_first && prev_e != line_s && next_s != line_e`, `nsg`, `kmax`,
    # `if (nsg > 0u) h0 = ...; if (nsg > 1u) h1 = ...`, sum_short_chunk_from's `te`
    ring, chains, tags = Ring(7200), [], []
    for l, st, par, lay in l_specs():
        pl, nl = 2 + par + 2 * (st % 3), 1 + (l + st) % 5
        a = ((ring.at >> 7) + (8 if lay == FAR else 3)) * 128 + st
        if lay == B2B:
            p_at, n_at = a - pl, a + l
        elif lay == ADJ:                    # wholly inside the line before / after, one byte clear
            p_at, n_at = (a & ~127) - 1 - pl, (((a + l - 1) >> 7) + 1) * 128 + 1
        else:
            p_at, n_at = a - 512 - pl, a + l + 512
        ch = []
        for at, ln in ((p_at, pl), (a, l), (n_at, nl)):
            ch.append((ring.place(ln, None, at - ring.at), ln))
        assert ch[1][0] == a and a % 128 == st
        chains.append(ch)
        tags.append((l, st, par, lay))
    for st in range(128):
        a = ((ring.at >> 7) + 2) * 128 + st
        chains.append([(ring.place(1, None, a - ring.at), 1), (ring.place(1), 1)])
        tags.append(("pair", st))
    return _finish(ring, chains, 7201, tags)


def short_rule(a, l, short_first=128, strict=False):
    """The two line tests of the short-first rule for one slice (lists of 64 addresses and
    lengths, lanes wrapping as ds_bpermute does; a shorter list that ends in an empty chunk at
    address 0 stands for the slice whose other lanes are such chunks): per lane (lone short chunk,
    prev_e != line_s, next_s != line_e)."""
    M = (1 << 64) - 1
    line_s = [(x >> 7) & 0xFFFFFFFF for x in a]
    line_e = [(((x + n - 1) & M) >> 7) & 0xFFFFFFFF for x, n in zip(a, l)]
    out = []
    k = len(a)
    assert k == 64 or (a[-1] == 0 and l[-1] == 0)
    for j in range(k):
        t1, t2 = line_e[(j - 1) % k] != line_s[j], line_s[(j + 1) % k] != line_e[j]
        small = l[j] < short_first if strict else l[j] <= short_first
        out.append((l[j] != 0 and small and t1 and t2, t1, t2))
    return out


# ---- family R: column runs -------------------------------------------------------------------------

R_LENS = (1, 15, 16, 17, 1460)
R_BREAK_NR = (2, 31, 32, 33, 63, 64)
HDR_LEN, HDR_STRIDE = 20, 256


def _r_order(nr, nh, inter):
    """The 64 lanes' kinds: 'H' lone short header, 'R' run chunk, 'E' empty."""
    ne = 64 - nr - nh
    if inter == 0:
        return "H" * nh + "R" * nr + "E" * ne
    if inter == 2:
        return "R" * nr + "E" * ne + "H" * nh
    out, h, r = "", nh, nr                  # a header, two run chunks (three at the end), in turn
    while h or r:
        if h:
            out, h = out + "H", h - 1
        k = r if r <= 3 else 2
        out, r = out + "R" * k, r - k
    return out + "E" * ne


def _r_slice(ring, order, lens, brk=None, far=None):
    """One slice as one chain: the headers in an area of their own at HDR_STRIDE, the run chunks
    back to back behind it (brk: (run chunk index, extra bytes in front of it); far: the index of
    a run chunk that lies elsewhere, its offset `far[1]` for now), the empty chunks in front. The
    runs' start is shifted until the kernel's rule counts the chunks as `order` names them (a run
    chunk that ends on a line's edge beside a header would count as a lone short one)."""
    nh = order.count("H")
    hdr0 = ((ring.at >> 7) + 4) * 128 + 64
    for shift in range(0, 128, 5):
        at = hdr0 + max(nh, 1) * HDR_STRIDE + 256 + (len(ring.off) * 5 + shift) % 128
        spots, h, r = [], 0, 0
        for kind in order:
            if kind == "H":
                spots.append((hdr0 + h * HDR_STRIDE, HDR_LEN))
                h += 1
            elif kind == "E":
                spots.append((hdr0 - 200, 0))   # in no line that a chunk of the slice touches
            else:
                ln = lens[r % len(lens)]
                if brk and brk[0] == r:
                    at += brk[1]
                if far and far[0] == r:
                    spots.append((hdr0 - 400, ln))
                else:
                    spots.append((at, ln))
                    at += ln
                r += 1
        if cols_slice([o for o, _ in spots], [l for _, l in spots])[:2] == (order.count("R"), nh):
            break
    else:
        raise AssertionError(order)
    if far:
        spots = [(far[1], ln) if o == hdr0 - 400 and ln else (o, ln) for o, ln in spots]
    # the ring wants its chunks in address order: place them so, keep the table's order
    for o, ln in sorted(set(s for s in spots if s[1] and s[0] >= 0)):
        ring.place(ln, None, o - ring.at)
    return spots


def r_specs():
    out = []
    for nr in range(65):
        for nh in sorted({0, 1, 2, 64 - nr}):
            if nr + nh > 64:
                continue
            for inter in range(3):
                k = len(out)
                lens = R_LENS[k % 5:k % 5 + 1] if k % 2 == 0 else R_LENS[k % 5:] + R_LENS[:k % 5]
                out.append(((nr, nh, inter), _r_order(nr, nh, inter), lens))
    return out


def r_case():
    # kernel (COLS): `nr`, `ns_`, `rank`, `stream_ok(a_p, a_p + l_p, lane, (int)nr)`,
    # `for (r0 = 0; r0 < nr; r0 += kChainColMax)`, `((lane + r0) & 63u)`, `((lane - r0) & 63u)`,
    # `mine = lane >= nr && lane < nr + ns_`
    ring, chains, tags = Ring(7300), [], []
    for (nr, nh, inter), order, lens in r_specs():
        # (one short chunk alone is a header by the kernel's rule: the run of one is a long chunk)
        chains.append(_r_slice(ring, order, (1460,) if nr == 1 else lens))
        tags.append((nr, nh, inter))
    chains.append(_r_slice(ring, "R" * 32 + "E" * 32, (65535,)))
    tags.append((32, 0, "max"))
    return _finish(ring, chains, 7301, tags)


def r_broken_case():
    """The runs of R_BREAK_NR broken at every position: by one byte, by 16 bytes, or with the chunk
    in another allocation (the offsets from `split` on: a device buffer of their own)."""
    # kernel (COLS): `stream_ok(...)` false -> `if (!done)`: the gathered stream
    ring, chains, tags = Ring(7402), [], []
    for nr in R_BREAK_NR:
        for p in range(1, nr):
            for how in (1, 16, "far"):
                k = len(chains)
                order = _r_order(nr, min((0, 1, 2)[k % 3], 64 - nr), k % 3)
                lens = (R_LENS[k % 4],) if k % 2 else R_LENS[k % 5:] + R_LENS[:k % 5]
                if nr == 2:
                    lens = (1460,)          # two short chunks apart would be two lone headers
                if how == "far":            # the moved chunk stays a run chunk only if it is long
                    long = {p} | ({0} if p == 1 else set()) | ({nr - 1} if p == nr - 2 else set())   # (nor leave one alone)
                    lens = tuple(1460 if r in long else lens[r % len(lens)] for r in range(64))
                    chains.append(_r_slice(ring, order, lens, far=(p, -1 - k)))
                else:
                    chains.append(_r_slice(ring, order, lens, brk=(p, how)))
                tags.append((nr, p, how))
    split = ring.at + GUARD + (-(ring.at + GUARD)) % 128
    ring.at = split + GUARD
    for k, ch in enumerate(chains):
        for i, (o, ln) in enumerate(ch):
            if o < 0:
                ch[i] = (ring.place(ln, (3 * k) % 16, 17), ln)
    return _finish(ring, chains, 7403, tags, split=split)


def cols_slice(a, l, short_first=128):
    """(nr, ns_, the run chunks lie back to back) of one slice, by the rule restated."""
    a = [int(x) for x in a] + [0] * (64 - len(a))
    l = [int(x) for x in l] + [0] * (64 - len(l))
    rule = short_rule(a, l, short_first)
    run = [j for j in range(64) if l[j] and not rule[j][0]]
    ok = all(a[i] + l[i] == a[j] for i, j in zip(run, run[1:]))
    return len(run), sum(1 for r in rule if r[0]), ok


# ---- family B: sums at the fold --------------------------------------------------------------------

B_STATES = (0, 0xFFFF, 0x10000, 0xFFFF0000, 0xFFFFFFFF)
B_CHUNKS = 128


def b_case(oracle):
    """Chains of B_CHUNKS chunks (so each starts a slice under every cpg) whose last two bytes are
    chosen so that state + sum folds to 0xFFFF: the two bytes across a chunk cut ("cut"), across
    the slice boundary between chunks 63 and 64 ("slice"), the first of them at every address mod
    16, or across a 16-byte boundary ("seg": the first at address 15 mod 16, 16 chains of other
    lengths); then chains of all-zero and all-0xFF chunks."""
    # kernel: `if (valid && r != 0)`, the 64-bit fold `s33`, `s32`, `t`, `r == 0` -> 0xFFFF
    rng = np.random.default_rng(7500)
    ring, chains, tags, fix, fills = Ring(7501), [], [], [], []
    for st in B_STATES:
        for kind in ("cut", "slice", "seg"):
            for r in range(16):
                lens = [int(x) for x in rng.integers(0, 40, B_CHUNKS)]
                lens[7::9] = [0] * len(lens[7::9])
                if kind == "slice":
                    lens[64:] = [1] + [0] * 63
                    lens[63] = max(lens[63], 1)
                elif kind == "cut":
                    lens[-1], lens[-2] = 1, max(lens[-2], 1)
                else:
                    lens[-1] = max(lens[-1], 2)
                if sum(lens) % 2:
                    lens[0] += 1
                last = max(i for i, x in enumerate(lens) if x)
                prev = max(i for i, x in enumerate(lens[:last]) if x)
                ch = []
                for i, ln in enumerate(lens):
                    al = None
                    if kind == "seg" and i == last:
                        al = (15 - (ln - 2)) % 16     # (r only varies the random lengths here)
                    elif kind != "seg" and i == prev:
                        al = (r - (ln - 1)) % 16
                    ch.append((ring.place(ln, al, 1 + (i + r) % 3), ln))
                if (len(chains) + r) % 4 == 1:          # an all-zero chunk beside an all-0xFF one
                    fills += [(ch[2], 0), (ch[3], 0xFF)]
                p = (ch[last][0] + lens[last] - 2) if lens[last] >= 2 else (ch[prev][0] + lens[prev] - 1)
                fix.append((len(chains), p, ch[last][0] + lens[last] - 1))
                chains.append(ch)
                tags.append((kind, st, r))
    for st in B_STATES:
        for k in range(8):
            ch = [(ring.place(ln, None, 1), ln) for ln in [int(x) for x in rng.integers(0, 70, B_CHUNKS)]]
            fills += [(c, 0xFF if (i + k) % 3 == 0 and k < 7 else 0) for i, c in enumerate(ch)]
            chains.append(ch)
            tags.append(("fill", st, k))
    case = _finish(ring, chains, 0, tags)
    c = case.chains
    for (o, ln), v in fills:
        c.payload[o:o + ln] = v
    c.states[:] = [t[1] for t in tags]
    for i, p, q in fix:
        c.payload[p] = c.payload[q] = 0
    first = c.expected(oracle)
    for i, p, q in fix:
        c.payload[p], c.payload[q] = first[i] >> 8, first[i] & 0xFF
    case.fix = fix
    return case


# ---- family C: cropped out of the others -----------------------------------------------------------

C_CHAINS = 513
C_PARTS = (150, 120, 150, 93)            # chains from T, S, L and R


def crop(sources):
    """[(Case, chain indices)] -> one Case: each chosen chain with the bytes round it (its span
    widened to whole 128-byte lines, so addresses mod 128 stay), laid out one behind the other.
    Bytes of the span that belong to chains not chosen are undescribed here."""
    parts, chains, states, at = [], [], [], 128
    for case, pick in sources:
        c = case.chains
        for i in pick:
            ch = c.chains[i]
            lo = min([o for o, _ in ch] + [1 << 62]) & ~127
            hi = -(-(max(o + l for o, l in ch) + 1) // 128) * 128 if ch else 0
            if not ch:
                lo = hi = 0
            parts.append(c.payload[lo:hi])
            chains.append([(o - lo + at, l) for o, l in ch])
            states.append(c.states[i])
            at += hi - lo + 128
            parts.append(np.full(128, 0x5A, dtype=np.uint8))
    payload = np.concatenate([np.full(128, 0x5A, dtype=np.uint8)] + parts)
    d = np.zeros(payload.size + 1, dtype=np.int64)
    for ch in chains:
        for o, l in ch:
            d[o] += 1
            d[o + l] -= 1
    return Case(Chains(chains, np.array(states, dtype=np.uint32), payload, np.cumsum(d)[:-1] > 0))


def c_case():
    t, s, l, r = (cached(("chain", k), f) for k, f in (("T", t_case), ("S", s_case), ("L", l_case), ("R", r_case)))
    tt = [i for i, tag in enumerate(t.tags) if tag is not None][::9][:150]
    ss = list(range(0, len(s.tags), 11))[:120]
    ll = [i for i, tag in enumerate(l.tags) if tag[0] != "pair" and tag[3] != B2B and tag[0] < 5000][::160][:150]
    rr = list(range(0, len(r.tags) - 1, 8))[:C_CHAINS - len(tt) - len(ss) - len(ll)]
    assert (len(tt), len(ss), len(ll), len(rr)) == C_PARTS
    return crop([(t, tt), (s, ss), (l, ll), (r, rr)])


def touching(c):
    """The number of chunk pairs of a Chains that lie back to back (end == start, both non-empty)."""
    ch = sorted((o, l) for chn in c.chains for o, l in chn if l)
    return sum(1 for (o, l), (o2, _) in zip(ch, ch[1:]) if o + l >= o2)


# ---- family F: the field pass ----------------------------------------------------------------------

F_EVERY = 4099
F_CHUNK = 6


def f_big(cus):
    """(n, index uint64, addr offsets, lens, states, payload): cus * 64 * 256 + 513 chains, all
    empty but one in F_EVERY, which has one chunk of F_CHUNK bytes."""
    # kernel (chain_field_scatter_kernel): `for (i = ...; i < n; i += stride)`, second iteration
    n = cus * 64 * 256 + 513
    full = np.arange(n) % F_EVERY == 17
    idx = np.zeros(n + 1, dtype=np.uint64)
    idx[1:] = np.cumsum(full)
    k = int(idx[-1])
    payload = np.random.default_rng(7600).integers(0, 256, GUARD + 8 * k + GUARD, dtype=np.uint8)
    off = GUARD + 8 * np.arange(k, dtype=np.int64) + (np.arange(k) & 1)
    lens = np.full(k, F_CHUNK, dtype=np.uint32)
    states = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.uint32)
    states[::5] = 0
    states[1::977] = 0xFFFF
    return n, idx, off, lens, states, payload


def f_big_expected(oracle, big):
    n, idx, off, lens, states, payload = big
    flat = np.concatenate([payload[o:o + F_CHUNK] for o in off] + [np.zeros(1, np.uint8)])
    return oracle.batch_seeded_csr(flat, idx * np.uint64(F_CHUNK), states)


def case(name, oracle=None):
    make = {"T": t_case, "S": s_case, "L": l_case, "R": r_case, "R-broken": r_broken_case, "C": c_case,
            "B": lambda: b_case(oracle)}[name]
    return cached(("chain", name), make)


def _expected(oracle, c, payload):
    """Chains.expected; a chain of more than 65535 bytes (longer than anything the oracle's
    one-piece sum is meant for) chunk by chunk through oracle.chain instead."""
    want = c.expected(oracle, payload)
    for i, ch in enumerate(c.chains):
        if len(ch) and sum(l for _, l in ch) > 65535:
            want[i] = oracle.chain(int(c.states[i]), c.payload if payload is None else payload, ch)
    return want


def expected(oracle, name, payload=None):
    c = case(name, oracle).chains
    if payload is not None:
        return _expected(oracle, c, payload)
    return cached(("chain-want", name), lambda: _expected(oracle, c, None))
