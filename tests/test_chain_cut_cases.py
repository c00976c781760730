"""The conditions test_gpu_chain_cut.py relies on, checked on the CPU: that the families of
chain_cut_cases.py hold every value they are built for, that the oracle's sums are what the stream
models of test_stream_model.py give on them, and that each family tells a deliberately wrong chain
model from the oracle."""
import numpy as np
import pytest

import chain_cut_cases as X
from test_stream_model import M32, _exact_halves, chain_cols_model, gathered_model


def _flat(c):
    """(addr, len, index) of a Chains as plain int64 arrays, offsets into its payload."""
    return X.cached(("flat", id(c)), lambda: tuple(np.asarray(t).astype(np.int64) for t in c.table(0)))


def _halves(c):
    """Each chunk's exact little-endian halves-sum (what every kernel form must reach)."""
    a, l, _ = _flat(c)
    return X.cached(("halves", id(c)), lambda: [_exact_halves(c.payload, int(o), int(o + n)) for o, n in zip(a, l)])


def _fold(x):
    while x >> 16:
        x = (x & 0xFFFF) + (x >> 16)
    return x


def _seg_sum(buf, lo, hi):
    return int(buf[lo:hi].view("<u2").astype(np.uint64).sum())


def _slice_bug(bug, buf, a, l, sums, nv):
    """The chunk sums of one slice under a wrong gathered stream / column-run model."""
    rs = [x & 15 for x in a]
    ns = [((r + n + 15) >> 4) if n else 0 for r, n in zip(rs, l)]
    T = sum(ns)
    full = [j for j in range(64) if ns[j]]
    if not full:
        return sums
    jl = full[-1]
    if bug == "cs==T read as 0" and T % 64 == 0 and jl < 63:
        G = sum(_seg_sum(buf, a[j] & ~15, (a[j] & ~15) + 16 * ns[j]) for j in full) & M32
        sums[jl] = (sums[jl] - G) & M32
        if nv == 64:
            sums[63] = G
    if bug == "padding lanes counted" and T % 64 and nv == 64:
        last = (a[jl] & ~15) + 16 * (ns[jl] - 1)
        sums[63] = (sums[63] + (64 - T % 64) * _seg_sum(buf, last, last + 16)) & M32
    if bug == "short < and ninth segment dropped":
        for j, (lone, _, _) in enumerate(X.short_rule(a, l, strict=True)):
            if lone and ns[j] == 9:
                sums[j] = _exact_halves(buf, a[j], (a[j] & ~15) + 128) & M32
    return sums


def chain_model(c, lo, hi, cpg, bug=None):
    """The chain kernel's table walk over chains [lo, hi) in groups of cpg: 64 chunks at a time from
    the group's first chunk, the chain of each chunk from the chain starts and the carried id, the
    parity of its place in the chain from the odd lengths and the carried parity, each chunk's
    exact halves-sum folded and swapped iff address and place have the same parity, added per
    chain; state, fold, inversion. `bug`: one of the wrong models."""
    A, Ln, idx = _flat(c)
    h = _halves(c)
    out = np.zeros(hi - lo, dtype=np.uint16)
    for p0 in range(lo, hi, cpg):
        cnt = min(cpg, hi - p0)
        K0, K1 = int(idx[p0]), int(idx[p0 + cnt])
        acc = [0] * cnt
        starts = {int(idx[p0 + j]) - K0: j for j in range(cnt) if idx[p0 + j + 1] > idx[p0 + j]}
        carry_cid, carry_par = -1, 0
        for kb in range(K0, K1, 64):
            nv = min(64, K1 - kb)
            sums = [h[kb + j] & M32 for j in range(nv)] + [0] * (64 - nv)
            if bug in ("cs==T read as 0", "padding lanes counted", "short < and ninth segment dropped"):
                a = [int(x) for x in A[kb:kb + nv]] + [0] * (64 - nv)
                l = [int(x) for x in Ln[kb:kb + nv]] + [0] * (64 - nv)
                sums = _slice_bug(bug, c.payload, a, l, sums, nv)
            cid, par = carry_cid, (0 if bug == "parity not carried" else carry_par)
            for j in range(nv):
                if kb - K0 + j in starts:
                    cid, par = starts[kb - K0 + j], 0
                r = _fold(sums[j])
                swap = (A[kb + j] & 1) == 0 if bug == "swap from the address alone" else (A[kb + j] & 1) == par
                if swap:
                    r = ((r & 0xFF) << 8) | (r >> 8)
                if cid >= 0:
                    acc[cid] += r
                par ^= int(Ln[kb + j]) & 1
            carry_cid, carry_par = (-1 if bug == "chain id not carried" else cid), par
        for j in range(cnt):
            r = _fold(int(c.states[p0 + j]) + _fold(acc[j]))
            out[p0 - lo + j] = ~r & 0xFFFF
    return out


def _disagrees(oracle, name, bug, cpg, pick=None):
    """The wrong model differs from the oracle somewhere; the right one nowhere (same chains)."""
    case = X.case(name, oracle)
    want = X.expected(oracle, name)
    lo, hi = pick or case.calls[0]
    assert (hi - lo) % cpg == 0 or hi == case.calls[0][1]
    right = X.cached(("chain-model", name, lo, hi, cpg), lambda: chain_model(case.chains, lo, hi, cpg))
    assert np.array_equal(right, want[lo:hi]), (name, "the model itself")
    assert not np.array_equal(chain_model(case.chains, lo, hi, cpg, bug), want[lo:hi]), (name, bug)


def _check_gathered(case, chain_ids, Us=(4,)):
    """gathered_model on the first slice of each chain given (S, L, R, B: a chain is a slice or
    less; T: the 64 chunks from the chain's first) against the exact halves-sums."""
    c = case.chains
    A, Ln, idx = _flat(c)
    h = _halves(c)
    for i in chain_ids:
        k0 = int(idx[i])
        k1 = min(k0 + 64, int(idx[-1]))
        for U in Us:
            got = gathered_model(c.payload, A[k0:k1], Ln[k0:k1], U)
            assert got[:k1 - k0] == [x & M32 for x in h[k0:k1]], (i, U)


# ---- forms -------------------------------------------------------------------------------------------

def test_forms_reach_every_value_and_kernel():
    vals = {k: set() for k in X.DEFAULTS}
    for t, jw in X.FORMS.values():
        assert set(t) <= set(X.DEFAULTS)
        for k in X.DEFAULTS:
            vals[k].add(t.get(k, X.DEFAULTS[k]))
    assert vals["stream"] >= {0, 2}
    assert vals["chunk_packets"] >= {0, 1, 2, 4, 8, 16, 32, 64}
    assert vals["chunks_per_wave"] >= {0, 2, 3, 4096}
    assert vals["chain_short"] >= {-1, 0, 1, 65535}
    hint = {name for name, (t, jw) in X.FORMS.items() if jw}
    assert {"jw", "jw-su2", "jw-short0", "jw-cpg64", "jw-cpg1"} <= hint
    assert X.FORMS["su2-cpg64"][0] == {"stream": 2, "chunk_packets": 64}
    assert X.FORMS["short0-cpg1"][0] == {"chain_short": 0, "chunk_packets": 1}
    # the product build: every (SU, COLS) launch_chain can instantiate
    assert {X.kernel_form(n) for n in X.FORMS} == X.PRODUCT_KERNELS
    assert X.kernel_form("jw") == (4, True) and X.kernel_form("jw-su2") == (2, False)
    assert X.kernel_form("jw-short0") == (4, False)
    for fam, names in X.FAMILY_FORMS.items():
        assert set(names) <= set(X.FORMS), fam


# ---- T -----------------------------------------------------------------------------------------------

def test_table_family_holds_every_start_crossing_and_parity(oracle):
    case = X.case("T")
    c = case.chains
    lo, hi = case.calls[0]
    assert {t for t in case.tags if isinstance(t, tuple)} == {(s, L) for s in range(64) for L in X.T_COUNTS}
    A, Ln, idx = _flat(c)
    full = {(s, x, p) for s in range(64) for x, p in ((False, None), (True, 0), (True, 1))}
    for cpg in X.CPGS:
        triples, carry = X.t_triples(c, cpg, lo, hi)
        if cpg == 1:
            # NARROWED: with one chain per group every chain starts at its group's first chunk, so
            # only s == 0 can occur, and lane 0 of a later slice always continues the one chain
            assert triples == {t for t in full if t[0] == 0} and carry == {"continued"}
        else:
            assert triples >= full, (cpg, sorted(full - triples)[:5])
            assert carry == {"continued", "fresh"}, cpg
    # the target's chunk at lane 63 and at lane 0 of a later slice: empty and not, and the chunk
    # at lane 0 (the one that crosses) at an odd and at an even address
    seen = set()
    for i, tag in enumerate(case.tags):
        if not isinstance(tag, tuple):
            continue
        s = tag[0]
        for k in range(int(idx[i]), int(idx[i + 1])):
            lane = (s + k - int(idx[i])) % 64
            if lane in (0, 63) and s + k - int(idx[i]) >= 63:
                seen.add((lane, Ln[k] == 0, int(A[k]) & 1 if lane == 0 else None))
    assert seen >= {(0, True, 0), (0, True, 1), (0, False, 0), (0, False, 1), (63, True, None), (63, False, None)}
    # the empty-chain edges
    tags = case.tags
    i = tags.index("first-empty")
    assert i % 64 == 1 and not c.chains[i - 1]
    assert not c.chains[tags.index("last-nonempty") + 63] and c.chains[tags.index("last-nonempty") + 62]
    e = tags.index("empty-between")
    assert not c.chains[e] and len(c.chains[e - 1]) == 70 and len(c.chains[e + 1]) == 70
    g = (tags.index("last-nonempty") + 64)
    assert g % 64 == 0 and not any(c.chains[g:g + 64]) and any(c.chains[g - 64:g]) and any(c.chains[g + 64:g + 128])
    # every batch size, so cnt < 64 at every residue for every cpg
    assert [b - a for a, b in case.calls[1:]] == list(range(1, X.T_BATCH_MAX + 1))
    for cpg in X.CPGS:
        assert {(b - a) % cpg for a, b in case.calls[1:]} == set(range(cpg))
    assert min(Ln) == 0 and max(Ln) == 3


def test_table_family_against_the_models(oracle):
    case = X.case("T")
    want = X.expected(oracle, "T")
    lo, hi = case.calls[0]
    part = (0, 64 * len(X.T_COUNTS) * 4)                       # s in 0..3, whole groups
    for cpg in (64, 2):
        assert np.array_equal(chain_model(case.chains, part[0], part[1], cpg), want[part[0]:part[1]])
    assert np.array_equal(chain_model(case.chains, hi - 320, hi, 64), want[hi - 320:hi])
    for a, b in case.calls[1::9]:
        assert np.array_equal(chain_model(case.chains, a, b, 64), want[a:b])
    _check_gathered(case, [i for i, t in enumerate(case.tags) if isinstance(t, tuple)])
    _disagrees(oracle, "T", "parity not carried", 64, part)
    _disagrees(oracle, "T", "chain id not carried", 64, part)
    _disagrees(oracle, "T", "swap from the address alone", 64, part)


# ---- S -----------------------------------------------------------------------------------------------

def test_stream_family_holds_every_geometry(oracle):
    case = X.case("S")
    A, Ln, idx = _flat(case.chains)
    assert (np.diff(idx) == 64).all()
    ns = np.where(Ln > 0, ((A & 15) + Ln + 15) >> 4, 0).reshape(-1, 64)
    T = ns.sum(axis=1)
    tags = case.tags
    assert [int(t) for t, tag in zip(T, tags) if tag[0] == "T"] == list(range(1, X.S_MAX + 1))
    for U in (2, 4):
        got = {X.s_geometry(int(t), U) for t in T}
        want = {(g, g % 2, r) for g in range(1, 6) for r in range(U)}
        assert got >= want, (U, sorted(want - got))
        assert max(X.s_geometry(int(t), U)[0] for t in T) >= 6          # the loop's second iteration
    full = Ln > 0
    assert {int(x) for x in (A[full] & 15)} == set(range(16))
    assert {int(x) for x in ((A[full] + Ln[full]) & 15)} == set(range(16))
    cs = np.cumsum(ns, axis=1) - ns
    for i, tag in enumerate(tags):
        if tag[0] == "trail":
            assert T[i] == tag[1] and (ns[i, 64 - tag[2]:] == 0).all() and ns[i, 63 - tag[2]] > 0
            assert (cs[i, 64 - tag[2]:] == T[i]).all()
        elif tag[0] == "own":
            assert ns[i, tag[2]] == tag[1] == T[i]
        elif tag[0] == "win":
            assert T[i] == tag[1] and ns[i, 0] == tag[2] and cs[i, 1] == tag[2]
    assert {t[1] for t in tags if t[0] == "win"} == set(range(64, X.S_MAX + 1, 64))
    assert int(Ln.max()) <= 65535
    assert X.touching(case.chains) == 0


def test_stream_family_against_the_models(oracle):
    case = X.case("S")
    want = X.expected(oracle, "S")
    n = len(case.tags)
    assert np.array_equal(chain_model(case.chains, 0, n, 1), want)
    # every case through gathered_model at U = 4 (about 5 s: the model visits every lane of every
    # window in Python). NARROWED for U = 2 alone, for time: the T up to 200 segments, which hold
    # every (groups, nwin mod 2) up to two groups, and every third variant
    _check_gathered(case, range(n), (4,))
    small = [i for i, t in enumerate(case.tags) if t[0] == "T" and t[1] <= 200]
    _check_gathered(case, small + [i for i, t in enumerate(case.tags) if t[0] != "T"][::3], (2,))
    trail = [i for i, t in enumerate(case.tags) if t[0] == "trail"]
    _disagrees(oracle, "S", "cs==T read as 0", 1, (trail[0], trail[-1] + 1))
    _disagrees(oracle, "S", "padding lanes counted", 1, (0, 200))


# ---- L -----------------------------------------------------------------------------------------------

def test_length_family_holds_every_length_start_and_line_outcome(oracle):
    case = X.case("L")
    c = case.chains
    A, Ln, idx = _flat(c)
    dense, edge, outcomes, lone_nsg = set(), set(), {True: set(), False: set()}, set()
    for i, tag in enumerate(case.tags):
        if tag[0] == "pair":
            continue
        l, st, par, lay = tag
        k = int(idx[i]) + 1
        assert Ln[k] == l and A[k] % 128 == st and Ln[k - 1] % 2 == par
        (dense if l <= X.L_DENSE else edge).add((l, int(A[k]) % (128 if l <= X.L_DENSE else 16), par if l <= X.L_DENSE else None))
        a = [int(x) for x in A[k - 1:k + 2]] + [0]
        n = [int(x) for x in Ln[k - 1:k + 2]] + [0]
        rule = X.short_rule(a, n)
        lone, t1, t2 = rule[1]
        outcomes[l <= 128].add((t1, t2))
        # under chunk_packets 1 the chain is a slice of its own: its run chunks (those not lone
        # short) lie back to back, so the column-run form takes it; away from its neighbours the
        # swept chunk is the one run chunk if it is over 128 bytes, else all three are lone short
        run = [j for j in range(3) if not rule[j][0]]
        assert all(a[i] + n[i] == a[j] for i, j in zip(run, run[1:])), tag
        assert lay == X.B2B or run == ([1] if l > 128 else []), tag
        if lone:
            lone_nsg.add(((a[1] & 15) + l + 15) >> 4)
    assert dense == {(l, st, p) for l in range(1, X.L_DENSE + 1) for st in range(128) for p in (0, 1)}
    assert edge == {(l, st, None) for l in X.L_EDGE for st in range(16)}
    both = {(x, y) for x in (False, True) for y in (False, True)}
    assert outcomes[True] == both and outcomes[False] == both
    assert lone_nsg == set(range(1, 10))                     # sum_short_chunk_from: every segment count
    # the 1-byte pairs are run chunks: each shares its line with the other, but at the line's edge
    pairs = [i for i, t in enumerate(case.tags) if t[0] == "pair"]
    assert len(pairs) == 128
    lone_pairs = 0
    for i in pairs:
        k = int(idx[i])
        assert Ln[k] == Ln[k + 1] == 1 and A[k] + 1 == A[k + 1]
        rule = X.short_rule([int(A[k]), int(A[k + 1]), 0], [1, 1, 0])
        lone_pairs += rule[0][0] + rule[1][0]
    assert lone_pairs == 2                                   # only the pair split by a line edge (start 127)


def test_length_family_against_the_models(oracle):
    case = X.case("L")
    want = X.expected(oracle, "L")
    n = len(case.tags)
    pick = list(range(0, n, 23))
    for i in pick[:400]:
        assert chain_model(case.chains, i, i + 1, 1)[0] == want[i], case.tags[i]
    # NARROWED, for time (all 39,000 chains would take about a minute): gathered_model on every
    # 601st chain under 5000 bytes
    _check_gathered(case, [i for i in range(0, n, 601) if case.tags[i][0] == "pair" or case.tags[i][0] < 5000])
    nine = [i for i, t in enumerate(case.tags) if t[0] != "pair" and t[3] != X.B2B and 113 <= t[0] <= 127 and t[1] % 16 == 15]
    assert nine
    got = np.concatenate([chain_model(case.chains, i, i + 1, 1, "short < and ninth segment dropped") for i in nine[:40]])
    assert not np.array_equal(got, want[nine[:40]])


# ---- R -----------------------------------------------------------------------------------------------

def test_run_family_holds_every_run_and_header_count(oracle):
    case = X.case("R")
    c = case.chains
    A, Ln, idx = _flat(c)
    assert (np.diff(idx) == 64).all()
    seen = {}
    for i, tag in enumerate(case.tags):
        nr, ns_, ok = X.cols_slice(A[64 * i:64 * i + 64], Ln[64 * i:64 * i + 64])
        assert ok and (nr, ns_) == tag[:2], (tag, nr, ns_)
        seen.setdefault(nr, set()).add((ns_, tag[2]))
    for nr in range(65):
        for ns_ in {0, 1, 2, 64 - nr}:
            if nr + ns_ <= 64:
                assert {(ns_, k) for k in range(3)} <= seen[nr], (nr, ns_)
    assert (32, 0, "max") in case.tags and int(Ln.max()) == 65535
    assert {int(x) for x in Ln} >= set(X.R_LENS)
    assert X.touching(c) > 0
    ch = sorted((int(o), int(n)) for o, n in zip(A, Ln) if n)
    assert all(o + n <= o2 for (o, n), (o2, _) in zip(ch, ch[1:]))     # nothing overlaps
    # the broken runs: the run chunks no longer back to back, nothing overlapping, the moved
    # chunk in the second allocation
    br = X.case("R-broken")
    A, Ln, idx = _flat(br.chains)
    assert {(t[0], t[2]) for t in br.tags} == {(nr, h) for nr in X.R_BREAK_NR for h in (1, 16, "far")}
    assert {(t[0], t[1]) for t in br.tags} == {(nr, p) for nr in X.R_BREAK_NR for p in range(1, nr)}
    for i, tag in enumerate(br.tags):
        a, n = A[64 * i:64 * i + 64], Ln[64 * i:64 * i + 64]
        nr, ns_, ok = X.cols_slice(a, n)
        assert nr == tag[0] and not ok, tag
        assert ((a >= br.split).sum() == 1) == (tag[2] == "far")
    ch = sorted((int(o), int(n)) for o, n in zip(A, Ln) if n)
    assert all(o + n <= o2 for (o, n), (o2, _) in zip(ch, ch[1:]))
    assert not br.chains.described[br.split - X.GUARD:br.split + X.GUARD].any()


def test_run_family_against_the_models(oracle):
    case = X.case("R")
    c = case.chains
    A, Ln, idx = _flat(c)
    h = _halves(c)
    want = X.expected(oracle, "R")
    n = len(case.tags)
    assert np.array_equal(chain_model(c, 0, n, 1), want)
    # NARROWED, for time (T and S run through gathered_model in full instead): every sixth
    # unbroken slice through the column-run model, the 32 x 65535-byte one left to the halves-sums
    # above, and some of them through the gathered stream too
    for i in range(0, n - 1, 6):
        got = chain_cols_model(c.payload, A[64 * i:64 * i + 64], Ln[64 * i:64 * i + 64])
        assert got is not None and got == [x & M32 for x in h[64 * i:64 * i + 64]], case.tags[i]
    _check_gathered(case, [i for i in range(0, n - 1, 5) if int(Ln[64 * i:64 * i + 64].sum()) < 20000][::6])
    br = X.case("R-broken")
    assert np.array_equal(chain_model(br.chains, 0, len(br.tags), 1), X.expected(oracle, "R-broken"))


# ---- B, C, F -------------------------------------------------------------------------------------------

def test_fold_family(oracle):
    case = X.case("B", oracle)
    c = case.chains
    want = X.expected(oracle, "B")
    A, Ln, idx = _flat(c)
    assert (np.diff(idx) == X.B_CHUNKS).all()
    kinds = set()
    for (i, p, q), tag in zip(case.fix, case.tags):
        assert want[i] == 0 and tag[0] in ("cut", "slice", "seg")
        ks = [k for k in range(int(idx[i]), int(idx[i + 1])) if A[k] <= p < A[k] + Ln[k] or A[k] <= q < A[k] + Ln[k]]
        if tag[0] == "seg":
            assert len(ks) == 1 and p % 16 == 15 and q == p + 1
        else:
            assert len(ks) == 2 and q != p + 1
            if tag[0] == "slice":
                assert ks[0] - int(idx[i]) == 63 and ks[1] - int(idx[i]) == 64
        kinds.add((tag[0], tag[1], p % 16))
    assert kinds >= {(k, st, r) for k in ("cut", "slice") for st in X.B_STATES for r in range(16)}
    assert {(t[0], t[1]) for t in case.tags} == {(k, st) for k in ("cut", "slice", "seg", "fill") for st in X.B_STATES}
    fills = [i for i, t in enumerate(case.tags) if t[0] == "fill"]
    for i in fills:
        if case.tags[i][2] == 7:                             # all-zero chunks: the state's own checksum
            assert want[i] == ~_fold(case.tags[i][1]) & 0xFFFF
    assert any(want[i] == 0xFFFF for i in fills) and X.touching(c) == 0
    n = len(case.tags)
    assert np.array_equal(chain_model(c, 0, n, 1), want)
    _check_gathered(case, range(0, n, 7))


def test_cropped_family(oracle):
    case = X.case("C")
    c = case.chains
    assert len(c.chains) == X.C_CHAINS
    A, Ln, idx = _flat(c)
    # back to back only where R's runs are: everywhere else an undescribed byte between two chunks
    ch = sorted((int(o), int(n)) for o, n in zip(A, Ln) if n)
    assert all(o + n <= o2 for (o, n), (o2, _) in zip(ch, ch[1:]))
    first_r = int(idx[X.C_CHAINS - X.C_PARTS[3]])
    touch = [(o, n) for (o, n), (o2, _) in zip(ch, ch[1:]) if o + n == o2]
    assert touch and all(o >= int(A[first_r:].min()) for o, _ in touch)
    want = X.expected(oracle, "C")
    assert np.array_equal(want, c.expected(oracle, X.alt(c.payload, c.described)))
    assert np.array_equal(chain_model(c, 0, X.C_CHAINS, 64), want)
    assert not c.described.all() and c.described.any()


def test_field_family(oracle):
    cus = 8
    big = X.f_big(cus)
    n, idx, off, lens, states, payload = big
    assert n == cus * 64 * 256 + 513 and n > cus * 64 * 256         # the scatter loop's second iteration
    full = np.diff(idx.astype(np.int64))
    assert full.sum() == len(off) == -(-(n - 17) // X.F_EVERY) and set(full) == {0, 1}
    want = X.f_big_expected(oracle, big)
    empty = np.flatnonzero(full == 0)[:2000]
    for i in empty[::97]:
        assert want[i] == ~_fold(int(states[i])) & 0xFFFF
    buf, v = X.filled_fields(n, want, True)
    assert buf.size == 3 * n + 2 and (X.field_offsets(n)[6::7] == -1).all()
    assert {int(o) & 1 for o in X.field_offsets(n) if o >= 0} == {0, 1}
