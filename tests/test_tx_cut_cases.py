"""The inputs of test_gpu_tx_cut.py are not vacuous: the coverage sets of tx_cut_cases.py's batches,
in numbers computed from the cases and the models alone, without a GPU.

Of the stand-alone host programs of tests/cpp on the send side only tx_resolve_build_test takes its
cases from a file: family C's header rings go through it. tcpseg_layout_test, ipfrag_layout_test,
tx_producer_test and linearise_plan_test carry their cases in their own text and take none from
outside; the header-split fill and the chained batch have no host program (their reference is the
CPU oracle)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import hsplit_cases as H
import ipfrag_cases as U
import tcpseg_cases as T
import tx_cut_cases as X
import tx_resolve_cases as RC

KINDS = ("tcp", "udp")
SHORTS = ["short%d" % a for a in range(16)]
CROSS = sum(D + 1 for D in range(X.SHORT + 1)) * 256           # 43,776: D 0..17 x cut x a0 x a1
ALL16 = set(range(16))


def _spec(c, x=0):
    """(D, l0, a0, a1, x) of a two-piece case as its offsets, not its builder, give it."""
    (o0, l0), (o1, l1) = c["pieces"]
    return l0 + l1, l0, o0 % 16, o1 % 16, x


# ---- family A, the producers -----------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_short_payloads_are_a_full_cross(oracle, kind):
    seen, mss_at, with_a0, with_a1 = set(), {}, set(), set()
    for name in SHORTS:
        b, _ = X.producer(oracle, kind, name)
        for c in b.cases:
            D, l0, a0, a1, _ = _spec(c)
            seen.add((D, l0, a0, a1))
            p = c["mss"] if kind == "tcp" else c["mtu"]
            mss_at.setdefault((D, l0), set()).add(p)
            with_a0.add((p, a0))
            with_a1.add((p, a1))
    assert len(seen) == CROSS == 43776
    assert seen == {(D, l0, a0, a1) for D in range(18) for l0 in range(D + 1) for a0 in range(16) for a1 in range(16)}
    params = set(X.MSS if kind == "tcp" else X.MTUS)
    assert all(v == params for v in mss_at.values())           # every mss / MTU at every (D, cut)
    assert with_a0 == with_a1 == {(p, a) for p in params for a in range(16)}
    assert X.MSS[:4] == (1, 7, 16, 33) and X.MSS[4] >= X.LONG
    assert [(m - 20) % 8 for m in X.MTUS] == [0, 2, 3] and X.MTUS[0] >= 28 + X.LONG
    # no datagram of this sweep is cut, whatever its MTU: the contract wants mtu >= MIN_MTU = 256
    # (ipfrag_cases.descriptor_ok), which leaves a datagram of up to MIN_MTU - 28 = 228 payload
    # bytes whole. Fragment boundaries are swept by the "frag" batch instead (payloads of 226 to 507
    # bytes at the two MTUs with (mtu - 20) % 8 != 0).
    assert min(X.MTUS) >= U.MIN_MTU == 256 and X.LONG <= U.MIN_MTU - 28


@pytest.mark.parametrize("kind", KINDS)
def test_longer_payloads_have_every_triple(oracle, kind):
    b, e = X.producer(oracle, kind, "long")
    specs = [_spec(c) for c in b.cases]
    assert {(D, l0) for D, l0, *_ in specs} == {(D, l0) for D in range(18, 131) for l0 in range(D + 1)}
    assert len(specs) == 8475
    first, second = X.triples(specs)
    # the first piece starts the datagram, so its bytes join the sum at offset 0 (UDP: behind the
    # 8 header bytes): parity 0 is the only one it can have; the second piece has both
    assert first == {(a, r, 0) for a in range(16) for r in range(16)}
    assert second == {(a, r, p) for a in range(16) for r in range(16) for p in (0, 1)}
    assert len(e.status) < 100000
    if kind == "tcp":
        assert {c["mss"] for c in b.cases} == set(X.MSS_LONG)


def test_tcp_segments_begin_at_every_alignment_and_parity(oracle):
    starts, two = set(), set()
    for name in SHORTS + ["long"]:
        b, e = X.producer(oracle, "tcp", name)
        for ch in e.seg_chunks:
            if ch:
                starts.add((ch[0][0] % 16, ch[0][1] % 16))
            if len(ch) == 2:
                two.add((ch[1][0] % 16, ch[0][1] & 1))
    assert starts == {(a, r) for a in range(16) for r in range(16)}      # first chunk: address x length
    assert two == {(a, p) for a in range(16) for p in (0, 1)}            # second chunk: address x parity


def _straddles_tcp(b):
    """Segments of two chunks with an odd first length, from the descriptors alone: the segment that
    holds the piece boundary, unless the boundary is a segment's edge."""
    n = 0
    for c in b.cases:
        (_, l0), (_, l1) = c["pieces"]
        if l0 and l1 and l0 % c["mss"]:
            n += (l0 % c["mss"]) & 1
    return n


@pytest.mark.parametrize("name", X.PRODUCER_BATCHES["tcp"] + ["mixed"])
def test_tcp_batches_hold_their_classes(oracle, name):
    b, e = X.producer(oracle, "tcp", name)
    assert T.model_layout(b.cases) is not None and (e.status == T.ACCEPT).all()
    assert T.count_straddle_odd_first(e) == _straddles_tcp(b)
    f = T.count_flags(e)
    if name == "fold":
        assert _straddles_tcp(b) >= 16 * len(X.FOLD_D) and f["fin_psh"] >= 100
    else:
        assert _straddles_tcp(b) >= (15 if name == "mixed" else 400)
        assert min(f.values()) >= (10 if name == "mixed" else 300), f
        assert not name.startswith("short") or any(len(ch) == 0 for ch in e.seg_chunks)     # FIN alone: D = 0
    buf, off, ids = T.linearise(e, b.payload)
    assert len(ids) == len(e.status) and (oracle.rx_verify_batch(buf, off) == T.ACCEPT).all()


@pytest.mark.parametrize("name", X.PRODUCER_BATCHES["udp"] + ["mixed"])
def test_udp_batches_hold_their_classes(oracle, name):
    b, e = X.producer(oracle, "udp", name)
    assert U.model_layout(b.cases) is not None and (e.status == U.ACCEPT).all()
    odd = U.count_straddle_odd_first(e)
    whole = [c for c in b.cases if len(U.ip_packets_of(c)) == 1]
    odd_whole = sum(1 for c in whole if c["pieces"][0][1] & 1 and c["pieces"][1][1])
    if name == "frag":
        # payloads above MIN_MTU - 28 = 228 bytes, the least that any valid MTU (>= ipfrag_cases.MIN_MTU)
        # can cut: a datagram of up to mtu - 28 bytes stays whole, the others are fragmented
        assert min(c["pieces"][0][1] + c["pieces"][1][1] for c in b.cases) <= U.MIN_MTU - 28 + 6
        br = U.branches(b, e)
        assert br >= {"S=1", "S>1", "straddle", "no_straddle", "edge", "clamped", "last>F"}, br
        assert {c["mtu"] for c in b.cases} == set(X.MTUS[1:]) and 200 <= len(whole) < len(b.cases) - 1000
        assert odd >= odd_whole + 500
        k1 = [ch for ch, k in zip(e.frag_chunks, e.frag_k) if k >= 1 and ch]
        # a later fragment starts at a multiple of 8 of the datagram: an even offset of the sum
        assert {ch[0][0] % 16 for ch in k1} == ALL16
    elif name == "mixed":
        assert odd >= odd_whole >= 16 and len(whole) < len(b.cases)
    else:
        assert len(whole) == len(b.cases) and odd == odd_whole >= 64
    udp = e.headers[:, 40].astype(int) << 8 | e.headers[:, 41]
    first = e.hdr_len == U.HDR0
    if name == "fold":
        assert (udp[first] == 0xFFFF).all() and first.sum() == len(b.cases) == 304
    else:
        assert (udp[first] == 0).sum() == 0
    buf, off, ids = U.linearise(e, b.payload)
    v = oracle.rx_verify_batch(buf, off)
    frag = (e.headers[:, 20] & 0x3F).astype(bool) | e.headers[:, 21].astype(bool)
    assert len(ids) == len(e.status) and np.array_equal(v, np.where(frag, X.FRAGMENT, U.ACCEPT))


# ---- family B ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_completing_bytes_lie_at_every_address_and_across_the_cut(oracle, kind):
    b, e = X.producer(oracle, kind, "fold")
    where = X.completing_bytes(b)
    for D in X.FOLD_D:
        rows = [w for w, s in zip(where, b.specs) if s[0] == D]
        cuts = {s[1] for s in b.specs if s[0] == D}
        assert cuts == set(range(max(D - 3, 0), D + 1))              # the last four positions
        for l0 in cuts:
            got = {w[0] for w, s in zip(where, b.specs) if s[0] == D and s[1] == l0}
            assert got == ALL16                                      # both parities, and 15: a segment's edge
        assert any(w[1] for w in rows)                               # the two bytes in two pieces
    if kind == "tcp":
        tcp = e.headers[:, 50].astype(int) << 8 | e.headers[:, 51]
        assert (tcp == 0).all() and len(tcp) == 304


# ---- the header-split fill -------------------------------------------------------------------------

def _split_specs(s):
    """(D, l0, a0, a1, x) of the segments of a two-chunk layout, from the layout's own offsets."""
    out = []
    for (variant, x, parts), ch in zip(s.seg, s.sp.chunks):
        at = iter(ch)
        a = [next(at)[0] % 16 if l else 0 for l, _ in parts]
        out.append((parts[0][0] + parts[1][0], parts[0][0], a[0], a[1], x))
    return out


@pytest.mark.parametrize("name", list(X.SPLIT_BATCHES))
def test_every_split_segment_is_in_layout_and_filled(oracle, name):
    s = X.split(name)
    want_h, want_st, st_lin, ok = H.expected(oracle, s.sp)
    assert ok.all() and (want_st == H.ACCEPT).all() and len(s.sp.chunks) < 100000
    # the filled segments as the linearise model lays them out: exact rooms, and every frame verifies
    sc = X.split_scenario(s.sp, want_h, want_st, "csr")
    dest, lens, status = sc.expected()
    buf, off = s.sp.linearise(headers=want_h)
    assert (status == X.LC.WRITTEN).all() and np.array_equal(dest, buf) and np.array_equal(off, sc.offsets)
    assert (oracle.rx_verify_batch(dest, sc.offsets) == H.ACCEPT).all()
    if name == "points":                   # what the producers never leave: these header lengths, three chunks
        assert set(s.sp.hdr_lens.tolist()) >= set(range(42, 147)) and lens.max() <= X.SLOT_STRIDE


def test_split_short_payloads_are_a_full_cross():
    seen = set()
    for name in SHORTS:
        s = X.split(name)
        for (D, l0, a0, a1, x), (variant, *_), ch in zip(_split_specs(s), s.seg, s.sp.chunks):
            # an empty chunk is not in the table: its address is nobody's
            seen.add((D, l0, a0 if l0 else -1, a1 if D - l0 else -1))
            assert variant in X.VARIANTS[:3]
    want = {(D, l0, a0 if l0 else -1, a1 if D - l0 else -1)
            for D in range(18) for l0 in range(D + 1) for a0 in range(16) for a1 in range(16)}
    assert seen == want
    assert sum(len(X.split(n).sp.chunks) for n in SHORTS) == CROSS


def test_split_longer_payloads_have_every_triple():
    s = X.split("long")
    specs = _split_specs(s)
    assert {(D, l0) for D, l0, *_ in specs} == {(D, l0) for D in range(18, 131) for l0 in range(D + 1)}
    first, second = X.triples(specs)
    full = {(a, r, p) for a in range(16) for r in range(16) for p in (0, 1)}
    assert first == full and second == full                         # x = 0 and 1: both parities for either
    assert {v for v, *_ in s.seg} == set(X.VARIANTS)


def test_split_points_and_pieces():
    s = X.split("points")
    seen, cuts = set(), set()
    for (v, x, parts), h, ch in zip(s.seg, s.sp.hdr_lens, s.sp.chunks):
        if len(v) > 3:                                   # x from the end of the fixed header on
            seen.add((v[:3], x + parts[0][0], x))
        else:
            P = sum(l for l, _ in parts)
            cuts.add((P, parts[0][0], parts[0][0] + parts[1][0]))
            assert len(ch) == sum(1 for l, _ in parts if l)
    for v in X.VARIANTS:
        opts = 4 * (v[2] - 5) if v[0] == "tcp" else 0
        for P in range(49):
            assert {x for vv, body, x in seen if vv == v and body == opts + P} == set(range(opts + P + 1))
    assert cuts == {(P, c1, c2) for P in range(25) for c1 in range(P + 1) for c2 in range(c1, P + 1)}
    assert {len(ch) for ch in s.sp.chunks} == {0, 1, 2, 3}
    assert {(v[1], v[2]) for v in X.VARIANTS if v[0] == "tcp"} == {(5, 5), (5, 15), (6, 5), (6, 15)}
    assert {v[1] for v in X.VARIANTS if v[0] == "udp"} == {5, 6}


def test_split_fold_places_the_folding_seed_at_every_address():
    s = X.split("fold")
    seen = set()
    for (v, x, parts), ch in zip(s.seg, s.sp.chunks):
        rest = parts[0][0] + parts[1][0]
        assert rest - parts[0][0] <= 3
        if len(ch) == 2:
            seen.add((x, ch[0][0] % 16, ch[1][0] % 2))
    assert seen == {(x, a, p) for x in range(4) for a in range(16) for p in (0, 1)}


# ---- the chained batch -----------------------------------------------------------------------------

def test_chains_cover_lengths_addresses_and_empty_chunks(oracle):
    specs = X.chain_specs()
    assert len(specs) == 34 * 16 + 34 * 34 * 32 + 34 ** 3 < 100000
    one = {(p[0][0], p[0][1]) for u, p in specs if len(p) == 1}
    assert one == {(l, a) for l in range(34) for a in range(16)}
    for under in (0, 1):
        two = {(p[0][0], p[1][0], p[under][1]) for u, p in specs if len(p) == 2 and u == under}
        assert two == {(l0, l1, a) for l0 in range(34) for l1 in range(34) for a in range(16)}
    assert {tuple(l for l, _ in p) for u, p in specs if len(p) == 3} == \
        {(a, b, c) for a in range(34) for b in range(34) for c in range(34)}
    # three chunks have no chunk under test: every address for each of them against every triple
    # of lengths would be 34^3 x 16 x 3 = 1.9 million chains where a batch is to stay below
    # 100,000. The addresses are dealt out instead so that per position every (address, length
    # mod 16, start parity) occurs, which is what selects a chunk's masks and its byte swap; every
    # address against every pair of lengths is held by the two-chunk chains above.
    t = X.chain_triples(specs, 3)
    assert t[0] == {(a, r, 0) for a in range(16) for r in range(16)}     # a chain's first chunk starts the sum
    full = {(a, r, p) for a in range(16) for r in range(16) for p in (0, 1)}
    assert t[1] == full and t[2] == full
    for pos in range(3):                                                 # an empty chunk first, in the middle, last
        assert sum(1 for u, p in specs if len(p) == 3 and p[pos][0] == 0 and
                   all(l for k, (l, _) in enumerate(p) if k != pos)) == 33 * 33
    c = X.cached("chainA", lambda: X.chain_batch(oracle, specs, 60))
    want = c.expected(oracle)
    assert (want[::50] == 0).all() and (want == 0).sum() >= 1537          # zero-as-0xFFFF has something to do
    assert [o % 16 for ch in c.chains for o, _ in ch] == [a for _, p in specs for _, a in p]


# ---- family C ------------------------------------------------------------------------------------

def _gaps(chunks):
    s = sorted(chunks)
    return {b[0] - (a[0] + a[1]) for a, b in zip(s, s[1:])}


def _both_kinds_of_byte(chunks, data, described):
    other = X.alt(data, described)
    assert np.array_equal(other[described], data[described]) and (other[~described] != data[~described]).all()
    same, after = X.end_alignments(chunks, described)
    assert same >= set(range(1, 16)) and after >= set(range(1, 16)), (same, after)
    assert _gaps(chunks) >= set(range(18))


@pytest.mark.parametrize("kind", KINDS)
def test_mixed_producer_batch(oracle, kind):
    b, e = X.producer(oracle, kind, "mixed")
    assert 460 <= len(e.status) <= X.C_SEGMENTS
    _both_kinds_of_byte(b.pieces(), b.payload, b.described)
    chunks = [c for ch in (e.seg_chunks if kind == "tcp" else e.frag_chunks) for c in ch]
    same, after = X.end_alignments(chunks, b.described)
    assert same >= set(range(1, 16)) and after >= set(range(1, 16))
    other = X.alt_templates(b)
    layout = T.model_layout if kind == "tcp" else U.model_layout
    assert layout(other.cases) is not None
    for c, d in zip(b.cases, other.cases):
        diff = {k for k in range(len(c["hdr"])) if c["hdr"][k] != d["hdr"][k]}
        assert diff == set(X.TEMPLATE_OVERWRITTEN[kind]) and len(diff) == 16
    e2 = X.expect(oracle, other)                              # the model does not see them either
    for k in ("headers", "status", "chunk_off", "chunk_len", "chunk_index"):
        assert np.array_equal(getattr(e, k), getattr(e2, k)), k
    if kind == "udp":
        assert (np.diff(U.caller_index(b.cases)[0].astype(np.int64)) > 1).sum() >= 20   # fragmented ones


def test_mixed_split_and_chain_batches(oracle):
    s = X.split("mixed")
    assert len(s.sp.chunks) == X.C_SEGMENTS
    _both_kinds_of_byte([c for ch in s.sp.chunks for c in ch], s.sp.payload, s.described)
    other = s.alt()
    one, two = H.expected(oracle, s.sp), H.expected(oracle, other)
    assert np.array_equal(one[1], two[1]) and one[3].all()
    h1, h2 = (w[0].reshape(-1, X.SPLIT_STRIDE) for w in (one, two))
    inside = np.arange(X.SPLIT_STRIDE)[None, :] < s.sp.hdr_lens[:, None]
    assert np.array_equal(h1[inside], h2[inside]) and (h1[~inside] != h2[~inside]).all()
    assert (s.sp.hdr_lens < X.SPLIT_STRIDE).all()             # every slot is wider than its header
    c = X.cached("chainC", lambda: X.chain_mixed(oracle))
    assert len(c.chains) == X.C_SEGMENTS
    _both_kinds_of_byte([x for ch in c.chains for x in ch], c.payload, c.described)
    assert np.array_equal(c.expected(oracle), c.expected(oracle, X.alt(c.payload, c.described)))


def _resolve_case(oracle, kind):
    """The mixed batch's header ring as Tx resolve takes it, and the model's answer."""
    b, e = X.producer(oracle, kind, "mixed")
    ring, lens = X.want_ring(b, e), X.hdr_lens_of(b, e)
    return ring, lens, e.status, RC.expected(ring, X.HDR_STRIDE, lens, RC.LAN, RC.lan_table(), seg_status=e.status)


@pytest.mark.parametrize("kind", KINDS)
def test_mixed_rings_through_the_tx_resolve_host_program(oracle, kind):
    import test_tx_resolve_host as TH
    ring, lens, ss, r = _resolve_case(oracle, kind)
    assert {RC.SENT, RC.ARP_QUERY, RC.BCAST_REJECTED, RC.NONLOCAL_SRC} <= set(r.status.tolist())
    assert (lens < X.HDR_STRIDE).all()
    other = X.alt_slack(ring, X.HDR_STRIDE, lens)
    slack = np.arange(X.HDR_STRIDE)[None, :] >= lens[:, None]
    assert ((other != ring).reshape(-1, X.HDR_STRIDE) == slack).all()
    r2 = RC.expected(other, X.HDR_STRIDE, lens, RC.LAN, RC.lan_table(), seg_status=ss)
    assert np.array_equal(r.status, r2.status) and r.routes.tobytes() == r2.routes.tobytes()
    rows = ring.reshape(-1, X.HDR_STRIDE)
    headers = [rows[i, :int(lens[i])].tobytes() for i in range(len(lens))]
    lines = []
    TH._tables(lines, RC.LAN, RC.lan_table())
    count = TH._cases(lines, headers, X.HDR_STRIDE, RC.LAN, RC.lan_table(), ss=ss)
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "tx_resolve.mk"], check=True, stdout=subprocess.DEVNULL)
    path = os.path.join(cpp, "build", "tx_cut_%s.txt" % kind)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "tx_resolve_build_test"), path], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK %d cases" % count in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
