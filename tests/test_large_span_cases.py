"""The generators of large_span_cases.py cover what test_gpu_large_span.py relies on -- run on
the CPU for three fake arena pointers: on a multiple of 2^32, 4 KiB below one, 2 MiB above one."""
import numpy as np
import pytest

import aipstack_amd as A

import large_span_cases as L

K = 0x7F3A
POINTERS = [K * L.E32, K * L.E32 - 4096, K * L.E32 + 2 * L.MiB]


# e - start of the packet that holds byte e (0: it starts there), for e = 2^31 and 2^32
ACROSS = {1500: (1148, 796), 9000: (2648, 5296), 65535: (32768, 1), 2048: (0, 0), 2049: (512, 1024)}


def _dist(kind, ln):
    return ln - 1 if kind == "len-1" else kind


def test_a4_lies_in_the_arena_with_room_after_it():
    for P in POINTERS:
        a4 = L.a4_of(P)
        assert a4 % L.E32 == 0 and P < a4 <= P + L.E32
        assert a4 - P + L.GiB <= L.ARENA_BYTES


@pytest.mark.parametrize("plen", [1500, 9000, 65535])
def test_strided_back_to_back(plen):
    for shift in L.SHIFTS:
        c = L.strided_dense(plen, plen, shift)
        L.check_windows(c.windows)
        last_end = (c.n - 1) * c.stride + c.len
        assert L.E32 + L.MiB <= last_end < L.E32 + L.MiB + 2 * plen     # no larger than needed
        assert shift + last_end <= L.ARENA_BYTES
        for e, (i0, cnt, w) in zip(L.EDGES, c.runs):
            assert i0 * plen <= e - L.SIDE and (i0 + cnt) * plen >= e + L.SIDE
            win, lo = L.strided_local(c, (i0, cnt, w))
            assert lo == 0 and win.data.size == cnt * plen
            i = e // plen                      # the packet that holds byte e, or starts at it
            assert i0 < i < i0 + cnt - 1
            # a fixed stride cannot choose e - start; what these lengths give is pinned here
            assert e - i * plen == ACROSS[plen][L.EDGES.index(e)] < plen
        assert c.runs[-1][0] + c.runs[-1][1] == c.n


@pytest.mark.parametrize("stride", [2048, 2049])
def test_strided_dense_gapped(stride):
    for shift in L.SHIFTS:
        c = L.strided_dense(stride, 1500, shift)
        L.check_windows(c.windows)
        assert (c.n - 1) * stride + 1500 >= L.E32 + L.MiB and (c.n - 2) * stride + 1500 < L.E32 + L.MiB
        assert shift + (c.n - 1) * stride + 1500 <= L.ARENA_BYTES
        for e, (i0, cnt, w) in zip(L.EDGES, c.runs):
            assert i0 * stride <= e - L.SIDE and (i0 + cnt) * stride >= e + L.SIDE
            # 2048: a packet starts at the edge (the one before ends 548 bytes short of it);
            # 2049: the packet that holds the edge starts 512 / 1024 bytes before it
            assert e - e // stride * stride == ACROSS[stride][L.EDGES.index(e)] < 1500
    # 2049 puts packets at every residue mod 16 inside a window
    c = L.strided_dense(2049, 1500, 0)
    i0, cnt, _ = c.runs[0]
    assert {(i * 2049) % 16 for i in range(i0, i0 + cnt)} == set(range(16))


@pytest.mark.parametrize("stride,n", L.SPARSE)
@pytest.mark.parametrize("plen", [1500, 65535])
def test_strided_sparse(stride, n, plen):
    for shift in L.SHIFTS:
        c = L.strided_sparse(stride, n, plen, shift)
        L.check_windows(c.windows)
        assert len(c.windows) == n
        for i, w in enumerate(c.windows):
            start = shift + i * stride
            assert w.start == max(start - 16, 0) and w.end == start + plen + 16
        last_end = (n - 1) * stride + plen            # past 2^32, or past 2^31 for the 2^31 stride
        assert last_end > (L.E31 if stride == L.E31 and plen < 65535 else L.E32)
        assert shift + last_end + 16 <= L.ARENA_BYTES


def _check_layout(c):
    L.check_windows(c.windows)
    assert np.all(np.diff(c.offsets.astype(np.int64)) >= 0)
    assert c.shift + int(c.offsets[-1]) <= L.ARENA_BYTES
    assert int(c.offsets[-1]) >= L.E32 + L.MiB
    o = c.offsets.astype(np.int64)
    for e, (i0, cnt, w), x in zip(c.edges, c.runs, c.across):
        assert c.windows[w].start == c.shift + o[i0] and c.windows[w].data.size == o[i0 + cnt] - o[i0]
        assert o[i0] <= e - L.SIDE and o[i0 + cnt] >= e + L.SIDE
        assert i0 <= x < i0 + cnt
        if c.kind == "ends_starts":
            assert o[x] == e and o[x - 1] < e          # one ends at the edge, one starts at it
            assert c.lens[x - 1] > 0 or o[x - 1] == e
        else:
            ln = int(c.lens[x])
            d = L.BIG_BACK if c.kind == "big" else _dist(c.kind, ln)
            assert e - o[x] == d and o[x] < e < o[x + 1]
    # outside the windows: zero fillers of at most 65535 bytes
    assert np.all(c.lens[~c.in_window] <= L.FILL)


@pytest.mark.parametrize("kind", L.CSR_KINDS)
def test_csr_layouts(kind):
    for shift in L.SHIFTS:
        c = L.csr_case(kind, shift)
        _check_layout(c)
        o = c.offsets.astype(np.int64)
        for i0, cnt, _ in c.runs:
            assert cnt >= 256
            ln = c.lens[i0:i0 + cnt]
            assert ln.min() == 0 and (ln[ln <= 1600] > 1500).any()
            assert {int(v) % 16 for v in o[i0:i0 + cnt]} == set(range(16))
        if kind == "big":
            assert all(c.lens[x] == L.FILL for x in c.across)
        assert c.states.size == c.n
        assert set(np.unique(c.states[~c.in_window])) <= set(c.fill_states.tolist())


@pytest.mark.parametrize("kind", L.FRAME_KINDS)
def test_frame_csr_layouts(oracle, kind):
    for shift in L.SHIFTS:
        c = L.frames_csr_case(oracle, kind, shift)
        _check_layout(c)
        assert L.span_of_64(c.offsets) <= 4 * L.MiB
        o = c.offsets.astype(np.int64)
        for (i0, cnt, w), x, e in zip(c.runs, c.across, c.edges):
            assert cnt >= 192 and len(c.frames[w]) == cnt
            assert {int(v) % 16 for v in o[i0:i0 + cnt]} == set(range(16))
            if kind in (1, 15, 16, 17):                    # a header straddles the edge
                assert 0 < e - o[x] < 34 and c.lens[x] >= 60
            buf, off = L.F.pack(c.frames[w])
            assert len(set(oracle.rx_verify_batch(buf, off).tolist())) >= 7   # rejected ones too


def test_frame_pool_has_tcp_hits_for_the_table(oracle):
    pool = L.frame_pool(oracle)
    buf, off = L.F.pack(pool)
    v = oracle.rx_verify_batch(buf, off)
    tbl = L.pcb_table(pool, v, A.TCP_PCB_KEY_DTYPE)
    assert 20 <= tbl.size < 1000
    e = L.R.expected(pool, v, tbl, A.TCP_RX_SEG_DTYPE)
    valid = (e.segs["opts"] & L.R.SEG_VALID) != 0
    assert (valid & (e.pcb != L.R.NO_PCB)).sum() >= 20 and (valid & (e.pcb == L.R.NO_PCB)).sum() >= 20
    assert (e.verdict == L.R.DROP_TCP_OFFSET).any()
    assert sorted(len(f) for f in L.jumbo_frames(oracle)) == [40000, 40000, 65521, 65521, 65535, 65535]


@pytest.mark.parametrize("stride,n", L.SLOTTED)
def test_slotted(oracle, stride, n):
    for frames in (None, L.frame_pool(oracle)):
        for shift in L.SHIFTS:
            c = L.slotted_case(stride, n, shift, frames=frames, jumbo=L.jumbo_frames(oracle))
            L.check_windows(c.windows)
            assert n * stride > L.E32 and shift + n * stride <= L.ARENA_BYTES
            assert np.all(c.lens <= min(stride, L.FILL))
            nz = np.nonzero(c.lens)[0]
            assert nz.tolist() == c.slots and len(c.frames) == len(c.slots)
            full = min(stride, L.FILL)
            for e in L.EDGES:
                m = e // stride
                assert ((nz >= m - 64) & (nz < m + 64)).sum() >= 100
                if frames is None:
                    assert c.lens[m] == full and c.lens[m - 1] == full
                if e % stride:
                    assert m * stride < e < m * stride + int(c.lens[m])      # across the edge
                else:                  # one starts at the edge; the one before it ends 1 short
                    assert m * stride == e and c.lens[m] >= 60
                    assert (m - 1) * stride + int(c.lens[m - 1]) == e - 1
            assert np.all(c.lens[:L.E31 // stride - 64] == 0)
            if frames is None:
                assert (c.lens[nz] > 1600).sum() >= 16 and (c.lens[nz] <= 1600).sum() >= 180


@pytest.mark.parametrize("P", POINTERS)
def test_chains(P):
    c = L.chain_case(P)
    L.check_windows(c.windows)
    a4 = c.a4
    assert (P + a4) % L.E32 == 0
    assert c.far_high - c.far_low > L.E32
    flat = [(o, l) for chn in c.chains for o, l in chn]
    assert 24 <= len(c.chains) <= 96
    room = min(a4, L.HALF)
    across = {a4 - o for o, l in flat if o < a4 < o + l}
    for ln in (100, 1460, 9000, L.FILL):
        for d in L.DISTANCES:
            dd = _dist(d, ln)
            if dd <= room:
                assert dd in across
    assert {1, 15, 16, 17} <= across
    assert any(o + l == a4 for o, l in flat) and any(o == a4 for o, l in flat)
    assert any(o + l <= a4 for o, l in flat) and any(o > a4 for o, l in flat)
    assert {(P + o) % 16 for o, l in flat if o < a4 < o + l or o == a4} == set(range(16))
    # back to back across A4, and chunks more than 2^32 apart in both orders
    b2b = [c.chains[i] for i in c.groups["back_to_back"]]
    assert all(chn[k][0] + chn[k][1] == chn[k + 1][0] for chn in b2b for k in range(len(chn) - 1))
    assert any(chn[0][0] < a4 < chn[-1][0] + chn[-1][1] for chn in b2b)
    far = [c.chains[i] for i in c.groups["far"]]
    assert any(chn[1][0] - chn[0][0] > L.E32 for chn in far)
    assert any(chn[0][0] - chn[1][0] > L.E32 for chn in far)
    assert any(chn[0][0] == a4 and chn[1][0] < a4 for chn in far) or a4 < c.far_low
    assert any(chn[0][0] == a4 for chn in far)
    addr, ln, idx = L.chain_table(c)
    assert addr.size == ln.size == int(idx[-1]) and np.all(ln <= L.FILL)


@pytest.mark.parametrize("P", POINTERS)
def test_chain_fill_fields(oracle, P):
    c = L.chain_fill_case(P)
    L.check_windows(c.windows)
    lo, hi = max(c.a4 - L.FIELD_ZONE, 0), c.a4 + L.FIELD_ZONE
    assert len(c.chains) >= 12
    for chn in c.chains:
        assert all(o + l <= lo or o >= hi for o, l in chn)
    w = c.windows[0]
    assert not w.data[lo - w.start:hi - w.start].any()
    offs = [o for o in c.field_off if o is not None]
    assert all(lo <= o and o + 2 <= hi for o in offs) and c.field_off[-1] is None
    assert c.a4 - 1 in offs                                   # a field across A4
    assert any(o + 2 <= c.a4 for o in offs) and any(o >= c.a4 for o in offs)
    assert {o % 2 for o in offs} == {0, 1}
    got = sorted(offs)
    assert all(b - a >= 2 for a, b in zip(got, got[1:]))
    assert L.chain_expected(oracle, c).size == len(c.chains)


@pytest.mark.parametrize("P", POINTERS)
def test_tx_builders_round_a4(oracle, P):
    room = min(L.a4_of(P) - P, L.HALF)
    t = L.tcpseg_abs_case(oracle, P)
    g = L.ipfrag_abs_case(oracle, P)
    h = L.hsplit_abs_case(oracle, P, A.SplitFrames)
    for c, pieces in ((t, [x["pieces"] for x in t.batch.cases]),
                      (g, [x["pieces"] for x in g.batch.cases]),
                      (h, [[p for p in seg] + [(0, 0)] * (2 - len(seg)) for seg in h.sp.chunks])):
        L.check_windows(c.windows)
        assert c.base_addr == P + c.windows[0].start
        w = c.windows[0]
        assert all(o + l <= w.data.size for pp in pieces for o, l in pp)
        dist, ends, starts = L.pieces_cover(c, pieces)
        assert starts and {d for d in (1, 15, 16, 17) if d <= room} <= dist
        if room >= 5000:
            assert ends
    assert np.all(t.e.status == L.S.ACCEPT) and t.e.status.size >= 20
    assert np.all(g.e.status == L.I.ACCEPT) and g.e.status.size >= 20
    assert np.all(h.want_st == L.H.ACCEPT) and h.ok.all()


# ---- the header ring of the Tx builders ------------------------------------------------------------

def _check_ring(c):
    n = c.n
    assert 65536 + 256 < n <= 65536 + 1024                      # just over 65536 slots
    assert 15 + n * L.RING_STRIDE <= L.ARENA_BYTES
    for e in L.EDGES:
        m = e // L.RING_STRIDE
        assert m * L.RING_STRIDE == e                            # a slot starts at the edge
        assert set(range(m - 256, m + 257)) <= set(c.near.tolist())
    assert c.near.max() < n and c.near.size * 64 < L.MAX_WINDOW


def test_header_ring_hsplit(oracle):
    c = L.hsplit_ring_case(oracle, A.SplitFrames)
    _check_ring(c)
    assert np.all(c.want_near == L.H.ACCEPT) and (c.want_h != c.in_h).any(axis=1).all()
    rest = np.ones(c.n, dtype=bool)
    rest[c.near] = False
    assert len(set(c.want_st[rest].tolist())) == 1 and c.want_st[rest][0] != L.H.ACCEPT
    assert int(c.chunk_index[-1]) == c.near.size == c.chunk_len.size


def test_header_ring_tcpseg(oracle):
    c = L.tcpseg_ring_case(oracle)
    _check_ring(c)
    assert c.n == L.RING_SLOTS and len(c.batch.cases) <= 8      # a handful of bursts
    assert 32768 in c.si.tolist()                               # a burst starts in the slot at 2^31
    assert any(int(a) < 65536 < int(b) - 1 for a, b in zip(c.si, c.si[1:]))
    assert set(c.near.tolist()) <= set(c.rows.tolist()) and c.rows.size < 2200
    two = np.diff(c.chunk_index.astype(np.int64)) == 2
    assert 2 <= two.sum() <= len(c.batch.cases)                 # segments across the piece boundary
    assert c.headers[:, :54].any(axis=1).all() and not c.headers[:, 54:].any()


def test_header_ring_ipfrag(oracle):
    c = L.ipfrag_ring_case(oracle)
    _check_ring(c)
    assert all(x["mtu"] == 256 for x in c.batch.cases)
    assert set(c.near.tolist()) <= set(c.rows.tolist()) and c.rows.size < 2200
    assert (c.hdr_len == 42).sum() == len(c.batch.cases) and (c.hdr_len == 34).sum() == c.n - len(c.batch.cases)
    near_first = np.isin(np.nonzero(c.hdr_len == 42)[0], c.near)
    assert near_first.sum() >= 2                                # first fragments near the edges too
