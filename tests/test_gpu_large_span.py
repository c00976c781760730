"""Where in the address space the bytes lie: every device entry point with packets at offsets of
2^31 and 2^32 from its base, and with pieces on both sides of a device address that is a multiple
of 2^32 -- against the CPU oracle and the Python models, bit for bit.

One zero-filled arena of 5 GiB + 64 KiB; only small windows round the edges hold other bytes
(large_span_cases.py has the layouts, test_large_span_cases.py checks what they cover). A
32-bit-truncated offset lands inside the arena, so a truncation shows as a wrong value. Expected
values come from the windows' bytes, copied back from the device, with window-local offsets, and
for the zero filler from one filler element of that length. Every test leaves the arena zero."""
from contextlib import contextmanager

import numpy as np
import pytest

import aipstack_amd as A

import frame_cases as F
import large_span_cases as L
import tcprx_cases as R
import test_gpu_ipfrag as GF
import test_gpu_tcpseg as GS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def arena():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    a = torch.zeros(L.ARENA_BYTES, dtype=torch.uint8, device=DEV)     # a failure fails the tests
    A.contract_violations(clear=True)
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _arena_left_zero(arena):
    yield
    assert not bool(arena.view(torch.int64).any()), "a test left bytes in the arena"
    assert A.contract_violations(clear=True) == 0


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy()


@contextmanager
def placed(arena, windows):
    """The windows' bytes in the arena; yields their host copies, read back from the device (one
    per window, in order); zeroes them again on the way out."""
    try:
        for w in windows:
            arena[w.start:w.end].copy_(torch.from_numpy(w.data))
        yield [_np(arena[w.start:w.end]) for w in windows]
    finally:
        for w in windows:
            arena[w.start:w.end].zero_()


def _same(got, want, what=""):
    got = np.asarray(got).view(want.dtype) if got.dtype != want.dtype else got
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def _zeros(n):
    return np.zeros(max(n, 1), dtype=np.uint8)


# ---- 1, 2: chksum_batch_strided -------------------------------------------------------------

def _strided(arena, oracle, make):
    for shift in L.SHIFTS:
        c = make(shift)
        with placed(arena, c.windows) as host:
            for final in (False, True):
                filler = oracle.batch_strided(_zeros(c.len), c.len, c.len, 1, final)[0]
                want = np.full(c.n, filler, dtype=np.uint16)
                for run in c.runs:
                    i0, cnt, w = run
                    _, lo = L.strided_local(c, run)
                    want[i0:i0 + cnt] = oracle.batch_strided(host[w], c.stride, c.len, cnt, final,
                                                             base_off=lo)
                for jw in (False, True):
                    got = _np(A.chksum_batch_strided(arena, c.stride, c.len, c.n, final=final,
                                                     byte_offset=shift, just_written=jw))
                    _same(got, want, (shift, final, jw))


@pytest.mark.parametrize("plen", [1500, 9000, 65535])
def test_strided_back_to_back(arena, oracle, plen):
    _strided(arena, oracle, lambda shift: L.strided_dense(plen, plen, shift))


@pytest.mark.parametrize("stride", [2048, 2049])
def test_strided_dense_gaps(arena, oracle, stride):
    _strided(arena, oracle, lambda shift: L.strided_dense(stride, 1500, shift))


@pytest.mark.parametrize("plen", [1500, 65535])
@pytest.mark.parametrize("stride,n", L.SPARSE)
def test_strided_threshold_and_huge_strides(arena, oracle, stride, n, plen):
    _strided(arena, oracle, lambda shift: L.strided_sparse(stride, n, plen, shift))


# ---- 3: chksum_batch_csr, chksum_batch_seeded_csr -----------------------------------------------

def _tune(key, value):
    assert A._lib.load().aipstack_chksum_tune(key.encode(), value) == A.AIPSTACK_CHKSUM_OK


@pytest.fixture
def stream_mode():
    """Sets the stream-mode tunable; the automatic setting comes back afterwards."""
    yield lambda v: _tune("stream", v)
    _tune("stream", 0)


@pytest.mark.parametrize("su", [-1, 0, 4])
@pytest.mark.parametrize("kind", L.CSR_KINDS)
def test_csr_and_seeded_csr(arena, oracle, stream_mode, kind, su):
    stream_mode(su)
    for shift in L.SHIFTS:
        c = L.csr_case(kind, shift)
        base = arena[shift:]
        doff = _d(c.offsets.view(np.int64))
        dst = _d(c.states.view(np.int32))
        out_w = ~c.in_window
        with placed(arena, c.windows) as host:
            want = {f: np.zeros(c.n, dtype=np.uint16) for f in (False, True, "seeded")}
            for ln in np.unique(c.lens[out_w]):             # the zero fillers, one of each length
                sel = out_w & (c.lens == ln)
                z = _zeros(int(ln))
                for f in (False, True):
                    want[f][sel] = oracle.batch_csr(z, [0, ln], f)[0]
                for s in c.fill_states:
                    want["seeded"][sel & (c.states == s)] = oracle.batch_seeded_csr(z, [0, ln], [s])[0]
            for run in c.runs:
                i0, cnt, w = run
                _, loc = L.csr_local(c, run)
                for f in (False, True):
                    want[f][i0:i0 + cnt] = oracle.batch_csr(host[w], loc, f)
                want["seeded"][i0:i0 + cnt] = oracle.batch_seeded_csr(host[w], loc,
                                                                      c.states[i0:i0 + cnt])
            for f in (False, True):
                _same(_np(A.chksum_batch_csr(base, doff, final=f)), want[f], (shift, f))
            _same(_np(A.chksum_batch_seeded_csr(base, doff, dst)), want["seeded"], (shift, "seeded"))


# ---- 4: ring slots --------------------------------------------------------------------------------

@pytest.mark.parametrize("stride,n", L.SLOTTED)
def test_slotted_checksums(arena, oracle, stride, n):
    for shift in L.SHIFTS:
        c = L.slotted_case(stride, n, shift)
        ring = arena[shift:shift + n * stride]
        dlen = _d(c.lens.view(np.int32))
        with placed(arena, c.windows) as host:
            for final in (False, True):
                want = np.full(n, oracle.batch_strided(_zeros(0), 1, 0, 1, final)[0], dtype=np.uint16)
                for i, h in zip(c.slots, host):
                    want[i] = oracle.batch_strided(h, stride, int(c.lens[i]), 1, final)[0]
                for jw in (False, True):
                    got = _np(A.chksum_batch_slotted(ring, stride, dlen, final=final, just_written=jw))
                    _same(got, want, (shift, final, jw))


def _slot_frames(c, host):
    """The slots' frames as the device holds them, packed for the oracle."""
    return [h[:int(c.lens[i])].tobytes() for i, h in zip(c.slots, host)]


def _restore(arena, windows):
    for w in windows:
        arena[w.start:w.end].copy_(torch.from_numpy(w.data))


@pytest.mark.parametrize("stride,n", L.SLOTTED)
def test_slotted_frames(arena, oracle, stride, n):
    pool, jumbo = L.frame_pool(oracle), L.jumbo_frames(oracle)
    empty = _zeros(0)
    v0 = int(oracle.rx_verify_batch(empty, [0, 0])[0])              # an empty slot's verdict
    s0 = int(oracle.tx_fill_batch(empty.copy(), [0, 0])[0])
    for shift in L.SHIFTS:
        c = L.slotted_case(stride, n, shift, frames=pool, jumbo=jumbo)
        ring = arena[shift:shift + n * stride]
        dlen = _d(c.lens.view(np.int32))
        slots = np.array(c.slots)
        with placed(arena, c.windows) as host:
            frames = _slot_frames(c, host)
            buf, off = F.pack(frames)
            o = off.astype(np.int64)
            verdicts = oracle.rx_verify_batch(buf, off)
            assert len(set(verdicts.tolist())) >= 7
            want_v = np.full(n, v0, dtype=np.uint8)
            want_v[slots] = verdicts
            _same(_np(A.rx_verify_slotted(ring, stride, dlen)), want_v, (shift, "verify"))
            # the parse: a small table with hits in the windows
            tbl = L.pcb_table(frames, verdicts, A.TCP_PCB_KEY_DTYPE)
            e = R.expected(frames, verdicts, tbl, A.TCP_RX_SEG_DTYPE)
            assert ((e.pcb != R.NO_PCB).sum() >= 8) and tbl.size >= 8
            res = A.tcp_rx_parse_slotted(ring, stride, dlen, tbl)
            want_v[slots] = e.verdict
            _same(_np(res.verdict), want_v, (shift, "parse verdict"))
            segs, pcb = res.segs_numpy(), res.pcb_numpy()
            rest = np.ones(n, dtype=bool)
            rest[slots] = False
            assert not segs[rest].view(np.uint8).any() and np.all(pcb[rest] == R.NO_PCB)
            assert segs[slots].tobytes() == e.segs.tobytes()
            _same(pcb[slots], e.pcb, (shift, "pcb"))
            # the Tx forms
            filled = buf.copy()
            st = oracle.tx_fill_batch(filled, off)
            want_s = np.full(n, s0, dtype=np.uint8)
            want_s[slots] = st
            rec = _np(A.tx_fill_records_slotted(ring, stride, dlen)).view(np.uint64)
            assert all(np.array_equal(_np(arena[w.start:w.end]), w.data) for w in c.windows)
            mine = buf.copy()
            _same(A.apply_tx_records(mine, off[:-1], rec[slots]), st, (shift, "record status"))
            assert np.array_equal(mine, filled)
            _same(((rec >> np.uint64(48)) & np.uint64(0xFF)).astype(np.uint8), want_s, "records")
            assert not (rec[rest] & np.uint64(0x0000_0300_0000_0000)).any()     # no field to write
            for split in (False, True):
                _same(_np(A.tx_fill_slotted(ring, stride, dlen, split=split)), want_s, (shift, split))
                for k, w in enumerate(c.windows):
                    ln = int(c.lens[c.slots[k]])
                    got = _np(arena[w.start:w.end])
                    assert np.array_equal(got[:ln], filled[o[k]:o[k + 1]]), (shift, split, k)
                    assert np.array_equal(got[ln:], w.data[ln:])
                _restore(arena, c.windows)


# ---- 5: frames at CSR offsets --------------------------------------------------------------------

@pytest.mark.parametrize("kind", L.FRAME_KINDS)
def test_frames_at_csr_offsets(arena, oracle, kind):
    for shift in L.SHIFTS:
        c = L.frames_csr_case(oracle, kind, shift)
        base = arena[shift:]
        doff = _d(c.offsets.view(np.int64))
        out_w = ~c.in_window
        n = c.n
        with placed(arena, c.windows) as host:
            want_v = np.zeros(n, dtype=np.uint8)
            want_s = np.zeros(n, dtype=np.uint8)
            for ln in np.unique(c.lens[out_w]):              # the zero filler frames
                z = _zeros(int(ln))
                want_v[out_w & (c.lens == ln)] = oracle.rx_verify_batch(z, [0, ln])[0]
                want_s[out_w & (c.lens == ln)] = oracle.tx_fill_batch(z.copy(), [0, ln])[0]
                assert not z.any()
            want_pv = want_v.copy()
            want_segs = np.zeros(n, dtype=A.TCP_RX_SEG_DTYPE)
            want_pcb = np.full(n, R.NO_PCB, dtype=np.uint32)
            allf, allv = [], []
            for run in c.runs:
                i0, cnt, w = run
                _, loc = L.csr_local(c, run)
                v = oracle.rx_verify_batch(host[w], loc)
                want_v[i0:i0 + cnt] = v
                o = loc.astype(np.int64)
                allf += [host[w][o[k]:o[k + 1]].tobytes() for k in range(cnt)]
                allv += v.tolist()
            tbl = L.pcb_table(allf, allv, A.TCP_PCB_KEY_DTYPE)
            e = R.expected(allf, allv, tbl, A.TCP_RX_SEG_DTYPE)
            assert (e.pcb != R.NO_PCB).sum() >= 8
            at = 0
            filled = []
            for run in c.runs:
                i0, cnt, w = run
                _, loc = L.csr_local(c, run)
                want_pv[i0:i0 + cnt] = e.verdict[at:at + cnt]
                want_segs[i0:i0 + cnt] = e.segs[at:at + cnt]
                want_pcb[i0:i0 + cnt] = e.pcb[at:at + cnt]
                at += cnt
                f = host[w].copy()
                want_s[i0:i0 + cnt] = oracle.tx_fill_batch(f, loc)
                filled.append(f)
            _same(_np(A.rx_verify(base, doff)), want_v, (shift, "verify"))
            res = A.tcp_rx_parse(base, doff, tbl)
            _same(_np(res.verdict), want_pv, (shift, "parse verdict"))
            assert res.segs_numpy().tobytes() == want_segs.tobytes()
            _same(res.pcb_numpy(), want_pcb, (shift, "pcb"))
            rec = _np(A.tx_fill_records(base, doff)).view(np.uint64)
            _same(((rec >> np.uint64(48)) & np.uint64(0xFF)).astype(np.uint8), want_s, "records")
            assert not (rec[out_w] & np.uint64(0x0000_0300_0000_0000)).any()
            for run, f in zip(c.runs, filled):
                i0, cnt, w = run
                _, loc = L.csr_local(c, run)
                mine = host[w].copy()
                A.apply_tx_records(mine, loc[:-1], rec[i0:i0 + cnt])
                assert np.array_equal(mine, f), (shift, "records", w)
                assert np.array_equal(_np(arena[c.windows[w].start:c.windows[w].end]), host[w])
            for split in (False, True):
                _same(_np(A.tx_fill(base, doff, split=split)), want_s, (shift, split))
                for w, f in zip(c.windows, filled):
                    assert np.array_equal(_np(arena[w.start:w.end]), f), (shift, split)
                _restore(arena, c.windows)


# ---- 6: absolute addresses -----------------------------------------------------------------------

def _chain_table(c):
    addr, ln, idx = L.chain_table(c)
    return _d(addr.view(np.int64)), _d(ln.view(np.int32)), _d(idx.view(np.int64))


def test_chains_round_a_4gib_address(arena, oracle):
    c = L.chain_case(arena.data_ptr())
    addr, ln, idx = _chain_table(c)
    dst = _d(c.states.view(np.int32))
    with placed(arena, c.windows) as host:
        want = L.chain_expected(oracle, c, np.concatenate(host))
        zero = c.states.copy()
        zero[:] = 0
        c0 = L.chain_case(arena.data_ptr())
        c0.states = zero
        want0 = L.chain_expected(oracle, c0, np.concatenate(host))
        for jw in (False, True):
            _same(_np(A.chksum_batch_chain(addr, ln, idx, dst, final=True, just_written=jw)), want, jw)
            _same(_np(A.chksum_batch_chain(addr, ln, idx, dst, final=False, just_written=jw)),
                  ~want, jw)
            _same(_np(A.chksum_batch_chain(addr, ln, idx, None, final=True, just_written=jw)),
                  want0, jw)


@pytest.mark.parametrize("zero_as_ffff", [False, True])
def test_chain_fill_fields_round_a_4gib_address(arena, oracle, zero_as_ffff):
    c = L.chain_fill_case(arena.data_ptr())
    addr, ln, idx = _chain_table(c)
    dst, dfld = _d(c.states.view(np.int32)), _d(c.fields.view(np.int64))
    with placed(arena, c.windows) as host:
        want = L.chain_expected(oracle, c, np.concatenate(host))
        if zero_as_ffff:
            want[want == 0] = 0xFFFF
        w0 = c.windows[0]
        after = w0.data.copy()
        for o, v in zip(c.field_off, want):
            if o is not None:
                after[o - w0.start], after[o - w0.start + 1] = int(v) >> 8, int(v) & 0xFF
        for jw in (False, True):
            got = A.chksum_chain_fill(addr, ln, idx, dst, dfld, zero_as_ffff=zero_as_ffff,
                                      just_written=jw)
            _same(_np(got), want, jw)
            assert np.array_equal(_np(arena[w0.start:w0.end]), after)
            for w in c.windows[1:]:
                assert np.array_equal(_np(arena[w.start:w.end]), w.data)
            _restore(arena, c.windows)


@pytest.mark.parametrize("just_written", [False, True])
def test_tcp_tx_segment_data_round_a_4gib_address(arena, oracle, just_written):
    c = L.tcpseg_abs_case(oracle, arena.data_ptr())
    w = c.windows[0]
    with placed(arena, c.windows):
        dpay = arena[w.start:w.end]
        assert dpay.data_ptr() == c.base_addr
        desc = L.S.descriptors(c.batch, c.base_addr, A.TCP_BURST_DTYPE)
        for stride, shift in ((64, 0), (72, 9)):
            out = GS.Outputs(int(c.si[-1]), int(c.cb[-1]), stride, shift)
            A.tcp_tx_segment(desc, c.si, c.cb, out=out.seg, just_written=just_written)
            GS._compare(c.e, out, stride, dpay, c.batch.payload)


@pytest.mark.parametrize("just_written", [False, True])
def test_udp_tx_fragment_data_round_a_4gib_address(arena, oracle, just_written):
    c = L.ipfrag_abs_case(oracle, arena.data_ptr())
    w = c.windows[0]
    with placed(arena, c.windows):
        dpay = arena[w.start:w.end]
        desc = L.I.descriptors(c.batch, c.base_addr, A.UDP_DGRAM_DTYPE)
        for stride, shift in ((64, 0), (80, 8)):
            out = GF.Outputs(int(c.fi[-1]), int(c.cb[-1]), len(c.batch.cases), stride, shift)
            A.udp_tx_fragment(desc, c.fi, c.cb, out=out.frags, just_written=just_written)
            GF._compare(c.e, out, stride, dpay, c.batch.payload)


@pytest.mark.parametrize("just_written", [False, True])
def test_header_split_payload_round_a_4gib_address(arena, oracle, just_written):
    c = L.hsplit_abs_case(oracle, arena.data_ptr(), A.SplitFrames)
    sp = c.sp
    with placed(arena, c.windows):
        addr, ln, idx = sp.chunk_table(c.base_addr)
        headers = _d(sp.headers)
        st = A.tx_fill_header_split(headers, sp.hdr_stride, _d(sp.hdr_lens.view(np.int32)),
                                    _d(addr.view(np.int64)), _d(ln.view(np.int32)),
                                    _d(idx.view(np.int64)), just_written=just_written)
        _same(_np(st), c.want_st, "status")
        got = _np(headers)
        rows = np.nonzero((got != c.want_h).reshape(len(sp.chunks), -1).any(axis=1))[0]
        assert rows.size == 0, rows[:8]
        w = c.windows[0]
        assert np.array_equal(_np(arena[w.start:w.end]), w.data)        # the payload is only read


# ---- 6, the write side: the header ring of the Tx builders across offsets 2^31 and 2^32 ----------

def _ring(arena, shift, n):
    """(the ring as the entry point takes it, its rows as a 2-D view): n slots of 64 KiB from
    arena offset `shift`; slot 32768 starts 2^31 bytes from the ring's base, slot 65536 2^32."""
    flat = arena[shift:shift + n * L.RING_STRIDE]
    return flat, flat.view(n, L.RING_STRIDE)


def _rows_equal(got, want, rows, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, rows[bad[:8]], got[bad[0]].tobytes().hex(), want[bad[0]].tobytes().hex())


def _table_equal(res, c, base, what):
    _same(_np(res.chunk_index).view(np.uint64), c.chunk_index, (what, "index"))
    _same(_np(res.chunk_len).view(np.uint32), c.chunk_len, (what, "len"))
    _same(_np(res.chunk_addr).view(np.uint64), (base + c.chunk_off).astype(np.uint64), (what, "addr"))


def test_header_split_ring_across_the_edges(arena, oracle):
    c = L.hsplit_ring_case(oracle, A.SplitFrames)
    dpay = _d(c.payload)
    rows = torch.from_numpy(c.near).to(DEV)
    d_in = _d(c.in_h)
    args = (_d(c.hdr_lens.view(np.int32)), _d((dpay.data_ptr() + c.chunk_off).astype(np.int64)),
            _d(c.chunk_len.view(np.int32)), _d(c.chunk_index.view(np.int64)))
    for shift in L.SHIFTS:
        flat, ring = _ring(arena, shift, c.n)
        try:
            ring[rows, :64] = d_in
            for jw in (False, True):
                st = A.tx_fill_header_split(flat, L.RING_STRIDE, *args, just_written=jw)
                _same(_np(st), c.want_st, (shift, jw, "status"))
                _rows_equal(_np(ring[rows, :64]), c.want_h, c.near, (shift, jw))
        finally:
            ring[rows, :64] = 0              # the arena must now be zero: the fillers are untouched
    assert np.array_equal(_np(dpay), c.payload)


_ring_cases = {}


def _ring_case(oracle, name):
    if name not in _ring_cases:
        _ring_cases[name] = (L.tcpseg_ring_case if name == "tcpseg" else L.ipfrag_ring_case)(oracle)
    return _ring_cases[name]


@pytest.mark.parametrize("shift", L.SHIFTS)
def test_tcp_tx_segment_ring_across_the_edges(arena, oracle, shift):
    c = _ring_case(oracle, "tcpseg")
    dpay = _d(c.payload)
    desc = L.S.descriptors(c.batch, dpay.data_ptr(), A.TCP_BURST_DTYPE)
    rows = torch.from_numpy(c.rows).to(DEV)
    flat, ring = _ring(arena, shift, c.n)
    try:
        res = A.tcp_tx_segment(desc, c.si, c.cb, hdr_stride=L.RING_STRIDE, headers=flat,
                               just_written=bool(shift & 1))
        _same(_np(res.status), np.full(c.n, L.S.ACCEPT, dtype=np.uint8), "status")
        _table_equal(res, c, dpay.data_ptr(), shift)
        got = _np(ring[rows, :64])
        _rows_equal(got, c.headers, c.rows, shift)
        # every slot got a header (the first bytes are the template's MAC, never all zero)
        assert bool(ring[:, :14].any(dim=1).all())
        buf, off = F.pack(L.ring_frames(c, got, np.full(c.rows.size, 54)))
        assert np.all(oracle.rx_verify_batch(buf, off) == L.S.ACCEPT)
    finally:
        ring[:, :64].zero_()                 # bytes past 64 must have stayed zero
    assert np.array_equal(_np(dpay), c.payload)


@pytest.mark.parametrize("shift", L.SHIFTS)
def test_udp_tx_fragment_ring_across_the_edges(arena, oracle, shift):
    c = _ring_case(oracle, "ipfrag")
    dpay = _d(c.payload)
    desc = L.I.descriptors(c.batch, dpay.data_ptr(), A.UDP_DGRAM_DTYPE)
    rows = torch.from_numpy(c.rows).to(DEV)
    flat, ring = _ring(arena, shift, c.n)
    try:
        res = A.udp_tx_fragment(desc, c.fi, c.cb, hdr_stride=L.RING_STRIDE, headers=flat,
                                just_written=bool(shift & 1))
        _same(_np(res.status), np.full(c.n, L.I.ACCEPT, dtype=np.uint8), "status")
        _same(_np(res.dgram_status), np.full(len(c.batch.cases), L.I.ACCEPT, dtype=np.uint8), "dgram")
        _same(_np(res.hdr_lens).view(np.uint32), c.hdr_len, "hdr_len")
        _table_equal(res, c, dpay.data_ptr(), shift)
        got = _np(ring[rows, :64])
        _rows_equal(got, c.headers, c.rows, shift)
        assert bool(ring[:, :14].any(dim=1).all())
        # the sampled fragments verify: FRAGMENT (3) where MF or an offset is set
        buf, off = F.pack(L.ring_frames(c, got, c.hdr_len[c.rows]))
        assert np.all(oracle.rx_verify_batch(buf, off) == 3)
    finally:
        ring[:, :64].zero_()
    assert np.array_equal(_np(dpay), c.payload)
