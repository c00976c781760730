"""TCP burst segmentation (aipstack_tcp_tx_segment) on the GPU against the model of
tcpseg_cases.py (the reference's send loop restated in Python, checksums by the CPU oracle).

Every test compares, byte for byte: the statuses, every header slot with its slack, chunk_addr,
chunk_len, chunk_index, the unmodified payload, and guard bytes round every output."""
import numpy as np
import pytest

import aipstack_amd as A

import tcpseg_cases as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256          # bytes before and after every output (keeps 64-byte alignment)
GUARD_BYTE, RING_BYTE, TABLE_BYTE = 0xA7, 0xEE, 0x5C


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)   # whatever ran before this module
    yield


_BATCHES = {
    "sizes": lambda o: T.sizes_batch(),
    "ones65": lambda o: T.one_segment_bursts(65),
    "ones257": lambda o: T.one_segment_bursts(257),
    "zeros": lambda o: T.zero_segment_batch(),
    "boundary": lambda o: T.boundary_batch(),
    "psh": lambda o: T.psh_batch(),
    "zero_tcp": T.zero_tcp_checksum_batch,
    "zero_ip": T.zero_ip_checksum_batch,
    "invalid": lambda o: T.invalid_batch(),
    "mismatch": lambda o: T.mismatch_batch(),
}
_cache = {}


def _case(oracle, name):
    """(batch, caller's seg_index, chunk_base, expectation): computed once, shared, unchanged."""
    if name not in _cache:
        batch = _BATCHES[name](oracle)
        si, cb = T.caller_index(batch.cases)
        e = T.expected(oracle, batch, si, cb)
        for a in (batch.payload, si, cb, e.headers, e.status, e.chunk_off, e.chunk_len, e.chunk_index):
            a.setflags(write=False)
        _cache[name] = (batch, si, cb, e)
    return _cache[name]


class Guarded:
    """`nbytes` bytes of device memory preset to `fill`, with guard bytes on both sides;
    `shift` moves the start off its 64-byte boundary."""

    def __init__(self, nbytes, fill, shift=0):
        self.lo, self.hi = GUARD + shift, GUARD + shift + nbytes
        self.buf = torch.full((self.hi + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.view = self.buf[self.lo:self.hi]
        self.view.fill_(fill)

    def intact(self):
        h = self.buf.cpu().numpy()
        return (h[:self.lo] == GUARD_BYTE).all() and (h[self.hi:] == GUARD_BYTE).all()


class Outputs:
    def __init__(self, n, nc, stride, shift=0):
        self.ring = Guarded(n * stride, RING_BYTE, shift)
        self.addr = Guarded(nc * 8, TABLE_BYTE)
        self.len = Guarded(nc * 4, TABLE_BYTE)
        self.index = Guarded((n + 1) * 8, TABLE_BYTE)
        self.status = Guarded(n, TABLE_BYTE)
        self.seg = A.TcpSegments(self.ring.view, stride, self.addr.view.view(torch.int64),
                                 self.len.view.view(torch.int32), self.index.view.view(torch.int64),
                                 self.status.view)

    def reset(self):
        self.ring.view.fill_(RING_BYTE)
        for g in (self.addr, self.len, self.index, self.status):
            g.view.fill_(TABLE_BYTE)


def _compare(e, out, stride, dpay, payload):
    n, base = len(e.status), dpay.data_ptr()
    st = out.seg.status.cpu().numpy()
    bad = np.nonzero(st != e.status)[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], e.status[bad[:8]])
    want = np.full((n, stride), RING_BYTE, dtype=np.uint8)
    ok = e.status == T.ACCEPT
    want[ok, :T.HDR] = e.headers[ok]
    want[ok, T.HDR:min(stride, 64)] = 0
    got = out.seg.headers.cpu().numpy().reshape(n, stride)
    rows = np.nonzero((got != want).any(axis=1))[0]
    assert rows.size == 0, (rows[:8], got[rows[0]].tobytes().hex(), want[rows[0]].tobytes().hex())
    want_addr = np.where(e.chunk_off >= 0, base + e.chunk_off, 0).astype(np.uint64)
    assert np.array_equal(out.seg.chunk_addr.cpu().numpy().view(np.uint64), want_addr)
    assert np.array_equal(out.seg.chunk_len.cpu().numpy().view(np.uint32), e.chunk_len)
    assert np.array_equal(out.seg.chunk_index.cpu().numpy().view(np.uint64), e.chunk_index)
    assert np.array_equal(dpay.cpu().numpy(), payload)
    for g in (out.ring, out.addr, out.len, out.index, out.status):
        assert g.intact()


def _run(oracle, name, stride=64, shift=0, **kw):
    batch, si, cb, e = _case(oracle, name)
    dpay = torch.from_numpy(batch.payload.copy()).to(DEV)
    desc = T.descriptors(batch, dpay.data_ptr(), A.TCP_BURST_DTYPE)
    out = Outputs(int(si[-1]), int(cb[-1]), stride, shift)
    res = A.tcp_tx_segment(desc, si, cb, out=out.seg, **kw)
    assert res is out.seg
    _compare(e, out, stride, dpay, batch.payload)
    return batch, si, cb, e, desc, dpay, out


# ---- 1. shapes ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["sizes", "ones65", "ones257", "zeros", "boundary", "psh"])
def test_shapes(oracle, name):
    batch, si, cb, e, desc, _, _ = _run(oracle, name)
    assert (e.status == T.ACCEPT).all()
    # the host layout agrees with the index the model made
    li, lb = A.tcp_burst_layout(desc)
    assert np.array_equal(li, si) and np.array_equal(lb, cb)
    d = np.diff(si.astype(np.int64))
    if name == "sizes":
        assert 200 in d and T.count_flags(e)["fin_psh"] == 3
        assert any(len(ch) == 0 for ch in e.seg_chunks)              # FIN only
        assert {1, 2, 3} <= {int(x) for x in d[:3]} and batch.cases[0]["mss"] == 1
    if name.startswith("ones"):
        assert (d == 1).all() and d.size in (65, 257)
    if name == "zeros":
        assert d[0] == 0 and d[-1] == 0 and (d == 0).sum() >= 70 and d.max() == 64
    if name == "boundary":
        assert T.count_straddle_odd_first(e) >= 1
        assert any(len(ch) == 2 and not ch[0][1] & 1 for ch in e.seg_chunks)
        assert any(c["pieces"][0][1] == 0 for c in batch.cases)
        assert any(c["pieces"][1][1] == 0 for c in batch.cases)
        assert any(c["pieces"][0][0] & 1 for c in batch.cases)
        assert any(c["pieces"][1][0] & 1 for c in batch.cases)
    if name == "psh":
        f = T.count_flags(e)
        assert f["psh_only"] >= 3 and f["fin_psh"] >= 3 and f["neither"] >= 3


def test_tcp_checksum_of_zero_stays_zero(oracle):
    _, _, _, e, _, _, out = _run(oracle, "zero_tcp")
    tcp = e.headers[:, 50].astype(int) << 8 | e.headers[:, 51]
    assert (tcp == 0).sum() == 3                                     # the model has them
    got = out.seg.headers.cpu().numpy().reshape(len(e.status), 64)
    assert ((got[:, 50].astype(int) << 8 | got[:, 51]) == 0).sum() == 3


def test_ip_checksum_of_zero(oracle):
    _, _, _, e, _, _, _ = _run(oracle, "zero_ip")
    ip = e.headers[:, 24].astype(int) << 8 | e.headers[:, 25]
    assert (ip == 0).sum() == 3 and (ip == 0xFFFF).sum() == 0


# ---- 2. ring strides and alignments -------------------------------------------------------

@pytest.mark.parametrize("stride,shift", [(54, 0), (64, 0), (72, 0), (128, 0), (64, 4), (64, 1),
                                          (54, 1), (128, 32)])
def test_strides_and_ring_alignment(oracle, stride, shift):
    _, _, _, _, _, _, out = _run(oracle, "sizes", stride=stride, shift=shift)
    assert out.seg.headers.data_ptr() % 64 == shift % 64
    _run(oracle, "boundary", stride=stride, shift=shift)


# ---- 3. bursts that break the contract ------------------------------------------------------

def test_invalid_bursts_between_valid_ones(oracle):
    _, _, _, e, _, _, _ = _run(oracle, "invalid")
    assert (e.status == T.BURST_INVALID).sum() == 2 * len(T.INVALID_CLASSES)
    assert (e.status == T.ACCEPT).sum() >= 2 * len(T.INVALID_CLASSES)
    assert (e.chunk_off < 0).sum() == 3 * len(T.INVALID_CLASSES)
    for stride, shift in ((72, 3), (54, 0)):
        _run(oracle, "invalid", stride=stride, shift=shift)


def test_counts_that_disagree_with_the_descriptor(oracle):
    """Too few / too many segments or chunks for the descriptor, chunks without a segment:
    status 10, nothing outside the arrays (the guards), neighbours exact."""
    _, _, _, e, _, _, _ = _run(oracle, "mismatch")
    assert (e.status == T.BURST_INVALID).sum() == 13 and (e.status == T.ACCEPT).sum() == 24
    _run(oracle, "mismatch", stride=128, shift=8)


# ---- 4. closing the loop with the header-split fill and Rx verify -------------------------

@pytest.mark.parametrize("name", ["sizes", "boundary", "zero_tcp"])
def test_fixed_point_of_header_split_fill_and_rx_verify(oracle, name):
    batch, si, cb, e, _, dpay, out = _run(oracle, name)
    n = len(e.status)
    seg = out.seg
    before = seg.headers.cpu().numpy().copy()
    st = A.tx_fill_header_split(seg.headers, seg.hdr_stride, seg.hdr_lens, seg.chunk_addr,
                                seg.chunk_len, seg.chunk_index)
    assert (st.cpu().numpy() == T.ACCEPT).all()
    assert np.array_equal(seg.headers.cpu().numpy(), before)
    # the chunk table is what the chained batch takes: NOT(sum) of data alone, against the oracle
    sums = A.chksum_batch_chain(seg.chunk_addr, seg.chunk_len, seg.chunk_index).cpu().numpy()
    for i in (0, n // 2, n - 1):
        assert sums[i] == oracle.chain(0, batch.payload, e.seg_chunks[i]) ^ 0xFFFF
    # linearised from what the GPU left: every frame verifies
    got = before.reshape(n, 64)
    addr = seg.chunk_addr.cpu().numpy().view(np.uint64).astype(np.int64) - dpay.data_ptr()
    ln = seg.chunk_len.cpu().numpy().astype(np.int64)
    idx = seg.chunk_index.cpu().numpy().astype(np.int64)
    parts, offs = [], [0]
    for i in range(n):
        parts.append(got[i, :T.HDR])
        parts += [batch.payload[addr[k]:addr[k] + ln[k]] for k in range(idx[i], idx[i + 1])]
        offs.append(offs[-1] + T.HDR + int(ln[idx[i]:idx[i + 1]].sum()))
    frames = torch.from_numpy(np.concatenate(parts)).to(DEV)
    v = A.rx_verify(frames, torch.from_numpy(np.array(offs, dtype=np.int64)).to(DEV))
    assert (v.cpu().numpy() == T.ACCEPT).all()


# ---- 5. repetition, the hint, graph capture ---------------------------------------------

def test_repeated_call_gives_identical_bytes(oracle):
    batch, si, cb, e, desc, dpay, out = _run(oracle, "boundary")
    once = [t.cpu().numpy().copy() for t in (out.seg.headers, out.seg.chunk_addr, out.seg.chunk_len,
                                             out.seg.chunk_index, out.seg.status)]
    A.tcp_tx_segment(desc, si, cb, out=out.seg)
    _compare(e, out, 64, dpay, batch.payload)
    for a, t in zip(once, (out.seg.headers, out.seg.chunk_addr, out.seg.chunk_len,
                           out.seg.chunk_index, out.seg.status)):
        assert np.array_equal(a, t.cpu().numpy())


@pytest.mark.parametrize("name", ["boundary", "invalid"])
def test_just_written_gives_identical_results(oracle, name):
    _run(oracle, name, just_written=True)


def test_fresh_outputs_and_default_ring(oracle):
    """Without `out`: the wrapper allocates a zeroed ring of stride 64 and the tables."""
    batch, si, cb, e = _case(oracle, "sizes")
    dpay = torch.from_numpy(batch.payload.copy()).to(DEV)
    seg = A.tcp_tx_segment(T.descriptors(batch, dpay.data_ptr(), A.TCP_BURST_DTYPE), si, cb)
    n = len(e.status)
    got = seg.headers.cpu().numpy().reshape(n, 64)
    assert np.array_equal(got[:, :T.HDR], e.headers) and (got[:, T.HDR:] == 0).all()
    assert np.array_equal(seg.chunk_index.cpu().numpy().view(np.uint64), e.chunk_index)
    assert (seg.status.cpu().numpy() == T.ACCEPT).all() and seg.n_segments == n


def test_captured_in_a_graph_on_a_side_stream(oracle):
    batch, si, cb, e = _case(oracle, "boundary")
    n, nc = int(si[-1]), int(cb[-1])
    dpay = torch.from_numpy(batch.payload.copy()).to(DEV)
    desc = T.descriptors(batch, dpay.data_ptr(), A.TCP_BURST_DTYPE)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    d_si = torch.from_numpy(si.view(np.int64).copy()).to(DEV)
    d_cb = torch.from_numpy(cb.view(np.int64).copy()).to(DEV)
    out = Outputs(n, nc, 64)
    from aipstack_amd import _lib
    ws = torch.empty(int(_lib.load().aipstack_tcp_tx_segment_workspace_bytes(n)),
                     dtype=torch.uint8, device=DEV)
    kw = dict(out=out.seg, workspace=ws, n_segments=n, n_chunks=nc)
    A.tcp_tx_segment(d_desc, d_si, d_cb, **kw)   # warm-up outside the capture (the CU count is cached)
    torch.cuda.synchronize()
    _compare(e, out, 64, dpay, batch.payload)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        A.tcp_tx_segment(d_desc, d_si, d_cb, **kw)
    for _ in range(2):
        out.reset()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _compare(e, out, 64, dpay, batch.payload)


# ---- 6. later iterations of the grid-stride loops ----------------------------------------

def _tune(key, value):
    from aipstack_amd import _lib
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == A.AIPSTACK_CHKSUM_OK


for _n in (257, 1000, 1537):
    _BATCHES[f"multipass{_n}"] = lambda o, n=_n: T.multipass_batch(n)
_BATCHES["burst_loop"] = lambda o: T.burst_loop_batch()


def _wave_kinds(e, first):
    """What the waves from segment `first` on hold: {"one", "two", "more"} bursts, "invalid"."""
    kinds = set()
    for w in range(first, len(e.status), 64):
        nb = len(set(e.seg_case[w:w + 64].tolist()))
        kinds.add("one" if nb == 1 else "two" if nb == 2 else "more")
        if (e.status[w:w + 64] == T.BURST_INVALID).any():
            kinds.add("invalid")
    return kinds


def _all_bytes(out):
    return [t.cpu().numpy().tobytes() for t in (out.seg.headers, out.seg.chunk_addr,
                                                out.seg.chunk_len, out.seg.chunk_index, out.seg.status)]


@pytest.mark.parametrize("stride,shift", [(64, 0), (72, 3)])
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("n", [257, 1000, 1537])
def test_later_iterations_of_plan_and_emit(oracle, n, cap, stride, shift):
    """At most `cap` blocks ("aux_blocks"): the plan pass and both emit forms loop; every segment
    from 256 * cap on is produced by a later iteration alone, on poisoned memory."""
    name = f"multipass{n}"
    _, si, _, e = _case(oracle, name)
    assert int(si[-1]) == n
    if n == 1537:
        assert _wave_kinds(e, 256) == {"one", "two", "more", "invalid"}
        assert T.count_straddle_odd_first(e) >= 1
    _tune("aux_blocks", cap)
    try:
        batch, si, cb, e, desc, dpay, out = _run(oracle, name, stride=stride, shift=shift)
        torch.cuda.synchronize()
    finally:
        _tune("aux_blocks", -1)
    assert (out.seg.headers.data_ptr() % 64 == 0) == (shift == 0)
    capped = _all_bytes(out)
    out.reset()
    A.tcp_tx_segment(desc, si, cb, out=out.seg)
    _compare(e, out, stride, dpay, batch.payload)
    assert _all_bytes(out) == capped


def test_burst_loop_runs_past_the_grid(oracle):
    """One segment, so one block of 256 lanes, and 700 bursts that break the contract while
    owning chunk entries: bursts 256 to 700 are emptied by later iterations of the burst loop."""
    batch, si, cb, e, _, _, out = _run(oracle, "burst_loop")
    assert int(si[-1]) == 1 and len(batch.cases) == 701 and e.status[0] == T.ACCEPT
    first = int(cb[256])
    assert int(cb[-1]) - first == 223 * 2 + 222 * 3 and (e.chunk_off[first:] == -1).all()
    assert not out.seg.chunk_addr.cpu().numpy()[first:].any()
    assert not out.seg.chunk_len.cpu().numpy()[first:].any()
    idx = out.seg.chunk_index.cpu().numpy().view(np.uint64)
    assert (np.diff(idx.astype(np.int64)) >= 0).all() and idx[0] == 0 and idx[1] == cb[-1]
    assert e.chunk_off[0] == 5 and e.chunk_len[0] == 700          # the one valid entry
    _run(oracle, "burst_loop", stride=72, shift=5)


# ---- 7. diagnostics (last: after all of the above) ---------------------------------------

def test_no_contract_violations():
    assert A.contract_violations() == 0
