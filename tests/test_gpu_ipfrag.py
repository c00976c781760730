"""UDP send with IPv4 fragmentation (aipstack_udp_tx_fragment) on the GPU against the model of
ipfrag_cases.py (the reference's sendUdpIp4Packet / sendIp4Dgram / send_fragmented restated in
Python, checksums by the CPU oracle).

Every test compares, byte for byte: both statuses, every header slot with its slack, hdr_lens,
chunk_addr, chunk_len, chunk_index, the unmodified payload, and guard bytes round every output."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import ipfrag_cases as T

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
    "boundary": lambda o: T.boundary_batch(),
    "spanning": lambda o: T.spanning_batch(),
    "zero_udp": T.zero_udp_checksum_batch,
    "invalid": lambda o: T.invalid_batch(),
    "mismatch": lambda o: T.mismatch_batch(),
}
for _n in (257, 1000, 1537):
    _BATCHES[f"multipass{_n}"] = lambda o, n=_n: T.multipass_batch(n)
_cache = {}


def _case(oracle, name):
    """(batch, caller's frag_index, chunk_base, expectation): computed once, shared, unchanged."""
    if name not in _cache:
        batch = _BATCHES[name](oracle)
        fi, cb = T.caller_index(batch.cases)
        e = T.expected(oracle, batch, fi, cb)
        for a in (batch.payload, fi, cb, e.headers, e.hdr_len, e.status, e.dgram_status, e.chunk_off,
                  e.chunk_len, e.chunk_index):
            a.setflags(write=False)
        _cache[name] = (batch, fi, cb, e)
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
    def __init__(self, n, nc, nd, stride, shift=0):
        self.ring = Guarded(n * stride, RING_BYTE, shift)
        self.hdr_len = Guarded(n * 4, TABLE_BYTE)
        self.addr = Guarded(nc * 8, TABLE_BYTE)
        self.len = Guarded(nc * 4, TABLE_BYTE)
        self.index = Guarded((n + 1) * 8, TABLE_BYTE)
        self.status = Guarded(n, TABLE_BYTE)
        self.dgram_status = Guarded(nd, TABLE_BYTE)
        self.all = (self.ring, self.hdr_len, self.addr, self.len, self.index, self.status,
                    self.dgram_status)
        self.frags = A.UdpFragments(self.ring.view, stride, self.hdr_len.view.view(torch.int32),
                                    self.addr.view.view(torch.int64), self.len.view.view(torch.int32),
                                    self.index.view.view(torch.int64), self.status.view,
                                    self.dgram_status.view)

    def reset(self):
        self.ring.view.fill_(RING_BYTE)
        for g in self.all[1:]:
            g.view.fill_(TABLE_BYTE)

    def tensors(self):
        f = self.frags
        return (f.headers, f.hdr_lens, f.chunk_addr, f.chunk_len, f.chunk_index, f.status,
                f.dgram_status)

    def all_bytes(self):
        return [t.cpu().numpy().tobytes() for t in self.tensors()]


def _compare(e, out, stride, dpay, payload):
    n, base = len(e.status), dpay.data_ptr()
    f = out.frags
    st = f.status.cpu().numpy()
    bad = np.nonzero(st != e.status)[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], e.status[bad[:8]])
    assert np.array_equal(f.dgram_status.cpu().numpy(), e.dgram_status)
    assert np.array_equal(f.hdr_lens.cpu().numpy().view(np.uint32), e.hdr_len)
    want = np.full((n, stride), RING_BYTE, dtype=np.uint8)
    ok = e.status == T.ACCEPT
    want[ok, :min(stride, 64)] = 0                       # header, then zeros up to min(stride, 64)
    want[ok, :T.HDR0] = e.headers[ok]                    # (the model's rows are 0 past hdr_len)
    got = f.headers.cpu().numpy().reshape(n, stride)
    rows = np.nonzero((got != want).any(axis=1))[0]
    assert rows.size == 0, (rows[:8], got[rows[0]].tobytes().hex(), want[rows[0]].tobytes().hex())
    want_addr = np.where(e.chunk_off >= 0, base + e.chunk_off, 0).astype(np.uint64)
    assert np.array_equal(f.chunk_addr.cpu().numpy().view(np.uint64), want_addr)
    assert np.array_equal(f.chunk_len.cpu().numpy().view(np.uint32), e.chunk_len)
    assert np.array_equal(f.chunk_index.cpu().numpy().view(np.uint64), e.chunk_index)
    assert np.array_equal(dpay.cpu().numpy(), payload)
    for g in out.all:
        assert g.intact()


def _run(oracle, name, stride=64, shift=0, **kw):
    batch, fi, cb, e = _case(oracle, name)
    dpay = torch.from_numpy(batch.payload.copy()).to(DEV)
    desc = T.descriptors(batch, dpay.data_ptr(), A.UDP_DGRAM_DTYPE)
    out = Outputs(int(fi[-1]), int(cb[-1]), len(batch.cases), stride, shift)
    res = A.udp_tx_fragment(desc, fi, cb, out=out.frags, **kw)
    assert res is out.frags
    _compare(e, out, stride, dpay, batch.payload)
    return batch, fi, cb, e, desc, dpay, out


# ---- 1. shapes ----------------------------------------------------------------------------

def test_boundary_batch(oracle):
    batch, fi, cb, e, desc, _, _ = _run(oracle, "boundary")
    assert len(batch.cases) == 300 and int(fi[-1]) < 2000
    assert T.branches(batch, e) >= {"S=0", "S=1", "S>1", "S>64", "straddle", "no_straddle", "edge",
                                    "clamped", "last>F"}
    assert {c["mtu"] for c in batch.cases} == set(T.MTUS)
    D = [c["pieces"][0][1] + c["pieces"][1][1] for c in batch.cases]
    assert 0 in D and 65527 in D and 283 in np.diff(fi.astype(np.int64))
    assert any(c["pieces"][0][0] & 1 and c["pieces"][0][1] & 1 for c in batch.cases)
    assert any(c["pieces"][1][0] & 1 and c["pieces"][1][1] & 1 for c in batch.cases)
    # the host layout agrees with the index the model made
    li, lb, ls = A.udp_dgram_layout(desc)
    assert np.array_equal(li, fi) and np.array_equal(lb, cb) and np.array_equal(ls, e.dgram_status)


def test_one_datagram_over_several_waves(oracle):
    batch, fi, cb, e, _, _, _ = _run(oracle, "spanning")
    d = np.diff(fi.astype(np.int64))
    big = int(np.argmax(d))
    assert d[big] == 87 and int(fi[big]) % 64 != 0 and int(fi[big + 1]) % 64 != 0
    assert int(fi[big + 1]) // 64 - int(fi[big]) // 64 >= 2          # whole waves inside it
    assert d[big - 1] == 0 and d[big + 1] == 0 and d[0] == 0 and d[-1] == 0   # S = 0 between owners
    for w in (int(fi[big]) // 64, int(fi[big + 1]) // 64):           # first and last owners differ
        assert len(set(e.frag_case[64 * w:64 * w + 64].tolist())) >= 2
    _run(oracle, "spanning", stride=80, shift=8)


def test_udp_checksum_of_zero_is_sent_as_ffff(oracle):
    batch, _, _, e, _, _, out = _run(oracle, "zero_udp")
    first = e.hdr_len == T.HDR0
    udp = e.headers[:, 40].astype(int) << 8 | e.headers[:, 41]
    assert (udp[first] == 0xFFFF).sum() == 4 and (udp[first] == 0).sum() == 0   # the model has them
    got = out.frags.headers.cpu().numpy().reshape(len(e.status), 64)
    assert ((got[first, 40].astype(int) << 8 | got[first, 41]) == 0xFFFF).sum() == 4


# ---- 2. ring strides and alignments -------------------------------------------------------

@pytest.mark.parametrize("stride,shift", [(64, 0), (48, 0), (80, 0), (64, 4), (64, 1), (42, 1),
                                          (128, 32)])
def test_strides_and_ring_alignment(oracle, stride, shift):
    """A 64-byte ring on a 64-byte boundary is stored in whole lines, any other stride or base per
    lane; bytes past min(stride, 64) and the slots of invalid fragments stay as they were."""
    _, _, _, _, _, _, out = _run(oracle, "spanning", stride=stride, shift=shift)
    assert out.frags.headers.data_ptr() % 64 == shift % 64
    _run(oracle, "invalid", stride=stride, shift=shift)


# ---- 3. datagrams that break the contract ---------------------------------------------------

def test_invalid_datagrams_between_valid_ones(oracle):
    _, _, _, e, _, _, _ = _run(oracle, "invalid")
    assert (e.status == T.DGRAM_INVALID).sum() == 2 * len(T.INVALID_CLASSES)
    assert (e.dgram_status == T.DGRAM_INVALID).sum() == len(T.INVALID_CLASSES)
    assert (e.status == T.ACCEPT).sum() >= 2 * len(T.INVALID_CLASSES)
    assert (e.chunk_off < 0).sum() == 3 * len(T.INVALID_CLASSES)


def test_counts_that_disagree_with_the_descriptor(oracle):
    """Too few / too many fragments or chunks for the descriptor, chunks without a fragment, a
    fragment for a DF datagram above its MTU: status 13, nothing outside the arrays (the guards),
    neighbours exact."""
    _, _, _, e, _, _, _ = _run(oracle, "mismatch")
    assert (e.status == T.DGRAM_INVALID).sum() == 2 + 5 + 3 + 3 + 0 + 1
    assert (e.dgram_status == T.DGRAM_INVALID).sum() == 6 and (e.status == T.ACCEPT).sum() == 7 * 3
    _run(oracle, "mismatch", stride=128, shift=8)


def test_an_index_that_lies(oracle):
    """Running sums that are shifted, cut short, decreasing, past the totals or huge, on valid
    descriptors: whatever comes out, nothing is written outside the described outputs (the
    guards), every status is one of the two, every index entry lies in [0, n_chunks], every chunk
    entry is empty or lies inside the payload (every entry is written in every call, so none
    keeps its preset), and no contract violation is recorded (no entry the chained batch read was
    out of contract)."""
    batch, fi, cb, e = _case(oracle, "mismatch")
    honest = T.Batch([c for c in batch.cases if "give" not in c], batch.payload)
    fi, cb = T.caller_index(honest.cases)
    n, nc, nd = int(fi[-1]), int(cb[-1]), len(honest.cases)
    dpay = torch.from_numpy(honest.payload.copy()).to(DEV)
    base = dpay.data_ptr()
    desc = T.descriptors(honest, base, A.UDP_DGRAM_DTYPE)
    lies = T.lying_indices(honest)
    assert {name for name, _, _ in lies} >= {"frags_past_the_total", "frags_too_few", "frags_decreasing"}
    for name, lfi, lcb in lies:
        out = Outputs(n, nc, nd, 64)
        A.udp_tx_fragment(desc, lfi, lcb, out=out.frags, n_frags=n, n_chunks=nc)
        torch.cuda.synchronize()
        for g in out.all:
            assert g.intact(), name
        f = out.frags
        assert set(f.status.cpu().numpy().tolist()) <= {T.ACCEPT, T.DGRAM_INVALID}, name
        assert set(f.dgram_status.cpu().numpy().tolist()) <= {T.ACCEPT, T.DGRAM_INVALID}, name
        idx = f.chunk_index.cpu().numpy().view(np.uint64)
        assert idx.max() <= nc and idx[n] == nc, name
        ln = f.chunk_len.cpu().numpy().view(np.uint32).astype(np.int64)
        ad = f.chunk_addr.cpu().numpy().view(np.uint64)
        live = ln > 0
        assert (ad[~live] == 0).all() and ln.max() <= 65535, name
        assert (ad[live] >= base).all() and (ad[live].astype(np.int64) + ln[live] <= base + dpay.numel()).all(), name
        assert set(f.hdr_lens.cpu().numpy().tolist()) <= {0, T.HDRK, T.HDR0}, name
        assert np.array_equal(dpay.cpu().numpy(), honest.payload)
        assert A.contract_violations(clear=True) == 0, name
    # the honest index on the same buffers: exact again
    out = Outputs(n, nc, nd, 64)
    A.udp_tx_fragment(desc, fi, cb, out=out.frags)
    _compare(T.expected(oracle, honest, fi, cb), out, 64, dpay, honest.payload)


# ---- 4. closing the loop with the header-split fill and Rx verify -------------------------

@pytest.mark.parametrize("name", ["boundary", "zero_udp"])
def test_closure_through_header_split_fill_and_rx_verify(oracle, name):
    batch, fi, cb, e, _, dpay, out = _run(oracle, name)
    n = len(e.status)
    f = out.frags
    before = f.headers.cpu().numpy().copy()
    got = before.reshape(n, 64)
    # linearised ON THE DEVICE from what the GPU left (slots and chunk table): every fragment of a
    # fragmented datagram is FRAGMENT (IPv4 header checksum good), every whole datagram ACCEPT
    # (UDP checksum good too)
    hl = f.hdr_lens.cpu().numpy().astype(np.int64)
    addr = f.chunk_addr.cpu().numpy().view(np.uint64).astype(np.int64) - dpay.data_ptr()
    ln = f.chunk_len.cpu().numpy().astype(np.int64)
    idx = f.chunk_index.cpu().numpy().astype(np.int64)
    ring = f.headers
    parts, offs = [], [0]
    for i in range(n):
        parts.append(ring[64 * i:64 * i + int(hl[i])])
        parts += [dpay[int(addr[k]):int(addr[k] + ln[k])] for k in range(idx[i], idx[i + 1])]
        offs.append(offs[-1] + int(hl[i]) + int(ln[idx[i]:idx[i + 1]].sum()))
    frames = torch.cat(parts)
    v = A.rx_verify(frames, torch.from_numpy(np.array(offs, dtype=np.int64)).to(DEV)).cpu().numpy()
    S = np.diff(fi.astype(np.int64))[e.frag_case]
    assert (v[S == 1] == T.ACCEPT).all() and (v[S > 1] == 3).all()
    assert (S == 1).sum() >= 2 and (S > 1).sum() >= 5
    # reassembled by offset, as one frame, each datagram verifies as a whole (UDP checksum good)
    ds = [d for d in range(len(batch.cases)) if e.dgram_status[d] == T.ACCEPT
          and 42 + sum(p[1] for p in batch.cases[d]["pieces"]) <= 65535][:60]
    re = [T.reassemble(e, batch.payload, d, headers=got) for d in ds]
    ro = np.concatenate([[0], np.cumsum([len(r) for r in re])]).astype(np.int64)
    rv = A.rx_verify(torch.from_numpy(np.frombuffer(b"".join(re), dtype=np.uint8).copy()).to(DEV),
                     torch.from_numpy(ro).to(DEV)).cpu().numpy()
    assert len(ds) >= 5 and (rv == T.ACCEPT).all(), rv
    # S = 1 datagrams: the slots are a fixed point of the header-split fill ...
    one = S == 1
    st = A.tx_fill_header_split(f.headers, 64, f.hdr_lens, f.chunk_addr, f.chunk_len, f.chunk_index)
    after = f.headers.cpu().numpy().reshape(n, 64)
    assert (st.cpu().numpy()[one] == T.ACCEPT).all() and np.array_equal(after[one], got[one])
    # ... and equal what it leaves on host-built headers with both fields zeroed
    zeroed = got.copy()
    zeroed[:, 24:26] = 0
    zeroed[one, 40:42] = 0
    dz = torch.from_numpy(zeroed.reshape(-1).copy()).to(DEV)
    A.tx_fill_header_split(dz, 64, f.hdr_lens, f.chunk_addr, f.chunk_len, f.chunk_index)
    assert np.array_equal(dz.cpu().numpy().reshape(n, 64)[one], got[one])


# ---- 5. repetition, the hint, graph capture ---------------------------------------------

@pytest.mark.parametrize("name", ["boundary", "invalid"])
def test_just_written_gives_identical_results(oracle, name):
    _, _, _, _, _, _, a = _run(oracle, name)
    _, _, _, _, _, _, b = _run(oracle, name, just_written=True)
    # (the payloads lie at different addresses: everything but chunk_addr)
    for x, y, t in zip(a.all_bytes(), b.all_bytes(), range(7)):
        assert t == 2 or x == y


def test_fresh_outputs_and_default_ring(oracle):
    """Without `out`: the wrapper allocates a zeroed ring of stride 64 and the tables."""
    batch, fi, cb, e = _case(oracle, "spanning")
    dpay = torch.from_numpy(batch.payload.copy()).to(DEV)
    f = A.udp_tx_fragment(T.descriptors(batch, dpay.data_ptr(), A.UDP_DGRAM_DTYPE), fi, cb)
    n = len(e.status)
    got = f.headers.cpu().numpy().reshape(n, 64)
    assert np.array_equal(got[:, :T.HDR0], e.headers) and (got[:, T.HDR0:] == 0).all()
    assert np.array_equal(f.chunk_index.cpu().numpy().view(np.uint64), e.chunk_index)
    assert (f.status.cpu().numpy() == T.ACCEPT).all() and f.n_frags == n
    assert np.array_equal(f.dgram_status.cpu().numpy(), e.dgram_status)


def test_captured_in_a_graph_on_a_side_stream(oracle):
    batch, fi, cb, e = _case(oracle, "spanning")
    n, nc, nd = int(fi[-1]), int(cb[-1]), len(batch.cases)
    dpay = torch.from_numpy(batch.payload.copy()).to(DEV)
    desc = T.descriptors(batch, dpay.data_ptr(), A.UDP_DGRAM_DTYPE)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    d_fi = torch.from_numpy(fi.view(np.int64).copy()).to(DEV)
    d_cb = torch.from_numpy(cb.view(np.int64).copy()).to(DEV)
    out = Outputs(n, nc, nd, 64)
    ws = torch.empty(int(_lib.load().aipstack_udp_tx_fragment_workspace_bytes(nd, n)),
                     dtype=torch.uint8, device=DEV)
    kw = dict(out=out.frags, workspace=ws, n_frags=n, n_chunks=nc)
    A.udp_tx_fragment(d_desc, d_fi, d_cb, **kw)   # warm-up outside the capture (the CU count is cached)
    torch.cuda.synchronize()
    _compare(e, out, 64, dpay, batch.payload)
    first = out.all_bytes()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        A.udp_tx_fragment(d_desc, d_fi, d_cb, **kw)
    for _ in range(2):
        out.reset()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _compare(e, out, 64, dpay, batch.payload)
        assert out.all_bytes() == first


# ---- 6. later iterations of the grid-stride loops ----------------------------------------

def _tune(key, value):
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == A.AIPSTACK_CHKSUM_OK


@pytest.mark.parametrize("stride,shift", [(64, 0), (80, 3)])
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("n", [257, 1000, 1537])
def test_later_iterations_of_plan_and_emit(oracle, n, cap, stride, shift):
    """At most `cap` blocks ("aux_blocks"): the plan pass's three loops and both emit forms loop;
    every fragment from 256 * cap on is produced by a later iteration alone, on poisoned memory."""
    name = f"multipass{n}"
    batch, fi, cb, e = _case(oracle, name)
    assert int(fi[-1]) == n
    if n == 1537:
        assert len(batch.cases) > 256 * 3                       # the datagram loop runs again too
        assert (e.status[768:] == T.DGRAM_INVALID).any() and (e.status[768:] == T.ACCEPT).any()
        assert (e.chunk_off[768:] < 0).any() and int(cb[-1]) > 768
    _tune("aux_blocks", cap)
    try:
        batch, fi, cb, e, desc, dpay, out = _run(oracle, name, stride=stride, shift=shift)
        torch.cuda.synchronize()
    finally:
        _tune("aux_blocks", -1)
    assert (out.frags.headers.data_ptr() % 64 == 0) == (shift == 0)
    capped = out.all_bytes()
    out.reset()
    A.udp_tx_fragment(desc, fi, cb, out=out.frags)
    _compare(e, out, stride, dpay, batch.payload)
    assert out.all_bytes() == capped


# ---- 7. diagnostics (last: after all of the above) ---------------------------------------

def test_no_contract_violations():
    assert A.contract_violations() == 0
