"""The send entry points on the three families of tx_cut_cases.py: every payload length, cut and
address mod 16 (A), the sum that folds to 0 with its completing bytes across a cut or a 16-byte
boundary (B), and a mixed batch run twice, the second time with every byte inverted that no chunk,
header or documented template field describes (C). test_tx_cut_cases.py shows on the CPU that the
inputs hold the coverage sets they are built for.

tcp_tx_segment and udp_tx_fragment are compared through the comparisons of their own GPU tests
(statuses, every header slot with its slack, hdr_lens, the chunk table, the index, the payload
afterwards, guard bytes round every output); what they leave on the device is then linearised by
tx_linearise and tx_linearise_slotted into a guarded destination preset to the sentinel, compared
byte for byte with linearise_cases' model, and the frames go through rx_verify. tx_fill_header_split,
chksum_batch_chain and chksum_chain_fill write into guarded, poisoned outputs and are compared with
hsplit_cases.expected and with the oracle's seeded sum over each chain's concatenated bytes; the
ring the header-split fill leaves is linearised and Rx-verified in the same way as the producers'.
tx_resolve runs in family C alone, on the header rings the producers left. No existing chain test
is exhaustive over lengths or addresses, so nothing of the chain sweep is left out here.

Every expected value comes from the models and the CPU oracle, none from a GPU call."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import hsplit_cases as H
import ipfrag_cases as U
import linearise_cases as LC
import tcpseg_cases as T
import tx_cut_cases as X
import tx_resolve_cases as RC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_ipfrag as GU       # noqa: E402
import test_gpu_tcpseg as GT       # noqa: E402
import test_gpu_tx_resolve as GR   # noqa: E402

DEV = "cuda"
POISON = X.POISON
Guarded = GT.Guarded


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


def _tune(key, value):
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == A.AIPSTACK_CHKSUM_OK


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _payload(host):
    """The payload buffer on the device, on a 16-byte boundary: offsets mod 16 are addresses mod 16."""
    t = _d(host)
    assert t.data_ptr() % 16 == 0
    return t


# ---- the producers ---------------------------------------------------------------------------------

class Produced:
    """One producer call on a batch: `out` (the guarded outputs of the producer's own GPU test),
    `seg` (its TcpSegments / UdpFragments), the device payload."""

    def __init__(self, b, e, dpay=None):
        self.b, self.e = b, e
        self.dpay = _payload(b.payload) if dpay is None else dpay
        self.dpay.copy_(torch.from_numpy(b.payload))
        M = T if b.kind == "tcp" else U
        index, base = M.caller_index(b.cases)
        n, nc = int(index[-1]), int(base[-1])
        assert n == len(e.status) and n > 0
        if b.kind == "tcp":
            self.out = GT.Outputs(n, nc, X.HDR_STRIDE)
            self.seg = A.tcp_tx_segment(T.descriptors(b, self.dpay.data_ptr(), A.TCP_BURST_DTYPE), index, base,
                                        out=self.out.seg)
            GT._compare(e, self.out, X.HDR_STRIDE, self.dpay, b.payload)
            self.tensors = (self.seg.headers, self.seg.chunk_addr, self.seg.chunk_len, self.seg.chunk_index,
                            self.seg.status)
        else:
            self.out = GU.Outputs(n, nc, len(b.cases), X.HDR_STRIDE)
            self.seg = A.udp_tx_fragment(U.descriptors(b, self.dpay.data_ptr(), A.UDP_DGRAM_DTYPE), index, base,
                                         out=self.out.frags)
            GU._compare(e, self.out, X.HDR_STRIDE, self.dpay, b.payload)
            self.tensors = self.out.tensors()

    def all_bytes(self):
        return [t.cpu().numpy().tobytes() for t in self.tensors]

    def ring(self):
        return self.seg.headers.cpu().numpy().reshape(-1)


def _linearise(oracle, key, make_sc, form, payload, dpay, **call):
    """tx_linearise (form "csr") or tx_linearise_slotted ("slots") on device tensors (`call`: the
    segments object, or the tensors by keyword) into a guarded destination preset to the sentinel:
    every byte, the lengths and the statuses against linearise_cases' model of the scenario
    `make_sc()` (computed once per `key`); the CSR frames through rx_verify, whose verdicts are the
    frame oracle's. Returns (the destination's bytes, the verdicts or None)."""
    sc, (want_dest, want_lens, want_st) = X.cached(("lin", key, form), lambda: (lambda sc: (sc, sc.expected()))(make_sc()))
    n = sc.n
    dest = Guarded(sc.dest_bytes(), LC.SENTINEL)
    lens, status = Guarded(4 * n, POISON), Guarded(n, POISON)
    kw = dict(frame_max=sc.frame_max, lens=lens.view.view(torch.int32), status=status.view, **call)
    if form == "csr":
        off = _d(sc.offsets.view(np.int64))
        A.tx_linearise(dest.view, off, **kw)
    else:
        A.tx_linearise_slotted(dest.view, sc.slot_stride, **kw)
    torch.cuda.synchronize()
    got = dest.view.cpu().numpy()
    assert (want_st == LC.WRITTEN).all()
    assert np.array_equal(status.view.cpu().numpy(), want_st)
    assert np.array_equal(lens.view.cpu().numpy().view(np.int32), want_lens)
    bad = np.flatnonzero(got != want_dest)
    assert bad.size == 0, (form, bad[:8], got[bad[:8]], want_dest[bad[:8]])
    assert dest.intact() and lens.intact() and status.intact()
    assert np.array_equal(dpay.cpu().numpy(), payload)
    v = None
    if form == "csr":
        v = A.rx_verify(dest.view, off).cpu().numpy()
        assert np.array_equal(v, oracle.rx_verify_batch(want_dest, sc.offsets))
    return got.tobytes(), v


def _linearised(oracle, p, form, key):
    """Linearise what the producer left on the device; returns the destination's bytes."""
    b, e = p.b, p.e
    got, v = _linearise(oracle, (b.kind,) + key, lambda: X.scenario(b, e, form), form, b.payload, p.dpay,
                        segments=p.seg)
    if v is not None and b.kind == "tcp":
        assert (v == T.ACCEPT).all()
    elif v is not None:     # a fragment of a datagram that was cut is Rx verify's FRAGMENT, the others ACCEPT
        cut = (np.diff(U.caller_index(b.cases)[0].astype(np.int64)) > 1)[e.frag_case]
        assert np.array_equal(v, np.where(cut, X.FRAGMENT, T.ACCEPT))
    return got


@pytest.mark.parametrize("name", X.PRODUCER_BATCHES["tcp"])
def test_tcp_tx_segment(oracle, name):
    b, e = X.producer(oracle, "tcp", name)
    p = Produced(b, e)
    for form in ("csr", "slots"):
        _linearised(oracle, p, form, (name,))
    if name == "fold":
        got = p.ring().reshape(-1, X.HDR_STRIDE)
        assert not got[:, 50:52].any()                           # a computed 0 stays 0x0000


@pytest.mark.parametrize("name", X.PRODUCER_BATCHES["udp"])
def test_udp_tx_fragment(oracle, name):
    b, e = X.producer(oracle, "udp", name)
    p = Produced(b, e)
    for form in ("csr", "slots"):
        _linearised(oracle, p, form, (name,))
    if name == "fold":
        got = p.ring().reshape(-1, X.HDR_STRIDE)
        assert (got[:, 40:42] == 0xFF).all()                     # a computed 0 goes out as 0xFFFF


# ---- the header-split fill -------------------------------------------------------------------------

def _filled(oracle, key, sp, dpay=None):
    """tx_fill_header_split on a SplitFrames layout, ring and statuses guarded; then the filled
    ring and the layout's chunk table through tx_linearise and tx_linearise_slotted (every hdr_len
    of the split-point sweep, IHL 6, data offset 15, up to three chunks, a stride of 256) and the
    frames through rx_verify: ACCEPT. Returns (statuses, ring, device payload, the two
    destinations' bytes)."""
    want_h, want_st, _, ok = X.cached(("filled", key), lambda: H.expected(oracle, sp))
    assert ok.all()
    n = len(sp.chunks)
    dpay = _payload(sp.payload) if dpay is None else dpay
    dpay.copy_(torch.from_numpy(sp.payload))
    ring, status = Guarded(n * sp.hdr_stride, 0), Guarded(n, POISON)
    ring.view.copy_(torch.from_numpy(sp.headers))
    addr, lens, index = sp.chunk_table(dpay.data_ptr())
    tab = dict(hdr_lens=_d(sp.hdr_lens.view(np.int32)), chunk_addr=_d(addr.view(np.int64)),
               chunk_len=_d(lens.view(np.int32)), chunk_index=_d(index.view(np.int64)))
    st = A.tx_fill_header_split(ring.view, sp.hdr_stride, *tab.values(), out=status.view)
    torch.cuda.synchronize()
    got_st, got_h = st.cpu().numpy(), ring.view.cpu().numpy()
    bad = np.flatnonzero(got_st != want_st)
    assert bad.size == 0, (bad[:8], got_st[bad[:8]], want_st[bad[:8]])
    rows = np.flatnonzero((got_h != want_h).reshape(n, -1).any(axis=1))
    assert rows.size == 0, (rows[:8], [sp.chunks[i] for i in rows[:4]], sp.hdr_lens[rows[:4]])
    assert np.array_equal(dpay.cpu().numpy(), sp.payload) and ring.intact() and status.intact()
    dests = []
    for form in ("csr", "slots"):
        got, v = _linearise(oracle, ("split", key), lambda: X.split_scenario(sp, want_h, want_st, form), form,
                            sp.payload, dpay, headers=ring.view, hdr_stride=sp.hdr_stride, seg_status=status.view,
                            **tab)
        assert v is None or (v == H.ACCEPT).all()
        dests.append(got)
    assert np.array_equal(ring.view.cpu().numpy(), want_h) and ring.intact()
    return got_st, got_h, dpay, dests


@pytest.mark.parametrize("name", [n for n in X.SPLIT_BATCHES if n != "mixed"])
def test_tx_fill_header_split(oracle, name):
    _filled(oracle, name, X.split(name).sp)


# ---- the chained batch and the chain fill --------------------------------------------------------

def _chained(oracle, c, payload, dpay=None):
    """chksum_batch_chain (final and inverted) and chksum_chain_fill (0 as 0x0000 and as 0xFFFF) on
    the chains over `payload`; every output guarded. Returns all output bytes."""
    n = len(c.chains)
    dpay = _payload(payload) if dpay is None else dpay
    dpay.copy_(torch.from_numpy(payload))
    addr, lens, index = c.table(dpay.data_ptr())
    tab = (_d(addr.view(np.int64)), _d(lens.view(np.int32)), _d(index.view(np.int64)), _d(c.states.view(np.int32)))
    want = c.expected(oracle, payload)
    outs = []
    for final in (True, False):
        o = Guarded(2 * n, POISON)
        A.chksum_batch_chain(*tab, out=o.view.view(torch.int16), final=final)
        got = o.view.cpu().numpy().view(np.uint16)
        bad = np.flatnonzero(got != (want if final else want ^ 0xFFFF))
        assert bad.size == 0, (final, bad[:8], got[bad[:8]], want[bad[:8]], [c.chains[i] for i in bad[:4]])
        assert o.intact()
        outs.append(got.tobytes())
    off = X.field_offsets(n)
    for ffff in (False, True):
        fields, o = Guarded(3 * n + 2, POISON), Guarded(2 * n, POISON)
        fa = np.where(off >= 0, fields.view.data_ptr() + off, 0).astype(np.int64)
        A.chksum_chain_fill(*tab, _d(fa), out=o.view.view(torch.int16), zero_as_ffff=ffff)
        torch.cuda.synchronize()
        want_buf, want_v = X.filled_fields(n, want, ffff)
        assert np.array_equal(o.view.cpu().numpy().view(np.uint16), want_v)
        assert np.array_equal(fields.view.cpu().numpy(), want_buf) and fields.intact() and o.intact()
        outs += [o.view.cpu().numpy().tobytes(), fields.view.cpu().numpy().tobytes()]
    assert np.array_equal(dpay.cpu().numpy(), payload)
    return outs, dpay


def test_chained_batch_and_chain_fill(oracle):
    c = X.cached("chainA", lambda: X.chain_batch(oracle, X.chain_specs(), 60))
    _chained(oracle, c, c.payload)


# ---- family C: nothing outside the described bytes is read -------------------------------------------

class _FirstBlock:
    """The calls inside run on the first block alone: "aux_blocks" = 1 caps every
    one-element-per-lane pass (the producers' plan and emit, the header-split fill's passes,
    linearise, resolve) at one block, and "chunks_per_wave" = 4096 gives the chain kernel, whose
    grid comes from the batch's shape and not from aux_blocks, one wave that walks every group of
    chains itself (the chain pass inside the producers and inside the header-split fill too). The
    chain fill's field pass has one lane per chain and no loop to shorten."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            _tune("aux_blocks", 1)
            _tune("chunks_per_wave", 4096)

    def __exit__(self, *exc):
        if self.on:
            try:
                torch.cuda.synchronize()
            finally:
                _tune("aux_blocks", -1)
                _tune("chunks_per_wave", 0)


def _resolved(ring, lens, status):
    """tx_resolve on a header ring of HDR_STRIDE slots, over test_gpu_tx_resolve's guarded buffers,
    against the model on that same ring. Returns every output's bytes and the ring afterwards."""
    n, table = len(lens), RC.lan_table()
    b = GR.Buffers(n, X.HDR_STRIDE, len(table))
    b.ring.copy_(torch.from_numpy(ring))
    got = A.tx_resolve(b.ring, X.HDR_STRIDE, _d(lens.view(np.int32)), RC.iface_table(RC.LAN), table,
                       seg_status=_d(status), workspace=b.workspace, **b.out)
    e = RC.expected(ring, X.HDR_STRIDE, lens, RC.LAN, table, seg_status=status)
    GR._compare(e, got, b, n)
    return [b.out[k].cpu().numpy().tobytes() for k in sorted(b.out)], b.ring.cpu().numpy()


@pytest.mark.parametrize("first_block", [False, True], ids=["grid", "first_block"])
@pytest.mark.parametrize("kind", ["tcp", "udp"])
def test_producers_read_nothing_outside(oracle, kind, first_block):
    b, e = X.producer(oracle, kind, "mixed")
    other = X.alt_templates(b)
    e2 = X.cached((kind, "mixed-alt"), lambda: X.expect(oracle, other))
    lens = X.hdr_lens_of(b, e)
    with _FirstBlock(first_block):
        one = Produced(b, e)
        first = one.all_bytes() + [_linearised(oracle, one, f, ("mixed",)) for f in ("csr", "slots")]
        ring1 = one.ring()
        res1, after1 = _resolved(ring1, lens, e.status)
        two = Produced(other, e2, dpay=one.dpay)               # the same addresses, the other bytes
        assert two.all_bytes() == first[:-2]
        ring2 = X.alt_slack(two.ring(), X.HDR_STRIDE, lens)    # the slots' bytes from hdr_len on
        two.seg.headers.view(-1).copy_(torch.from_numpy(ring2))
        assert [_linearised(oracle, two, f, ("mixed-alt",)) for f in ("csr", "slots")] == first[-2:]
        res2, after2 = _resolved(ring2, lens, e.status)
    assert res1 == res2
    # the slack stays as each run had it; every other byte of the ring is the same
    inside = (np.arange(X.HDR_STRIDE)[None, :] < lens[:, None]).reshape(-1)
    assert np.array_equal(after1[inside], after2[inside])
    assert np.array_equal(after1[~inside], ring1[~inside]) and np.array_equal(after2[~inside], ring2[~inside])


@pytest.mark.parametrize("first_block", [False, True], ids=["grid", "first_block"])
def test_header_split_fill_reads_nothing_outside(oracle, first_block):
    s = X.split("mixed")
    other = s.alt()
    with _FirstBlock(first_block):
        st1, h1, dpay, lin1 = _filled(oracle, "mixed", s.sp)
        st2, h2, _, lin2 = _filled(oracle, "mixed-alt", other, dpay=dpay)
    assert np.array_equal(st1, st2) and lin1 == lin2
    inside = (np.arange(X.SPLIT_STRIDE)[None, :] < s.sp.hdr_lens[:, None]).reshape(-1)
    assert np.array_equal(h1[inside], h2[inside])
    assert np.array_equal(h1[~inside], s.sp.headers[~inside]) and np.array_equal(h2[~inside], other.headers[~inside])


@pytest.mark.parametrize("first_block", [False, True], ids=["grid", "first_block"])
def test_chains_read_nothing_outside(oracle, first_block):
    c = X.cached("chainC", lambda: X.chain_mixed(oracle))
    with _FirstBlock(first_block):
        one, dpay = _chained(oracle, c, c.payload)
        two, _ = _chained(oracle, c, X.alt(c.payload, c.described), dpay=dpay)
    assert one == two
