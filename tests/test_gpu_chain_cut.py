"""chksum_batch_chain and chksum_chain_fill on the families of chain_cut_cases.py, in every kernel
form its FORMS name: the chunk table's geometry (T), the gathered stream's (S), chunk lengths and
the short-first rule (L), column runs whole and broken (R), sums at the fold (B), a cropped batch
run twice with every byte outside its chunks inverted (C), and the field pass with its loop's
second iteration (F). test_chain_cut_cases.py shows on the CPU that the inputs hold the coverage
they are built for.

Every call of a test writes into its own slice of one poisoned uint16 buffer with guard bytes on
both sides; the slices start at even and at odd elements in turn with a poisoned element between
them (the final and the inverted form each at both), and the whole buffer is compared: the
final and the inverted form, with the states and with None. Every expected value comes from the CPU oracle, none from a GPU call."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import chain_cut_cases as X

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_tcpseg as GT       # noqa: E402

DEV = "cuda"
POISON = 0xC3
Guarded = GT.Guarded


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


def _tune(key, value):
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == A.AIPSTACK_CHKSUM_OK


@pytest.fixture
def form():
    """Yields a setter for a form's tunables; restores every default afterwards."""
    def apply(name):
        tunables, jw = X.FORMS[name]
        for k, v in tunables.items():
            _tune(k, v)
        return jw
    try:
        yield apply
    finally:
        try:
            torch.cuda.synchronize()
        finally:
            for k, v in X.DEFAULTS.items():
                _tune(k, v)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Device:
    """A case on the device, uploaded once per module: the payload (two allocations where the case
    has a `split`), the chunk table with the addresses of these allocations, the states."""

    def __init__(self, case):
        c = case.chains
        cut = case.split if case.split is not None else c.payload.size
        self.host = c.payload
        self.parts = [(0, cut, _d(c.payload[:cut]))]
        if cut < c.payload.size:
            self.parts.append((cut, c.payload.size, _d(c.payload[cut:])))
        off, ln, idx = c.table(0)
        off = off.astype(np.int64)
        addr = np.zeros(off.size, dtype=np.int64)
        for lo, hi, t in self.parts:
            assert t.data_ptr() % 16 == 0 and lo % 16 == 0     # offsets mod 16 are addresses mod 16
            m = (off >= lo) & (off < hi)
            assert (off[m] + ln[m] <= hi).all()                 # every chunk inside its allocation
            addr[m] = t.data_ptr() + off[m] - lo
        assert (addr[ln > 0] != 0).all() and int(ln.max(initial=0)) <= 65535
        self.addr, self.len = _d(addr), _d(ln.view(np.int32))
        self.idx, self.states = _d(idx.view(np.int64)), _d(c.states.view(np.int32))

    def load(self, payload):
        for lo, hi, t in self.parts:
            t.copy_(torch.from_numpy(payload[lo:hi]))

    def unchanged(self, payload):
        return all(np.array_equal(t.cpu().numpy(), payload[lo:hi]) for lo, hi, t in self.parts)


_dev = {}


def _device(oracle, name):
    if name not in _dev:
        _dev[name] = Device(X.case(name, oracle))
    return _dev[name]


def _wants(oracle, name, payload=None):
    """(the final checksums with the states, with no states) of a case, from the oracle."""
    def make():
        c = X.case(name, oracle).chains
        p = c.payload if payload is None else payload
        zero = X.Chains(c.chains, np.zeros_like(c.states), c.payload, c.described)
        return X._expected(oracle, c, p), X._expected(oracle, zero, p)
    return make() if payload is not None else X.cached(("chain-wants", name), make)


def _run(case, dev, wants, jw, shift=0):
    """Every call of the case, final and inverted, with and without states, each into its slice of
    one guarded output; the whole output against the oracle's, the guards intact."""
    plan, pos = [], 1
    for k, (lo, hi) in enumerate([call for call in case.calls for _ in range(4)]):
        # the start's parity from bit 1 of k and the call's number, final from bit 0: either form
        # lands on an even and on an odd element; cases of several calls also give the
        # states and None either parity
        pos += (pos ^ (k >> 1) ^ (k >> 2)) & 1
        plan.append((lo, hi, pos, bool(k & 1), bool(k & 2)))
        pos += hi - lo + 1
    o = Guarded(2 * pos, POISON, shift)
    out = o.view.view(torch.int16)
    want = np.full(pos, POISON * 0x0101, dtype=np.uint16)
    for lo, hi, at, final, stateless in plan:
        A.chksum_batch_chain(dev.addr, dev.len, dev.idx[lo:hi + 1], None if stateless else dev.states[lo:hi],
                             out=out[at:at + hi - lo], final=final, just_written=jw)
        w = wants[1 if stateless else 0][lo:hi]
        want[at:at + hi - lo] = w if final else w ^ 0xFFFF
    torch.cuda.synchronize()
    got = o.view.cpu().numpy().view(np.uint16)
    bad = np.flatnonzero(got != want)
    if bad.size:
        lo, hi, at, final, stateless = [p for p in plan if p[2] <= bad[0]][-1]
        i = lo + int(bad[0]) - at
        tag = case.tags[i] if case.tags and i < hi else None
        raise AssertionError((bad.size, "first: chain", i, "of call", (lo, hi), "final", final, "stateless", stateless,
                              tag, hex(int(got[bad[0]])), hex(int(want[bad[0]]))))
    assert o.intact()
    return got.tobytes()


def _fill(case, dev, want, jw, ffff, shift=0):
    """chksum_chain_fill on the case's first call: fields at field_offsets in a guarded buffer."""
    lo, hi = case.calls[0]
    n = hi - lo
    off = X.field_offsets(n)
    fields, o = Guarded(3 * n + 2, POISON), Guarded(2 * n, POISON, shift)
    fa = np.where(off >= 0, fields.view.data_ptr() + off, 0).astype(np.int64)
    A.chksum_chain_fill(dev.addr, dev.len, dev.idx[lo:hi + 1], dev.states[lo:hi], _d(fa),
                        out=o.view.view(torch.int16), zero_as_ffff=ffff, just_written=jw)
    torch.cuda.synchronize()
    want_buf, want_v = X.filled_fields(n, want[lo:hi], ffff)
    got = o.view.cpu().numpy().view(np.uint16)
    bad = np.flatnonzero(got != want_v)
    assert bad.size == 0, (bad.size, bad[:4], got[bad[:4]], want_v[bad[:4]])
    assert np.array_equal(fields.view.cpu().numpy(), want_buf) and fields.intact() and o.intact()
    return got, want_v


def _family(oracle, form, name, form_name):
    case, dev = X.case(name, oracle), _device(oracle, name)
    shift = 2 * (list(X.FORMS).index(form_name) & 1)    # the whole output one element further, in turn
    _run(case, dev, _wants(oracle, name), form(form_name), shift)
    assert dev.unchanged(dev.host)


@pytest.mark.parametrize("name", X.FAMILY_FORMS["T"])
def test_table_geometry(oracle, form, name):
    """Family T: every start lane, chunk count round each slice boundary, carried parity and chain
    id, the empty-chain edges, every batch size 1..130."""
    _family(oracle, form, "T", name)


@pytest.mark.parametrize("name", X.FAMILY_FORMS["S"])
def test_stream_geometry(oracle, form, name):
    """Family S: a slice's stream of every length 1..1344 segments, trailing empty chunks on a
    window edge, one chunk owning the stream, chunks starting on and before a window edge."""
    _family(oracle, form, "S", name)


@pytest.mark.parametrize("name", X.FAMILY_FORMS["L"])
def test_lengths_and_short_first(oracle, form, name):
    """Family L: every chunk length 1..144 at every start mod 128, the edge lengths at every start
    mod 16, between neighbours back to back, a line away and far away."""
    _family(oracle, form, "L", name)


@pytest.mark.parametrize("batch", ["R", "R-broken"])
@pytest.mark.parametrize("name", X.FAMILY_FORMS["R"])
def test_column_runs(oracle, form, name, batch):
    """Family R: every count of run chunks and lone headers in three interleavings; the runs
    broken at every position, which must take the gathered stream and stay exact."""
    _family(oracle, form, batch, name)


@pytest.mark.parametrize("name", X.FAMILY_FORMS["B"])
def test_sums_at_the_fold(oracle, form, name):
    """Family B through the chained batch and through the chain fill with both zero_as_ffff."""
    case, dev = X.case("B", oracle), _device(oracle, "B")
    wants = _wants(oracle, "B")
    jw = form(name)
    _run(case, dev, wants, jw)
    crafted = [i for i, p, q in case.fix]
    for ffff in (False, True):
        got, _ = _fill(case, dev, wants[0], jw, ffff, 2 * ffff)
        assert (got[crafted] == (0xFFFF if ffff else 0)).all()
    assert dev.unchanged(dev.host)


@pytest.mark.parametrize("name", X.FAMILY_FORMS["C"])
def test_bytes_outside_the_chunks_change_nothing(oracle, form, name):
    """Family C at the same addresses twice, the second time with every byte outside the chunks
    inverted: identical outputs, the oracle's, and the payload as it was."""
    case, dev = X.case("C"), _device(oracle, "C")
    c = case.chains
    other = X.cached(("chain", "C-alt"), lambda: X.alt(c.payload, c.described))
    wants = _wants(oracle, "C")
    jw = form(name)
    try:
        one = _run(case, dev, wants, jw)
        dev.load(other)
        two = _run(case, dev, wants, jw)
        assert dev.unchanged(other)
    finally:
        dev.load(c.payload)
    assert one == two


@pytest.mark.parametrize("name", ["su4", "su2", "jw", "cpg64", "cpw3"])
def test_field_pass_on_the_table_family(oracle, form, name):
    """Family F, first batch: T's chains with a field each (every address parity, every seventh
    null), 0 as 0x0000 and as 0xFFFF."""
    case, dev = X.case("T"), _device(oracle, "T")
    wants = _wants(oracle, "T")
    jw = form(name)
    for ffff in (False, True):
        _fill(case, dev, wants[0], jw, ffff, 2 * ffff)


def test_field_pass_loops_twice(oracle):
    """Family F, second batch: more chains than the field pass has threads (cus * 64 blocks of
    256), so its grid-stride loop runs a second time; every stored field, every skipped one and
    the guards."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = X.f_big(cus)
    n, idx, off, lens, states, payload = big
    assert n > cus * 64 * 256
    want = X.f_big_expected(oracle, big)
    dpay = _d(payload)
    fields, o = Guarded(3 * n + 2, POISON), Guarded(2 * n, POISON, 2)
    foff = X.field_offsets(n)
    fa = np.where(foff >= 0, fields.view.data_ptr() + foff, 0).astype(np.int64)
    assert off.size == lens.size and (off + lens <= payload.size).all()
    A.chksum_chain_fill(_d(dpay.data_ptr() + off), _d(lens.view(np.int32)), _d(idx.view(np.int64)),
                        _d(states.view(np.int32)), _d(fa), out=o.view.view(torch.int16), zero_as_ffff=True)
    torch.cuda.synchronize()
    want_buf, want_v = X.filled_fields(n, want, True)
    got = o.view.cpu().numpy().view(np.uint16)
    bad = np.flatnonzero(got != want_v)
    assert bad.size == 0, (bad.size, bad[:4], got[bad[:4]], want_v[bad[:4]])
    gotf = fields.view.cpu().numpy()
    bad = np.flatnonzero(gotf != want_buf)
    assert bad.size == 0, (bad.size, "first field", int(bad[0]) // 3, "of", n)
    assert fields.intact() and o.intact()
    assert np.array_equal(dpay.cpu().numpy(), payload)
