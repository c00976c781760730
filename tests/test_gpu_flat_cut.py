"""The four flat checksum batches (strided, CSR, seeded CSR, ring slots) on the three families of
flat_cut_cases.py, in every kernel form its FORMS name: every packet length at every start mod 16
(A), sums that fold to +0 / -0 and saturating data (B), and a mixed batch run twice, the second
time with every byte outside every packet inverted (C). test_flat_cut_cases.py shows on the CPU
that the inputs hold the coverage they are built for.

Every call writes into its own slice of one poisoned uint16 buffer with 64 guard elements on each
side; the slices follow each other, so they start at even and at odd elements (an odd one leaves
the address 2 mod 4: a paired 4-byte store would show) and hold odd and even counts. The whole
buffer is compared with the oracle's, guards and all. Buffers are uploaded once per module and the
expectation is computed once per (layout, family): a result never depends on a form.

Every expected value comes from the CPU oracle, none from a GPU call."""
import ctypes

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import flat_cut_cases as X

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON_I16 = int(np.array([X.POISON16], dtype=np.uint16).view(np.int16)[0])


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
    yield apply
    torch.cuda.synchronize()
    for k, v in X.DEFAULTS.items():
        _tune(k, v)


_dev = {}


def _d(a):
    """The array on the device, uploaded once per module (the arrays of flat_cut_cases are cached
    and never change); on a 16-byte boundary, so offsets mod 16 are addresses mod 16."""
    if id(a) not in _dev:
        host = a.view(np.int32) if a.dtype == np.uint32 else a
        t = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
        assert t.data_ptr() % 16 == 0
        _dev[id(a)] = (a, t)
    return _dev[id(a)][1]


_want = {}


def _expected(oracle, key, plan):
    if key not in _want:
        _want[key] = X.expect(oracle, plan)
    return _want[key]


def _run(plan, jw=False):
    """Every call of the plan, each into its slice of one guarded output; returns it whole."""
    raw = torch.full((plan.out_size,), POISON_I16, dtype=torch.int16, device=DEV)
    for c, pos in zip(plan.calls, plan.out_pos.tolist()):
        out, d = raw[pos:pos + c.n], _d(plan.bufs[c.buf])
        if c.kind == "strided":
            A.chksum_batch_strided(d, c.stride, c.length, c.n, out=out, final=c.final, byte_offset=c.base,
                                   just_written=jw)
        elif c.kind == "csr":
            A.chksum_batch_csr(d, _d(c.offsets), out=out, final=c.final)
        elif c.kind == "seeded":
            A.chksum_batch_seeded_csr(d, _d(c.offsets), _d(c.states), out=out)
        else:
            A.chksum_batch_slotted(d[c.base:c.base + c.n * c.stride], c.stride, _d(c.lens), out=out, final=c.final,
                                   just_written=jw)
    return raw.cpu().numpy().view(np.uint16)


def _compare(plan, got, want, what):
    bad = np.flatnonzero(got != want)
    if bad.size:
        k = int(np.searchsorted(plan.out_pos, bad[0], side="right")) - 1
        c = plan.calls[min(max(k, 0), len(plan.calls) - 1)]
        i = int(bad[0] - plan.out_pos[k]) if 0 <= k < len(plan.calls) else -1
        where = (c.kind, c.buf, "base", c.base, "stride", c.stride, "packet", i,
                 "len", int(c.plen[i]) if 0 <= i < c.n else None, "start", int(c.start[i]) % 16 if 0 <= i < c.n else None)
        raise AssertionError((what, bad.size, "first", where, hex(int(got[bad[0]])), hex(int(want[bad[0]]))))


@pytest.mark.parametrize("name", list(X.FORMS))
@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_every_length_and_start(oracle, form, layout, name):
    """Family A: the default form on every (length, start mod 16) pair, the others on all of
    DENSE and on EDGE at starts 0, 1, 8 and 15."""
    full = name == "default"
    plan = X.plan(layout, "A", full)
    want = _expected(oracle, (layout, "A", full), plan)
    _compare(plan, _run(plan, form(name)), want, (layout, name))


@pytest.mark.parametrize("name", list(X.FORMS))
@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_values(oracle, form, layout, name):
    """Family B: packets whose sum is a non-zero multiple of 0xFFFF beside all-zero twins, and
    the saturating patterns."""
    plan = X.plan(layout, "B", False)
    want = _expected(oracle, (layout, "B"), plan)
    _compare(plan, _run(plan, form(name)), want, (layout, name))


@pytest.mark.parametrize("name", list(X.FORMS))
@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_bytes_outside_the_packets_change_nothing(oracle, form, layout, name):
    """Family C, laid out twice: identical results, the oracle's, and the inputs as they were."""
    plan = X.plan(layout, "C", False)
    other = X.cached((layout, "C-alt"), lambda: X.alt(plan))
    want = _expected(oracle, (layout, "C"), plan)
    assert np.array_equal(want, _expected(oracle, (layout, "C-alt"), other))
    jw = form(name)
    one, two = _run(plan, jw), _run(other, jw)
    _compare(plan, one, want, (layout, name, "plain"))
    _compare(other, two, want, (layout, name, "inverted"))
    for p in (plan, other):
        for b in p.bufs.values():
            assert np.array_equal(_d(b).cpu().numpy(), b)


def _is_large(n):
    """Whether a batch of n packets takes the large-batch shape on this device (pick_shape):
    strided batches then get 2 stream windows, small ones 8."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cp, sw = ctypes.c_uint32(0), ctypes.c_int(0)
    assert _lib.load().aipstack_chksum_launch_shape(n, cus, 0, ctypes.addressof(cp), ctypes.addressof(sw)) == 0
    return cp.value == 64 and sw.value == 2


@pytest.mark.parametrize("layout", ["csr", "seeded", "slotted"])
def test_large_batches_default_dispatch(oracle, layout):
    """chunk_packets 0 on a batch large enough for the default dispatch: short runs of 16-packet
    chunks for CSR, the 16-packet gathered stream for ring slots; the pairs test_flat_cut_cases.py
    shows the plans to hold."""
    plan = X.cached((layout, "large"), lambda: X.large_plan(layout))
    assert all(_is_large(c.n) for c in plan.calls)
    want = _expected(oracle, (layout, "large"), plan)
    _compare(plan, _run(plan), want, layout)


def _large_strided(oracle, gapped, length, bases, jw, odd):
    """The default dispatch of a strided batch of LARGE_N + 67 packets and more, of `length` bytes,
    back to back or at the gap16 stride, once per base. The batch repeats 67 packets of the random
    buffer (built on the device); a packet's sum depends on its bytes alone, so the oracle's 67
    sums repeat likewise, whatever start mod 16 the base and the stride give each packet. The
    guarded output is compared on the device, with the oracle's sums."""
    k, n = 67, X.LARGE_N + 67 + odd
    assert _is_large(n)
    host = X.random_buffer()
    stride = X._gap_stride(length) if gapped else length
    period, src = k * stride, X.GUARD + 32
    if period == 0:                                   # length 0 back to back: every packet at the base
        big, hp = _d(host)[:64], host
    else:
        reps = -(-(16 + n * stride) // period) + 1
        big = torch.empty(16 + reps * period + 256, dtype=torch.uint8, device=DEV)
        pat = _d(host)[src:src + period]
        big[16:16 + reps * period].view(reps, period).copy_(pat)
        big[:16] = pat[-16:]
        big[16 + reps * period:] = 0x5C
        hpat = host[src:src + period]
        hp = np.concatenate([hpat[-16:], hpat, np.resize(hpat, 64)])      # the period, continued both ways
    raw = torch.empty(X.OUT_GUARD + n + X.OUT_GUARD + 1, dtype=torch.int16, device=DEV)
    for b in bases:
        at = X.OUT_GUARD + (b & 1)
        raw.fill_(POISON_I16)
        A.chksum_batch_strided(big, stride, length, n, out=raw[at:at + n], byte_offset=16 + b, just_written=jw)
        sums = oracle.batch_strided(hp, stride, length, k, base_off=16 + b)
        want = torch.from_numpy(sums.view(np.int16)).to(DEV).repeat(-(-n // k))[:n]
        ok = torch.equal(raw[at:at + n], want) and bool((raw[:at] == POISON_I16).all()) and \
            bool((raw[at + n:] == POISON_I16).all())
        if not ok:
            got, w = raw[at:at + n].cpu().numpy().view(np.uint16), np.resize(sums, n)
            bad = np.flatnonzero(got != w)
            raise AssertionError((length, stride, b, jw, bad.size, bad[:8], got[bad[:4]], w[bad[:4]]))
    del big


@pytest.mark.parametrize("jw", [False, True], ids=["plain", "just_written"])
@pytest.mark.parametrize("gapped", [False, True], ids=["b2b", "gap16"])
def test_large_strided_batches_at_every_threshold(oracle, gapped, jw):
    """Both sides of each length threshold of the default dispatch (LARGE_LENGTHS), with and
    without the JUST_WRITTEN hint, at one base each."""
    for j, length in enumerate(X.LARGE_LENGTHS):
        _large_strided(oracle, gapped, length, (j % 16,), jw, j & 1)


_BANDS = [(layout, band) for layout in ("b2b", "gap16") for band, _ in X.large_strided(layout)]


@pytest.mark.parametrize("layout,band", _BANDS, ids=["%s-%s" % lb for lb in _BANDS])
def test_large_strided_batches_every_length_and_start(oracle, layout, band):
    """The "large" form of the strided layouts, one band of lengths per case: all of DENSE at all
    16 starts, EDGE round each threshold at starts 0, 1, 8 and 15 (flat_cut_cases.large_strided)."""
    calls = dict(X.large_strided(layout))[band]
    for j, (length, bases) in enumerate(calls):
        _large_strided(oracle, layout == "gap16", length, bases, False, j & 1)


def test_length_over_the_slot_is_clamped_and_reported(oracle):
    """The one deliberate contract violation: clamped to the slot, reported, and cleared here."""
    buf, base, stride, lens = X.clamp_case()
    assert A.contract_violations(clear=True) == 0
    raw = torch.full((X.OUT_GUARD + lens.size + X.OUT_GUARD,), POISON_I16, dtype=torch.int16, device=DEV)
    d = torch.from_numpy(buf).to(DEV)
    A.chksum_batch_slotted(d[base:base + lens.size * stride], stride, torch.from_numpy(lens.view(np.int32)).to(DEV),
                           out=raw[X.OUT_GUARD:X.OUT_GUARD + lens.size])
    want = np.full(raw.numel(), X.POISON16, dtype=np.uint16)
    want[X.OUT_GUARD:X.OUT_GUARD + lens.size] = oracle.batch_slotted(buf[base:], stride, np.minimum(lens, stride))
    assert np.array_equal(raw.cpu().numpy().view(np.uint16), want)
    assert A.contract_violations(clear=True) == A.VIOLATION_PACKET_LEN


# ---- the engine's zero-copy host forms --------------------------------------------------------------

def _engine_run(eng, plan):
    """The plan's calls through the engine, on registered host memory, into a guarded numpy output."""
    out = np.full(plan.out_size, X.POISON16, dtype=np.uint16)
    for c, pos in zip(plan.calls, plan.out_pos.tolist()):
        o, b = out[pos:pos + c.n], plan.bufs[c.buf]
        if c.kind == "strided":
            eng.strided(b[c.base:], c.stride, c.length, c.n, out=o, final=c.final)
        elif c.kind == "csr":
            eng.csr(b, c.offsets, out=o, final=c.final)
        else:
            eng.slotted(b[c.base:c.base + c.n * c.stride], c.stride, c.lens, out=o, final=c.final)
    return out


def _dense_only(plan):
    """The calls of a family-A plan that hold DENSE lengths alone."""
    return X.Plan(plan.bufs, [c for c in plan.calls if int(c.plen.max()) <= X.DENSE[-1] + 1])


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("layout", ["b2b", "gap16", "odd", "csr", "slotted"])
def test_engine_zero_copy_host_forms(oracle, layout, family):
    """aipstack_chksum_engine_host_strided, _csr and _slotted on registered memory with zero copy
    on: GappedHostDesc, host CSR and SlottedHostDesc mask the packet edges in the stream by code of
    their own. Family A's DENSE lengths (CSR: the whole batch of the other forms) and family B."""
    plan = X.plan(layout, family, False)
    if family == "A" and layout != "csr":
        plan = X.cached((layout, "A-dense"), lambda: _dense_only(plan))
    want = _expected(oracle, (layout, family, "engine"), plan)
    assert _lib.load().aipstack_chksum_tune(b"engine_zero_copy", 1) == 0
    with A.ChksumEngine(0, chunk_bytes=8 << 20, nstreams=2) as eng:
        for b in plan.bufs.values():
            eng.register(b)
            # read in place by the kernels, not staged: else the host forms would not run at all
            assert _lib.load().aipstack_chksum_engine_region_mapped(eng._h, b.ctypes.data) == 1
        got = _engine_run(eng, plan)
    _compare(plan, got, want, (layout, family, "engine"))
