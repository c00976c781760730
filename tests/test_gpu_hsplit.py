"""Header-split Tx fill (aipstack_chksum_tx_fill_hsplit) on the GPU against the CPU oracle.

The expected result never comes from the GPU's own tx_fill: it is oracle.tx_fill_batch on the
linearised copy plus the layout rule written out in hsplit_cases.layout_ok. Every test compares
the statuses, every header slot byte for byte (slack included), and the payload buffer."""
import struct

import numpy as np
import pytest

import aipstack_amd as A

import hsplit_cases as H

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tune(key, value):
    from aipstack_amd import _lib
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == A.AIPSTACK_CHKSUM_OK


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)   # whatever ran before this module
    yield


class Dev:
    """A SplitFrames layout on the device."""

    def __init__(self, sp):
        self.sp = sp
        self.headers = _d(sp.headers)
        self.hdr_lens = _d(sp.hdr_lens.view(np.int32))
        self.payload = _d(sp.payload)
        addr, lens, index = sp.chunk_table(self.payload.data_ptr())
        self.addr, self.len = _d(addr.view(np.int64)), _d(lens.view(np.int32))
        self.index = _d(index.view(np.int64))

    def fill(self, **kw):
        return A.tx_fill_header_split(self.headers, self.sp.hdr_stride, self.hdr_lens, self.addr,
                                      self.len, self.index, **kw)


def _check(oracle, sp, dev=None, **kw):
    """Run the fill on `sp` and compare with the CPU expectation; returns (dev, want_h, want_st,
    linear statuses, in-layout mask)."""
    want_h, want_st, st_lin, ok = H.expected(oracle, sp)
    dev = dev or Dev(sp)
    st = dev.fill(**kw).cpu().numpy()
    got_h = dev.headers.cpu().numpy()
    bad = np.nonzero(st != want_st)[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], want_st[bad[:8]])
    rows = np.nonzero((got_h != want_h).reshape(len(sp.chunks), -1).any(axis=1))[0]
    assert rows.size == 0, (rows[:8], want_st[rows[:8]])
    assert np.array_equal(dev.payload.cpu().numpy(), sp.payload)
    return dev, want_h, want_st, st_lin, ok


# ---- 1. golden frames -------------------------------------------------------------------

@pytest.mark.parametrize("stride", [128, 256])
@pytest.mark.parametrize("cls", H.SPLIT_CLASSES)
def test_golden_frames_every_split(oracle, cls, stride):
    frs = H.golden_frames()
    assert len(frs) == 3000
    buf, off = H.pack(frs)
    at = H.split_points(frs, cls, stride)
    sp = A.split_frames(buf, off, at, hdr_stride=stride)
    _, want_h, want_st, st_lin, ok = _check(oracle, sp)
    protos = np.array([f[23] if len(f) > 23 else 0 for f in frs])
    accept_lin = st_lin == H.ACCEPT
    if cls == "l4_fixed":
        # not vacuous: what the oracle alone gives on this generator is 1,256 filled
        # (602 TCP / 318 UDP / 336 ICMP), 24 of the UDP fields holding 0xFFFF
        filled = accept_lin & ok
        assert filled.sum() >= 1200
        for p in (6, 17, 1):
            assert (filled & (protos == p)).sum() >= 300, p
        ffff = 0
        for i in np.nonzero(filled & (protos == 17))[0]:
            fld = 14 + (frs[i][14] & 0xF) * 4 + 6
            ffff += bytes(want_h[i * stride + fld:i * stride + fld + 2]) == b"\xff\xff"
        assert ffff >= 20
        # the other frames the linear fill accepts carry trailing bytes: status 9, untouched
        rest = accept_lin & ~ok
        assert rest.sum() > 0 and (want_st[rest] == H.SPLIT_LAYOUT).all()
        for i in np.nonzero(rest)[0]:
            f = frs[i]
            assert len(f) > 14 + struct.unpack_from(">H", f, 16)[0] or f[23] == 17
    if cls in ("l4_plus1", "l4_plus3"):
        odd = np.array([(at[i] - H._l4_fixed_end(f)[0]) & 1 for i, f in enumerate(frs)])
        assert (accept_lin & ok & (odd == 1)).sum() >= 300   # odd in-slot counts are covered
    if cls == "whole":
        nochunk = np.array([len(c) == 0 for c in sp.chunks])
        assert (accept_lin & ok & nochunk).sum() >= 300
    if cls == "short4":
        assert accept_lin.sum() >= 1200 and (want_st[accept_lin] == H.SPLIT_LAYOUT).all()


# ---- 2. payload shapes ------------------------------------------------------------------

PAYLOADS = [0, 1, 2, 3, 1459, 1460, 8960]


def _shape_segments():
    """(frame, split point) list: exact-length TCP / UDP segments over every payload size, IPv4
    IHL 5 / 6 / 15, TCP data offsets 5 / 15, split at the end of the fixed header, one byte on
    (an odd in-slot count) and, for TCP with options, at their end; the all-zero ICMP datagram;
    TCP segments whose in-slot part folds to 0xFFFF (even and odd in-slot counts)."""
    rng = np.random.default_rng(77)
    segs = []
    for plen in PAYLOADS:
        pay = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
        for ihl in (5, 6, 15):
            for doff in (5, 15):
                f, fixed, opts = H.tcp_segment(pay, ihl=ihl, doff=doff)
                segs += [(f, fixed), (f, opts)]
                if len(f) > fixed:
                    segs.append((f, fixed + 1))
                if len(f) > opts:
                    segs.append((f, opts + 1))
            f, fixed = H.udp_segment(pay, ihl=ihl)
            segs.append((f, fixed))
            if len(f) > fixed:
                segs.append((f, fixed + 1))
    f, fixed = H.icmp_zero_segment()
    segs += [(f, fixed), (f, fixed + 1), (f, len(f))]
    for pay in (bytes(64), rng.integers(0, 256, 1460, dtype=np.uint8).tobytes(), b"\x00\x00\x01"):
        for extra in (0, 1, 2, 3):
            segs.append(H.tcp_inslot_ffff(pay, 20 + extra))
    return segs


@pytest.mark.parametrize("gap,reverse", [(0, False), (1, False), (3, True)])
@pytest.mark.parametrize("pieces", [None, (1,), (1, 3)])
def test_payload_shapes(oracle, pieces, gap, reverse):
    """Payloads cut into 1, 2 and 3 chunks (1, 3, the rest), back to back, at odd addresses
    (gap), and in reverse memory order."""
    segs = _shape_segments()
    buf, off = H.pack([f for f, _ in segs])
    sp = A.split_frames(buf, off, [a for _, a in segs], hdr_stride=256,
                        payload_pieces=None if pieces is None else [pieces] * len(segs),
                        payload_gap=gap, reverse=reverse)
    if pieces == (1, 3):
        assert max(len(c) for c in sp.chunks) == 3
    if gap == 1:
        assert any(o & 1 for c in sp.chunks for o, _ in c)
    _, want_h, want_st, st_lin, ok = _check(oracle, sp)
    # exact-length segments with their headers in the slot: every one is filled
    assert ok.all() and (want_st == H.ACCEPT).all()
    # the pinned zero cases: the all-zero ICMP datagram gets 0xFFFF
    k = next(i for i, (f, _) in enumerate(segs) if f[23] == 1)
    assert bytes(want_h[k * 256 + 36:k * 256 + 38]) == b"\xff\xff"


# ---- 3. batch-shape edges ---------------------------------------------------------------

@pytest.fixture(scope="module")
def ring_want():
    """Per batch size: the layout and what the oracle makes of its linear frames (computed
    once, shared, never modified)."""
    cache = {}

    def get(oracle, n):
        if n not in cache:
            slots, lens, payload, linear = H.ring_batch(n, seed=300 + n)
            flat = linear.reshape(-1).copy()
            off = np.arange(n + 1, dtype=np.uint64) * np.uint64(linear.shape[1])
            st = oracle.tx_fill_batch(flat, off)
            want = slots.reshape(n, -1).copy()
            want[:, :54] = flat.reshape(n, -1)[:, :54]
            assert np.array_equal(flat.reshape(n, -1)[:, 54:], linear[:, 54:])
            for a in (slots, lens, payload, want, st):
                a.setflags(write=False)
            cache[n] = (slots, lens, payload, want.reshape(-1), st)
        return cache[n]
    return get


@pytest.mark.parametrize("cpk", [1, 64])
@pytest.mark.parametrize("just_written", [False, True])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 4096])
def test_batch_shape_edges(oracle, ring_want, n, just_written, cpk):
    slots, lens, payload, want, want_st = ring_want(oracle, n)
    assert (want_st == H.ACCEPT).all()
    dh, dl, dp = _d(slots.copy()), _d(lens.view(np.int32).copy()), _d(payload.copy())
    addr = _d(dp.data_ptr() + 1460 * np.arange(n, dtype=np.int64))
    clen = _d(np.full(n, 1460, dtype=np.int32))
    index = _d(np.arange(n + 1, dtype=np.int64))
    _tune("chunk_packets", cpk)
    try:
        st = A.tx_fill_header_split(dh, 64, dl, addr, clen, index, just_written=just_written)
        torch.cuda.synchronize()
    finally:
        _tune("chunk_packets", 0)
    assert np.array_equal(st.cpu().numpy(), want_st)
    assert np.array_equal(dh.cpu().numpy(), want)
    assert np.array_equal(dp.cpu().numpy(), payload)


# ---- 4. idempotence and graph capture ---------------------------------------------------

def _mixed_layout():
    frs = H.golden_frames()[:1000]
    buf, off = H.pack(frs)
    return A.split_frames(buf, off, H.split_points(frs, "l4_plus1", 128), hdr_stride=128,
                          payload_pieces=[(3,)] * len(frs), payload_gap=1)


def test_idempotent(oracle):
    sp = _mixed_layout()
    dev, want_h, want_st, _, _ = _check(oracle, sp)
    once = dev.headers.cpu().numpy()
    st2 = dev.fill().cpu().numpy()
    assert np.array_equal(st2, want_st)
    assert np.array_equal(dev.headers.cpu().numpy(), once)


def test_captured_in_a_graph_on_a_side_stream(oracle):
    sp = _mixed_layout()
    want_h, want_st, _, _ = H.expected(oracle, sp)
    dev = Dev(sp)
    n = len(sp.chunks)
    out = torch.empty(n, dtype=torch.uint8, device=DEV)
    from aipstack_amd import _lib
    ws = torch.empty(int(_lib.load().aipstack_chksum_tx_fill_hsplit_workspace_bytes(n)),
                     dtype=torch.uint8, device=DEV)
    dev.fill(out=out, workspace=ws)   # warm-up outside the capture (the CU count is cached)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        dev.fill(out=out, workspace=ws)
    fresh = _d(sp.headers)
    for _ in range(2):
        dev.headers.copy_(fresh)
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want_st)
        assert np.array_equal(dev.headers.cpu().numpy(), want_h)
    assert np.array_equal(dev.payload.cpu().numpy(), sp.payload)


# ---- 5. prefilled fields ----------------------------------------------------------------

def test_prefilled_fields_are_taken_as_zero(oracle):
    """Both checksum fields hold 0xA5A5 before the call: the result is what zeroed fields give
    (the oracle zeroes them itself), and out-of-layout segments keep the 0xA5A5."""
    frs = H.golden_frames()[:1500]
    buf, off = H.pack(frs)
    buf = buf.copy()
    for i, f in enumerate(frs):
        a, hl, proto = H._l4_fixed_end(f)
        o = int(off[i])
        if len(f) >= 26:
            buf[o + 24:o + 26] = 0xA5
        fo = {6: 16, 17: 6, 1: 2}.get(proto)
        if fo is not None and len(f) >= 14 + hl + fo + 2:
            buf[o + 14 + hl + fo:o + 14 + hl + fo + 2] = 0xA5
    sp = A.split_frames(buf, off, H.split_points(frs, "l4_fixed", 128), hdr_stride=128)
    _, _, want_st, _, ok = _check(oracle, sp)
    assert ((want_st == H.ACCEPT) & ok).sum() >= 500


# ---- 6. later iterations of the grid-stride loops ----------------------------------------

GUARD, GUARD_BYTE, POISON = 256, 0xA7, 0xC3
_ring_cache = {}


def _ring_case(oracle, n, stride):
    """ring_batch(n) at `stride` and what the oracle makes of its linear frames (computed once,
    shared, never modified)."""
    if (n, stride) not in _ring_cache:
        slots, lens, payload, linear = H.ring_batch(n, seed=700 + n, stride=stride)
        flat = linear.reshape(-1).copy()
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(linear.shape[1])
        st = oracle.tx_fill_batch(flat, off)
        want = slots.reshape(n, -1).copy()
        want[:, :54] = flat.reshape(n, -1)[:, :54]
        assert np.array_equal(flat.reshape(n, -1)[:, 54:], linear[:, 54:]) and (st == H.ACCEPT).all()
        for a in (slots, lens, payload, want, st):
            a.setflags(write=False)
        _ring_cache[n, stride] = (slots, lens, payload, want.reshape(-1), st)
    return _ring_cache[n, stride]


def _ring_fill(case, stride, cap):
    """The fill at block cap `cap` on fresh copies, statuses poisoned, guards round the ring and
    the statuses: (statuses, ring) as the GPU left them."""
    slots, lens, payload, _, _ = case
    n = lens.size
    ring = torch.full((GUARD + n * stride + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    ring[GUARD:GUARD + n * stride] = _d(slots.copy())
    status = torch.full((GUARD + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    status[GUARD:GUARD + n] = POISON
    dp = _d(payload.copy())
    addr = _d(dp.data_ptr() + 1460 * np.arange(n, dtype=np.int64))
    _tune("aux_blocks", cap)
    try:
        A.tx_fill_header_split(ring[GUARD:GUARD + n * stride], stride, _d(lens.view(np.int32).copy()),
                               addr, _d(np.full(n, 1460, dtype=np.int32)),
                               _d(np.arange(n + 1, dtype=np.int64)), out=status[GUARD:GUARD + n])
        torch.cuda.synchronize()
    finally:
        _tune("aux_blocks", -1)
    assert np.array_equal(dp.cpu().numpy(), payload)
    hs, hr = status.cpu().numpy(), ring.cpu().numpy()
    for h, m in ((hs, n), (hr, n * stride)):
        assert (h[:GUARD] == GUARD_BYTE).all() and (h[GUARD + m:] == GUARD_BYTE).all()
    return hs[GUARD:GUARD + n], hr[GUARD:GUARD + n * stride]


@pytest.mark.parametrize("stride", [64, 72])
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("n", [257, 1000, 1537])
def test_later_iterations_of_both_passes(oracle, n, cap, stride):
    """At most `cap` blocks ("aux_blocks"): the header and the finish pass loop (1000 segments at
    cap 1: four iterations, the last with a partial wave; 1537 at cap 3: a third iteration in
    which only block 0 has work). Every segment from 256 * cap on is produced by a later
    iteration alone."""
    case = _ring_case(oracle, n, stride)
    st, ring = _ring_fill(case, stride, cap)
    bad = np.nonzero(st != case[4])[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]])
    rows = np.nonzero((ring != case[3]).reshape(n, stride).any(axis=1))[0]
    assert rows.size == 0, rows[:8]
    st0, ring0 = _ring_fill(case, stride, -1)
    assert np.array_equal(st, st0) and np.array_equal(ring, ring0)


def test_later_iterations_on_a_mixed_layout(oracle):
    """Every status class, odd in-slot lengths and three chunks per segment at one block."""
    _tune("aux_blocks", 1)
    try:
        _check(oracle, _mixed_layout())
    finally:
        _tune("aux_blocks", -1)


def test_later_iterations_of_the_split_fill_scatter(oracle):
    """tx_fill(split=True) and tx_fill_slotted(split=True) on 1000 frames with the scatter pass
    at one block, against the frame oracle."""
    from aipstack_amd import synth
    fr, off = synth.frames_host(1000, seed=4321, max_payload=600)
    want = fr.copy()
    want_st = oracle.tx_fill_batch(want, off)
    ring, lens = synth.to_slots(fr, off, 2048, slack_seed=9)
    want_ring = ring.copy()
    want_rst = oracle.tx_fill_slotted(want_ring, 2048, lens)
    assert set(want_st[256:].tolist()) == {0, 3, 6, 8} and np.array_equal(want_st, want_rst)
    _tune("aux_blocks", 1)
    try:
        d = _d(fr)
        st = A.tx_fill(d, _d(off), split=True).cpu().numpy()
        dr = _d(ring)
        rst = A.tx_fill_slotted(dr, 2048, _d(lens.view(np.int32)), split=True).cpu().numpy()
    finally:
        _tune("aux_blocks", -1)
    assert np.array_equal(st, want_st) and np.array_equal(d.cpu().numpy(), want)
    assert np.array_equal(rst, want_rst) and np.array_equal(dr.cpu().numpy(), want_ring)


# ---- 7. diagnostics (last: after all of the above) ---------------------------------------

def test_no_contract_violations():
    assert A.contract_violations() == 0
