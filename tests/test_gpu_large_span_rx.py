"""aipstack_udp_rx_demux / _slotted and aipstack_icmp_rx_respond / _slotted with frames on both
sides of a 2^31 and a 2^32 byte offset from their base and of a device address that is a multiple
of 2^32, and the responder's header ring across the two offsets (large_span_rx_cases.py, on the
arena and windows of large_span_cases.py): every output whole against the models, between guards.
A 32-bit-truncated offset or address lands inside the zero arena, so a truncation shows as a
wrong value. Every test leaves the arena zero."""
import numpy as np
import pytest

import aipstack_amd as A

import icmp_cases as IC
import large_span_cases as L
import large_span_rx_cases as C
import test_gpu_icmp as TI
import test_gpu_udprx as TU

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOT = 2048


@pytest.fixture(scope="module")
def arena():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    a = torch.zeros(L.ARENA_BYTES, dtype=torch.uint8, device=DEV)
    A.contract_violations(clear=True)
    yield a
    del a
    torch.cuda.empty_cache()


def _demux(call, e, n):
    """The demux through `call(**outputs)` into poisoned, guarded outputs, compared whole."""
    out = TU.Guarded(n)
    call(verdict=out.verdict, dgrams=out.dgrams, unreach_code=out.unreach,
         deliver_frame=out.deliver_frame, counts=out.counts, workspace=out.workspace)
    torch.cuda.synchronize()
    assert np.array_equal(out.verdict.cpu().numpy(), e.verdict)
    assert out.dgrams.cpu().numpy().tobytes() == e.dgrams.tobytes()
    assert np.array_equal(out.unreach.cpu().numpy(), e.unreach)
    assert np.array_equal(out.deliver_frame.cpu().numpy().view(np.uint64), e.deliver_frame)
    assert np.array_equal(out.counts.cpu().numpy().view(np.uint64), e.counts)
    out.guards_intact()
    return out


def _respond(call, e, n, frame_addr):
    """The responder through `call(out=)` into dirty outputs with a 64-byte header ring, compared
    whole; frame_addr: the device address of every frame that has a chunk (uint64, n)."""
    got = call(out=TI._dirty(n, 64))
    torch.cuda.synchronize()
    _tables(e, got, n, frame_addr)
    ring = np.full((n, 64), TI.POISON, dtype=np.uint8)
    rows = np.fromiter(e.headers.keys(), dtype=np.int64)
    ring[rows, :42] = np.frombuffer(b"".join(e.headers.values()), dtype=np.uint8).reshape(-1, 42)
    ring[rows, 42:] = 0
    assert got.headers.cpu().numpy()[:n * 64].tobytes() == ring.tobytes()
    return got


def _tables(e, got, n, frame_addr):
    for name, want in (("verdict", e.verdict), ("status", e.status), ("hdr_lens", e.hdr_len),
                       ("chunk_index", e.chunk_index), ("response_frame", e.response_frame),
                       ("counts", e.counts)):
        assert getattr(got, name).cpu().numpy().tobytes() == want.tobytes(), name
    ch = np.array(e.chunks, dtype=np.int64).reshape(-1, 3)
    addr, ln = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    addr[:len(ch)] = frame_addr[ch[:, 0]] + ch[:, 1].astype(np.uint64)
    ln[:len(ch)] = ch[:, 2]
    assert np.array_equal(got.chunk_addr.cpu().numpy().view(np.uint64), addr)     # 64-bit values
    assert got.chunk_len.cpu().numpy().tobytes() == ln.tobytes()
    return addr[:len(ch)]


def _linearised(e, got, n):
    """The responses as frames of a send ring (the copy reads every chunk where it lies): the
    model's packets at the responders, nothing anywhere else."""
    ring = torch.full((n * SLOT,), TI.POISON, dtype=torch.uint8, device=DEV)
    lin = A.tx_linearise_slotted(ring, SLOT, got)
    lens = lin.lens.cpu().numpy()
    rows = np.flatnonzero(e.hdr_len)
    want = np.zeros(n, dtype=lens.dtype)
    pk = {int(e.rows[i]): IC.response_packet(e.local, e.local_frames, i) for i in e.local.headers}
    want[rows] = [14 + len(pk[int(r)]) for r in rows]
    assert np.array_equal(lens, want)
    h = ring.view(n, SLOT)[torch.from_numpy(rows).to(DEV)].cpu().numpy()
    for k, r in enumerate(rows):
        assert h[k, 14:lens[r]].tobytes() == pk[int(r)] and (h[k, lens[r]:] == TI.POISON).all(), r
    ring.view(n, SLOT)[torch.from_numpy(rows).to(DEV)] = TI.POISON
    assert bool((ring == TI.POISON).all())
    del ring


def _both(arena, oracle, c, frame_off, demux, respond):
    """Both entry points on a case whose windows' frames start at base offsets `frame_off`."""
    P = arena.data_ptr()
    n = c.n
    frame_addr = np.uint64(P + c.shift) + frame_off.astype(np.uint64)
    idx = sorted(c.frames)
    eu = C.expected_udp(oracle, n, c.lens, c.frames)
    host = dict(zip(idx, C.host_codes([c.frames[i] for i in idx])))
    ei = C.expected_icmp(oracle, n, c.lens, c.frames, host)
    fed = C.expected_icmp(oracle, n, c.lens, c.frames, {i: int(eu.unreach[i]) for i in idx})
    try:
        for w in c.windows:
            arena[w.start:w.end].copy_(torch.from_numpy(w.data))
        tbl, lis = C.tables()
        out = _demux(lambda **kw: demux(tbl, lis, **kw), eu, n)
        codes = np.full(n, IC.NO_UNREACH, dtype=np.uint8)
        codes[idx] = [host[i] for i in idx]
        got = _respond(lambda **kw: respond(torch.from_numpy(codes).to(DEV), **kw), ei, n, frame_addr)
        ca = got.chunk_addr.cpu().numpy().view(np.uint64)[:int(ei.counts[1])]
        for e in c.edges:                                # a chunk on the far side of every edge
            assert ((ca >= np.uint64(P + c.shift + e)) & (ca < np.uint64(P + c.shift + e + 8 * 65536))).any(), e
        _linearised(ei, got, n)
        # the demux's codes as they are: a response exactly where nobody took the datagram
        got = _respond(lambda **kw: respond(out.unreach, **kw), fed, n, frame_addr)
        assert int(fed.counts[0]) < int(ei.counts[0]) and (fed.status == IC.UNREACH).any()
        _linearised(fed, got, n)
        for w in c.windows:                              # the frames are only read
            assert np.array_equal(arena[w.start:w.end].cpu().numpy(), w.data)
    finally:
        for w in c.windows:
            arena[w.start:w.end].zero_()
    assert A.contract_violations(clear=True) == 0


# ---- (a) CSR frames across the edges ----------------------------------------------------------

@pytest.mark.parametrize("kind", C.DISTANCES)
def test_csr_frames_across_4gib_offsets_and_addresses(arena, oracle, kind):
    P = arena.data_ptr()
    for shift in (0, 15):
        c = C.csr_case(P, shift, kind)
        L.check_windows(c.windows)
        assert C.filler_verdicts(oracle, [L.FILL]) == {L.FILL: 0}            # NOT_IP4
        base = arena[shift:]
        doff = torch.from_numpy(c.offsets.view(np.int64)).to(DEV)
        f = TI._np_iface(C.IFACE)
        _both(arena, oracle, c, c.offsets[:-1],
              lambda tbl, lis, **kw: A.udp_rx_demux(base, doff, f, tbl, lis, **kw),
              lambda codes, **kw: A.icmp_rx_respond(base, doff, f, codes, **kw))
    assert not bool(arena.view(torch.int64).any()), "the test left bytes in the arena"


# ---- (b) ring slots -----------------------------------------------------------------------------

@pytest.mark.parametrize("stride,n", C.SLOTTED)
def test_ring_slots_past_4gib(arena, oracle, stride, n):
    for shift in L.SHIFTS:
        c = C.slotted_case(stride, n, shift)
        L.check_windows(c.windows)
        base = arena[shift:shift + n * stride]
        lens = torch.from_numpy(c.lens.astype(np.int32)).to(DEV)
        f = TI._np_iface(C.IFACE)
        _both(arena, oracle, c, np.arange(n, dtype=np.int64) * stride,
              lambda tbl, lis, **kw: A.udp_rx_demux_slotted(base, stride, lens, f, tbl, lis, **kw),
              lambda codes, **kw: A.icmp_rx_respond_slotted(base, stride, lens, f, codes, **kw))
    assert not bool(arena.view(torch.int64).any()), "the test left bytes in the arena"


# ---- (c) the responder's header ring across the edges -------------------------------------------

def test_header_ring_past_4gib(arena, oracle):
    c = C.ring_case(oracle)
    n, e, stride = c.n, c.e, C.RING_STRIDE
    buf = torch.from_numpy(c.buf).to(DEV)
    lens = torch.from_numpy(c.lens.astype(np.int32)).to(DEV)
    frame_addr = np.uint64(buf.data_ptr()) + (np.arange(n, dtype=np.int64) * C.FRAME_SLOT).astype(np.uint64)
    rows = torch.from_numpy(c.rows).to(DEV)
    want = np.zeros((c.rows.size, 64), dtype=np.uint8)
    want[:, :42] = np.frombuffer(b"".join(e.headers[int(r)] for r in c.rows), dtype=np.uint8).reshape(-1, 42)
    for shift in L.SHIFTS:
        out = TI._dirty(n, 64)
        out.headers, out.hdr_stride = arena[shift:shift + n * stride], stride
        slots = out.headers.view(n, stride)
        try:
            got = A.icmp_rx_respond_slotted(buf, C.FRAME_SLOT, lens, TI._np_iface(C.IFACE), None, out=out)
            torch.cuda.synchronize()
            _tables(e, got, n, frame_addr)
            assert np.array_equal(slots[rows, :64].cpu().numpy(), want), shift    # 42 bytes, zero up to 64
        finally:
            slots[rows, :64] = 0
        # every other byte of the ring, the shift bytes before it and the arena behind it
        assert not bool(arena.view(torch.int64).any()), "bytes outside the responders' slots"
        assert A.contract_violations(clear=True) == 0
    assert np.array_equal(buf.cpu().numpy(), c.buf)
