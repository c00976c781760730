"""aipstack_arp_rx_respond / _slotted with frames at, before and across a 2^31 and a 2^32 byte
offset from their base (and across a device address that is a multiple of 2^32), and the header
ring across the two offsets, on the arena, windows and filler of large_span_cases.py as
large_span_rx_cases.py uses them: every output whole against the model of arp_cases.py. A
32-bit-truncated offset or address lands inside the zero arena, so a truncation shows as a wrong
value. Every test leaves the arena zero."""
import numpy as np
import pytest

import aipstack_amd as A

import arp_cases as C
import arp_ref as R
import large_span_rx_cases as LR
import test_gpu_arp as TA

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

L, LI = LR.L, LR.LI
DEV = "cuda"
IFACE = C.iface()
DISTANCES = (1, 13, 41, 60)      # the straddler starts this far before the edge; 60: it ends at it


@pytest.fixture(scope="module")
def arena():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    a = torch.zeros(L.ARENA_BYTES, dtype=torch.uint8, device=DEV)
    A.contract_violations(clear=True)
    yield a
    del a
    torch.cuda.empty_cache()


def _sides(k):
    return [C.other(k, IFACE), C.not_arp(k), C.request(k + 1, IFACE, pad=0), R.arp(1, 5, 6)[:41],
            C.request(k + 2, IFACE), C.other(k + 3, IFACE)]


def expected(n, frames):
    """arp_cases.Expected of a batch of n frames whose `frames` {index: bytes} are the only ones
    with bytes other than zero (a zero frame, or none at all, is _ARP_NONE)."""
    g = np.array(sorted(frames), dtype=np.int64)
    local = C.respond([frames[int(i)] for i in g], IFACE)
    e = C.Expected()
    e.status = np.full(n, C.NONE, dtype=np.uint8)
    e.status[g] = local.status
    e.records = np.zeros(n, dtype=C.RECORD)
    e.records["status"] = C.NONE
    e.records[g] = local.records
    e.hdr_len = np.zeros(n, dtype=np.uint32)
    e.hdr_len[g] = local.hdr_len
    e.chunk_index = np.zeros(n + 1, dtype=np.uint64)
    e.counts = local.counts.copy()
    e.reply_frame = np.full(n, C.NO_FRAME, dtype=np.uint64)
    e.seen_frame = np.full(n, C.NO_FRAME, dtype=np.uint64)
    j, k = int(local.counts[0]), int(local.counts[1])
    e.reply_frame[:j] = g[local.reply_frame[:j].astype(np.int64)]
    e.seen_frame[:k] = g[local.seen_frame[:k].astype(np.int64)]
    e.headers = {int(g[i]): h for i, h in local.headers.items()}
    return e


def _run(arena, windows, n, frames, call):
    e = expected(n, frames)
    try:
        for w in windows:
            arena[w.start:w.end].copy_(torch.from_numpy(w.data))
        o = TA.Outputs(n)
        call(o)
        TA._compare(e, o, None, n, 64)
        for w in windows:                                # the frames are only read
            assert np.array_equal(arena[w.start:w.end].cpu().numpy(), w.data)
    finally:
        for w in windows:
            arena[w.start:w.end].zero_()
    assert A.contract_violations(clear=True) == 0
    return e


def test_csr_frames_across_4gib_offsets_and_addresses(arena):
    """Round each edge: side frames, a request that starts 1, 13 or 41 bytes before the edge or
    ends at it (the next frame, a request too, then starts at it), and the sides again; 65535-byte
    zero frames in between."""
    P = arena.data_ptr()
    for shift in (0, 15):
        edges = LI.edges_of(P, shift)
        lens, windows, frames, at = [], [], {}, 0
        for w, edge in enumerate(edges):
            d = DISTANCES[(w + shift) % 4]
            pre = _sides(w)
            items = pre + [C.request(100 + w, IFACE)] + [C.request(200 + w, IFACE, pad=0)] + _sides(w + 7)
            ws = edge - d - sum(len(f) for f in pre)
            q, r = divmod(ws - at, L.FILL)
            lens += [L.FILL] * q + ([r] if r else [])
            for j, f in enumerate(items):
                frames[len(lens) + j] = f
            data = np.frombuffer(b"".join(items), dtype=np.uint8).copy()
            windows.append(L.Window(shift + ws, data))
            lens += [len(f) for f in items]
            at = ws + data.size
        lens += [L.FILL] * 3
        n = len(lens)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.array(lens, dtype=np.uint64), out=offsets[1:])
        assert shift + int(offsets[-1]) <= L.ARENA_BYTES
        L.check_windows(windows)
        doff = torch.from_numpy(offsets.view(np.int64)).to(DEV)
        e = _run(arena, windows, n, frames,
                 lambda o: A.arp_rx_respond(arena[shift:], doff, TA._np_iface(IFACE), out=o.res,
                                            workspace=o.workspace))
        for edge in edges:                               # a reply on either side of every edge
            rows = np.flatnonzero(e.hdr_len)
            assert (offsets[rows] < edge).any() and (offsets[rows] >= edge).any()
    assert not bool(arena.view(torch.int64).any()), "the test left bytes in the arena"


@pytest.mark.parametrize("stride,n", [(65536, 65600), (65530, 65600)])
def test_ring_slots_past_4gib(arena, stride, n):
    """65536-byte slots start at the two offsets; of the 65530-byte slots one starts 18 bytes
    before 2^31 and one 36 bytes before 2^32, so their ARP packets lie across them."""
    if stride == 65530:
        assert (L.E31 - 18) % stride == 0 and (L.E32 - 36) % stride == 0
    for shift in (0, 15):
        slots = {0, n - 1}
        for edge in L.EDGES:
            slots |= set(range(edge // stride - 4, edge // stride + 5))
        every = _sides(shift) + [C.request(300 + k, IFACE) for k in range(4)]
        frames = {s: every[j % len(every)] if j % 3 else C.request(400 + j, IFACE)
                  for j, s in enumerate(sorted(slots))}
        lens = np.zeros(n, dtype=np.int32)
        for s, f in frames.items():
            lens[s] = len(f)
        windows = [L.Window(shift + s * stride, np.frombuffer(f, dtype=np.uint8).copy())
                   for s, f in frames.items() if f]
        L.check_windows(windows)
        assert shift + (n - 1) * stride + 65535 <= L.ARENA_BYTES
        dl = torch.from_numpy(lens).to(DEV)
        e = _run(arena, windows, n, frames,
                 lambda o: A.arp_rx_respond_slotted(arena[shift:shift + n * stride], stride, dl,
                                                    TA._np_iface(IFACE), out=o.res, workspace=o.workspace))
        assert int(e.counts[0]) >= 8
    assert not bool(arena.view(torch.int64).any()), "the test left bytes in the arena"


def test_header_ring_past_4gib(arena):
    """The header ring in 65536-byte slots: slot 32768 starts at offset 2^31 of the ring, slot
    65536 at 2^32 (plain stores; a 64-byte ring past 4 GiB would need 2^26 frames)."""
    n, stride = LR.RING_SLOTS, LR.RING_STRIDE
    _, rows = L.ring_rows(n)
    frames = {int(r): C.request(j, IFACE) for j, r in enumerate(rows)}
    buf = np.zeros(n * 64, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.int32)
    for r, f in frames.items():
        lens[r] = len(f)
        buf[r * 64:r * 64 + len(f)] = np.frombuffer(f, dtype=np.uint8)
    e = expected(n, frames)
    dbuf, dl, drows = torch.from_numpy(buf).to(DEV), torch.from_numpy(lens).to(DEV), torch.from_numpy(rows).to(DEV)
    want = np.zeros((rows.size, 64), dtype=np.uint8)
    want[:, :42] = np.frombuffer(b"".join(e.headers[int(r)] for r in rows), dtype=np.uint8).reshape(-1, 42)
    for shift in (0, 15):
        o = TA.Outputs(n)
        o.res.headers, o.res.hdr_stride = arena[shift:shift + n * stride], stride
        slots = o.res.headers.view(n, stride)
        try:
            A.arp_rx_respond_slotted(dbuf, 64, dl, TA._np_iface(IFACE), out=o.res, workspace=o.workspace)
            torch.cuda.synchronize()
            r = o.res
            for name, w in (("status", e.status), ("records", e.records), ("hdr_lens", e.hdr_len),
                            ("chunk_index", e.chunk_index), ("reply_frame", e.reply_frame),
                            ("seen_frame", e.seen_frame), ("counts", e.counts)):
                assert getattr(r, name).cpu().numpy().tobytes() == w.tobytes(), name
            assert np.array_equal(slots[drows, :64].cpu().numpy(), want), shift   # 42 bytes, zero up to 64
            o.guards_intact()
        finally:
            slots[drows, :64] = 0
        # every other byte of the ring, the shift bytes before it and the arena behind it
        assert not bool(arena.view(torch.int64).any()), "bytes outside the repliers' slots"
        assert A.contract_violations(clear=True) == 0
    assert np.array_equal(dbuf.cpu().numpy(), buf)
