"""aipstack_icmp_rx_unreach / _slotted with frames at, before and across a 2^31 and a 2^32 byte
offset from their base (and across a device address that is a multiple of 2^32), on the arena,
windows and filler of large_span_cases.py as test_gpu_large_span_arp.py uses them: every output
whole against the model of icmp_du_cases.py. A 32-bit-truncated offset or address lands inside the
zero arena, so a truncation shows as a wrong value. The slotted batches have 65,600 frames: 257
tiles, so the one-workgroup scan takes a second step. Every test leaves the arena zero."""
import numpy as np
import pytest

import aipstack_amd as A

import icmp_du_cases as C
import large_span_rx_cases as LR
import test_gpu_icmp_du as TD

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

L, LI = LR.L, LR.LI
DEV = "cuda"
IFACE = C.iface()
TABLE = C.pcb_table(64)
DISTANCES = (1, 43, 70, 74)      # the straddler starts this far before the edge; 74: it ends at it


@pytest.fixture(scope="module")
def arena():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    a = torch.zeros(L.ARENA_BYTES, dtype=torch.uint8, device=DEV)
    A.contract_violations(clear=True)
    yield a
    del a
    torch.cuda.empty_cache()


def _hit(k):
    """A 74-byte frag-needed message of connection k: Ethernet, IPv4, ICMP, quoted IPv4 and 12
    quoted TCP bytes end 14, 34, 42, 62 and 74 bytes in."""
    return C.frag_needed(C.key_of(TABLE, k % len(TABLE)), l4=12, seq=k, mtu=600 + k)


def _sides(k):
    return [C.other_frames(k), _hit(k + 1), C.frag_needed(C.near_miss(TABLE, k % 64, k)), C.other_frames(k + 3),
            C.R.frame(C.R.quoted(17, C.R.udp_head(8), src=C.LOCAL), src=C.PEER, dst=C.LOCAL, code=3)]


def expected(oracle, n, lens, frames):
    """icmp_du_cases.Expected of a batch of n frames whose `frames` {index: bytes} are the only
    ones with bytes other than zero."""
    g, fr, v = LR._window_frames(oracle, frames)
    local = C.expected(fr, v, IFACE, TABLE)
    e = C.Expected()
    e.verdict = LR._verdicts(oracle, n, np.asarray(lens), g, v)
    e.status = np.full(n, C.NONE, dtype=np.uint8)
    e.status[g] = local.status
    e.records = np.zeros(n, dtype=C.RECORD)
    e.records[g] = local.records
    e.counts = local.counts.copy()
    j = int(local.counts[0])
    e.pcb_frame = np.full(n, C.NO_FRAME, dtype=np.uint64)
    e.pcb_frame[:j] = g[local.pcb_frame[:j].astype(np.int64)]
    return e


def _run(oracle, arena, windows, n, lens, frames, call):
    e = expected(oracle, n, lens, frames)
    try:
        for w in windows:
            arena[w.start:w.end].copy_(torch.from_numpy(w.data))
        o = TD.Guarded(n)
        call(o)
        TD._compare(e, o, None)
        for w in windows:                                # the frames are only read
            assert np.array_equal(arena[w.start:w.end].cpu().numpy(), w.data)
    finally:
        for w in windows:
            arena[w.start:w.end].zero_()
    assert A.contract_violations(clear=True) == 0
    return e


def _kw(o):
    return dict(verdict=o.verdict, status=o.status, records=o.records, pcb_frame=o.pcb_frame, counts=o.counts,
                workspace=o.workspace)


def test_csr_frames_across_4gib_offsets_and_addresses(oracle, arena):
    """Round each edge: side frames, a message with a PCB that starts 1, 43 or 70 bytes before
    the edge (its Ethernet header, its quoted IPv4 header, its quoted TCP bytes lie across it) or
    ends at it (the next frame, another such message, then starts at it), and the sides again;
    65535-byte zero frames in between."""
    P = arena.data_ptr()
    table = torch.from_numpy(A.tcp_pcb_table_sort(TABLE).view(np.uint8).copy()).to(DEV)
    for shift in (0, 15):
        edges = LI.edges_of(P, shift)
        lens, windows, frames, at = [], [], {}, 0
        for w, edge in enumerate(edges):
            d = DISTANCES[(w + shift) % 4]
            pre = _sides(w)
            items = pre + [_hit(100 + w), _hit(200 + w)] + _sides(w + 7)
            assert len(items[len(pre)]) == 74
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
        e = _run(oracle, arena, windows, n, lens, frames,
                 lambda o: A.icmp_rx_unreach(arena[shift:], doff, TD._np_iface(IFACE), table, **_kw(o)))
        rows = e.pcb_frame[:int(e.counts[0])].astype(np.int64)
        for edge in edges:                               # a PCB on either side of every edge
            assert (offsets[rows] < edge).any() and (offsets[rows] >= edge).any()
    assert not bool(arena.view(torch.int64).any()), "the test left bytes in the arena"


@pytest.mark.parametrize("stride,n", [(65536, 65600), (65530, 65600)])
def test_ring_slots_past_4gib(oracle, arena, stride, n):
    """65536-byte slots start at the two offsets; of the 65530-byte slots one starts 18 bytes
    before 2^31 and one 36 bytes before 2^32, so the IPv4 and the ICMP header lie across them."""
    if stride == 65530:
        assert (L.E31 - 18) % stride == 0 and (L.E32 - 36) % stride == 0
    table = torch.from_numpy(A.tcp_pcb_table_sort(TABLE).view(np.uint8).copy()).to(DEV)
    for shift in (0, 15):
        slots = {0, n - 1}
        for edge in L.EDGES:
            slots |= set(range(edge // stride - 4, edge // stride + 5))
        every = _sides(shift) + [_hit(300 + k) for k in range(4)]
        frames = {s: every[j % len(every)] if j % 3 else _hit(400 + j) for j, s in enumerate(sorted(slots))}
        frames[n - 1] = _hit(999)                        # in the scan's second step
        lens = np.zeros(n, dtype=np.int32)
        for s, f in frames.items():
            lens[s] = len(f)
        windows = [L.Window(shift + s * stride, np.frombuffer(f, dtype=np.uint8).copy())
                   for s, f in frames.items() if f]
        L.check_windows(windows)
        assert shift + (n - 1) * stride + 65535 <= L.ARENA_BYTES
        dl = torch.from_numpy(lens).to(DEV)
        e = _run(oracle, arena, windows, n, lens, frames,
                 lambda o: A.icmp_rx_unreach_slotted(arena[shift:shift + n * stride], stride, dl,
                                                     TD._np_iface(IFACE), table, **_kw(o)))
        assert int(e.counts[0]) >= 8 and int(e.pcb_frame[int(e.counts[0]) - 1]) >= 65536
    assert not bool(arena.view(torch.int64).any()), "the test left bytes in the arena"
