"""aipstack_tcp_rx_respond / _slotted with frames at, before and across a 2^31 and a 2^32 byte
offset from their base (and across a device address that is a multiple of 2^32), on the arena,
windows and filler of large_span_cases.py as test_gpu_large_span_arp.py uses them: every output
whole against the model of tcp_rsp_cases.py. The emit pass reads a frame a second time (its source
MAC) and addresses the records, the lengths and both lists by frame index; a 32-bit-truncated
offset or address lands inside the zero arena, so a truncation shows as a wrong MAC, record or
list entry. Every test leaves the arena zero."""
import numpy as np
import pytest

import aipstack_amd as A

import large_span_rx_cases as LR
import tcp_rsp_cases as C
import tcp_rsp_ref as R
import test_gpu_tcp_rsp as TT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

L, LI = LR.L, LR.LI
DEV = "cuda"
IFACE = C.iface(ip_id=0xFFF0)
DISTANCES = (1, 13, 41, 60)      # the straddler starts this far before the edge; 60: it ends at it


@pytest.fixture(scope="module")
def arena():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    a = torch.zeros(L.ARENA_BYTES, dtype=torch.uint8, device=DEV)
    A.contract_violations(clear=True)
    yield a
    del a
    torch.cuda.empty_cache()


def rst_frame(k):
    """A 60-byte segment that gets an RST, from a MAC and an address of its own."""
    mac = bytes([0x02, 0xBB, (k >> 16) & 0xFF, (k >> 8) & 0xFF, k & 0xFF, 0x07])
    f = R.frame((R.SYN, R.ACK)[k & 1], src=(C.LOCAL & 0xFFFFFF00) | (1 + k % 30), dst=C.LOCAL,
                sport=2000 + k, dport=(R.CLOSED, R.SPECIFIC)[k & 1], seq=0x01010101 * (k % 255),
                ack=0x00020003 * k & 0xFFFFFFFF, pad60=True)
    assert len(f) == 60
    return f[:6] + mac + f[12:]


def _sides(k):
    return [C.no_rst(k), C.not_tcp(k), rst_frame(500 + k), C.no_rst(k + 1), rst_frame(600 + k), C.not_tcp(k + 3)]


def expected(oracle, n, frames):
    """tcp_rsp_cases.Expected of a batch of n frames whose `frames` {index: bytes} are the only
    ones with bytes other than zero (a zero frame, or none at all, is not IPv4: _RSP_NONE)."""
    g = np.array(sorted(frames), dtype=np.int64)
    sub = [frames[int(i)] for i in g]
    local = C.respond(sub, C.verdicts_of(oracle, sub), IFACE, None, C.LISTENERS)
    zero = int(C.verdicts_of(oracle, [bytes(L.FILL), b""])[0])
    assert zero == int(C.verdicts_of(oracle, [b"", bytes(60)])[0]) == 0
    e = C.Expected()
    e.verdict = np.full(n, zero, dtype=np.uint8)
    e.verdict[g] = local.verdict
    e.segs = np.zeros(n, dtype=C.SEG)
    e.segs[g] = local.segs
    e.pcb = np.full(n, C.T.NO_PCB, dtype=np.uint32)
    e.status = np.full(n, C.NONE, dtype=np.uint8)
    e.status[g] = local.status
    e.listener = np.full(n, C.NO_LISTENER, dtype=np.uint32)
    e.listener[g] = local.listener
    e.hdr_len = np.zeros(n, dtype=np.uint32)
    e.hdr_len[g] = local.hdr_len
    e.chunk_index = np.zeros(n + 1, dtype=np.uint64)
    e.counts = local.counts.copy()
    e.response_frame = np.full(n, C.NO_FRAME, dtype=np.uint64)
    e.syn_frame = np.full(n, C.NO_FRAME, dtype=np.uint64)
    j, k = int(local.counts[0]), int(local.counts[1])
    e.response_frame[:j] = g[local.response_frame[:j].astype(np.int64)]
    e.syn_frame[:k] = g[local.syn_frame[:k].astype(np.int64)]
    e.headers = {int(g[i]): h for i, h in local.headers.items()}
    return e


def _run(oracle, arena, windows, n, frames, call):
    e = expected(oracle, n, frames)
    try:
        for w in windows:
            arena[w.start:w.end].copy_(torch.from_numpy(w.data))
        o = TT.Outputs(n)
        call(o)
        TT._compare(e, o, None, n, 64)
        for w in windows:                                # the frames are only read
            assert np.array_equal(arena[w.start:w.end].cpu().numpy(), w.data)
    finally:
        for w in windows:
            arena[w.start:w.end].zero_()
    assert A.contract_violations(clear=True) == 0
    return e


def _kw(o):
    return dict(tcp_ttl=IFACE["ttl"], out=o.res, workspace=o.workspace)


def csr_case(P, shift):
    """(lens, windows, frames, edges): round each edge side frames, an RST-due segment that
    starts 1, 13 or 41 bytes before the edge or ends at it (the next frame, one too, then starts
    at it), and the sides again; 65535-byte zero frames in between."""
    edges = LI.edges_of(P, shift)
    lens, windows, frames, at = [], [], {}, 0
    for w, edge in enumerate(edges):
        d = DISTANCES[(w + shift) % 4]
        pre = _sides(w)
        items = pre + [rst_frame(100 + w), rst_frame(200 + w)] + _sides(w + 7)
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
    return lens, windows, frames, edges


def test_csr_frames_across_4gib_offsets_and_addresses(oracle, arena):
    P = arena.data_ptr()
    for shift in (0, 15):
        lens, windows, frames, edges = csr_case(P, shift)
        n = len(lens)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.array(lens, dtype=np.uint64), out=offsets[1:])
        assert shift + int(offsets[-1]) <= L.ARENA_BYTES
        L.check_windows(windows)
        doff = torch.from_numpy(offsets.view(np.int64)).to(DEV)
        lis = A.tcp_listeners(C.LISTENERS)
        e = _run(oracle, arena, windows, n, frames,
                 lambda o: A.tcp_rx_respond(arena[shift:], doff, TT._np_iface(IFACE), None, lis, None, **_kw(o)))
        rows = np.flatnonzero(e.hdr_len)
        for edge in edges:                               # an RST on either side of every edge
            assert (offsets[rows] < edge).any() and (offsets[rows] >= edge).any()
        # the one beyond 2^32: its own MAC, its own record, its place in the list
        high = int(rows[offsets[rows] >= L.E32][0])
        assert e.headers[high][:6] == frames[high][6:12] and e.headers[high][:2] == b"\x02\xbb"
        assert int(e.segs["remote_port"][high]) == int.from_bytes(frames[high][34:36], "big")
        assert int(e.response_frame[list(rows).index(high)]) == high
    assert not bool(arena.view(torch.int64).any()), "the test left bytes in the arena"


def slots_case(stride, n, shift):
    slots = {0, n - 1}
    for edge in L.EDGES:
        slots |= set(range(edge // stride - 4, edge // stride + 5))
    every = _sides(shift) + [rst_frame(300 + k) for k in range(4)]
    frames = {s: every[j % len(every)] if j % 3 else rst_frame(400 + j) for j, s in enumerate(sorted(slots))}
    lens = np.zeros(n, dtype=np.int32)
    for s, f in frames.items():
        lens[s] = len(f)
    windows = [L.Window(shift + s * stride, np.frombuffer(f, dtype=np.uint8).copy())
               for s, f in frames.items() if f]
    return frames, lens, windows


@pytest.mark.parametrize("stride,n", [(65536, 65600), (65530, 65600)])
def test_ring_slots_past_4gib(oracle, arena, stride, n):
    """65536-byte slots start at the two offsets; of the 65530-byte slots one starts 18 bytes
    before 2^31 and one 36 bytes before 2^32, so their TCP headers lie across them."""
    if stride == 65530:
        assert (L.E31 - 18) % stride == 0 and (L.E32 - 36) % stride == 0
    for shift in (0, 15):
        frames, lens, windows = slots_case(stride, n, shift)
        L.check_windows(windows)
        assert shift + (n - 1) * stride + 65535 <= L.ARENA_BYTES
        dl = torch.from_numpy(lens).to(DEV)
        lis = A.tcp_listeners(C.LISTENERS)
        e = _run(oracle, arena, windows, n, frames,
                 lambda o: A.tcp_rx_respond_slotted(arena[shift:shift + n * stride], stride, dl,
                                                    TT._np_iface(IFACE), None, lis, None, **_kw(o)))
        rows = np.flatnonzero(e.hdr_len)
        assert int(e.counts[0]) >= 8 and (rows * stride >= L.E32).any() and (rows * stride < L.E31).any()
    assert not bool(arena.view(torch.int64).any()), "the test left bytes in the arena"
