"""The ICMP responder (aipstack_icmp_rx_respond / _slotted) on the GPU against the model of
icmp_cases.py, which test_icmp_host.py pins byte for byte to packets recorded from the reference's
own stack; verdicts from the frame oracle.

Every comparison covers status, verdict, hdr_len, the chunk table with its index, both lists and
counts, every header slot (a response's 42 bytes, the zeros behind them, the pre-filled pattern
wherever the contract says untouched) and the frames themselves, over outputs that were dirty
before the call."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import frame_cases as F
import icmp_cases as C
import icmp_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = 0xC3
SLOT = 2048


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


def _tune(key, value):
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == 0


def _verdicts(oracle, frames):
    buf, off = F.pack(frames)
    return oracle.rx_verify_batch(buf, off)


def _np_iface(ifc):
    return A.icmp_iface(ifc["local"], ifc["bcast"], ifc["mac"], mtu=ifc["mtu"], ip_id=ifc["ip_id"],
                        ttl=ifc["ttl"], allow_broadcast_ping=ifc["allow"])


class Layout:
    """The frames on the device: CSR (back to back from an odd address) or ring slots."""

    def __init__(self, frames, slotted, slot=SLOT):
        n = len(frames)
        self.slotted, self.n, self.slot = slotted, n, slot
        if slotted:
            self.start = np.arange(n, dtype=np.int64) * slot
            host = np.full(n * slot, 0x5C, dtype=np.uint8)
            self.lens = torch.from_numpy(np.array([len(f) for f in frames], dtype=np.int32)).to(DEV)
        else:
            ln = np.array([len(f) for f in frames], dtype=np.int64)
            self.start = 1 + np.concatenate([[0], np.cumsum(ln)[:-1]]) if n else np.zeros(0, np.int64)
            host = np.full(1 + int(ln.sum()) + 64, 0x5C, dtype=np.uint8)
            off = np.concatenate([self.start, [1 + int(ln.sum())]]).astype(np.int64)
            self.offsets = torch.from_numpy(off).to(DEV)
        for i, f in enumerate(frames):
            host[self.start[i]:self.start[i] + len(f)] = np.frombuffer(f, dtype=np.uint8)
        self.host = host
        self.dev = torch.from_numpy(host).to(DEV)

    def call(self, ifc, codes, **kw):
        dc = None if codes is None else torch.tensor(codes, dtype=torch.uint8, device=DEV)
        if self.slotted:
            return A.icmp_rx_respond_slotted(self.dev, self.slot, self.lens, _np_iface(ifc), dc, **kw)
        return A.icmp_rx_respond(self.dev, self.offsets, _np_iface(ifc), dc, **kw)


def _dirty(n, hdr_stride, shift=0):
    """An IcmpResponses of pre-dirtied tensors; `shift` moves the ring off its 64-byte boundary."""
    def t(k, dtype):
        return torch.full((k,), -0x3C3C3C3D if dtype != torch.uint8 else POISON, dtype=dtype, device=DEV)
    ring = torch.full((n * hdr_stride + 64,), POISON, dtype=torch.uint8, device=DEV)
    return A.IcmpResponses(ring[shift:shift + n * hdr_stride], hdr_stride, t(n, torch.int32),
                           t(n, torch.int64), t(n, torch.int32), t(n + 1, torch.int64),
                           t(n, torch.uint8), t(n, torch.uint8), t(n, torch.int64), t(2, torch.int64))


def _compare(e, got, lay, frames, hdr_stride):
    n = len(frames)
    torch.cuda.synchronize()
    assert np.array_equal(got.verdict.cpu().numpy(), e.verdict)
    assert np.array_equal(got.status.cpu().numpy(), e.status)
    assert np.array_equal(got.hdr_lens.cpu().numpy().view(np.uint32), e.hdr_len)
    assert np.array_equal(got.chunk_index.cpu().numpy().view(np.uint64), e.chunk_index)
    assert np.array_equal(got.response_frame.cpu().numpy().view(np.uint64), e.response_frame)
    assert np.array_equal(got.counts.cpu().numpy().view(np.uint64), e.counts)
    addr, ln = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    for k, (fi, off, length) in enumerate(e.chunks):
        addr[k], ln[k] = lay.dev.data_ptr() + int(lay.start[fi]) + off, length
    assert np.array_equal(got.chunk_addr.cpu().numpy().view(np.uint64), addr)
    assert np.array_equal(got.chunk_len.cpu().numpy().view(np.uint32), ln)
    ring = got.headers.cpu().numpy()[:n * hdr_stride].reshape(n, hdr_stride)
    zero_to = min(hdr_stride, 64)
    for i in range(n):
        if i in e.headers:
            assert ring[i, :42].tobytes() == e.headers[i], i
            assert not ring[i, 42:zero_to].any() and (ring[i, zero_to:] == POISON).all(), i
        else:
            assert (ring[i] == POISON).all(), i
    assert np.array_equal(lay.dev.cpu().numpy(), lay.host)                   # the frames: only read


def _check(frames, verdicts, codes, ifc, *, slotted, hdr_stride=64, shift=0):
    e = C.respond(frames, verdicts, codes, ifc)
    lay = Layout(frames, slotted)
    out = _dirty(len(frames), hdr_stride, shift)
    got = lay.call(ifc, codes, out=out)
    assert got.headers is out.headers and got.n == len(frames)
    _compare(e, got, lay, frames, hdr_stride)
    return e, lay, got


_cache = {}


def _fixture_batches(oracle):
    if "fixture" not in _cache:
        _cache["fixture"] = [b for s in R.load()
                             for b in C.stack_batches(s, _verdicts(oracle, C.stack_frames(s)))]
    return _cache["fixture"]


def _crafted(oracle):
    if "crafted" not in _cache:
        fr = C.crafted_frames()
        _cache["crafted"] = (fr, _verdicts(oracle, fr), C.crafted_codes(fr))
    return _cache["crafted"]


# ---- every fixture case and the model's crafted cases, through both entry points ----------------

@pytest.mark.parametrize("hdr_stride,shift", [(64, 0), (64, 8), (42, 0), (96, 0)])
@pytest.mark.parametrize("slotted", [False, True])
def test_fixture_cases(oracle, slotted, hdr_stride, shift):
    """The batches of the reference-recorded stacks (a batch ends behind a TOO_LARGE frame and
    the next starts one Ident later), in whole lines (64-byte slots on a 64-byte boundary) and in
    plain stores (a shifted ring, the smallest stride, a stride with bytes past 64)."""
    seen = 0
    for _, frames, verdicts, codes, ifc, e in _fixture_batches(oracle):
        _check(frames, verdicts, codes, ifc, slotted=slotted, hdr_stride=hdr_stride, shift=shift)
        seen += int(e.counts[0])
    assert seen >= 100


@pytest.mark.parametrize("slotted", [False, True])
def test_crafted_cases(oracle, slotted):
    frames, v, codes = _crafted(oracle)
    for ifc in (C.iface(ip_id=0xFFF0, ttl=17), C.iface(mtu=256, allow=True, ip_id=5)):
        e, _, _ = _check(frames, v, codes, ifc, slotted=slotted)
        assert int(e.counts[0]) > 60
    # no requests at all: a NULL code array
    e, _, _ = _check(frames, v, None, C.iface(), slotted=slotted)
    assert not (e.status == C.UNREACH).any() and (e.status == C.ECHO_REPLY).any()


# ---- batch sizes: the Ident and the compact index across waves and blocks ----------------------

def _places(n):
    """Responders at lanes 0 and 63 of a wave, at the first and last frame of a block, a block
    where every frame responds (the third, where there is one) and blocks with none."""
    p = {i for i in (0, 63, 64, 127, 255, 256, n - 1) if 0 <= i < n}
    if n > 768:
        p |= set(range(512, 768))
    return p


@pytest.mark.parametrize("n,cap", [(1, -1), (63, -1), (64, -1), (65, -1), (256, -1), (257, -1), (257, 1),
                                   (1400, -1), (1400, 2)])
def test_batch_sizes(oracle, n, cap):
    """1400 frames are six blocks of the scan with a last block of 120; with at most two
    workgroups ("aux_blocks") the decide and emit passes loop over the tiles."""
    key = ("sizes", n)
    if key not in _cache:
        fr = C.mixed_batch(n, _places(n), seed=20261020 + n)
        # frames 768 .. 1279: two blocks without any responder (no ICMP, no UDP)
        for i in range(768, min(n, 1280)):
            if len(fr[i]) > 23 and fr[i][23] in (1, 17):
                fr[i] = F.LOCAL_MAC + F.peer_mac(1) + b"\x08\x06" + bytes(46)
        _cache[key] = (fr, _verdicts(oracle, fr))
    fr, v = _cache[key]
    codes = C.host_codes(fr)
    ifc = C.iface(ip_id=0xFF00)
    _tune("aux_blocks", cap)
    try:
        got = {}
        for slotted in (False, True):
            e, _, g = _check(fr, v, codes, ifc, slotted=slotted)
            got[slotted] = g.headers.cpu().numpy().tobytes()
    finally:
        _tune("aux_blocks", -1)
    assert got[False] == got[True]
    assert all(e.status[i] == C.ECHO_REPLY for i in _places(n))
    if n == 1400:
        assert len(set(np.unique(v))) >= 8 and (e.status == C.UNREACH).any()
        assert not e.hdr_len[768:1280].any() and e.hdr_len[512:768].all()
        assert int(e.counts[0]) > 300


# ---- several steps of the scan: more than 65,536 frames ----------------------------------------

SCAN_STEP = 256 * 256        # frames per step of the one-workgroup scan: 256 tiles of 256 frames


def _scan_batch(oracle):
    """Five whole steps of the scan and a part of a sixth (3 tiles and 77 frames), of 44- to
    60-byte frames. Step 1: every frame responds; step 3: none does; steps 0, 2, 4 and the part:
    responders in their first and last tile (so on both sides of every boundary that the empty
    step does not touch), at lanes 0 and 63, at a block's first and last frame, and every 97th
    frame. The other frames: ARP, an echo request with a bad checksum, a short TCP frame."""
    if "scan" not in _cache:
        n = 5 * SCAN_STEP + 3 * 256 + 77
        echo = [C.eth(R.echo(R.pattern(k % 19, k), ident=k), pad60=True) for k in range(64)]
        none = [F.LOCAL_MAC + F.peer_mac(1) + b"\x08\x06" + bytes(46),
                C.eth(R.ip_packet(1, R.icmp(8, 0, R.REST, R.pattern(18, 3), bad=True))),
                C.eth(R.ip_packet(6, R.pattern(10, 2)))]
        resp = np.zeros(n, dtype=bool)
        resp[SCAN_STEP:2 * SCAN_STEP] = True
        for step in (0, 2, 4, 5):
            lo, hi = step * SCAN_STEP, min((step + 1) * SCAN_STEP, n)
            resp[lo:hi:97] = True
            for edge in (lo, hi - 256 if hi - lo >= 256 else lo):
                resp[[edge, min(edge + 63, hi - 1), min(edge + 64, hi - 1), min(edge + 255, hi - 1)]] = True
            resp[hi - 1] = True
        fr = [echo[i % 64] if resp[i] else none[i % 3] for i in range(n)]
        v = _verdicts(oracle, fr)
        ifc = C.iface(ip_id=0xFFF0)
        e = C.respond(fr, v, None, ifc)
        assert np.array_equal(e.hdr_len != 0, resp) and set(np.unique(v)) >= {0, 4, 5, 6}
        _cache["scan"] = (fr, ifc, e)
    return _cache["scan"]


@pytest.mark.parametrize("slotted", [False, True])
def test_scan_over_several_steps(oracle, slotted):
    """328,525 frames: the scan's loop runs six times and carries its sums from step to step.
    Every output is compared whole with the model (numpy comparisons, no loop per frame)."""
    fr, ifc, e = _scan_batch(oracle)
    n = len(fr)
    assert n > 5 * SCAN_STEP and int(e.counts[0]) > SCAN_STEP
    lay = Layout(fr, slotted, slot=64)
    out = _dirty(n, 64)
    got = lay.call(ifc, None, out=out)
    torch.cuda.synchronize()
    for name, want in (("verdict", e.verdict), ("status", e.status), ("hdr_lens", e.hdr_len),
                       ("chunk_index", e.chunk_index), ("response_frame", e.response_frame),
                       ("counts", e.counts)):
        assert getattr(got, name).cpu().numpy().tobytes() == want.tobytes(), name
    addr, ln = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    ch = np.array(e.chunks, dtype=np.int64).reshape(-1, 3)
    addr[:len(ch)] = (lay.dev.data_ptr() + lay.start[ch[:, 0]] + ch[:, 1]).astype(np.uint64)
    ln[:len(ch)] = ch[:, 2]
    assert got.chunk_addr.cpu().numpy().tobytes() == addr.tobytes()
    assert got.chunk_len.cpu().numpy().tobytes() == ln.tobytes()
    ring = np.full((n, 64), POISON, dtype=np.uint8)
    rows = np.fromiter(e.headers.keys(), dtype=np.int64)
    ring[rows, :42] = np.frombuffer(b"".join(e.headers.values()), dtype=np.uint8).reshape(-1, 42)
    ring[rows, 42:] = 0
    assert got.headers.cpu().numpy().tobytes() == ring.tobytes()
    assert np.array_equal(lay.dev.cpu().numpy(), lay.host)


# ---- round trip: respond -> linearise -> Rx verify ---------------------------------------------

def test_round_trip(oracle):
    frames, v, codes = _crafted(oracle)
    ifc = C.iface(ip_id=77)
    e, lay, got = _check(frames, v, codes, ifc, slotted=True)
    n = len(frames)
    before = got.headers.cpu().numpy().copy()
    st = A.tx_fill_header_split(got.headers, got.hdr_stride, got.hdr_lens, got.chunk_addr,
                                got.chunk_len, got.chunk_index)
    torch.cuda.synchronize()
    assert np.array_equal(got.headers.cpu().numpy(), before)              # every field was right
    st = st.cpu().numpy()
    resp = e.hdr_len != 0
    assert (st[resp] == C.ACCEPT).all()
    ring = torch.full((n * SLOT,), POISON, dtype=torch.uint8, device=DEV)
    lin = A.tx_linearise_slotted(ring, SLOT, got)
    ls = lin.status.cpu().numpy()
    assert (ls[resp] == A.AIPSTACK_TX_LIN_WRITTEN).all() and (ls[~resp] == A.AIPSTACK_TX_LIN_SKIPPED).all()
    verdict = A.rx_verify_slotted(ring, SLOT, lin.lens).cpu().numpy()
    assert (verdict[resp] == C.ACCEPT).all()
    h = ring.cpu().numpy().reshape(n, SLOT)
    lens = lin.lens.cpu().numpy()
    for i in range(n):
        if resp[i]:
            pkt = C.response_packet(e, frames, i)
            assert lens[i] == 14 + len(pkt) and h[i, 14:lens[i]].tobytes() == pkt
            assert (h[i, lens[i]:] == POISON).all()
        else:
            assert lens[i] == 0 and (h[i] == POISON).all()                 # a skipped slot
    # the CSR form takes the object too: a frame of exactly its room
    room = np.concatenate([[0], np.cumsum(np.where(resp, lens, 0))]).astype(np.int64)
    flat = torch.full((int(room[-1]) + 1,), POISON, dtype=torch.uint8, device=DEV)
    lin2 = A.tx_linearise(flat, torch.from_numpy(room).to(DEV), got)
    assert (lin2.status.cpu().numpy()[resp] == A.AIPSTACK_TX_LIN_WRITTEN).all()


# ---- replay from a graph -------------------------------------------------------------------------

def test_graph_replay(oracle):
    frames, v, codes = _crafted(oracle)
    ifc = C.iface(ip_id=0xFFFA)
    e = C.respond(frames, v, codes, ifc)
    lay = Layout(frames, False)
    n = len(frames)
    out = _dirty(n, 64)
    ws = torch.empty(A.icmp_rx_respond_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    dc = torch.tensor(codes, dtype=torch.uint8, device=DEV)
    f = _np_iface(ifc)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.icmp_rx_respond(lay.dev, lay.offsets, f, dc, out=out, workspace=ws)   # warm-up
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        A.icmp_rx_respond(lay.dev, lay.offsets, f, dc, out=out, workspace=ws)
    tensors = (out.hdr_lens, out.chunk_addr, out.chunk_len, out.chunk_index, out.status, out.verdict,
               out.response_frame, out.counts, ws)
    seen = []
    for _ in range(2):
        for t in tensors:
            t.view(torch.uint8).fill_(0x99)
        out.headers.fill_(POISON)
        g.replay()
        _compare(e, out, lay, frames, 64)
        seen.append(b"".join(t.cpu().numpy().tobytes() for t in tensors[:-1]) +
                    out.headers.cpu().numpy().tobytes())
    assert seen[0] == seen[1]


# ---- the argument list, on the host only ---------------------------------------------------------

def test_einval_paths():
    fr = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    off = torch.tensor([0, 60, 120], dtype=torch.int64, device=DEV)
    good = A.icmp_iface(R.LOCAL, R.BCAST, C.LOCAL_MAC)
    assert A.icmp_rx_respond(fr, off, good).n == 2
    for change in (dict(mtu=255), dict(flags=2), dict(reserved=7)):
        bad = good.copy()
        for k, val in change.items():
            bad[k] = val
        with pytest.raises(A.ChksumError) as err:
            A.icmp_rx_respond(fr, off, bad)
        assert err.value.status == A.AIPSTACK_CHKSUM_EINVAL
    for kw in (dict(hdr_stride=41), dict(workspace=torch.empty(24, dtype=torch.uint8, device=DEV)),
               dict(workspace=torch.empty(72, dtype=torch.uint8, device=DEV)[4:])):
        with pytest.raises(A.ChksumError) as err:
            A.icmp_rx_respond(fr, off, good, **kw)
        assert err.value.status == A.AIPSTACK_CHKSUM_EINVAL
    with pytest.raises(A.ChksumError):
        A.icmp_rx_respond_slotted(fr, 2048, torch.tensor([60, 60], dtype=torch.int32, device=DEV),
                                  good, hdr_stride=41)
    e = A.icmp_rx_respond(fr[:0], off[:1], good)                          # n == 0
    assert e.n == 0 and e.counts.cpu().tolist() == [0, 0]
    assert _lib.load().aipstack_chksum_last_hip_error() == 0
