"""TCP segments without a connection (aipstack_tcp_rx_respond / _slotted) on the GPU against the
model of tcp_rsp_cases.py, which test_tcp_rsp_host.py pins to what the reference's own stack sent
for the frames of tests/golden/tcp_rsp_ref_cases.json.

Every comparison covers verdict, records and PCB cookies (also against aipstack_tcp_rx_parse on
the same batch), status, listener, hdr_len, the zero chunk index, both lists and the counts, every
header slot (an RST's 54 bytes, the zeros behind them, the pre-filled pattern wherever the
contract says untouched), the guard bytes in front of and behind every output, and the frames
themselves, over outputs that were dirty before the call."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import tcp_rsp_cases as C
import tcp_rsp_ref as R
import test_gpu_icmp as TI

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = 0xC3
GUARD = 64
SLOT = 2048
_OUTS = ("verdict", "segs", "pcb", "status", "listener", "hdr_lens", "chunk_index", "response_frame",
         "syn_frame", "counts")


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


def _tune(key, value):
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == 0


def _np_iface(ifc):
    return A.icmp_iface(ifc["local"], ifc["bcast"], ifc["mac"], mtu=ifc["mtu"], ip_id=ifc["ip_id"], ttl=1)


class Outputs:
    """A TcpResponses (`res`) of poisoned tensors, each between GUARD poisoned bytes of its own
    allocation; `shift` moves the header ring off its 64-byte boundary, `seg_shift` the records
    off their 16-byte boundary."""

    def __init__(self, n, hdr_stride=64, shift=0, seg_shift=0):
        self.raw = []

        def t(nbytes, dtype, off=0):
            raw = torch.full((GUARD + off + nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
            self.raw.append((raw, GUARD + off, nbytes))
            return raw[GUARD + off:GUARD + off + nbytes].view(dtype)

        self.workspace = t(A.tcp_rx_respond_workspace_bytes(n), torch.uint8)
        outs = dict(verdict=t(n, torch.uint8), segs=t(32 * n, torch.uint8, seg_shift), pcb=t(4 * n, torch.int32),
                    status=t(n, torch.uint8), listener=t(4 * n, torch.int32), hdr_lens=t(4 * n, torch.int32),
                    chunk_index=t(8 * (n + 1), torch.int64), response_frame=t(8 * n, torch.int64),
                    syn_frame=t(8 * n, torch.int64), counts=t(16, torch.int64))
        self.res = A.TcpResponses(t(n * hdr_stride, torch.uint8, shift), hdr_stride, outs)
        assert self.res.headers.data_ptr() % 64 == shift % 64 and self.res.segs.data_ptr() % 16 == seg_shift

    def poison(self):
        for raw, _, _ in self.raw:
            raw.fill_(POISON)

    def guards_intact(self):
        for raw, at, nbytes in self.raw:
            assert bool((raw[:at] == POISON).all()) and bool((raw[at + nbytes:] == POISON).all())


def _compare(e, o, lay, n, hdr_stride):
    got = o.res
    torch.cuda.synchronize()
    assert got.n == n
    assert np.array_equal(got.verdict.cpu().numpy(), e.verdict)
    assert got.segs.cpu().numpy().tobytes() == e.segs.tobytes()
    assert np.array_equal(got.pcb_numpy(), e.pcb)
    assert np.array_equal(got.status.cpu().numpy(), e.status)
    assert np.array_equal(got.listener_numpy(), e.listener)
    assert np.array_equal(got.hdr_lens.cpu().numpy().view(np.uint32), e.hdr_len)
    assert np.array_equal(got.chunk_index.cpu().numpy().view(np.uint64), e.chunk_index)
    assert np.array_equal(got.response_frame.cpu().numpy().view(np.uint64), e.response_frame)
    assert np.array_equal(got.syn_frame.cpu().numpy().view(np.uint64), e.syn_frame)
    assert np.array_equal(got.counts.cpu().numpy().view(np.uint64), e.counts)
    ring = np.full((n, hdr_stride), POISON, dtype=np.uint8)
    if e.headers:
        rows = np.fromiter(e.headers.keys(), dtype=np.int64)
        ring[rows, :54] = np.frombuffer(b"".join(e.headers.values()), dtype=np.uint8).reshape(-1, 54)
        ring[rows, 54:min(hdr_stride, 64)] = 0
    assert got.headers.cpu().numpy().tobytes() == ring.tobytes()
    o.guards_intact()
    if lay is not None:
        assert np.array_equal(lay.dev.cpu().numpy(), lay.host)                # the frames: only read


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)


def _call(lay, ifc, o, pcbs, lis, req):
    f = _np_iface(ifc)
    table = A.tcp_listeners(lis) if lis else None
    kw = dict(tcp_ttl=ifc["ttl"], out=o.res, workspace=o.workspace)
    if lay.slotted:
        return A.tcp_rx_respond_slotted(lay.dev, lay.slot, lay.lens, f, pcbs, table, _dev(req), **kw)
    return A.tcp_rx_respond(lay.dev, lay.offsets, f, pcbs, table, _dev(req), **kw)


def _check(oracle, frames, ifc, *, slotted, pcbs=None, lis=C.LISTENERS, req=None, hdr_stride=64, shift=0,
           seg_shift=0, slot=SLOT, e=None):
    """`pcbs`: an unsorted KEY array; the call gets it sorted."""
    if e is None:
        e = C.respond(frames, C.verdicts_of(oracle, frames), ifc, pcbs, lis, req)
    lay = TI.Layout(frames, slotted, slot)
    o = Outputs(len(frames), hdr_stride, shift, seg_shift)
    got = _call(lay, ifc, o, None if pcbs is None else A.tcp_pcb_table_sort(pcbs), lis, req)
    assert got.headers is o.res.headers
    _compare(e, o, lay, len(frames), hdr_stride)
    return e, lay, o


def _linearised(e, res, n):
    """The RSTs as frames of a send ring, through the lineariser: the model's 54 bytes at the
    frames that got one, nothing anywhere else."""
    ring = torch.full((n * 64,), POISON, dtype=torch.uint8, device=DEV)
    lin = A.tx_linearise_slotted(ring, 64, res, frame_max=64)
    torch.cuda.synchronize()
    rst = e.hdr_len != 0
    ls = lin.status.cpu().numpy()
    assert (ls[rst] == A.AIPSTACK_TX_LIN_WRITTEN).all() and (ls[~rst] == A.AIPSTACK_TX_LIN_SKIPPED).all()
    assert np.array_equal(lin.lens.cpu().numpy().view(np.uint32), e.hdr_len)
    got = ring.cpu().numpy().reshape(n, 64)
    assert (got[~rst] == POISON).all() and (got[rst, 54:] == POISON).all()
    return [got[i, :54].tobytes() for i in sorted(e.headers)]


# ---- every fixture case, through both entry points; the sessions through the lineariser --------

@pytest.mark.parametrize("hdr_stride,shift,seg_shift", [(64, 0, 0), (64, 8, 8), (54, 0, 0), (128, 0, 8)])
@pytest.mark.parametrize("slotted", [False, True])
def test_fixture_cases(oracle, slotted, hdr_stride, shift, seg_shift):
    """The frames of each reference-recorded stack (/24, /30) as one batch: in whole lines (64-byte
    slots on a 64-byte boundary, records on a 16-byte one) and in plain stores. A case whose
    reference stack sent an RST gets one that differs from the recorded frame in the Ident and the
    header checksum only (every case ran on a fresh stack); a SYN-ACK case is _SYN."""
    for stack in R.load():
        frames, ifc, lis = C.stack_frames(stack), C.stack_iface(stack), C.stack_listeners(stack)
        e, _, _ = _check(oracle, frames, ifc, slotted=slotted, lis=lis, hdr_stride=hdr_stride, shift=shift,
                         seg_shift=seg_shift)
        for i, case in enumerate(stack["cases"]):
            sent = C.sent(case["out"])
            assert (e.status[i] == C.SYN) == (case["out"] == ["SYNACK"])
            assert (i in e.headers) == bool(sent), case["name"]
            if sent:
                h = e.headers[i]
                assert h[:18] + h[20:24] + h[26:] == sent[0][:18] + sent[0][20:24] + sent[0][26:], case["name"]
        assert int(e.counts[0]) >= 60 and int(e.counts[1]) >= 20


@pytest.mark.parametrize("slotted", [False, True])
def test_sessions_linearised_equal_the_reference(oracle, slotted):
    """One stack over 50 frames: the batch's RSTs, linearised, are the frames the reference sent,
    byte for byte and in order (RST j carries Ident j)."""
    for stack in R.load():
        frames = [bytes.fromhex(f) for f in stack["session"]["in"]]
        e, _, o = _check(oracle, frames, C.stack_iface(stack), slotted=slotted, lis=C.stack_listeners(stack))
        want = [f for out in stack["session"]["out"] for f in C.sent(out)]
        assert len(want) >= 25 and _linearised(e, o.res, len(frames)) == want


# ---- what the TCP Rx parse writes, byte for byte -----------------------------------------------

@pytest.mark.parametrize("slotted", [False, True])
def test_parse_outputs_equal_tcp_rx_parse(oracle, slotted):
    table = C.pcb_table(300)
    frames, req = C.random_batch(3, 1100, table)
    frames += C.stack_frames(R.load()[0])
    req = np.concatenate([req, np.zeros(len(frames) - len(req), dtype=np.uint8)])
    e, lay, o = _check(oracle, frames, C.iface(), slotted=slotted, pcbs=table, req=req)
    keys = A.tcp_pcb_table_sort(table)
    p = (A.tcp_rx_parse_slotted(lay.dev, lay.slot, lay.lens, keys) if slotted
         else A.tcp_rx_parse(lay.dev, lay.offsets, keys))
    torch.cuda.synchronize()
    assert torch.equal(p.verdict, o.res.verdict) and torch.equal(p.segs, o.res.segs)
    assert torch.equal(p.pcb, o.res.pcb)
    assert (e.verdict == 11).any() and (e.pcb != C.T.NO_PCB).sum() > 100


# ---- batch sizes: the lists across waves and blocks --------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("kind", ["all", "none", "mixed"])
def test_batch_sizes(oracle, n, kind):
    frames = C.sized_batch(n, kind)
    got = {}
    for slotted in (False, True):
        e, _, o = _check(oracle, frames, C.iface(), slotted=slotted, slot=128)
        got[slotted] = o.res.headers.cpu().numpy().tobytes()
    assert got[False] == got[True]
    assert int(e.counts[0]) == {"all": n, "none": 0}.get(kind, int(e.counts[0]))
    if kind == "mixed" and n == 513:   # with at most two workgroups the passes loop over the tiles
        _tune("aux_blocks", 2)
        try:
            _check(oracle, frames, C.iface(), slotted=True, slot=128, e=e)
        finally:
            _tune("aux_blocks", -1)


_cache = {}


def _scan_batch(oracle, kind):
    """256 * 256 + 300 frames: one whole step of the one-workgroup scan (256 tiles of 256 frames)
    and a part of a second. Frames repeat with period 1029 ("mixed": RSTs at every place of a
    wave and a tile over the batch, and a tile in which every frame gets one)."""
    if kind not in _cache:
        n = 256 * 256 + 300
        pool = C.sized_batch(1029, kind)
        assert max(len(f) for f in pool) <= 128
        frames = [pool[i % 1029] for i in range(n)]
        ifc = C.iface(ip_id=0xFF00)
        _cache[kind] = (frames, ifc, C.respond(frames, C.verdicts_of(oracle, frames), ifc, None, C.LISTENERS))
    return _cache[kind]


@pytest.mark.parametrize("kind", ["all", "none", "mixed"])
@pytest.mark.parametrize("slotted", [False, True])
def test_scan_takes_a_second_step(oracle, slotted, kind):
    frames, ifc, e = _scan_batch(oracle, kind)
    assert {"all": int(e.counts[0]) == len(frames), "none": int(e.counts[0]) == 0,
            "mixed": 256 < int(e.counts[0]) < len(frames) - 256}[kind]
    _check(oracle, frames, ifc, slotted=slotted, slot=128, e=e)


# ---- the tables ---------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [0, 1, 256])
def test_listener_tables(oracle, count):
    """0, 1 and 256 listeners. With 256: entry k listens on port 3000 + k // 2, the even ones on
    the interface's address and the odd ones on any, so that a specific entry stands in front of
    a wildcard on every port; the reversed table has the wildcard in front; the last entry alone
    matches port 9999."""
    ifc = C.iface()
    if count == 256:
        lis = [(C.LOCAL if k % 2 == 0 else 0, 3000 + k // 2, 500 + k) for k in range(255)] + [(0, 9999, 755)]
        ports = [3000 + k for k in range(0, 128, 5)] + [9999, 2999, 3128]
    else:
        lis = [(0, 80, 42)][:count]
        ports = [80, 81]
    frames = [R.frame(fl, src=C.PEER, dst=C.LOCAL, dport=p, sport=1000 + p) for p in ports
              for fl in (R.SYN, R.ACK, R.RST, R.SYN | R.ACK)]
    for table in (lis, lis[::-1]):
        for slotted in (False, True):
            e, _, _ = _check(oracle, frames, ifc, slotted=slotted, lis=table)
        if count == 256:
            syn = e.listener[::4]
            first = 500 if table is lis else 501
            assert int(syn[0]) == first and int(syn[-3]) == 755 and int(syn[-1]) == C.NO_LISTENER
            assert (e.status[::4][:-2] == C.SYN).all() and (e.status[::4][-2:] == C.RST).all()
        elif count == 1:
            assert e.status.tolist() == [C.SYN, C.RST, C.DROP, C.RST, C.RST, C.RST, C.DROP, C.RST]
        else:
            assert e.status.tolist() == [C.RST, C.RST, C.DROP, C.RST] * 2


@pytest.mark.parametrize("count", [0, 1, 4096])
def test_pcb_tables(oracle, count):
    table = C.pcb_table(count)
    frames = [C.rst_due(k) for k in range(40)] + [C.no_rst(k) for k in range(40)]
    for i in list(range(0, count, 97)) + ([count - 1] if count else []):
        frames += [C.pcb_frame(table, i), C.pcb_frame(table, i, R.SYN, data=b"xy")]
    frames.append(R.frame(R.ACK, src=0x0A141E01, dst=C.LOCAL, sport=19999, dport=5000))     # beside the table
    for slotted in (False, True):
        e, _, _ = _check(oracle, frames, C.iface(), slotted=slotted, pcbs=table if count else None)
    assert (e.status == C.PCB).sum() == (0 if not count else 2 * (len(range(0, count, 97)) + 1))
    assert e.status[-1] == C.RST


def test_rst_requests(oracle):
    """The host's requests: on a PCB frame, on a SYN a listener would take, on a frame that gets an
    RST anyway, on a bad source, on another host's segment and on frames without a record."""
    table = C.pcb_table(8)
    frames = [C.pcb_frame(table, 3), C.pcb_frame(table, 4), R.frame(R.SYN, src=C.PEER, dst=C.LOCAL, dport=80),
              R.frame(R.SYN, src=C.PEER, dst=C.LOCAL, dport=80), C.rst_due(1),
              R.frame(R.SYN, src=0xE0000001, dst=C.LOCAL), R.frame(R.SYN, src=0xFFFFFFFF, dst=C.LOCAL),
              R.frame(R.SYN, src=C.PEER, dst=C.LOCAL ^ 1), C.not_tcp(0), C.not_tcp(6),
              R.frame(R.RST, src=C.PEER, dst=C.LOCAL)]
    req = np.array([1, 0, 7, 0, 255, 1, 1, 1, 1, 1, 1], dtype=np.uint8)
    for slotted in (False, True):
        e, _, _ = _check(oracle, frames, C.iface(), slotted=slotted, pcbs=table, req=req)
        assert e.status.tolist() == [C.RST, C.PCB, C.RST, C.SYN, C.RST, C.DROP, C.DROP, C.NOT_LOCAL, C.NONE,
                                     C.NONE, C.RST]
        assert e.listener.tolist()[2:4] == [C.NO_LISTENER, 7]
        none, _, _ = _check(oracle, frames, C.iface(), slotted=slotted, pcbs=table, req=None)
        zero, _, _ = _check(oracle, frames, C.iface(), slotted=slotted, pcbs=table, req=np.zeros(11, np.uint8))
        assert none.status.tolist() == zero.status.tolist() == [C.PCB, C.PCB, C.SYN, C.SYN, C.RST, C.DROP,
                                                                C.DROP, C.NOT_LOCAL, C.NONE, C.NONE, C.DROP]


def test_ident_wraps(oracle):
    frames = [C.rst_due(0), C.no_rst(0), C.rst_due(1), C.rst_due(2), C.not_tcp(0), C.rst_due(3), C.rst_due(4)]
    e, _, _ = _check(oracle, frames, C.iface(ip_id=0xFFFE, ttl=255), slotted=True)
    assert [int.from_bytes(e.headers[i][18:20], "big") for i in sorted(e.headers)] == \
        [0xFFFE, 0xFFFF, 0, 1, 2]
    assert all(h[22] == 255 for h in e.headers.values())


# ---- seeded random batches ----------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(30))
def test_random_batches(oracle, seed):
    rng = np.random.default_rng(1000 + seed)
    table = C.pcb_table(int(rng.integers(0, 400)))
    frames, req = C.random_batch(seed, int(rng.integers(900, 1100)), table)
    ifc = C.iface(ip_id=int(rng.integers(0, 1 << 16)), ttl=int(rng.integers(1, 256)),
                  mtu=int(rng.integers(256, 1501)))
    lis = C.LISTENERS[:int(rng.integers(0, 5))]
    _check(oracle, frames, ifc, slotted=bool(seed & 1), pcbs=table if len(table) else None, lis=lis,
           req=req if seed % 3 else None, shift=8 * (seed % 2), seg_shift=8 * (seed // 2 % 2),
           slot=128 if seed % 4 == 1 else SLOT)


# ---- replay from a graph, with other inputs in place the second time ---------------------------

def test_graph_replay(oracle):
    ifc = C.iface(ip_id=77)
    first = [f + bytes(128 - len(f)) for f in C.sized_batch(513, "mixed")]
    lens = [len(f) for f in C.sized_batch(513, "mixed")]
    second = first[1:] + first[:1]                                        # every frame moves by one
    lay = TI.Layout(first, True, 128)
    n = len(first)
    o = Outputs(n)
    f = _np_iface(ifc)
    lis = _dev(A.tcp_listeners(C.LISTENERS))
    args = (lay.dev, 128, lay.lens, f, None, lis, None)
    kw = dict(tcp_ttl=ifc["ttl"], out=o.res, workspace=o.workspace)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.tcp_rx_respond_slotted(*args, **kw)                             # warm-up
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        A.tcp_rx_respond_slotted(*args, **kw)
    for frames, ln in ((first, lens), (second, lens[1:] + lens[:1]), (first, lens)):
        cut = [fr[:k] for fr, k in zip(frames, ln)]
        other = TI.Layout(cut, True, 128)
        lay.dev.copy_(other.dev)
        lay.lens.copy_(other.lens)
        lay.host = other.host
        o.poison()
        g.replay()
        _compare(C.respond(cut, C.verdicts_of(oracle, cut), ifc, None, C.LISTENERS), o, lay, n, 64)


# ---- the argument list, through the wrappers ---------------------------------------------------

def test_einval_paths():
    """What the wrappers let through to the library with device tensors; null pointers, counts and
    alignments are covered on host buffers in test_tcp_rsp_host.py."""
    fr = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    off = torch.tensor([0, 60, 120], dtype=torch.int64, device=DEV)
    lens = torch.tensor([60, 60], dtype=torch.int32, device=DEV)
    good = A.icmp_iface(C.LOCAL, C.LOCAL | 0xFF, R.LOCAL_MAC)
    assert A.tcp_rx_respond(fr, off, good).n == 2

    def rejected(call):
        with pytest.raises(A.ChksumError) as err:
            call()
        assert err.value.status == A.AIPSTACK_CHKSUM_EINVAL

    for change in (dict(flags=2), dict(mtu=255), dict(reserved=7)):
        bad = good.copy()
        for k, val in change.items():
            bad[k] = val
        rejected(lambda: A.tcp_rx_respond(fr, off, bad))
        rejected(lambda: A.tcp_rx_respond_slotted(fr, 2048, lens, bad))
    need = A.tcp_rx_respond_workspace_bytes(2)
    many = A.tcp_listeners([(0, 1 + k, k) for k in range(257)])
    for kw in (dict(hdr_stride=53), dict(tcp_ttl=0), dict(tcp_ttl=256), dict(listeners=many),
               dict(workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV)),
               dict(workspace=torch.empty(need + 8, dtype=torch.uint8, device=DEV)[4:])):
        rejected(lambda: A.tcp_rx_respond(fr, off, good, **kw))
        rejected(lambda: A.tcp_rx_respond_slotted(fr, 2048, lens, good, **kw))
    e = A.tcp_rx_respond(fr[:0], off[:1], good)                           # n == 0
    assert e.n == 0 and e.counts.cpu().tolist() == [0, 0]
    torch.cuda.synchronize()
    assert _lib.load().aipstack_chksum_last_hip_error() == 0
