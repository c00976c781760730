"""ARP on receive (aipstack_arp_rx_respond / _slotted) on the GPU against the model of
arp_cases.py, which test_arp_host.py pins to what the reference's own EthIpIface did with the
frames of tests/golden/arp_ref_cases.json.

Every comparison covers status, the records, hdr_len, the zero chunk index, both lists and the
counts, every header slot (a reply's 42 bytes, the zeros behind them, the pre-filled pattern
wherever the contract says untouched), the guard bytes in front of and behind every output, and
the frames themselves, over outputs that were dirty before the call."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import arp_cases as C
import arp_ref as R
import frame_cases as F
import icmp_cases as IC
import test_gpu_icmp as TI

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = 0xC3
GUARD = 64
SLOT = 2048


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


def _tune(key, value):
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == 0


def _np_iface(ifc):
    return A.arp_iface(ifc["local"], ifc["netmask"], ifc["mac"], have_addr=ifc["have"])


class Outputs:
    """An ArpResponses (`res`) of poisoned tensors, each between GUARD poisoned bytes of its own
    allocation; `shift` moves the header ring off its 64-byte boundary, `arp_shift` the records
    off their 16-byte boundary."""

    def __init__(self, n, hdr_stride=64, shift=0, arp_shift=0):
        self.raw = []

        def t(nbytes, dtype, off=0):
            raw = torch.full((GUARD + off + nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
            self.raw.append((raw, GUARD + off, nbytes))
            return raw[GUARD + off:GUARD + off + nbytes].view(dtype)

        self.workspace = t(A.arp_rx_respond_workspace_bytes(n), torch.uint8)
        self.res = A.ArpResponses(t(n * hdr_stride, torch.uint8, shift), hdr_stride, t(4 * n, torch.int32),
                                  t(8 * (n + 1), torch.int64), t(n, torch.uint8),
                                  t(16 * n, torch.uint8, arp_shift), t(8 * n, torch.int64),
                                  t(8 * n, torch.int64), t(16, torch.int64))
        assert self.res.headers.data_ptr() % 64 == shift % 64 and self.res.records.data_ptr() % 16 == arp_shift

    def guards_intact(self):
        for raw, at, nbytes in self.raw:
            assert bool((raw[:at] == POISON).all()) and bool((raw[at + nbytes:] == POISON).all())


def _compare(e, o, lay, n, hdr_stride):
    got = o.res
    torch.cuda.synchronize()
    assert got.n == n
    assert np.array_equal(got.status.cpu().numpy(), e.status)
    assert got.records.cpu().numpy().tobytes() == e.records.tobytes()
    assert np.array_equal(got.records_numpy(), e.records)
    assert np.array_equal(got.hdr_lens.cpu().numpy().view(np.uint32), e.hdr_len)
    assert np.array_equal(got.chunk_index.cpu().numpy().view(np.uint64), e.chunk_index)
    assert np.array_equal(got.reply_frame.cpu().numpy().view(np.uint64), e.reply_frame)
    assert np.array_equal(got.seen_frame.cpu().numpy().view(np.uint64), e.seen_frame)
    assert np.array_equal(got.counts.cpu().numpy().view(np.uint64), e.counts)
    ring = np.full((n, hdr_stride), POISON, dtype=np.uint8)
    if e.headers:
        rows = np.fromiter(e.headers.keys(), dtype=np.int64)
        ring[rows, :42] = np.frombuffer(b"".join(e.headers.values()), dtype=np.uint8).reshape(-1, 42)
        ring[rows, 42:min(hdr_stride, 64)] = 0
    assert got.headers.cpu().numpy().tobytes() == ring.tobytes()
    o.guards_intact()
    if lay is not None:
        assert np.array_equal(lay.dev.cpu().numpy(), lay.host)                # the frames: only read


def _call(lay, ifc, o):
    f = _np_iface(ifc)
    if lay.slotted:
        return A.arp_rx_respond_slotted(lay.dev, lay.slot, lay.lens, f, out=o.res, workspace=o.workspace)
    return A.arp_rx_respond(lay.dev, lay.offsets, f, out=o.res, workspace=o.workspace)


def _check(frames, ifc, *, slotted, hdr_stride=64, shift=0, arp_shift=0, slot=SLOT, e=None):
    e = C.respond(frames, ifc) if e is None else e
    lay = TI.Layout(frames, slotted, slot)
    o = Outputs(len(frames), hdr_stride, shift, arp_shift)
    got = _call(lay, ifc, o)
    assert got.headers is o.res.headers
    _compare(e, o, lay, len(frames), hdr_stride)
    return e, lay, o


def _linearised(e, res, n):
    """The replies as frames of a send ring, through both forms of the lineariser: the model's 42
    bytes at the repliers, nothing anywhere else."""
    ring = torch.full((n * 64,), POISON, dtype=torch.uint8, device=DEV)
    lin = A.tx_linearise_slotted(ring, 64, res, frame_max=64)
    torch.cuda.synchronize()
    reply = e.hdr_len != 0
    ls = lin.status.cpu().numpy()
    assert (ls[reply] == A.AIPSTACK_TX_LIN_WRITTEN).all() and (ls[~reply] == A.AIPSTACK_TX_LIN_SKIPPED).all()
    assert np.array_equal(lin.lens.cpu().numpy().view(np.uint32), e.hdr_len)
    want = np.full((n, 64), POISON, dtype=np.uint8)
    for i, h in e.headers.items():
        want[i, :42] = np.frombuffer(h, dtype=np.uint8)
    assert ring.cpu().numpy().tobytes() == want.tobytes()
    room = np.concatenate([[0], np.cumsum(e.hdr_len)]).astype(np.int64)
    flat = torch.full((int(room[-1]) + 1,), POISON, dtype=torch.uint8, device=DEV)
    lin2 = A.tx_linearise(flat, torch.from_numpy(room).to(DEV), res)
    assert (lin2.status.cpu().numpy()[reply] == A.AIPSTACK_TX_LIN_WRITTEN).all()
    assert flat.cpu().numpy().tobytes() == b"".join(e.headers[i] for i in sorted(e.headers)) + bytes([POISON])
    return [bytes(want[i, :42]) for i in sorted(e.headers)]


# ---- every fixture case, through both entry points and the lineariser --------------------------

@pytest.mark.parametrize("hdr_stride,shift,arp_shift", [(64, 0, 0), (64, 8, 4), (42, 0, 8), (128, 0, 12)])
@pytest.mark.parametrize("slotted", [False, True])
def test_fixture_cases(slotted, hdr_stride, shift, arp_shift):
    """The frames of each reference-recorded stack (/24, /30, no address) as one batch: in whole
    lines (64-byte slots on a 64-byte boundary, records on a 16-byte one) and in plain stores;
    linearised, the replies are the frames the reference sent, byte for byte."""
    replies = 0
    for stack in R.load():
        frames, ifc = C.stack_frames(stack), C.stack_iface(stack)
        e, _, o = _check(frames, ifc, slotted=slotted, hdr_stride=hdr_stride, shift=shift, arp_shift=arp_shift)
        sent = [f for c in stack["cases"] for f in C.sent(c["out"])]
        assert _linearised(e, o.res, len(frames)) == sent
        assert (len(sent) == 0) == (not stack["have"])
        replies += len(sent)
    assert replies >= 28


# ---- batch sizes: the lists across waves and blocks --------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("kind", ["all", "none", "no_arp", "mixed"])
def test_batch_sizes(n, kind):
    frames = C.sized_batch(n, kind)
    got = {}
    for slotted in (False, True):
        e, _, o = _check(frames, C.iface(), slotted=slotted, slot=128)
        got[slotted] = o.res.headers.cpu().numpy().tobytes()
    assert got[False] == got[True]
    assert int(e.counts[0]) == {"all": n, "none": 0, "no_arp": 0}.get(kind, int(e.counts[0]))
    if kind == "mixed" and n == 513:   # with at most two workgroups the passes loop over the tiles
        _tune("aux_blocks", 2)
        try:
            _check(frames, C.iface(), slotted=True, slot=128, e=e)
        finally:
            _tune("aux_blocks", -1)


def test_no_address_interface():
    """Without an address nothing replies and nothing may be created; the observers still hear."""
    frames = C.sized_batch(513, "mixed")
    for slotted in (False, True):
        e, _, _ = _check(frames, C.iface(have=False), slotted=slotted, slot=128)
        assert int(e.counts[0]) == 0 and int(e.counts[1]) > 100      # the requests and every third other frame
        assert not (e.records["flags"] & (C.NEW_OK | C.REC_REPLY)).any()
        assert (e.records["flags"] & C.NOTIFY).any()


# ---- among other traffic, and beside Rx verify -------------------------------------------------

def test_mixed_traffic_and_rx_verify(oracle):
    """ARP among the TCP / UDP / ICMP frames of frame_cases.frames: the same batch's Rx verify
    verdict for every ARP frame is DROP_NOT_IP4, and every other frame is _ARP_NONE."""
    n = 700
    fr = F.frames(seed=20261021, n=n)
    ifc = C.iface()
    arp_at = sorted({0, 63, 64, 255, 256, 699} | set(range(5, n, 7)))
    for k, i in enumerate(arp_at):
        fr[i] = (C.request(k, ifc), C.other(k, ifc), R.arp(1, 9, 9, plen=6))[k % 3]
    for slotted in (False, True):
        e, lay, _ = _check(fr, ifc, slotted=slotted)
        v = (A.rx_verify_slotted(lay.dev, lay.slot, lay.lens) if slotted
             else A.rx_verify(lay.dev, lay.offsets)).cpu().numpy()
        is_arp = e.status != C.NONE
        assert np.array_equal(np.flatnonzero(is_arp), np.array(arp_at))
        assert (v[is_arp] == 0).all() and len(set(v[~is_arp])) >= 6        # AIPSTACK_RX_DROP_NOT_IP4
        buf, off = F.pack(fr)
        assert np.array_equal(v, oracle.rx_verify_batch(buf, off))
    assert int(e.counts[0]) >= 30 and int(e.counts[1]) >= 60 and (e.status == C.MALFORMED).sum() >= 30


# ---- every frame alignment, with frames that end at the allocation's last byte -----------------

@pytest.mark.parametrize("align", range(16))
def test_frame_alignments_up_to_the_last_byte(align):
    """CSR frames from `align` bytes behind a 256-byte boundary, back to back, the last one (42
    bytes, a request) ending at the allocation's last byte; and slots of 42 bytes, whose starts
    take every residue, the last one ending there too."""
    ifc = C.iface()
    frames = [C.request(k, ifc, pad=k % 5) if k % 3 == 0 else (C.other(k, ifc), C.not_arp(k))[k % 2]
              for k in range(70)] + [R.arp(1, 7, ifc["local"])[:41], C.request(99, ifc, pad=0)]
    e = C.respond(frames, ifc)
    assert e.status[-1] == C.REPLY and e.status[-2] == C.MALFORMED
    lens = np.array([len(f) for f in frames], dtype=np.int64)
    total = int(lens.sum())
    host = np.frombuffer(b"".join(frames), dtype=np.uint8)
    alloc = torch.zeros(align + total, dtype=torch.uint8, device=DEV)
    assert alloc.data_ptr() % 256 == 0
    alloc[align:].copy_(torch.from_numpy(host.copy()))
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).to(DEV)
    o = Outputs(len(frames))
    A.arp_rx_respond(alloc[align:], off, _np_iface(ifc), out=o.res, workspace=o.workspace)
    _compare(e, o, None, len(frames), 64)
    assert np.array_equal(alloc[align:].cpu().numpy(), host)
    # slots of exactly 42 bytes
    reqs = [C.request(k, ifc, pad=0) if k % 2 else C.other(k, ifc)[:42] for k in range(40)]
    e = C.respond(reqs, ifc)
    ring = torch.zeros(align + 42 * len(reqs), dtype=torch.uint8, device=DEV)
    ring[align:].copy_(torch.from_numpy(np.frombuffer(b"".join(reqs), dtype=np.uint8).copy()))
    o = Outputs(len(reqs))
    A.arp_rx_respond_slotted(ring[align:], 42, torch.full((len(reqs),), 42, dtype=torch.int32, device=DEV),
                             _np_iface(ifc), out=o.res, workspace=o.workspace)
    _compare(e, o, None, len(reqs), 64)


# ---- slots: 128 bytes, and lengths that are clamped to the stride ------------------------------

def test_slot_lengths_are_clamped():
    """A length above the stride counts as the stride (as Rx verify clamps it): a 60-byte request
    in a 128-byte slot with length 5000 is still the request; in a 40-byte slot its length is 40,
    below an ARP packet, and nothing behind the slot's end is read as its bytes."""
    ifc = C.iface()
    frames = [C.request(k, ifc) for k in range(130)]
    lay = TI.Layout(frames, True, 128)
    lay.lens = torch.tensor([5000 if k % 2 else 60 for k in range(130)], dtype=torch.int32, device=DEV)
    o = Outputs(130)
    _call(lay, ifc, o)
    _compare(C.respond(frames, ifc), o, lay, 130, 64)
    # 40-byte slots: the next slot's bytes lie where the ARP packet would go on
    cut = [f[:40] for f in frames]
    lay = TI.Layout(cut, True, 40)
    lay.lens = torch.full((130,), 60, dtype=torch.int32, device=DEV)
    o = Outputs(130)
    _call(lay, ifc, o)
    e = C.respond(cut, ifc)
    assert (e.status == C.MALFORMED).all()
    _compare(e, o, lay, 130, 64)


# ---- several steps of the scan -----------------------------------------------------------------

_cache = {}


def _scan_batch():
    """131,917 frames: two whole steps of the one-workgroup scan (256 tiles of 256 frames each)
    and a part of a third (3 tiles and 77 frames). Step 0: repliers in its first and last tile,
    at lanes 0 and 63 and every 97th frame; step 1: every frame replies; the part: as step 0."""
    if "scan" not in _cache:
        n, step = 131917, 256 * 256
        ifc = C.iface()
        resp = np.zeros(n, dtype=bool)
        resp[step:2 * step] = True
        for lo, hi in ((0, step), (2 * step, n)):
            resp[lo:hi:97] = True
            for edge in (lo, hi - 256 if hi - lo >= 256 else lo):
                resp[[edge, min(edge + 63, hi - 1), min(edge + 64, hi - 1), min(edge + 255, hi - 1)]] = True
            resp[hi - 1] = True
        none = [C.other(1, ifc), C.other(2, ifc), R.arp(1, 5, 6)[:41], C.not_arp(0), C.not_arp(2)]
        fr = [C.request(i, ifc, pad=0) if resp[i] else none[i % 5] for i in range(n)]
        e = C.respond(fr, ifc)
        assert np.array_equal(e.hdr_len != 0, resp) and int(e.counts[1]) > int(e.counts[0]) > step
        _cache["scan"] = (fr, ifc, e)
    return _cache["scan"]


@pytest.mark.parametrize("slotted", [False, True])
def test_scan_over_several_steps(slotted):
    fr, ifc, e = _scan_batch()
    _check(fr, ifc, slotted=slotted, slot=64, e=e)


# ---- replay from a graph, with other inputs in place the second time ---------------------------

def test_graph_replay():
    ifc = C.iface()
    first = [f + bytes(60 - len(f)) if len(f) < 60 else f[:60] for f in C.sized_batch(513, "mixed")]
    second = first[1:] + first[:1]                                        # every frame moves by one
    lay = TI.Layout(first, True, 64)
    n = len(first)
    o = Outputs(n)
    f = _np_iface(ifc)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.arp_rx_respond_slotted(lay.dev, 64, lay.lens, f, out=o.res, workspace=o.workspace)   # warm-up
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        A.arp_rx_respond_slotted(lay.dev, 64, lay.lens, f, out=o.res, workspace=o.workspace)
    r = o.res
    for frames in (first, second, first):
        other = TI.Layout(frames, True, 64)
        lay.dev.copy_(other.dev)
        lay.host = other.host
        for t in (r.hdr_lens, r.chunk_index, r.status, r.records, r.reply_frame, r.seen_frame, r.counts,
                  o.workspace, r.headers):
            t.view(torch.uint8).fill_(POISON)
        g.replay()
        _compare(C.respond(frames, ifc), o, lay, n, 64)


# ---- an ARP request, then an echo request from the same peer -----------------------------------

def test_arp_then_echo_yields_the_reference_frames(oracle):
    """The fixture case that records the sequence: the batch [ARP request, echo request] through
    arp_rx_respond and icmp_rx_respond, each linearised, gives the two frames the reference sent
    (its echo reply left for the MAC it had just learned, which is the request's Ethernet source)."""
    stack = R.load()[0]
    case, = [c for c in stack["cases"] if c["name"] == "arp_then_echo_one_peer"]
    frames = [bytes.fromhex(case["in"]), bytes.fromhex(case["probe"])]
    want = C.sent(case["out"]) + C.sent(case["probe_out"])
    assert len(want) == 2 and want[0][12:14] == b"\x08\x06" and want[1][12:14] == b"\x08\x00"
    lay = TI.Layout(frames, False)
    arp = A.arp_rx_respond(lay.dev, lay.offsets, _np_iface(C.stack_iface(stack)))
    assert arp.status.cpu().tolist() == [C.REPLY, C.NONE]
    icmp = A.icmp_rx_respond(lay.dev, lay.offsets,
                             A.icmp_iface(stack["addr"], stack["addr"] | 0xFF, bytes.fromhex(stack["mac"])))
    assert icmp.status.cpu().tolist() == [IC.NONE, IC.ECHO_REPLY] and icmp.verdict.cpu().tolist() == [0, 6]
    out = []
    for seg in (arp, icmp):
        ring = torch.zeros(2 * 128, dtype=torch.uint8, device=DEV)
        lin = A.tx_linearise_slotted(ring, 128, seg, frame_max=128)
        lens, h = lin.lens.cpu().numpy(), ring.cpu().numpy().reshape(2, 128)
        out += [h[i, :lens[i]].tobytes() for i in range(2) if lens[i]]
    assert out == want


# ---- the argument list, through the wrappers ---------------------------------------------------

def test_einval_paths():
    """What the wrappers let through to the library with device tensors: the interface, the header
    stride, the workspace, every alignment, the slot stride. Null pointers and n > 2^40 are
    rejected before any HIP call and are covered, with the rest again, on host buffers in
    test_arp_host.py (test_csr_einval_before_any_hip_call and its neighbours)."""
    fr = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    off = torch.tensor([0, 60, 120], dtype=torch.int64, device=DEV)
    lens = torch.tensor([60, 60], dtype=torch.int32, device=DEV)
    good = A.arp_iface(0x0A141E28, 0xFFFFFF00, R.LOCAL_MAC)
    assert A.arp_rx_respond(fr, off, good).n == 2

    def rejected(call):
        with pytest.raises(A.ChksumError) as err:
            call()
        assert err.value.status == A.AIPSTACK_CHKSUM_EINVAL

    for change in (dict(flags=2), dict(flags=0x81), dict(reserved=7)):
        bad = good.copy()
        for k, val in change.items():
            bad[k] = val
        rejected(lambda: A.arp_rx_respond(fr, off, bad))
        rejected(lambda: A.arp_rx_respond_slotted(fr, 2048, lens, bad))
    need = A.arp_rx_respond_workspace_bytes(2)
    for kw in (dict(hdr_stride=41), dict(workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV)),
               dict(workspace=torch.empty(need + 8, dtype=torch.uint8, device=DEV)[4:])):
        rejected(lambda: A.arp_rx_respond(fr, off, good, **kw))
        rejected(lambda: A.arp_rx_respond_slotted(fr, 2048, lens, good, **kw))
    for name, by in (("records", 2), ("hdr_lens", 2), ("chunk_index", 4), ("reply_frame", 4),
                     ("seen_frame", 4), ("counts", 4)):
        o = Outputs(2)
        t = getattr(o.res, name)
        raw = torch.empty(t.numel() * t.element_size() + 16, dtype=torch.uint8, device=DEV)
        moved = torch.as_strided(raw, (t.numel() * t.element_size(),), (1,), by)
        assert moved.data_ptr() % 8 == by
        lib = _lib.load()
        ptr = {k: getattr(o.res, k).data_ptr() for k in ("status", "records", "headers", "hdr_lens",
                                                       "chunk_index", "reply_frame", "seen_frame", "counts")}
        ptr[name] = moved.data_ptr()
        st = lib.aipstack_arp_rx_respond(fr.data_ptr(), off.data_ptr(), 2, good.ctypes.data, ptr["status"],
                                         ptr["records"], ptr["headers"], 64, ptr["hdr_lens"],
                                         ptr["chunk_index"], ptr["reply_frame"], ptr["seen_frame"],
                                         ptr["counts"], o.workspace.data_ptr(), need, None)
        assert st == A.AIPSTACK_CHKSUM_EINVAL, name
    rejected(lambda: _lib_slot_stride(fr, lens, good))
    e = A.arp_rx_respond(fr[:0], off[:1], good)                           # n == 0
    assert e.n == 0 and e.counts.cpu().tolist() == [0, 0]
    torch.cuda.synchronize()
    assert _lib.load().aipstack_chksum_last_hip_error() == 0


def _lib_slot_stride(fr, lens, good):
    """A slot stride above the bound, which the wrapper's own size check would not let through."""
    o = Outputs(2)
    r = o.res
    st = _lib.load().aipstack_arp_rx_respond_slotted(
        fr.data_ptr(), 65537, lens.data_ptr(), 2, good.ctypes.data, r.status.data_ptr(),
        r.records.data_ptr(), r.headers.data_ptr(), 64, r.hdr_lens.data_ptr(), r.chunk_index.data_ptr(),
        r.reply_frame.data_ptr(), r.seen_frame.data_ptr(), r.counts.data_ptr(), o.workspace.data_ptr(),
        A.arp_rx_respond_workspace_bytes(2), None)
    if st != 0:
        raise A.ChksumError(st, "aipstack_arp_rx_respond_slotted")
