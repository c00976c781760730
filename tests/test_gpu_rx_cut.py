"""Every receive entry point, in its CSR and its ring-slot form, on the three families of
rx_cut_cases.py: a frame's result depends only on the bytes inside its length, and it is right at
every length. test_rx_cut_cases.py shows on the CPU that the inputs are not vacuous.

Each run compares every output of the call whole with the model (through the comparison of the
stage's own GPU test: verdicts, statuses, records, the compacted lists with their filler, the counts,
the header ring with the poison of the slots without a reply), over poisoned outputs between guard
bytes, and the frames are unchanged afterwards. Families A and B hold both tails of every frame in
one batch: the two entries' per-frame outputs are asserted equal directly (of a reply all bytes but
the Ident and the header checksum, which count the replies in front of it). Family C runs twice on
one device buffer, the second time with every byte outside the frames inverted: every output
tensor is byte-identical. The replies of families A and B (ICMP echo and unreachable, TCP RST, ARP)
go back through rx_verify, the ARP replies through arp_rx_respond as well: each is an accepted
frame, or a well-formed ARP reply.

No entry point takes a verdict from its caller: each runs Rx verify itself and returns the
verdict, which is compared with the frame oracle's like every other output."""
import numpy as np
import pytest

import aipstack_amd as A

import frame_cases as F
import rx_cut_cases as X

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ipreass_gpu as H            # noqa: E402
import test_gpu_arp as TA          # noqa: E402
import test_gpu_icmp as TI         # noqa: E402
import test_gpu_icmp_du as TD      # noqa: E402
import test_gpu_tcp_rsp as TR      # noqa: E402
import test_gpu_tcprx as TT        # noqa: E402
import test_gpu_udprx as TU        # noqa: E402

DEV = "cuda"
POISON, GUARD = 0xC3, 64


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


class OnDevice:
    """A layout of rx_cut_cases.lay_out on the device, with the names the stages' own GPU tests
    give a layout: dev / host (what the call gets: in the slotted form the buffer from its first
    slot on, behind the guard area), start (per entry, in dev), offsets or lens, slot."""

    def __init__(self, lay):
        self.lay, self.slotted, self.slot, self.n = lay, lay.slotted, lay.stride, len(lay.frames)
        self.full = torch.from_numpy(lay.host).to(DEV)
        first = X.GUARD if lay.slotted else 0
        self.dev, self.host, self.start = self.full[first:], lay.host[first:], lay.start - first
        if lay.slotted:
            self.lens = torch.from_numpy(lay.lens.astype(np.int32)).to(DEV)
        else:
            self.offsets = torch.from_numpy(lay.offsets.astype(np.int64)).to(DEV)
        self.addr = np.uint64(self.dev.data_ptr()) + self.start.astype(np.uint64)

    def where(self):
        return (self.dev, self.slot, self.lens) if self.slotted else (self.dev, self.offsets)

    def load(self, lay):
        """Another layout of the same frames into the same device bytes."""
        assert lay.host.size == self.lay.host.size and np.array_equal(lay.lens, self.lay.lens)
        self.full.copy_(torch.from_numpy(lay.host).to(DEV))
        self.lay = lay
        self.host = lay.host[X.GUARD if lay.slotted else 0:]

    def unchanged(self):
        assert np.array_equal(self.full.cpu().numpy(), self.lay.host)


class IcmpOutputs:
    """An IcmpResponses (`res`) of poisoned tensors, each between GUARD poisoned bytes of its own
    allocation (as test_gpu_tcp_rsp.Outputs)."""

    def __init__(self, n, hdr_stride=64):
        self.raw = []

        def t(nbytes, dtype):
            raw = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
            self.raw.append((raw, GUARD, nbytes))
            return raw[GUARD:GUARD + nbytes].view(dtype)

        self.workspace = t(A.icmp_rx_respond_workspace_bytes(n), torch.uint8)
        self.res = A.IcmpResponses(t(n * hdr_stride, torch.uint8), hdr_stride, t(4 * n, torch.int32),
                                   t(8 * n, torch.int64), t(4 * n, torch.int32), t(8 * (n + 1), torch.int64),
                                   t(n, torch.uint8), t(n, torch.uint8), t(8 * n, torch.int64), t(16, torch.int64))

    guards_intact = TR.Outputs.guards_intact


def _np(t):
    return t.cpu().numpy().view(np.uint8).copy()


def _masked(ring, n, stride, ipv4=True):
    """The header ring as rows, without what depends on the replies in front: Ident and header
    checksum."""
    r = ring.reshape(n, stride).copy()
    if ipv4:
        r[:, 18:20] = 0
        r[:, 24:26] = 0
    return r


# ---- one run per stage: (every output tensor as bytes, the per-frame outputs as rows) -------------

def _verify(st, d, e):
    g = TT.Guarded(d.n)
    got = A.rx_verify_slotted(*d.where(), out=g.view) if d.slotted else A.rx_verify(*d.where(), out=g.view)
    v = _np(g.view)
    assert got.data_ptr() == g.view.data_ptr() and np.array_equal(v, e.verdict) and g.intact()
    return {"verdict": v}, {"verdict": v}


def _tcprx(st, d, e):
    o = TT.Outputs(d.n)
    tbl = A.tcp_pcb_table_sort(st.pcbs)
    res = (A.tcp_rx_parse_slotted if d.slotted else A.tcp_rx_parse)(*d.where(), tbl, **o.kw())
    TT._compare(e, o)
    assert res.n == d.n
    v, s, p = (np.frombuffer(x, dtype=np.uint8) for x in o.bytes())
    return {"verdict": v, "segs": s, "pcb": p}, {"verdict": v, "segs": s.reshape(-1, 32), "pcb": p.reshape(-1, 4)}


def _reass(st, d, e):
    o = H.Outputs(d.n)
    res = (A.ip4_rx_reassemble_slotted if d.slotted else A.ip4_rx_reassemble)(*d.where(), **o.kw())
    H.compare(e, o, d.addr)
    assert res.n == d.n
    snap = {k: np.frombuffer(x, dtype=np.uint8) for (k, _), x in zip(H.Outputs.SIZES, o.bytes())}
    dg = snap["dgram"].reshape(-1, 16)
    rows = {"verdict": snap["verdict"], "chunk_len": snap["chunk_len"].reshape(-1, 4),
            "dgram": np.concatenate([dg[:, :4], dg[:, 8:12]], axis=1)}      # all but the last frame's index
    return snap, rows


def _icmp(st, d, e):
    o = IcmpOutputs(d.n)
    codes = torch.tensor(st.codes_of(d.lay.frames), dtype=torch.uint8, device=DEV)
    call = A.icmp_rx_respond_slotted if d.slotted else A.icmp_rx_respond
    got = call(*d.where(), TI._np_iface(st.ifc), codes, out=o.res, workspace=o.workspace)
    TI._compare(e, got, d, d.lay.frames, 64)
    o.guards_intact()
    r = o.res
    snap = {k: _np(getattr(r, k)) for k in ("headers", "hdr_lens", "chunk_addr", "chunk_len", "chunk_index",
                                            "status", "verdict", "response_frame", "counts")}
    rows = {"status": snap["status"], "verdict": snap["verdict"], "hdr_lens": snap["hdr_lens"].reshape(-1, 4),
            "headers": _masked(snap["headers"], d.n, 64)}
    return snap, rows


def _udp(st, d, e):
    o = TU.Guarded(d.n)
    kw = dict(verdict=o.verdict, dgrams=o.dgrams, unreach_code=o.unreach, deliver_frame=o.deliver_frame,
              counts=o.counts, workspace=o.workspace)
    call = A.udp_rx_demux_slotted if d.slotted else A.udp_rx_demux
    got = call(*d.where(), TU._np_iface(st.ifc), st.assocs, st.listeners, **kw)
    TU._compare(e, o, d)
    assert got.n == d.n
    snap = {k: _np(getattr(o, k)) for k in ("verdict", "dgrams", "unreach", "deliver_frame", "counts")}
    return snap, {"verdict": snap["verdict"], "dgrams": snap["dgrams"].reshape(-1, 32), "unreach": snap["unreach"]}


def _arp(st, d, e):
    o = TA.Outputs(d.n)
    TA._call(d, st.ifc, o)
    TA._compare(e, o, d, d.n, 64)
    r = o.res
    snap = {k: _np(getattr(r, k)) for k in ("headers", "hdr_lens", "chunk_index", "status", "records",
                                            "reply_frame", "seen_frame", "counts")}
    rows = {"status": snap["status"], "records": snap["records"].reshape(-1, 16),
            "hdr_lens": snap["hdr_lens"].reshape(-1, 4), "headers": _masked(snap["headers"], d.n, 64, ipv4=False)}
    return snap, rows


def _tcprsp(st, d, e):
    o = TR.Outputs(d.n)
    TR._call(d, st.ifc, o, A.tcp_pcb_table_sort(st.pcbs), st.lis, None)
    TR._compare(e, o, d, d.n, 64)
    r = o.res
    snap = {k: _np(getattr(r, k)) for k in ("headers",) + TR._OUTS}
    rows = {"verdict": snap["verdict"], "segs": snap["segs"].reshape(-1, 32), "pcb": snap["pcb"].reshape(-1, 4),
            "status": snap["status"], "listener": snap["listener"].reshape(-1, 4),
            "hdr_lens": snap["hdr_lens"].reshape(-1, 4), "headers": _masked(snap["headers"], d.n, 64)}
    return snap, rows


def _icmpdu(st, d, e):
    o = TD.Guarded(d.n)
    kw = dict(verdict=o.verdict, status=o.status, records=o.records, pcb_frame=o.pcb_frame, counts=o.counts,
              workspace=o.workspace)
    call = A.icmp_rx_unreach_slotted if d.slotted else A.icmp_rx_unreach
    got = call(*d.where(), TD._np_iface(st.ifc), TD._sorted(st.pcbs), **kw)
    assert got.n == d.n
    TD._compare(e, o, d)
    snap = {k: _np(getattr(o, k)) for k in TD.Guarded.NAMES}
    return snap, {"verdict": snap["verdict"], "status": snap["status"], "records": snap["records"].reshape(-1, 32)}


RUN = {"rx_verify": _verify, "tcp_rx_parse": _tcprx, "ip4_rx_reassemble": _reass, "icmp_rx_respond": _icmp,
       "udp_rx_demux": _udp, "arp_rx_respond": _arp, "tcp_rx_respond": _tcprsp, "icmp_rx_unreach": _icmpdu}


# ---- the replies, back through the receive path ---------------------------------------------------

def _replies(st, d, snap):
    """The frames the stage's header ring and chunk table stand for, from the device's outputs."""
    n = d.n
    ring = snap["headers"].reshape(n, 64)
    lens = snap["hdr_lens"].view(np.uint32)
    out = []
    for i in np.flatnonzero(lens):
        f = ring[i, :lens[i]].tobytes()
        if "chunk_addr" in snap:
            ci = snap["chunk_index"].view(np.uint64)
            for c in range(int(ci[i]), int(ci[i + 1])):
                at = int(snap["chunk_addr"].view(np.uint64)[c]) - d.dev.data_ptr()
                f += d.host[at:at + int(snap["chunk_len"].view(np.uint32)[c])].tobytes()
        out.append(f)
    return out


def _replies_are_valid(st, d, snap):
    frames = _replies(st, d, snap)
    assert len(frames) == int(snap["counts"].view(np.uint64)[0]) and len(frames) >= 4
    assert all(len(f) >= st.header for f in frames)
    buf, off = F.pack(frames)
    dbuf, doff = torch.from_numpy(buf).to(DEV), torch.from_numpy(off.view(np.int64)).to(DEV)
    v = A.rx_verify(dbuf, doff).cpu().numpy()
    if st.name != "arp_rx_respond":
        assert (v == 6).all(), np.flatnonzero(v != 6)[:8]                  # AIPSTACK_RX_ACCEPT
        return
    assert (v == 0).all()
    back = A.arp_rx_respond(dbuf, doff, TA._np_iface(st.ifc))
    assert (back.status.cpu().numpy() == A.AIPSTACK_ARP_SEEN).all()
    rec = back.records_numpy()
    assert (rec["op"] == 2).all() and (rec["sender_addr"] == st.ifc["local"]).all()


# ---- the tests ------------------------------------------------------------------------------------

_e = {}


def _expected(oracle, name, family, slotted):
    """(batch, layout, the model's Expected): computed once per module and left unchanged."""
    key = (name, family, slotted)
    if key not in _e:
        b = X.cached(oracle, name, family)
        lay = X.lay_out(b, slotted)
        _e[key] = (b, lay, X.STAGES[name].expect(oracle, lay.frames))
    return _e[key]


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("slotted", [False, True], ids=["csr", "slotted"])
@pytest.mark.parametrize("name", list(X.STAGES))
def test_every_length_and_both_tails(oracle, name, slotted, family):
    st = X.STAGES[name]
    b, lay, e = _expected(oracle, name, family, slotted)
    d = OnDevice(lay)
    snap, rows = RUN[name](st, d, e)
    d.unchanged()
    case = np.arange(len(b.cases))
    one = lay.index
    two = lay.index[np.asarray(b.partner)]
    if name == "ip4_rx_reassemble" and not slotted:
        # the whole members of a train answer for the train, and in the CSR form a tail is an entry
        # of the batch: a member's own continuation from k = 0 is that member once more
        case, one, two = case[b.seed >= 0], one[b.seed >= 0], two[b.seed >= 0]
    for k, r in rows.items():
        bad = np.flatnonzero((r[one] != r[two]).reshape(len(one), -1).any(axis=1))
        assert bad.size == 0, (k, bad[:8], [(len(b.cases[i][0]), int(b.variant[i])) for i in case[bad[:8]]])
    if getattr(st, "has_headers", False):
        _replies_are_valid(st, d, snap)


@pytest.mark.parametrize("slotted", [False, True], ids=["csr", "slotted"])
@pytest.mark.parametrize("name", list(X.STAGES))
def test_bytes_outside_the_frames_change_nothing(oracle, name, slotted):
    st = X.STAGES[name]
    b, lay, e = _expected(oracle, name, "C", slotted)
    d = OnDevice(lay)
    first, _ = RUN[name](st, d, e)
    d.unchanged()
    other = X.lay_out(b, slotted, alt=True)
    d.load(other)
    second, _ = RUN[name](st, d, st.expect(oracle, other.frames))
    d.unchanged()
    assert first.keys() == second.keys()
    for k in first:
        assert np.array_equal(first[k], second[k]), k
