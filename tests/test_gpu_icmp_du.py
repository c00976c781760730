"""Received ICMP Destination Unreachable (aipstack_icmp_rx_unreach / _slotted) on the GPU against
the model of icmp_du_cases.py, which test_icmp_du_host.py pins to the handler calls recorded from
the reference's own stack; verdicts from the frame oracle.

Every comparison is byte for byte and covers the verdicts, the statuses, the records, the list of
frames with a PCB with its ~0 tail and the counts, over outputs that were poisoned before the call
and lie between guard bytes that must come back untouched (the workspace's too), and the frames
themselves, which are only read."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import icmp_du_cases as C
import icmp_du_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = 0xC3
GUARD = 64
KEY, RECORD = A.TCP_PCB_KEY_DTYPE, A.ICMP_DU_RECORD_DTYPE


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


def _tune(key, value):
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == 0


def _np_iface(ifc):
    return A.icmp_iface(ifc["local"], ifc["bcast"], ifc["mac"])


def _sorted(table):
    return None if table is None or len(table) == 0 else A.tcp_pcb_table_sort(table)


class Layout:
    """The frames on the device: CSR (back to back, the first at byte `lead`) or ring slots."""

    def __init__(self, frames, slotted, *, slot=2048, lead=1):
        n = len(frames)
        self.slotted, self.n, self.slot = slotted, n, slot
        ln = np.array([len(f) for f in frames], dtype=np.int64)
        if slotted:
            self.start = np.arange(n, dtype=np.int64) * slot
            host = np.full(n * slot, 0x5C, dtype=np.uint8)
            self.lens = torch.from_numpy(ln.astype(np.int32)).to(DEV)
        else:
            self.start = lead + np.concatenate([[0], np.cumsum(ln)[:-1]])
            host = np.full(lead + int(ln.sum()) + 64, 0x5C, dtype=np.uint8)
            off = np.concatenate([self.start, [lead + int(ln.sum())]]).astype(np.int64)
            self.offsets = torch.from_numpy(off).to(DEV)
        for i, f in enumerate(frames):
            host[self.start[i]:self.start[i] + len(f)] = np.frombuffer(f, dtype=np.uint8)
        self.host = host
        self.dev = torch.from_numpy(host).to(DEV)

    def call(self, ifc, pcbs, out, **kw):
        kw = dict(verdict=out.verdict, status=out.status, records=out.records, pcb_frame=out.pcb_frame,
                  counts=out.counts, workspace=out.workspace, **kw)
        if self.slotted:
            return A.icmp_rx_unreach_slotted(self.dev, self.slot, self.lens, _np_iface(ifc), pcbs, **kw)
        return A.icmp_rx_unreach(self.dev, self.offsets, _np_iface(ifc), pcbs, **kw)


class Guarded:
    """The outputs and the workspace of one call, each a poisoned view between two guards of its
    own poisoned buffer; `record_shift` 8 puts d_records on an 8-byte boundary that is no 16-byte
    boundary (the plain-store path)."""

    NAMES = ("verdict", "status", "records", "pcb_frame", "counts")

    def __init__(self, n, record_shift=0):
        self.bufs = {}

        def view(name, nbytes, shift=0):
            b = torch.full((GUARD + shift + nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
            assert b.data_ptr() % 16 == 0
            self.bufs[name] = (b, GUARD + shift, nbytes)
            return b[GUARD + shift:GUARD + shift + nbytes]

        self.verdict = view("verdict", n)
        self.status = view("status", n)
        self.records = view("records", n * 32, record_shift)
        self.pcb_frame = view("pcb_frame", n * 8).view(torch.int64)
        self.counts = view("counts", 16).view(torch.int64)
        self.workspace = view("workspace", A.icmp_rx_unreach_workspace_bytes(n))

    def poison(self):
        for b, _, _ in self.bufs.values():
            b.fill_(POISON)

    def guards_intact(self):
        for name, (b, at, nbytes) in self.bufs.items():
            h = b.cpu().numpy()
            assert (h[:at] == POISON).all() and (h[at + nbytes:] == POISON).all(), name

    def bytes(self):
        return b"".join(getattr(self, k).cpu().numpy().tobytes() for k in self.NAMES)


def _compare(e, out, lay, *, pcb=True):
    torch.cuda.synchronize()
    assert np.array_equal(out.verdict.cpu().numpy(), e.verdict)
    got = out.records.cpu().numpy().view(RECORD)
    if pcb:
        assert np.array_equal(out.status.cpu().numpy(), e.status)
        assert got.tobytes() == e.records.tobytes(), np.flatnonzero(got != e.records)[:8]
        assert np.array_equal(out.pcb_frame.cpu().numpy().view(np.uint64), e.pcb_frame)
        assert np.array_equal(out.counts.cpu().numpy().view(np.uint64), e.counts)
    else:  # an unsorted table: everything but what the search decides
        for name in RECORD.names:
            if name != "pcb":
                assert np.array_equal(got[name], e.records[name]), name
        assert int(out.counts.cpu().numpy().view(np.uint64)[1]) == int(e.counts[1])
    out.guards_intact()
    if lay is not None:
        assert np.array_equal(lay.dev.cpu().numpy(), lay.host)               # the frames: only read


def _check(frames, verdicts, ifc, table, *, slotted, record_shift=0, **lay_kw):
    e = C.expected(frames, verdicts, ifc, table)
    lay = Layout(frames, slotted, **lay_kw)
    out = Guarded(len(frames), record_shift)
    got = lay.call(ifc, _sorted(table), out)
    assert got.n == len(frames) and got.records.data_ptr() == out.records.data_ptr()
    assert got.records.data_ptr() % 16 == record_shift
    _compare(e, out, lay)
    return e, lay, out


_cache = {}


def _cached(oracle, key, make):
    if key not in _cache:
        fr = make()
        _cache[key] = (fr, C.verdicts_of(oracle, fr))
    return _cache[key]


def _fixture(oracle):
    if "fixture" not in _cache:
        out = []
        for s in R.load():
            fr = C.stack_frames(s)
            t = np.array([(s["addr"], R.FAR, 5000, 80, 77), (0xC0A80909, R.FAR, 5000, 80, 78),
                          (s["addr"], R.FAR, 5000, 53, 79)], dtype=KEY)
            out.append((s, fr, C.verdicts_of(oracle, fr), C.stack_iface(s), t))
        _cache["fixture"] = out
    return _cache["fixture"]


# ---- the fixture's frames, without and with their connections in the table ----------------------

@pytest.mark.parametrize("record_shift", [0, 8])
@pytest.mark.parametrize("slotted", [False, True])
def test_fixture_cases(oracle, slotted, record_shift):
    for s, fr, v, ifc, t in _fixture(oracle):
        e0, _, _ = _check(fr, v, ifc, None, slotted=slotted, record_shift=record_shift)
        e1, _, _ = _check(fr, v, ifc, t, slotted=slotted, record_shift=record_shift)
        assert int(e0.counts[0]) == 0 and int(e1.counts[0]) >= 25
        assert e0.counts[1] == e1.counts[1] >= 60
        assert set(np.unique(e1.status)) >= {C.NONE, C.PARSED, C.TCP_PCB}


# ---- batch sizes: the compaction's block edges and the ~0 tail ---------------------------------

@pytest.mark.parametrize("n,cap", [(1, -1), (255, -1), (256, -1), (257, -1), (513, -1), (513, 1)])
def test_batch_sizes(oracle, n, cap):
    """PCB hits at frames 0, 255, 256 and n - 1: a block's first and last frame. 513 frames are
    three tiles, the last of one frame; with one workgroup ("aux_blocks") the decide and emit
    passes loop over the tiles."""
    table = C.pcb_table(64)
    hits = [i for i in (0, 255, 256, n - 1) if i < n]
    fr, v = _cached(oracle, ("sizes", n), lambda: C.sized_batch(n, table, hits))
    _tune("aux_blocks", cap)
    try:
        for slotted in (False, True):
            e, _, _ = _check(fr, v, C.iface(), table, slotted=slotted)
    finally:
        _tune("aux_blocks", -1)
    assert e.pcb_frame[:int(e.counts[0])].tolist() == sorted(set(hits))
    assert (e.pcb_frame[int(e.counts[0]):] == C.NO_FRAME).all()


@pytest.mark.parametrize("slotted", [False, True])
def test_every_frame_has_a_pcb(oracle, slotted):
    table = C.pcb_table(64)
    fr, v = _cached(oracle, "all", lambda: C.sized_batch(513, table, range(513)))
    e, _, _ = _check(fr, v, C.iface(), table, slotted=slotted)
    assert e.counts.tolist() == [513, 513] and e.pcb_frame.tolist() == list(range(513))


# ---- table sizes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n_pcbs", [0, 1, 2, 3, 4096])
def test_table_sizes(oracle, n_pcbs):
    """Messages about every entry of the first and the last group of eight of the full table
    (whose entries differ in remote_port, local_port or remote_addr alone), about the sorted
    table's first and last entry, and near misses of each in every field: found exactly when the
    table in use holds the connection."""
    full = C.pcb_table(4096)
    order = A.tcp_pcb_table_sort(full)["cookie"].astype(np.int64) - 1000
    picks = sorted(set(range(8)) | set(range(4088, 4096)) | {int(i) for i in order[:3]} | {int(order[-1])} |
                   set(range(0, 4096, 97)))

    def make():
        out = []
        for i in picks:
            out.append(C.frag_needed(C.key_of(full, i), seq=i))
            out += [C.frag_needed(C.near_miss(full, i, k)) for k in range(4)]
        return out
    fr, v = _cached(oracle, "tables", make)
    # the table in use: the sorted table's first entries, so that its own first and last are hit
    table = full[np.sort(order[:n_pcbs])] if n_pcbs else None
    for slotted in (False, True):
        e, _, _ = _check(fr, v, C.iface(), table, slotted=slotted)
    have = set() if table is None else set(table["cookie"].tolist())
    found = set(e.records["pcb"][e.status == C.TCP_PCB].tolist())
    assert found == {1000 + i for i in picks} & have and int(e.counts[1]) == len(fr)
    if n_pcbs:
        s = A.tcp_pcb_table_sort(table)
        assert {int(s["cookie"][0]), int(s["cookie"][-1])} <= found
    # the table on the device already, as a tensor
    if n_pcbs == 4096:
        dev_tbl = torch.from_numpy(_sorted(table).view(np.uint8).copy()).to(DEV)
        lay, out = Layout(fr, False), Guarded(len(fr))
        lay.call(C.iface(), dev_tbl, out)
        _compare(e, out, lay)


@pytest.mark.parametrize("slotted", [False, True])
def test_unsorted_table_stays_inside_it(oracle, slotted):
    """The table lies between guards of entries that would match; pcb is unspecified, every other
    field of the records is the model's, and nothing outside the outputs is written."""
    full = C.pcb_table(1024)
    fr, v = _cached(oracle, "unsorted", lambda: [C.frag_needed(C.key_of(full, i)) for i in range(0, 1024, 3)])
    rng = np.random.default_rng(7)
    mixed = full[rng.permutation(len(full))]
    e = C.expected(fr, v, C.iface(), full)
    dev_tbl = torch.from_numpy(mixed.view(np.uint8).copy()).to(DEV)
    lay, out = Layout(fr, slotted), Guarded(len(fr))
    lay.call(C.iface(), dev_tbl, out)
    _compare(e, out, lay, pcb=False)
    got = out.records.cpu().numpy().view(RECORD)["pcb"]
    assert set(got.tolist()) <= set(full["cookie"].tolist()) | {C.NO_PCB}    # only entries of the table
    st = out.status.cpu().numpy()
    assert set(st.tolist()) <= {C.TCP_PCB, C.TCP_NO_PCB} and ((got != C.NO_PCB) == (st == C.TCP_PCB)).all()
    assert np.array_equal(dev_tbl.cpu().numpy(), mixed.view(np.uint8))


# ---- a random batch, and the same frames through the ICMP responder --------------------------------

def test_random_batch_and_the_icmp_responder(oracle):
    """2048 frames, one in four a Destination Unreachable with random quoted fields among the UDP,
    TCP, ARP and echo frames of the other case modules. No frame has both a response from
    aipstack_icmp_rx_respond and a valid record here."""
    table = C.pcb_table(64)
    fr, v = _cached(oracle, "random", lambda: C.random_batch(20261021, 2048, table))
    for slotted in (False, True):
        e, lay, out = _check(fr, v, C.iface(), table, slotted=slotted)
    assert set(np.unique(e.status)) == {C.NONE, C.PARSED, C.TCP_NO_PCB, C.TCP_PCB}
    resp = A.icmp_rx_respond_slotted(lay.dev, lay.slot, lay.lens, _np_iface(C.iface()))
    torch.cuda.synchronize()
    st = resp.status.cpu().numpy()
    assert (st == A.AIPSTACK_ICMP_ECHO_REPLY).sum() >= 50
    assert (st[e.status != C.NONE] == A.AIPSTACK_ICMP_NONE).all() and not resp.hdr_lens.cpu().numpy()[e.status != C.NONE].any()
    assert np.array_equal(resp.verdict.cpu().numpy(), e.verdict)


# ---- layout -------------------------------------------------------------------------------------

@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_frame_alignment(oracle, lead):
    s, fr, v, ifc, t = _fixture(oracle)[0]
    for shift in (0, 8):
        _check(fr, v, ifc, t, slotted=False, record_shift=shift, lead=lead)


def test_small_slots(oracle):
    """Slots of 192 bytes: the shortest valid message (62 bytes) and the longest the parse reads
    into (both headers with all their options and 28 quoted bytes: 170 bytes)."""
    table = C.pcb_table(8)

    def make():
        out = []
        for k in range(70):
            key = C.key_of(table, k % 8)
            out.append(R.frame(R.quoted(6, b"", src=key[0], dst=key[1]), src=C.PEER, dst=C.LOCAL))
            out.append(R.frame(R.quoted(6, R.tcp_head(28, sport=key[2], dport=key[3]), src=key[0], dst=key[1],
                                        ihl=15), src=C.PEER, dst=C.LOCAL, ihl=15))
        return out
    fr, v = _cached(oracle, "slots", make)
    assert {len(f) for f in fr} == {62, 170}
    e, _, _ = _check(fr, v, C.iface(), table, slotted=True, slot=192)
    assert e.counts.tolist() == [70, 140] and set(e.records["ip_off"].tolist()) == {42, 82}


# ---- replay from a graph -------------------------------------------------------------------------

def test_graph_replay(oracle):
    s, fr, v, ifc, t = _fixture(oracle)[0]
    e = C.expected(fr, v, ifc, t)
    lay, out = Layout(fr, False), Guarded(len(fr))
    dt = torch.from_numpy(_sorted(t).view(np.uint8).copy()).to(DEV)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        lay.call(ifc, dt, out)                                               # warm-up
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lay.call(ifc, dt, out)
    seen = []
    for _ in range(2):
        out.poison()
        g.replay()
        _compare(e, out, lay)
        seen.append(out.bytes())
    assert seen[0] == seen[1]


# ---- the argument list, on the host only ---------------------------------------------------------

def test_einval_paths():
    fr = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    off = torch.tensor([0, 60, 120], dtype=torch.int64, device=DEV)
    good = A.icmp_iface(C.LOCAL, C.iface()["bcast"], R.LOCAL_MAC)
    assert A.icmp_rx_unreach(fr, off, good).n == 2
    bad = good.copy()
    bad["mtu"] = 255
    for kw in (dict(iface=bad), dict(workspace=torch.empty(40, dtype=torch.uint8, device=DEV)),
               dict(workspace=torch.empty(72, dtype=torch.uint8, device=DEV)[4:])):
        args = dict(iface=good)
        args.update(kw)
        with pytest.raises(A.ChksumError) as err:
            A.icmp_rx_unreach(fr, off, args.pop("iface"), **args)
        assert err.value.status == A.AIPSTACK_CHKSUM_EINVAL
    for kw in (dict(records=torch.empty(80, dtype=torch.uint8, device=DEV)[4:]),
               dict(records=torch.empty(63, dtype=torch.uint8, device=DEV)),
               dict(status=torch.empty(2, dtype=torch.int32, device=DEV)),
               dict(pcb_frame=torch.empty(2, dtype=torch.int64)),
               dict(pcbs=torch.empty(24, dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            A.icmp_rx_unreach(fr, off, good, **kw)
    with pytest.raises(A.ChksumError):
        A.icmp_rx_unreach_slotted(torch.zeros(65537, dtype=torch.uint8, device=DEV), 65537,
                                  torch.tensor([60], dtype=torch.int32, device=DEV), good)
    e = A.icmp_rx_unreach(fr[:0], off[:1], good)                             # n == 0
    assert e.n == 0 and e.counts.cpu().tolist() == [0, 0]
    assert _lib.load().aipstack_chksum_last_hip_error() == 0
