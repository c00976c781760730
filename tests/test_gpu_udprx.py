"""The UDP Rx demux (aipstack_udp_rx_demux / _slotted) on the GPU against the model of
udp_rx_cases.py, which test_udprx_host.py pins to the handler calls and the port unreachables
recorded from the reference's own stack; verdicts from the frame oracle.

Every comparison is byte for byte and covers the verdicts, the records, the unreach codes, the
delivery list with its ~0 tail and the counts, over outputs that were poisoned before the call
and lie between guard bytes that must come back untouched (the workspace's too), and the frames
themselves, which are only read."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import frame_cases as F
import icmp_cases as IC
import udp_rx_cases as C
import udp_rx_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = 0xC3
GUARD = 64
KEY, LIS, DGRAM = A.TCP_PCB_KEY_DTYPE, A.UDP_LISTENER_DTYPE, A.UDP_RX_DGRAM_DTYPE


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

    def call(self, ifc, assocs, listeners, out, **kw):
        kw = dict(verdict=out.verdict, dgrams=out.dgrams, unreach_code=out.unreach,
                  deliver_frame=out.deliver_frame, counts=out.counts, workspace=out.workspace, **kw)
        if self.slotted:
            return A.udp_rx_demux_slotted(self.dev, self.slot, self.lens, _np_iface(ifc), assocs, listeners, **kw)
        return A.udp_rx_demux(self.dev, self.offsets, _np_iface(ifc), assocs, listeners, **kw)


class Guarded:
    """The outputs and the workspace of one call, each a poisoned view between two guards of its
    own poisoned buffer; `dgram_shift` 8 puts d_dgrams on an 8-byte boundary that is no 16-byte
    boundary (the plain-store path)."""

    def __init__(self, n, dgram_shift=0):
        self.bufs = {}

        def view(name, nbytes, shift=0):
            b = torch.full((GUARD + shift + nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
            assert b.data_ptr() % 16 == 0
            self.bufs[name] = (b, GUARD + shift, nbytes)
            return b[GUARD + shift:GUARD + shift + nbytes]

        self.verdict = view("verdict", n)
        self.dgrams = view("dgrams", n * 32, dgram_shift)
        self.unreach = view("unreach", n)
        self.deliver_frame = view("deliver_frame", n * 8).view(torch.int64)
        self.counts = view("counts", 16).view(torch.int64)
        self.workspace = view("workspace", A.udp_rx_demux_workspace_bytes(n))

    def poison(self):
        for b, _, _ in self.bufs.values():
            b.fill_(POISON)

    def guards_intact(self):
        for name, (b, at, nbytes) in self.bufs.items():
            h = b.cpu().numpy()
            assert (h[:at] == POISON).all() and (h[at + nbytes:] == POISON).all(), name

    def bytes(self, skip=()):
        return b"".join(getattr(self, k).cpu().numpy().tobytes()
                        for k in ("verdict", "dgrams", "unreach", "deliver_frame", "counts") if k not in skip)


def _compare(e, out, lay, *, assoc=True):
    torch.cuda.synchronize()
    assert np.array_equal(out.verdict.cpu().numpy(), e.verdict)
    got = out.dgrams.cpu().numpy().view(DGRAM)
    if assoc:
        assert got.tobytes() == e.dgrams.tobytes(), np.flatnonzero(got != e.dgrams)[:8]
        assert np.array_equal(out.unreach.cpu().numpy(), e.unreach)
        assert np.array_equal(out.deliver_frame.cpu().numpy().view(np.uint64), e.deliver_frame)
        assert np.array_equal(out.counts.cpu().numpy().view(np.uint64), e.counts)
    else:  # an unsorted table: everything of the records but assoc
        for name in DGRAM.names:
            if name != "assoc":
                assert np.array_equal(got[name], e.dgrams[name]), name
    out.guards_intact()
    assert np.array_equal(lay.dev.cpu().numpy(), lay.host)                   # the frames: only read


def _check(frames, verdicts, ifc, assocs, listeners, *, slotted, dgram_shift=0, **lay_kw):
    e = C.expected(frames, verdicts, ifc, assocs, listeners, DGRAM)
    lay = Layout(frames, slotted, **lay_kw)
    out = Guarded(len(frames), dgram_shift)
    got = lay.call(ifc, assocs, listeners, out)
    assert got.n == len(frames) and got.dgrams.data_ptr() == out.dgrams.data_ptr()
    assert got.dgrams.data_ptr() % 16 == dgram_shift
    _compare(e, out, lay)
    return e, lay, out


_cache = {}


def _cached(oracle, key, make):
    if key not in _cache:
        fr = make()
        _cache[key] = (fr, _verdicts(oracle, fr))
    return _cache[key]


def _fixture(oracle):
    if "fixture" not in _cache:
        out = []
        for s in R.load():
            fr = C.stack_frames(s)
            a, l = C.stack_tables(s, KEY, LIS)
            out.append((s, fr, _verdicts(oracle, fr), C.stack_iface(s), a, l))
        _cache["fixture"] = out
    return _cache["fixture"]


# ---- the fixture's packets with the fixture's tables -------------------------------------------

@pytest.mark.parametrize("dgram_shift", [0, 8])
@pytest.mark.parametrize("slotted", [False, True])
def test_fixture_cases(oracle, slotted, dgram_shift):
    seen = want = 0
    for s, fr, v, ifc, a, l in _fixture(oracle):
        e, _, _ = _check(fr, v, ifc, a, l, slotted=slotted, dgram_shift=dgram_shift)
        seen += int(e.counts[0]) + int(e.counts[1])
        want += sum(1 for c in s["cases"] if c["calls"] or c["out"])   # a handler, or an unreach sent
    assert seen >= want >= 60


# ---- batch sizes: the compaction's block edges and the ~0 tail ---------------------------------

@pytest.mark.parametrize("n,cap", [(1, -1), (255, -1), (256, -1), (257, -1), (513, -1), (513, 1)])
def test_batch_sizes(oracle, n, cap):
    """513 frames are three tiles, the last of one frame; with one workgroup ("aux_blocks") the
    demux and emit passes loop over the tiles."""
    fr, v = _cached(oracle, ("sizes", n), lambda: C.mixed(n, seed=20261020 + n))
    lis = C.listeners([(0, 5000, 0, 0, 9)], LIS)
    _tune("aux_blocks", cap)
    try:
        for slotted in (False, True):
            e, _, _ = _check(fr, v, C.iface(), None, lis, slotted=slotted)
    finally:
        _tune("aux_blocks", -1)
    assert int(e.counts[0]) + int(e.counts[1]) >= (n + 4) // 5
    assert (e.deliver_frame[int(e.counts[0]):] == C.NO_FRAME).all() and int(e.counts[0]) < n


# ---- several steps of the scan: more than 65,536 frames ----------------------------------------

SCAN_STEP = 256 * 256        # frames per step of the one-workgroup scan: 256 tiles of 256 frames
SCAN_KINDS = ("listener", "assoc", "unreach", "nothing")


def _scan_batches(oracle):
    """Two batches of two whole steps of the scan and a part of a third (3 tiles and 77 frames),
    of 42- to 60-byte frames, with eight listeners and 64 associations. Steps 0 and 2: deliveries
    (to a listener and to an association in turn) and unreach requests, alternating, in the
    step's first and last tile (so on both sides of both step boundaries), at lanes 0 and 63 of a
    wave, at a tile's first and last frame and at every 97th frame; the second batch swaps
    deliveries and requests, so that every such place sees both. Step 1: every frame is delivered
    (first batch), every frame asks for an unreach and none is delivered (second batch). The
    other frames: ARP, a datagram for another host, one with a bad checksum, a broadcast nobody
    takes.
    The frames come from a pool of a few dozen distinct ones, so the model runs on the pool and
    its per-frame answers are spread over the batch by index (the model treats every frame on its
    own; the lists are the frame numbers in order); the first and the last 600 frames of each
    batch are checked against the model run on them directly.
    [(frames, Expected)], interface, association table, listener table."""
    if "scan" not in _cache:
        n = 2 * SCAN_STEP + 3 * 256 + 77
        ifc, lis, tbl = C.iface(), C.bit_listeners(LIS, 8), C.many_assocs(KEY, 64)
        kinds = {
            "listener": [C.dgram(7000 + k % 8, n=k % 19) for k in range(16)],
            "assoc": [C.dgram(6000 + j % 7, dst=R.NONLOCAL if j % 3 == 2 else R.LOCAL, src=R.PEER + 1 + j,
                              sport=30000 + j % 11, n=j % 19) for j in range(64)],
            "unreach": [C.dgram(9 + k, n=k % 19, pad60=bool(k & 1)) for k in range(16)],
            "nothing": [F.LOCAL_MAC + F.peer_mac(1) + b"\x08\x06" + bytes(46), C.dgram(9, dst=R.NONLOCAL, n=5),
                        C.dgram(7003, chk="bad", n=7), C.dgram(7001, dst=R.BCAST, n=18)],
        }
        pool, first, count = [], [], []
        for name in SCAN_KINDS:
            first.append(len(pool))
            count.append(len(kinds[name]))
            pool += kinds[name]
        first, count = np.array(first), np.array(count)
        assert {len(f) for f in pool} <= set(range(42, 61)) and {42, 60} <= {len(f) for f in pool}
        v = _verdicts(oracle, pool)
        pe = C.expected(pool, v, ifc, tbl, lis, DGRAM)
        taken = np.zeros(len(pool), dtype=bool)
        taken[pe.deliver_frame[:int(pe.counts[0])].astype(np.int64)] = True
        k0, k1, k2, k3 = (slice(first[q], first[q] + count[q]) for q in range(4))
        assert taken[k0].all() and pe.dgrams["listeners"][k0].all() and (pe.dgrams["assoc"][k0] == C.NO_ASSOC).all()
        assert taken[k1].all() and (pe.dgrams["assoc"][k1] != C.NO_ASSOC).all() and not pe.dgrams["listeners"][k1].any()
        assert (pe.unreach[k2] == C.PORT_UNREACH).all() and not taken[k2].any()
        assert (pe.unreach[k3] == C.NO_UNREACH).all() and not taken[k3].any() and set(v[k3]) == {0, 5, 6}
        assert (pe.unreach[k0] == C.NO_UNREACH).all() and (pe.unreach[k1] == C.NO_UNREACH).all()
        special = np.zeros(n, dtype=bool)
        for step in (0, 2):
            lo, hi = step * SCAN_STEP, min((step + 1) * SCAN_STEP, n)
            special[lo:hi:97] = True
            for edge in (lo, hi - 256 if hi - lo >= 512 else hi - 77):
                special[[edge, min(edge + 63, hi - 1), min(edge + 64, hi - 1), min(edge + 255, hi - 1)]] = True
            special[[lo + 255, lo + 256, hi - 1]] = True
        pos = np.flatnonzero(special)
        k, i = np.arange(pos.size), np.arange(n)
        batches = []
        for b in (0, 1):
            kind = np.full(n, 3)
            kind[pos] = np.where((k + b) & 1, 2, (k >> 1) & 1)
            kind[SCAN_STEP:2 * SCAN_STEP] = i[:SCAN_STEP] & 1 if b == 0 else 2
            idx = first[kind] + i % count[kind]
            frames = [pool[j] for j in idx]
            e = C.Expected()
            e.verdict, e.dgrams, e.unreach = v[idx].copy(), pe.dgrams[idx].copy(), pe.unreach[idx].copy()
            rows = np.flatnonzero(taken[idx])
            e.deliver_frame = np.full(n, C.NO_FRAME, dtype=np.uint64)
            e.deliver_frame[:rows.size] = rows
            e.counts = np.array([rows.size, int((e.unreach != C.NO_UNREACH).sum())], dtype=np.uint64)
            for part in (slice(0, 600), slice(n - 600, n)):
                d = C.expected(frames[part], e.verdict[part], ifc, tbl, lis, DGRAM)
                assert d.dgrams.tobytes() == e.dgrams[part].tobytes() and np.array_equal(d.unreach, e.unreach[part])
                assert np.array_equal(d.deliver_frame[:int(d.counts[0])].astype(np.int64),
                                      np.flatnonzero(taken[idx][part]))
            # both kinds in the first and in the last tile of steps 0 and 2, on both sides of each boundary
            for lo, hi in ((0, 256), (SCAN_STEP - 256, SCAN_STEP), (2 * SCAN_STEP, 2 * SCAN_STEP + 256), (n - 77, n)):
                assert taken[idx][lo:hi].any() and (e.unreach[lo:hi] != C.NO_UNREACH).any(), (b, lo)
            batches.append((frames, e))
        (_, e0), (_, e1) = batches
        mid = slice(SCAN_STEP, 2 * SCAN_STEP)
        assert np.array_equal(e0.deliver_frame[e0.deliver_frame.searchsorted(SCAN_STEP):][:SCAN_STEP],
                              np.arange(SCAN_STEP, 2 * SCAN_STEP, dtype=np.uint64))
        assert (e0.unreach[mid] == C.NO_UNREACH).all() and (e1.unreach[mid] == C.PORT_UNREACH).all()
        assert not np.isin(e1.deliver_frame[:int(e1.counts[0])], np.arange(SCAN_STEP, 2 * SCAN_STEP)).any()
        assert int(e0.counts[0]) > SCAN_STEP and int(e1.counts[1]) > SCAN_STEP
        assert (e0.dgrams["assoc"][mid] != C.NO_ASSOC).any() and e0.dgrams["listeners"][mid].any()
        _cache["scan"] = (batches, ifc, tbl, lis)
    return _cache["scan"]


@pytest.mark.parametrize("slotted,cap", [(False, -1), (True, -1), (False, 1)])
def test_scan_over_several_steps(oracle, slotted, cap):
    """131,917 frames: the scan's loop runs three times and carries its sums from step to step;
    the ballots lie behind 517 scanned pairs, and the emit pass adds the tile sums of the second
    and third step to the ranks it takes from them. Every output is compared whole with the model
    (numpy comparisons, no loop per frame), between intact guards, the workspace's included."""
    batches, ifc, tbl, lis = _scan_batches(oracle)
    _tune("aux_blocks", cap)
    try:
        for frames, e in batches:
            n = len(frames)
            assert n == 2 * SCAN_STEP + 3 * 256 + 77
            lay = Layout(frames, slotted, slot=64)
            out = Guarded(n)
            got = lay.call(ifc, tbl, lis, out)
            assert got.n == n
            _compare(e, out, lay)
    finally:
        _tune("aux_blocks", -1)


# ---- table sizes --------------------------------------------------------------------------------

@pytest.mark.parametrize("n_lis", [0, 1, 64])
def test_listener_counts(oracle, n_lis):
    """64 listeners match bit by bit (bits 31, 32 and 63 included); their reserved bytes and
    undefined flag bits are set and change nothing."""
    fr, v = _cached(oracle, "bits", C.bit_frames)
    lis = C.bit_listeners(LIS, n_lis, dirty=True) if n_lis else None
    for slotted in (False, True):
        e, _, _ = _check(fr, v, C.iface(), None, lis, slotted=slotted)
    want = [1 << k if k < n_lis else 0 for k in range(64)]
    assert [int(m) for m in e.dgrams["listeners"][:64]] == want
    assert int(e.counts[0]) == n_lis and int(e.counts[1]) == 66 - n_lis


@pytest.mark.parametrize("n_assocs", [0, 1, 2, 1000])
def test_assoc_counts(oracle, n_assocs):
    fr, v = _cached(oracle, "assocs", lambda: C.assoc_frames(1000, 7) + C.assoc_frames(3))
    tbl = C.many_assocs(KEY, n_assocs) if n_assocs else None
    for slotted in (False, True):
        e, _, _ = _check(fr, v, C.iface(), tbl, None, slotted=slotted)
    found = set(e.dgrams["assoc"][e.dgrams["assoc"] != C.NO_ASSOC].tolist())
    assert found == {j for j in range(n_assocs) if j % 7 == 0 or j < 3}
    # the table on the device already, as a tensor
    if n_assocs:
        dev_tbl = torch.from_numpy(tbl.view(np.uint8).copy()).to(DEV)
        lay, out = Layout(fr, False), Guarded(len(fr))
        lay.call(C.iface(), dev_tbl, None, out)
        _compare(e, out, lay)


# ---- delivery patterns --------------------------------------------------------------------------

@pytest.mark.parametrize("slotted", [False, True])
def test_every_frame_asks_for_an_unreach(oracle, slotted):
    fr, v = _cached(oracle, "closed", lambda: C.flood(513))
    e, _, _ = _check(fr, v, C.iface(), None, C.bit_listeners(LIS, 8), slotted=slotted)
    assert e.counts.tolist() == [0, 513] and (e.deliver_frame == C.NO_FRAME).all()


@pytest.mark.parametrize("slotted", [False, True])
def test_every_frame_is_delivered(oracle, slotted):
    fr, v = _cached(oracle, "open", lambda: C.flood(513, open_port=7003))
    e, _, _ = _check(fr, v, C.iface(), None, C.bit_listeners(LIS, 8), slotted=slotted)
    assert e.counts.tolist() == [513, 0] and e.deliver_frame.tolist() == list(range(513))


@pytest.mark.parametrize("slotted", [False, True])
def test_no_udp_at_all(oracle, slotted):
    """Every non-UDP verdict: a zero record and 0xFF, whatever the tables would match."""
    fr, v = _cached(oracle, "no_udp", lambda: C.without_udp(600))
    e, _, _ = _check(fr, v, C.iface(), C.many_assocs(KEY, 2), C.listeners([(0, 0, 1, 1, 1)], LIS),
                     slotted=slotted)
    assert set(np.unique(v)) >= {0, 1, 2, 3, 4, 5, 6, 8}
    assert not e.dgrams.tobytes().strip(b"\0") and (e.unreach == C.NO_UNREACH).all() and not e.counts.any()


# ---- layout -------------------------------------------------------------------------------------

@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_frame_alignment(oracle, lead):
    s, fr, v, ifc, a, l = _fixture(oracle)[0]
    for shift in (0, 8):
        _check(fr, v, ifc, a, l, slotted=False, dgram_shift=shift, lead=lead)


def test_small_slots(oracle):
    """Slots of 128 bytes: frames of 42 bytes (no data) and frames that fill the slot."""
    def make():
        out = []
        for k in range(70):
            out.append(C.dgram(5000 + k % 3, n=0))
            out.append(C.dgram(5000 + k % 3, n=128 - 42, chk=("good", "zero")[k % 2]))
        return out
    fr, v = _cached(oracle, "slots", make)
    assert {len(f) for f in fr} == {42, 128}
    lis = C.listeners([(0, 5000, 0, 0, 1), (0, 5001, 1, 1, 2)], LIS)
    e, _, _ = _check(fr, v, C.iface(), None, lis, slotted=True, slot=128)
    assert int(e.counts[0]) > 90 and int(e.counts[1]) > 40
    assert set(e.dgrams["data_len"].tolist()) == {0, 86}


# ---- an unsorted association table ---------------------------------------------------------------

@pytest.mark.parametrize("slotted", [False, True])
def test_unsorted_table_stays_inside_it(oracle, slotted):
    """The table lies between guards of entries that would match; assoc is unspecified, every
    other field of the records is the model's, and nothing outside the outputs is written."""
    fr, v = _cached(oracle, "assocs", lambda: C.assoc_frames(1000, 7) + C.assoc_frames(3))
    tbl = C.many_assocs(KEY, 1000)
    rng = np.random.default_rng(7)
    mixed = tbl[rng.permutation(len(tbl))]
    e = C.expected(fr, v, C.iface(), tbl, None, DGRAM)
    dev_tbl = torch.from_numpy(mixed.view(np.uint8).copy()).to(DEV)
    lay, out = Layout(fr, slotted), Guarded(len(fr))
    lay.call(C.iface(), dev_tbl, None, out)
    _compare(e, out, lay, assoc=False)
    got = out.dgrams.cpu().numpy().view(DGRAM)["assoc"]
    handles = set((tbl["cookie"] & 0x7FFFFFFF).tolist()) | {C.NO_ASSOC}
    assert set(got[e.dgrams["flags"] != 0].tolist()) <= handles            # only entries of the table
    assert np.array_equal(dev_tbl.cpu().numpy(), mixed.view(np.uint8))


# ---- replay from a graph -------------------------------------------------------------------------

def test_graph_replay(oracle):
    s, fr, v, ifc, a, l = _fixture(oracle)[0]
    e = C.expected(fr, v, ifc, a, l, DGRAM)
    lay, out = Layout(fr, False), Guarded(len(fr))
    da = torch.from_numpy(a.view(np.uint8).copy()).to(DEV)
    dl = torch.from_numpy(l.view(np.uint8).copy()).to(DEV)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        lay.call(ifc, da, dl, out)                                           # warm-up
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lay.call(ifc, da, dl, out)
    seen = []
    for _ in range(2):
        out.poison()
        g.replay()
        _compare(e, out, lay)
        seen.append(out.bytes())
    assert seen[0] == seen[1]


# ---- end to end: the codes go straight into the ICMP responder ----------------------------------

def test_unreach_codes_feed_the_icmp_responder(oracle):
    """d_unreach_code as the demux leaves it is aipstack_icmp_rx_respond's input: a response
    exactly at the frames for which the reference, with handlers that accept, sent a port
    unreachable, and linearised it is that packet byte for byte (a fresh stack's j-th message
    carries the Ident j)."""
    seen = 0
    for s, fr, v, ifc, a, l in _fixture(oracle):
        lay, out = Layout(fr, True), Guarded(len(fr))
        lay.call(ifc, a, l, out)
        resp = A.icmp_rx_respond_slotted(lay.dev, lay.slot, lay.lens, _np_iface(ifc), out.unreach)
        torch.cuda.synchronize()
        status = resp.status.cpu().numpy()
        want = np.array([bool(c["out"]) for c in s["cases"]])
        assert np.array_equal(status == A.AIPSTACK_ICMP_UNREACH, want)
        assert (status[~want] == A.AIPSTACK_ICMP_NONE).all()
        refused = np.array([bool(c["src_rejected"]) for c in s["cases"]])
        codes = out.unreach.cpu().numpy()
        assert ((codes == C.PORT_UNREACH) == (want | (refused & (codes == C.PORT_UNREACH)))).all()
        ring = torch.full((len(fr) * 2048,), POISON, dtype=torch.uint8, device=DEV)
        lin = A.tx_linearise_slotted(ring, 2048, resp)
        h, lens = ring.cpu().numpy().reshape(len(fr), 2048), lin.lens.cpu().numpy()
        for i, c in enumerate(s["cases"]):
            if c["out"]:
                pkt = bytes.fromhex(c["out"][0])
                assert len(c["out"]) == 1 and lens[i] == 14 + len(pkt), c["name"]
                assert h[i, 14:lens[i]].tobytes() == pkt, c["name"]
                seen += 1
            else:
                assert lens[i] == 0
        out.guards_intact()
    assert seen >= 15


# ---- the argument list, on the host only ---------------------------------------------------------

def test_einval_paths():
    fr = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    off = torch.tensor([0, 60, 120], dtype=torch.int64, device=DEV)
    good = A.icmp_iface(R.LOCAL, R.BCAST, IC.LOCAL_MAC)
    assert A.udp_rx_demux(fr, off, good).n == 2
    bad = good.copy()
    bad["mtu"] = 255
    for kw in (dict(iface=bad), dict(listeners=C.bit_listeners(LIS, 64).repeat(2)[:65]),
               dict(workspace=torch.empty(56, dtype=torch.uint8, device=DEV)),
               dict(workspace=torch.empty(72, dtype=torch.uint8, device=DEV)[4:]),
               dict(dgrams=torch.empty(80, dtype=torch.uint8, device=DEV)[4:])):
        args = dict(iface=good)
        args.update(kw)
        with pytest.raises(A.ChksumError) as err:
            A.udp_rx_demux(fr, off, args.pop("iface"), **args)
        assert err.value.status == A.AIPSTACK_CHKSUM_EINVAL
    with pytest.raises(A.ChksumError):
        A.udp_rx_demux_slotted(torch.zeros(65537, dtype=torch.uint8, device=DEV), 65537,
                               torch.tensor([60], dtype=torch.int32, device=DEV), good)
    e = A.udp_rx_demux(fr[:0], off[:1], good)                              # n == 0
    assert e.n == 0 and e.counts.cpu().tolist() == [0, 0]
    assert _lib.load().aipstack_chksum_last_hip_error() == 0
