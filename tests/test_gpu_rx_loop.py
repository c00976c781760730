"""The whole receive loop of INTEGRATION.md section 2 on one mixed batch of frames on the GPU
(rx_loop_cases.py; test_rx_loop_cases.py checks on the CPU what the scenarios cover): rx_verify,
arp_rx_respond, udp_rx_demux, icmp_rx_respond fed the demux's unreach codes as they are,
tcp_rx_parse, ip4_rx_reassemble and the two tx_linearise_slotted calls that put the ARP and the
ICMP responses into ONE send ring, all reading the same device buffer.

Each call has its own poisoned outputs and workspace between guards (the helpers of the per-call
test files, imported). Every byte of every call is compared with its model; the verdict arrays of
the five calls that embed Rx verify are compared with each other on the device's own outputs; the
owner of every frame, computed from the device outputs as the host loop would, is the dispatch
table's; the send ring is the expected one byte for byte; a second interface receives it; the
outputs do not depend on the order of the calls or on the streams they run on; and the loop
replays from one graph over frames copied in place."""
import numpy as np
import pytest

import aipstack_amd as A

import arp_cases as AC
import icmp_cases as IC
import ipreass_cases as RC
import rx_loop_cases as G
import rx_loop_ref as LR
import tcprx_cases as TC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ipreass_gpu as RG  # noqa: E402
import test_gpu_arp as TA  # noqa: E402
import test_gpu_icmp as TI  # noqa: E402
import test_gpu_tcprx as TT  # noqa: E402
import test_gpu_udprx as TU  # noqa: E402

DEV = "cuda"
SLOT = G.SLOT
POISON = TT.POISON
SEEDS = range(G.SEEDS)
ORDER = ("verify", "tcp", "reass", "udp", "icmp", "lin_icmp", "arp", "lin_arp")     # as INTEGRATION.md goes
FORKS = (("verify",), ("tcp",), ("reass",), ("udp", "icmp", "lin_icmp"), ("arp", "lin_arp"))


@pytest.fixture(autouse=True)
def _no_contract_violation():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


def _dev(table):
    return None if table is None else torch.from_numpy(table.view(np.uint8).copy()).to(DEV)


class Outs:
    """The outputs and the workspace of every call of the loop, each poisoned and between guards of
    its own, and the one send ring."""

    def __init__(self, sc):
        n = sc.n
        self.verify = TT.Guarded(n)
        self.arp = TA.Outputs(n, 64, sc.hdr_shift, sc.rec_shift)
        self.udp = TU.Guarded(n, sc.rec_shift)
        self.icmp = TI._dirty(n, 64, sc.hdr_shift)
        self.icmp_ws = TT.Guarded(A.icmp_rx_respond_workspace_bytes(n))
        self.tcp = TT.Outputs(n, sc.rec_shift)
        self.reass = RG.Outputs(n)
        self.ring = TT.Guarded(n * SLOT)
        self.lin = {k: (TT.Guarded(4 * n), TT.Guarded(n)) for k in ("arp", "icmp")}

    def lin_lens(self, k):
        return self.lin[k][0].view.cpu().numpy().view(np.uint32)

    def bytes(self):
        """Every output byte of the loop (no workspace)."""
        torch.cuda.synchronize()
        i, a = self.icmp, self.arp.res
        ts = [self.verify.view, self.ring.view, self.udp.verdict, self.udp.dgrams, self.udp.unreach,
              self.udp.deliver_frame, self.udp.counts, i.headers, i.hdr_lens, i.chunk_addr, i.chunk_len,
              i.chunk_index, i.status, i.verdict, i.response_frame, i.counts, a.headers, a.hdr_lens,
              a.chunk_index, a.status, a.records, a.reply_frame, a.seen_frame, a.counts]
        ts += [g.view for k in ("arp", "icmp") for g in self.lin[k]]
        return tuple(t.cpu().numpy().tobytes() for t in ts) + self.tcp.bytes() + self.reass.bytes()


class Loop:
    """One scenario on the device: the frames (`lay`: a layout of test_gpu_udprx, or a Live one),
    the tables, the interface records."""

    def __init__(self, sc, lay=None):
        self.sc = sc
        self.lay = TU.Layout(sc.frames, sc.slotted, slot=SLOT, lead=sc.lead) if lay is None else lay
        if not hasattr(self.lay, "buf"):
            self.lay.buf = self.lay.dev
        self.assocs, self.listeners, self.pcbs = _dev(sc.assocs), _dev(sc.listeners), _dev(sc.pcbs)
        self.icmp_if = TI._np_iface(sc.ifc)
        self.arp_if = TA._np_iface(sc.arp_ifc)

    def call(self, name, o):
        lay = self.lay
        s = "_slotted" if lay.slotted else ""
        where = (lay.buf, lay.slot, lay.lens) if lay.slotted else (lay.buf, lay.offsets)
        if name == "verify":
            getattr(A, "rx_verify" + s)(*where, out=o.verify.view)
        elif name == "arp":
            getattr(A, "arp_rx_respond" + s)(*where, self.arp_if, out=o.arp.res, workspace=o.arp.workspace)
        elif name == "udp":
            getattr(A, "udp_rx_demux" + s)(
                *where, self.icmp_if, self.assocs, self.listeners, verdict=o.udp.verdict, dgrams=o.udp.dgrams,
                unreach_code=o.udp.unreach, deliver_frame=o.udp.deliver_frame, counts=o.udp.counts,
                workspace=o.udp.workspace)
        elif name == "icmp":        # the demux's codes as they are
            getattr(A, "icmp_rx_respond" + s)(*where, self.icmp_if, o.udp.unreach, out=o.icmp,
                                              workspace=o.icmp_ws.view)
        elif name == "tcp":
            getattr(A, "tcp_rx_parse" + s)(*where, self.pcbs, **o.tcp.kw())
        elif name == "reass":
            getattr(A, "ip4_rx_reassemble" + s)(*where, max_reass_size=RC.MAX_REASS, **o.reass.kw())
        else:
            k = name[4:]
            seg = o.arp.res if k == "arp" else o.icmp
            A.tx_linearise_slotted(o.ring.view, SLOT, seg, lens=o.lin[k][0].view.view(torch.int32),
                                   status=o.lin[k][1].view)

    def run(self, o, order=ORDER):
        for name in order:
            self.call(name, o)

    def compare(self, o, sc=None):
        """Every byte of every call against its model, the send ring against the expected one."""
        sc, lay, n = self.sc if sc is None else sc, self.lay, self.sc.n
        torch.cuda.synchronize()
        assert np.array_equal(o.verify.view.cpu().numpy(), sc.verdicts) and o.verify.intact()
        TA._compare(sc.e_arp, o.arp, lay, n, 64)
        TU._compare(sc.e_udp, o.udp, lay)
        TI._compare(sc.e_icmp, o.icmp, lay, sc.frames, 64)
        TT._compare(sc.e_tcp, o.tcp)
        RG.compare(sc.e_reass, o.reass, np.uint64(lay.buf.data_ptr()) + lay.start.astype(np.uint64))
        ring, lens = G.send_ring(sc, SLOT, POISON)
        assert o.ring.view.cpu().numpy().tobytes() == ring.tobytes()
        is_arp = sc.e_arp.hdr_len != 0
        assert np.array_equal(o.lin_lens("arp"), np.where(is_arp, lens, 0))
        assert np.array_equal(o.lin_lens("icmp"), np.where(is_arp, 0, lens))
        for k, written in (("arp", is_arp), ("icmp", sc.e_icmp.hdr_len != 0)):
            st = o.lin[k][1].view.cpu().numpy()
            assert (st[written] == A.AIPSTACK_TX_LIN_WRITTEN).all() and (st[~written] == A.AIPSTACK_TX_LIN_SKIPPED).all()
        for g in (o.icmp_ws, o.ring, *o.lin["arp"], *o.lin["icmp"]):
            assert g.intact()
        assert np.array_equal(lay.dev.cpu().numpy(), lay.host)               # the frames: only read


class Tuned:
    def __init__(self, sc):
        self.cap = sc.aux_blocks

    def __enter__(self):
        TI._tune("aux_blocks", self.cap)

    def __exit__(self, *exc):
        TI._tune("aux_blocks", -1)


# ---- 1 to 5: the bytes, one verdict, the partition, one send ring, the peer's view ---------------

@pytest.mark.parametrize("seed", SEEDS)
def test_loop(oracle, seed):
    sc = G.cached(oracle, seed)
    n = sc.n
    loop, o = Loop(sc), Outs(sc)
    with Tuned(sc):
        loop.run(o)
        loop.compare(o)
        # both orders of the two linearise calls give the same ring
        first = o.ring.view.cpu().numpy().tobytes()
        o.ring.view.fill_(POISON)
        for name in ("lin_arp", "lin_icmp"):
            loop.call(name, o)
        torch.cuda.synchronize()
        assert o.ring.view.cpu().numpy().tobytes() == first and o.ring.intact()

    # one verdict per frame, on the device's own outputs
    v = o.verify.view.cpu().numpy()
    arp_status = o.arp.res.status.cpu().numpy()
    icmp_status = o.icmp.status.cpu().numpy()
    tcp_v, reass_v = (np.frombuffer(x.bytes()[0], dtype=np.uint8) for x in (o.tcp, o.reass))
    rewrites = G.verdicts_agree(v, o.icmp.verdict.cpu().numpy(), o.udp.verdict.cpu().numpy(), tcp_v, reass_v)
    assert rewrites[0] >= 8 and rewrites[1] >= 20
    assert (arp_status != AC.NONE).sum() >= 20 and (v[arp_status != AC.NONE] == RC.NOT_IP4).all()

    # the partition, as the host loop computes it
    counts = o.udp.counts.cpu().numpy()
    delivered = G.delivered_mask(o.udp.deliver_frame.cpu().numpy(), counts[0], n)
    segs = np.frombuffer(o.tcp.bytes()[1], dtype=A.TCP_RX_SEG_DTYPE)
    owner, claims, host_sort = G.dispatch(sc.frames, v, arp_status, icmp_status, delivered,
                                          (segs["opts"] & TC.SEG_VALID) != 0, reass_v)
    assert (claims <= 1).all() and np.array_equal(owner, sc.owner) and np.array_equal(host_sort, sc.host_sort)
    assert np.isin(owner[claims == 0], (G.HOST, G.DROP)).all()
    assert (np.bincount(owner, minlength=len(G.OWNERS)) >= 20).all()

    # the peer's view: the send ring as the receive ring of an interface with a peer's address
    ring, lens = G.send_ring(sc, SLOT, POISON)
    got_lens = np.maximum(o.lin_lens("arp"), o.lin_lens("icmp"))
    assert np.array_equal(got_lens, lens)
    dl = torch.from_numpy(got_lens.view(np.int32).copy()).to(DEV)
    is_arp, is_icmp = sc.e_arp.hdr_len != 0, sc.e_icmp.hdr_len != 0
    assert is_arp.sum() >= 8 and is_icmp.sum() >= 40 and not (is_arp & is_icmp).any()
    pv = A.rx_verify_slotted(o.ring.view, SLOT, dl).cpu().numpy()
    assert (pv[is_icmp] == IC.ACCEPT).all() and (pv[~is_icmp] == RC.NOT_IP4).all()
    peer_mac = sc.frames[int(np.flatnonzero(is_icmp)[0])][6:12]
    pa = A.arp_rx_respond_slotted(o.ring.view, SLOT, dl, A.arp_iface(G.PEERS[0], AC.R.netmask(sc.prefix), peer_mac))
    st, rec = pa.status.cpu().numpy(), pa.records_numpy()
    assert (st[is_arp] == AC.SEEN).all() and (st[~is_arp] == AC.NONE).all()
    assert pa.counts.cpu().tolist() == [0, int(is_arp.sum())]
    assert (rec["op"][is_arp] == 2).all() and (rec["sender_addr"][is_arp] == sc.ifc["local"]).all()
    assert (rec["sender_mac"][is_arp] == np.frombuffer(sc.ifc["mac"], dtype=np.uint8)).all()
    pi = A.icmp_rx_respond_slotted(o.ring.view, SLOT, dl, A.icmp_iface(
        G.PEERS[0], sc.ifc["bcast"], peer_mac, allow_broadcast_ping=True))
    assert pi.counts.cpu().tolist() == [0, 0] and (pi.status.cpu().numpy() == IC.NONE).all()
    assert np.array_equal(pi.verdict.cpu().numpy(), pv)
    h = o.ring.view.cpu().numpy().reshape(n, SLOT)
    unreach = np.flatnonzero(icmp_status == IC.UNREACH)
    assert unreach.size == int((sc.owner == G.UDP_UNREACH).sum()) >= 20
    for i in unreach:
        f = sc.frames[i]
        quoted = f[14:14 + (f[14] & 0xF) * 4 + 8]
        assert h[i, 34] == 3 and h[i, 35] == 3 and h[i, 42:lens[i]].tobytes() == quoted, i


# ---- 6: order and streams --------------------------------------------------------------------------

def _orders(seed):
    """Two seeded orders of the calls: the demux before the responder, a linearise call behind the
    call whose responses it takes."""
    rng = np.random.default_rng(77000 + seed)
    out = []
    while len(out) < 2:
        p = [ORDER[int(j)] for j in rng.permutation(len(ORDER))]
        if p.index("udp") < p.index("icmp") < p.index("lin_icmp") and p.index("arp") < p.index("lin_arp") \
                and tuple(p) != ORDER and p not in out:
            out.append(p)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_order_and_streams(oracle, seed):
    """The outputs of the whole loop are bytewise the same on one stream in the documented order,
    in two other orders, and forked eagerly onto five streams from an event on the producing
    stream and joined again; each over freshly poisoned outputs."""
    sc = G.cached(oracle, seed)
    loop = Loop(sc)
    with Tuned(sc):
        o = Outs(sc)
        loop.run(o)
        loop.compare(o)
        want = o.bytes()
        for order in _orders(seed):
            o = Outs(sc)
            loop.run(o, order)
            assert o.bytes() == want, order
        o = Outs(sc)
        main = torch.cuda.current_stream()
        ready = torch.cuda.Event()
        ready.record(main)                       # the frames, the tables and the poison are in place
        streams = [torch.cuda.Stream() for _ in FORKS]
        for s, names in zip(streams, FORKS):
            s.wait_event(ready)
            with torch.cuda.stream(s):
                for name in names:
                    loop.call(name, o)
        for s in streams:
            main.wait_stream(s)
        assert o.bytes() == want
        loop.compare(o)


# ---- 7: one graph, in order --------------------------------------------------------------------------

class Live:
    """A device buffer that holds one of two layouts of the same shape at a time, copied in place."""

    def __init__(self, a, b):
        self.slotted, self.slot, self.n = a.slotted, a.slot, a.n
        self.buf = torch.full((max(a.host.size, b.host.size),), 0x5C, dtype=torch.uint8, device=DEV)
        if a.slotted:
            self.lens = a.lens.clone()
        else:
            self.offsets = a.offsets.clone()

    def load(self, lay):
        self.buf[:lay.host.size].copy_(lay.dev)
        if self.slotted:
            self.lens.copy_(lay.lens)
        else:
            self.offsets.copy_(lay.offsets)
        self.dev, self.host, self.start = self.buf[:lay.host.size], lay.host, lay.start


@pytest.mark.parametrize("seed", SEEDS)
def test_graph_replay(oracle, seed):
    """The whole loop, the linearise calls included, captured on one stream as a chain and
    replayed over scenario A, scenario B of the same setting, n and layout, then A again."""
    a, b = G.cached(oracle, seed), G.cached(oracle, seed, 1)
    assert a.n == b.n and a.ifc == b.ifc
    lays = {id(s): TU.Layout(s.frames, s.slotted, slot=SLOT, lead=s.lead) for s in (a, b)}
    live = Live(lays[id(a)], lays[id(b)])
    live.load(lays[id(a)])
    loop, o = Loop(a, live), Outs(a)
    with Tuned(a):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            loop.run(o)                                                       # warm-up
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            loop.run(o)
    fresh = Outs(a)          # poison to copy over the outputs, guards and all
    pairs = [(o.verify.buf, fresh.verify.buf), (o.icmp_ws.buf, fresh.icmp_ws.buf), (o.ring.buf, fresh.ring.buf)]
    pairs += [(x.buf, y.buf) for k in ("arp", "icmp") for x, y in zip(o.lin[k], fresh.lin[k])]
    pairs += [(x.buf, y.buf) for x, y in zip((o.tcp.verdict, o.tcp.segs, o.tcp.pcb),
                                            (fresh.tcp.verdict, fresh.tcp.segs, fresh.tcp.pcb))]
    pairs += [(o.reass.g[k].buf, fresh.reass.g[k].buf) for k in o.reass.g] + [(o.reass.ws.buf, fresh.reass.ws.buf)]
    pairs += [(x[0], y[0]) for x, y in zip(o.arp.raw, fresh.arp.raw)]
    pairs += [(o.udp.bufs[k][0], fresh.udp.bufs[k][0]) for k in o.udp.bufs]
    icmp = ("headers", "hdr_lens", "chunk_addr", "chunk_len", "chunk_index", "status", "verdict",
            "response_frame", "counts")
    pairs += [(getattr(o.icmp, k), getattr(fresh.icmp, k)) for k in icmp]
    seen = []
    for sc in (a, b, a):
        live.load(lays[id(sc)])
        for dst, src in pairs:
            dst.copy_(src)
        g.replay()
        loop.compare(o, sc)
        seen.append(o.bytes())
    assert seen[0] == seen[2] != seen[1]


# ---- 8: the sessions recorded from the reference ---------------------------------------------------

@pytest.mark.parametrize("slotted", [False, True])
@pytest.mark.parametrize("session", range(len(LR.SESSIONS)))
def test_reference_sessions(oracle, session, slotted):
    """A session of tests/golden/rx_loop_ref_cases.json in two or three batches, the next batch's
    Ident taken from the device's counts[0]: every byte of every call is the models', the one send
    ring holds exactly the frames the reference's own stack sent (same order, same bytes, the
    Ident running over echo replies and port unreachables as its m_next_id did), and the device's
    delivery list and records name the handler calls the reference made."""
    s = LR.load()[session]
    ip_id = sent = calls = 0
    for start, end in G.session_cuts(s):
        sc = G.session_batch(oracle, s, start, end, ip_id, slotted)
        want = G.session_sent(s, start, end)
        loop, o = Loop(sc), Outs(sc)
        with Tuned(sc):
            loop.run(o)
            loop.compare(o)
        ring = np.full((sc.n, SLOT), POISON, dtype=np.uint8)
        for i, w in want.items():
            ring[i, :len(w)] = np.frombuffer(w, dtype=np.uint8)
        assert o.ring.view.cpu().numpy().tobytes() == ring.tobytes()
        lens = np.maximum(o.lin_lens("arp"), o.lin_lens("icmp"))
        assert {int(i): int(lens[i]) for i in np.flatnonzero(lens)} == {i: len(w) for i, w in want.items()}
        counts = o.udp.counts.cpu().numpy()
        calls += G.session_calls_match(s, start, sc, o.udp.dgrams.cpu().numpy().view(G.DGRAM),
                                       o.udp.deliver_frame.cpu().numpy(), counts[0])
        made = int(o.icmp.counts.cpu().numpy()[0])
        assert made == sum(1 for w in want.values() if w[12:14] == b"\x08\x00")
        ip_id += made                                   # next_ip_id += counts[0]
        sent += len(want)
    assert sent >= 150 and calls >= 100 and ip_id >= 100
