"""The whole send loop on the GPU (tx_loop_cases.py): the producers, the ARP responder, tx_resolve,
the lineariser, ARP learning through arp_rx_respond and the retry, joined by a host that reads
nothing but what the calls return. Part 2 (below) is one mixed batch of tcp_tx_segment,
udp_tx_fragment, the ICMP and TCP responders' answers and ARP replies in one ring, two rounds and a
fresh send.

Part 1 plays the 1,194 steps recorded from the reference's own IpStack and EthIpIface
(tests/golden/tx_resolve_ref_cases.json) through the device in batches: every output of every call
is compared byte for byte with the model's between guard bytes, and what the device returned is
held to the recording (the IpErr, the frame's 14 bytes, the ARP requests at their first holders,
the replies). The ARP table of every resolve batch is built from the device's own
aipstack_arp_record records and ordered by aipstack_arp_table_sort."""
import numpy as np
import pytest

import aipstack_amd as A

import arp_cases as AC
import ipfrag_cases as IF
import tcpseg_cases as TS
import tx_loop_cases as L
import tx_resolve_cases as C
import tx_resolve_ref as R
import test_gpu_arp as TA
import test_gpu_icmp as TI
import test_gpu_tx_resolve as TR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = TR.POISON
GUARD = TR.GUARD
assert POISON == L.SENTINEL == TA.POISON


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _no_chunks(n):
    return dict(chunk_addr=torch.empty(0, dtype=torch.int64, device=DEV),
                chunk_len=torch.empty(0, dtype=torch.int32, device=DEV),
                chunk_index=torch.zeros(n + 1, dtype=torch.int64, device=DEV))


class ResolveOutputs:
    """Every output of tx_resolve and its workspace as poisoned tensors, each between GUARD
    poisoned bytes of its own allocation, for a call on `ring` (a tensor that lives elsewhere):
    what test_gpu_tx_resolve._compare takes in place of its Buffers."""

    def __init__(self, n, n_arp, ring):
        self.ring, self.raw = ring, []

        def t(nbytes, dtype):
            raw = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
            self.raw.append((raw, nbytes))
            return raw[GUARD:GUARD + nbytes].view(dtype)

        self.workspace = t(A.tx_resolve_workspace_bytes(n), torch.uint8)
        self.out = dict(status=t(n, torch.uint8), routes=t(16 * n, torch.uint8), send_lens=t(4 * n, torch.int32),
                        arp_used=t(n_arp, torch.uint8), held_seg=t(8 * n, torch.int64),
                        failed_seg=t(8 * n, torch.int64), counts=t(16, torch.int64))

    def guards_intact(self):
        for raw, nbytes in self.raw:
            assert bool((raw[:GUARD] == POISON).all()) and bool((raw[GUARD + nbytes:] == POISON).all())


def _resolved(got, ring):
    """The device's outputs as the model's Expected."""
    r = C.Expected()
    r.status = got.status.cpu().numpy()
    r.routes = got.routes_numpy().copy()
    r.send_len = got.send_lens.cpu().numpy().view(np.uint32)
    r.arp_used = got.arp_used.cpu().numpy()
    r.held = got.held_seg.cpu().numpy().view(np.uint64)
    r.failed = got.failed_seg.cpu().numpy().view(np.uint64)
    r.counts = got.counts.cpu().numpy().view(np.uint64)
    r.ring = ring.cpu().numpy().copy()
    return r


def _send_ring(n, headers, stride, send_lens, slot=L.FRAME_SLOT):
    """Header-only segments through tx_linearise_slotted into a sentinel-filled ring between
    guards: (frames (n, slot), lens)."""
    raw = torch.full((GUARD + n * slot + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    lin = A.tx_linearise_slotted(raw[GUARD:GUARD + n * slot], slot, headers=headers, hdr_stride=stride,
                                 hdr_lens=send_lens, frame_max=slot, **_no_chunks(n))
    torch.cuda.synchronize()
    host = raw.cpu().numpy()
    assert (host[:GUARD] == POISON).all() and (host[GUARD + n * slot:] == POISON).all()
    lens = lin.lens.cpu().numpy().view(np.uint32)
    st = lin.status.cpu().numpy()
    assert ((st == A.AIPSTACK_TX_LIN_WRITTEN) == (lens != 0)).all()
    assert np.isin(st, (A.AIPSTACK_TX_LIN_WRITTEN, A.AIPSTACK_TX_LIN_SKIPPED)).all()
    return host[GUARD:GUARD + n * slot].reshape(n, slot), lens


class DeviceBackend:
    """The two calls of play() on the device, each compared with the model's answer before its own
    outputs are handed back to the host. Strides, ring shifts and the frame layout rotate with
    the batch number."""

    def __init__(self):
        self.model = L.ModelBackend()
        self.launches = 0

    def resolve(self, ring, stride, hdr_len, ifaces, table, send_flags, force, where=0):
        n = len(hdr_len)
        e = self.model.resolve(ring, stride, hdr_len, ifaces, table, send_flags, force)
        b = TR.Buffers(n, stride, len(table), shift=(0, 2, 4)[where % 3])
        b.ring.copy_(torch.from_numpy(ring))
        dl = _dev(hdr_len.view(np.int32))
        tables = (C.iface_table(ifaces), table) if where % 2 else \
            (_dev(C.iface_table(ifaces).view(np.uint8)), _dev(table.view(np.uint8)) if len(table) else None)
        got = A.tx_resolve(b.ring, stride, dl, tables[0], tables[1] if len(table) else None,
                           send_flags=_dev(send_flags), force_iface=_dev(force.view(np.int16)),
                           workspace=b.workspace, **b.out)
        TR._compare(e, got, b, n)
        frames, lens = _send_ring(n, b.ring, stride, got.send_lens)
        assert frames.tobytes() == e.frames.tobytes() and np.array_equal(lens, e.frame_lens)
        assert np.array_equal(dl.cpu().numpy().view(np.uint32), hdr_len)           # intact for the retry
        b.guards_intact()
        r = _resolved(got, b.ring)
        r.frames, r.frame_lens = frames, lens
        self.launches += 2
        return r

    def arp(self, frames, k, keeper, table, where=0):
        n = len(frames)
        ifc = keeper.arp_iface(k)
        e = self.model.arp(frames, k, keeper, table)
        stride = (64, 42, 128)[where % 3]
        lay = TI.Layout(frames, bool(where % 2), 128)
        o = TA.Outputs(n, stride, shift=(0, 8)[where % 2], arp_shift=(0, 4, 8)[where % 3])
        TA._call(lay, ifc, o)
        TA._compare(e, o, lay, n, stride)
        # the replies ride through tx_resolve: nothing to resolve, every byte as emitted
        before = o.res.headers.cpu().numpy().copy()
        hdr_len = o.res.hdr_lens.cpu().numpy().view(np.uint32).copy()
        b = ResolveOutputs(n, len(table), o.res.headers)
        got = A.tx_resolve(o.res.headers, stride, o.res.hdr_lens, C.iface_table(keeper.ifaces),
                           table if len(table) else None,
                           force_iface=torch.full((n,), k, dtype=torch.int16, device=DEV),
                           workspace=b.workspace, **b.out)
        want = C.expected(before, stride, hdr_len, keeper.ifaces, table, force=np.full(n, k))
        assert (want.status == C.NONE).all() and np.array_equal(want.send_len, hdr_len)
        assert want.ring.tobytes() == before.tobytes()
        TR._compare(want, got, b, n)
        o.guards_intact()
        out, lens = _send_ring(n, o.res.headers, stride, got.send_lens)
        assert np.array_equal(lens, e.hdr_len)
        h = AC.Expected()
        h.status = o.res.status.cpu().numpy()
        h.records = o.res.records_numpy().copy()
        assert np.array_equal(h.records["status"], h.status)
        h.sent = {i: out[i, :lens[i]].tobytes() for i in range(n) if lens[i]}
        assert h.sent == e.sent and all((out[i, lens[i]:] == POISON).all() for i in range(n))
        self.launches += 3
        return h


# ---- part 1: the reference's recorded sequences ---------------------------------------------------

@pytest.mark.parametrize("stack", R.load(), ids=lambda s: s["name"])
def test_recorded_sequences_through_the_device_loop(stack):
    """play() asserts the recording for every step; the backend asserts the model for every byte.
    The model's own play (test_tx_loop_cases.py) must agree on what the host did."""
    backend = DeviceBackend()
    p = L.play(stack, backend, stride=(64, 128)[len(stack["ifaces"]) % 2])
    m = L.play(stack, L.ModelBackend())
    assert p.pinned == len(stack["steps"]) == m.pinned
    assert p.requests == m.requests and p.q_consumed == m.q_consumed
    assert all(p.route[j].tobytes() == m.route[j].tobytes() for j in m.route) and len(p.route) == len(m.route)
    assert backend.launches >= 2 * p.n_batches


# ---- part 2: one mixed batch from the real producers, two rounds with a retry ---------------------

RX_NOT_IP4, RX_FRAGMENT, RX_ACCEPT = 0, 3, 6      # AIPSTACK_RX_* (chksum.h)


class RingBackend(DeviceBackend):
    """tx_resolve in place on the device ring the producers filled: the ring must still hold what
    the host believes it holds (every byte, from one round to the next), and every output is the
    model's."""

    def __init__(self, ring):
        super().__init__()
        self.ring, self.got = ring, None

    def resolve(self, ring, stride, hdr_len, ifaces, table, send_flags, force, seg_status=None, where=0):
        n = len(hdr_len)
        torch.cuda.synchronize()
        assert self.ring.cpu().numpy().tobytes() == ring.tobytes()
        e = self.model.resolve(ring, stride, hdr_len, ifaces, table, send_flags, force, seg_status=seg_status)
        b = ResolveOutputs(n, len(table), self.ring)
        self.lens = _dev(hdr_len.view(np.int32))
        self.got = A.tx_resolve(self.ring, stride, self.lens, C.iface_table(ifaces), table,
                                seg_status=_dev(seg_status), send_flags=_dev(send_flags),
                                force_iface=_dev(force.view(np.int16)), workspace=b.workspace, **b.out)
        TR._compare(e, self.got, b, n)
        assert np.array_equal(self.lens.cpu().numpy().view(np.uint32), hdr_len)
        return _resolved(self.got, self.ring)


def _produce(sc, ring):
    """The producers and the three responders, each into its slice of the shared ring (through an
    aligned staging ring where the shared one is shifted off its boundary). Returns the result
    objects in ring order and the tensors that the chunk tables point into."""
    s, at = sc.stride, sc.at
    dest = ring if sc.shift == 0 else torch.full((sc.n * s,), L.FILL, dtype=torch.uint8, device=DEV)
    tpay, upay = _dev(sc.tcp_batch.payload), _dev(sc.udp_batch.payload)
    tcp = A.tcp_tx_segment(TS.descriptors(sc.tcp_batch, tpay.data_ptr(), A.TCP_BURST_DTYPE), sc.tcp_si, sc.tcp_cb,
                           hdr_stride=s, headers=dest[:at["icmp"] * s])
    lan = L.IFACES[L.K_LAN]
    rx = TI.Layout(sc.rx_frames, False)                  # one received batch, both responders over it
    icmp = A.icmp_rx_respond(rx.dev, rx.offsets, A.icmp_iface(L.OWN, L.SUBNET_BCAST, lan["mac"], ip_id=L.ICMP_ID),
                             hdr_stride=s, headers=dest[at["icmp"] * s:at["rst"] * s])
    rst = A.tcp_rx_respond(rx.dev, rx.offsets, A.icmp_iface(L.OWN, L.SUBNET_BCAST, lan["mac"], ip_id=L.RST_ID),
                           hdr_stride=s, headers=dest[at["rst"] * s:at["arp"] * s])
    lay = TI.Layout(sc.arp_frames, False)
    arp = A.arp_rx_respond(lay.dev, lay.offsets, TA._np_iface(L.start_keeper().arp_iface(L.K_LAN)), hdr_stride=s,
                           headers=dest[at["arp"] * s:at["udp"] * s])
    udp = A.udp_tx_fragment(IF.descriptors(sc.udp_batch, upay.data_ptr(), A.UDP_DGRAM_DTYPE), sc.udp_si, sc.udp_cb,
                            hdr_stride=s, headers=dest[at["udp"] * s:])
    if dest is not ring:
        ring.copy_(dest)
    torch.cuda.synchronize()
    return (tcp, icmp, rst, arp, udp), (tpay, upay, rx, lay)


def _linearise(sc, ring, send_lens, chunks, seg_status):
    """tx_linearise_slotted of the whole ring into a sentinel-filled send ring between guards:
    (frames (n, SEND_SLOT), lens, Rx verify's verdicts of the send ring)."""
    n, slot = sc.n, L.SEND_SLOT
    raw = torch.full((GUARD + n * slot + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    send = raw[GUARD:GUARD + n * slot]
    lin = A.tx_linearise_slotted(send, slot, headers=ring, hdr_stride=sc.stride, hdr_lens=send_lens,
                                 seg_status=seg_status, frame_max=1514, **chunks)
    verdict = A.rx_verify_slotted(send, slot, lin.lens).cpu().numpy()
    host = raw.cpu().numpy()
    assert (host[:GUARD] == POISON).all() and (host[GUARD + n * slot:] == POISON).all()
    lens = lin.lens.cpu().numpy().view(np.uint32)
    assert ((lin.status.cpu().numpy() == A.AIPSTACK_TX_LIN_WRITTEN) == (lens != 0)).all()
    return host[GUARD:GUARD + n * slot].reshape(n, slot), lens, verdict


def _check_send_ring(sc, r, written, frames, lens, verdict):
    """Slot i of `written`: the resolved ring's bytes 0..13, then what the producer's model says;
    every other slot and every byte behind a frame: sentinel. Rx verify: ACCEPT for whole TCP, UDP
    and ICMP frames (the producers' and the responders'), FRAGMENT for fragments, not IPv4 for the
    ARP replies."""
    want = np.full((sc.n, L.SEND_SLOT), POISON, dtype=np.uint8)
    want_len = np.zeros(sc.n, dtype=np.uint32)
    want_verdict = np.zeros(sc.n, dtype=np.uint8)
    for i in written:
        f = r.ring[i * sc.stride:i * sc.stride + 14].tobytes() + sc.body[i]
        want[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
        want_len[i] = len(f)
        if sc.group[i] != -1:
            whole = sc.group[i] < 1000 or (sc.group == sc.group[i]).sum() == 1
            want_verdict[i] = RX_ACCEPT if whole else RX_FRAGMENT
    assert np.array_equal(lens, want_len)
    assert frames.tobytes() == want.tobytes()
    assert np.array_equal(verdict, want_verdict)
    return want_verdict


@pytest.mark.parametrize("seed", L.SEEDS)
def test_mixed_batch_two_rounds_and_a_retry(oracle, seed):
    """tcp_tx_segment, udp_tx_fragment, the answers of icmp_rx_respond and tcp_rx_respond (naming
    their receive interface) and ARP replies in one header ring; tx_resolve and
    tx_linearise_slotted over the whole ring; Query entries, the peers' ARP answers through
    arp_rx_respond, the next snapshot; the retry of the held list on the same ring; a fresh send
    to the peer that changed its MAC."""
    sc = L.cached(oracle, seed)
    TR._tune("aux_blocks", sc.aux_blocks)
    try:
        _mixed(oracle, sc)
    finally:
        TR._tune("aux_blocks", -1)


def _mixed(oracle, sc):
    n, s = sc.n, sc.stride
    raw = torch.full((GUARD + sc.shift + n * s + GUARD,), L.FILL, dtype=torch.uint8, device=DEV)
    ring = raw[GUARD + sc.shift:GUARD + sc.shift + n * s]
    assert ring.data_ptr() % 16 == sc.shift
    (tcp, icmp, rst, arp, udp), keep = _produce(sc, ring)
    parts = (tcp, icmp, rst, arp, udp)
    # the producers left what their models say: statuses, lengths, the header bytes
    seg_status = torch.cat([p.status for p in parts])
    hdr_lens = torch.cat([p.hdr_lens for p in parts])
    assert np.array_equal(seg_status.cpu().numpy(), sc.seg_status)
    assert np.array_equal(hdr_lens.cpu().numpy().view(np.uint32), sc.hdr_len)
    ring0 = ring.cpu().numpy().copy()
    for i in sc.body:
        ln = int(sc.hdr_len[i])
        assert ring0[i * s:i * s + ln].tobytes() == sc.ring[i * s:i * s + ln].tobytes(), i
    # one chunk table for the whole ring: the tables of the parts one behind the other (an echo
    # reply's data is a chunk that points into the received frame; an RST or ARP reply has none)
    base, index = 0, []
    for p in parts:
        index.append(p.chunk_index[:-1] + base)
        base += p.chunk_addr.numel()
    index.append(torch.full((1,), base, dtype=torch.int64, device=DEV))
    chunks = dict(chunk_addr=torch.cat([p.chunk_addr for p in parts]),
                  chunk_len=torch.cat([p.chunk_len for p in parts]), chunk_index=torch.cat(index))
    own = [t for p in parts for t in (p.chunk_addr, p.chunk_len, p.chunk_index)]
    tables = [t.clone() for t in own]
    # round 1
    backend = RingBackend(ring)
    lp = L.Loop(sc, backend, ring0)
    r1 = lp.round1()
    frames1, lens1, verdict1 = _linearise(sc, ring, backend.got.send_lens, chunks, seg_status)
    written1 = [i for i in sc.body if r1.status[i] == C.SENT or sc.group[i] == -1]
    v1 = _check_send_ring(sc, r1, written1, frames1, lens1, verdict1)
    assert (v1 == RX_FRAGMENT).sum() >= 40 and (v1 == RX_ACCEPT).sum() >= 500
    # between the rounds: the ARP answers through the device, the next snapshot
    lp.between()
    # round 2: the retry
    r2 = lp.round2()
    frames2, lens2, verdict2 = _linearise(sc, ring, backend.got.send_lens, chunks, seg_status)
    sent1, sent2, held2 = L.check_rounds(sc, lp)
    assert set(written1) == sent1 | {i for i in sc.body if sc.group[i] == -1}
    v2 = _check_send_ring(sc, r2, sorted(sent2), frames2, lens2, verdict2)
    assert np.isin(v2[sorted(sent2)], (RX_ACCEPT, RX_FRAGMENT)).all() and len(sent2) >= 15 and len(held2) >= 3
    for i in sent2:                                     # the same bytes 14.. it would have had in round 1
        assert frames2[i, 14:lens2[i]].tobytes() == sc.body[i]
    # nothing but bytes 0..13 of the sent slots changed, in either round; the tables are as they were
    torch.cuda.synchronize()
    after = ring.cpu().numpy()
    changed = np.flatnonzero(after != ring0)
    assert set((changed // s).tolist()) <= sent1 | sent2 and (changed % s < 14).all()
    host = raw.cpu().numpy()
    assert (host[:GUARD + sc.shift] == L.FILL).all() and (host[GUARD + sc.shift + n * s:] == L.FILL).all()
    assert np.array_equal(hdr_lens.cpu().numpy().view(np.uint32), sc.hdr_len)
    for t, was in zip(own, tables):
        assert torch.equal(t, was)
    assert np.array_equal(keep[2].dev.cpu().numpy(), keep[2].host)         # the received frames: only read
    # a fresh segment to the peer that changed its MAC
    c = TS.burst((5, 700), mss=1460, hdr=TS.template(src=L.OWN, dst=C.PEER_SENT))
    one = TS.Batch([c], sc.tcp_batch.payload)
    si, cb = TS.caller_index([c])
    seg = A.tcp_tx_segment(TS.descriptors(one, keep[0].data_ptr(), A.TCP_BURST_DTYPE), si, cb)
    torch.cuda.synchronize()
    table3 = L.snapshot(lp.keeper)
    r3 = RingBackend(seg.headers[:64]).resolve(seg.headers[:64].cpu().numpy(), 64, np.array([54], dtype=np.uint32),
                                               L.IFACES, table3, np.zeros(1, dtype=np.uint8),
                                               np.array([C.ROUTE_ANY], dtype=np.uint16),
                                               seg_status=seg.status.cpu().numpy())
    assert r3.status.tolist() == [C.SENT]
    assert r3.ring[:14].tobytes() == R.peer_mac(C.PEER_SENT, 1) + L.IFACES[L.K_LAN]["mac"] + b"\x08\x00"
    used, = np.flatnonzero(r3.arp_used)
    assert (int(table3[used]["iface"]), int(table3[used]["addr"])) == (L.K_LAN, C.PEER_SENT)
