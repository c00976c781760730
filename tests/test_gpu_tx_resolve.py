"""Tx resolve (aipstack_tx_resolve) on the GPU against the model of tx_resolve_cases.py, which
test_tx_resolve_host.py pins to what the reference's own IpStack and EthIpIface did with the sends
of tests/golden/tx_resolve_ref_cases.json.

Every comparison covers status, the records, send_len, arp_used, both lists and the counts, every
byte of the header ring (a _SENT slot's bytes 0..13, every other byte as it was), the guard bytes in
front of and behind every output and the ring, and the inputs, over outputs that were dirty before
the call."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import tx_resolve_cases as C
import tx_resolve_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = 0xC3
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


def _tune(key, value):
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == 0


class Buffers:
    """The header ring and every output as poisoned tensors, each between GUARD poisoned bytes of
    its own allocation; `shift` moves the ring off its 16-byte boundary."""

    def __init__(self, n, stride, n_arp, shift=0):
        self.raw = []

        def t(nbytes, dtype, off=0):
            raw = torch.full((GUARD + off + nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
            self.raw.append((raw, GUARD + off, nbytes))
            return raw[GUARD + off:GUARD + off + nbytes].view(dtype)

        self.ring = t(n * stride, torch.uint8, shift)
        assert self.ring.data_ptr() % 16 == shift
        self.workspace = t(A.tx_resolve_workspace_bytes(n), torch.uint8)
        self.out = dict(status=t(n, torch.uint8), routes=t(16 * n, torch.uint8), send_lens=t(4 * n, torch.int32),
                        arp_used=t(n_arp, torch.uint8), held_seg=t(8 * n, torch.int64),
                        failed_seg=t(8 * n, torch.int64), counts=t(16, torch.int64))

    def guards_intact(self):
        for raw, at, nbytes in self.raw:
            assert bool((raw[:at] == POISON).all()) and bool((raw[at + nbytes:] == POISON).all())


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _compare(e, got, b, n):
    torch.cuda.synchronize()
    assert got.n == n
    assert np.array_equal(got.status.cpu().numpy(), e.status)
    assert got.routes.cpu().numpy().tobytes() == e.routes.tobytes()
    assert np.array_equal(got.routes_numpy(), e.routes)
    assert np.array_equal(got.send_lens.cpu().numpy().view(np.uint32), e.send_len)
    assert np.array_equal(got.arp_used.cpu().numpy(), e.arp_used)
    assert np.array_equal(got.held_seg.cpu().numpy().view(np.uint64), e.held)
    assert np.array_equal(got.failed_seg.cpu().numpy().view(np.uint64), e.failed)
    assert np.array_equal(got.counts.cpu().numpy().view(np.uint64), e.counts)
    assert b.ring.cpu().numpy().tobytes() == e.ring.tobytes()      # every slot whole
    b.guards_intact()


def _check(headers, stride, ifaces, table, *, sf=None, force=None, ss=None, shift=0, specified=True,
           device_tables=False):
    ring, lens = C.ring_of(headers, stride)
    n = len(headers)
    b = Buffers(n, stride, len(table), shift)
    b.ring.copy_(torch.from_numpy(ring))
    dl, dsf, dss = _dev(lens.view(np.int32)), _dev(sf), _dev(ss)
    dforce = _dev(None if force is None else np.asarray(force, dtype=np.uint16).view(np.int16))
    it, at = C.iface_table(ifaces), table
    if device_tables:
        it, at = _dev(it.view(np.uint8)), (_dev(table.view(np.uint8)) if len(table) else None)
    got = A.tx_resolve(b.ring, stride, dl, it, at if len(table) else None, seg_status=dss, send_flags=dsf,
                       force_iface=dforce, workspace=b.workspace, **b.out)
    assert got.status is b.out["status"]
    if not specified:       # a table outside the contract: only the bounds
        torch.cuda.synchronize()
        b.guards_intact()
        st = got.status.cpu().numpy()
        assert ((st >= C.NONE) & (st <= C.ARP_QUERY)).all()
        return None
    e = C.expected(ring, stride, lens, ifaces, table, seg_status=ss, send_flags=sf, force=force)
    _compare(e, got, b, n)
    for t, w in ((dl, lens.view(np.int32)), (dsf, sf), (dss, ss)):              # the inputs: only read
        assert t is None or np.array_equal(t.cpu().numpy(), w)
    return e


# ---- the reference-recorded sends -----------------------------------------------------------------

def _fixture_batches():
    """Per fixture stack one batch per round: the sends between two runs of injected frames,
    against the keeper's table at the start of the round (a round's later sends see the Query
    entries its earlier ones made, so the batch's own expectation comes from the model)."""
    import test_tx_resolve_host as H
    out = []
    for stack in R.load():
        ifaces = C.stack_ifaces(stack)
        n, batch, table0 = len(ifaces), [], None
        for step, table, d in H.replay(stack):
            if d is None:
                if batch:
                    out.append((stack["name"], ifaces, table0, batch))
                batch, table0 = [], None
                continue
            if table0 is None:
                table0 = table
            force = C.ROUTE_ANY if step["iface"] < 0 else n - 1 - step["iface"]
            batch.append((step["src"], step["dst"], step["flags"], force, d, table.tobytes() == table0.tobytes()))
        out.append((stack["name"], ifaces, table0, batch))
    return out


def test_fixture_cases():
    """Every recorded send in batches; where the table of a send's moment is the batch's table the
    kernel's status is the one pinned to the reference's IpErr."""
    pinned = 0
    for name, ifaces, table, batch in _fixture_batches():
        headers = [C.header(s, d, length=54) for s, d, *_ in batch]
        e = _check(headers, 64, ifaces, table, sf=np.array([x[2] for x in batch], dtype=np.uint8),
                   force=np.array([x[3] for x in batch], dtype=np.uint16))
        for i, (_, _, _, _, d, same) in enumerate(batch):
            if same or d[0] not in (C.ARP_QUERY,):
                assert int(e.status[i]) == d[0], (name, i)
                pinned += 1
    assert pinned >= 600


# ---- sizes, placements, tables, strides, alignments ---------------------------------------------

@pytest.mark.parametrize("kind", ["sent", "query", "error"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_sizes(n, kind):
    _check(C.placed_batch(n, kind), 64, C.LAN, C.lan_table())
    if n == 1000:   # the grid-stride loops run several times
        _tune("aux_blocks", 2)
        try:
            _check(C.placed_batch(n, kind), 64, C.LAN, C.lan_table(30))
        finally:
            _tune("aux_blocks", -1)


@pytest.mark.parametrize("n_ifaces", [1, 2, 16])
def test_interface_counts(n_ifaces):
    ifaces, table, headers, sf, force, ss = C.random_case(100 + n_ifaces, 600, n_ifaces=n_ifaces)
    e = _check(headers, 64, ifaces, table, sf=sf, force=force, ss=ss)
    assert len(set(e.routes["iface"].tolist())) >= min(n_ifaces, 3)


@pytest.mark.parametrize("n_arp", [0, 1, 2, 4096])
def test_table_sizes(n_arp):
    table = C.lan_table(n_arp - 3) if n_arp >= 3 else C.lan_table()[:n_arp]
    assert len(table) == n_arp
    e = _check(C.placed_batch(300, "sent"), 64, C.LAN, table, device_tables=n_arp == 4096)
    assert int(e.arp_used.sum()) == (0, 1, 2, 2)[(0, 1, 2, 4096).index(n_arp)]


def test_every_entry_of_a_large_table_is_found():
    table = C.lan_table(4093)
    ifaces = [C.LAN[0], C.iface(R.ip(10, 21, 0, 1), 8, None, R.mac_of(1))]
    ifaces[0] = C.iface(R.ip(10, 20, 30, 40), 8, None, R.mac_of(0))
    headers = [C.header(ifaces[int(t["iface"])]["addr"], int(t["addr"])) for t in table]
    force = table["iface"].astype(np.uint16)
    e = _check(headers, 64, ifaces, table, force=force)
    assert (e.arp_used == (table["state"] >= C.VALID)).all() and e.arp_used.sum() >= 4000


@pytest.mark.parametrize("kind", ["unsorted", "duplicates"])
def test_table_outside_the_contract_stays_in_bounds(kind):
    t = C.lan_table(500)
    bad = t[::-1].copy() if kind == "unsorted" else np.concatenate([t, t[100:300], t[:7]])
    _check(C.placed_batch(700, "sent"), 64, C.LAN, bad, specified=False)


@pytest.mark.parametrize("shift", [0, 1, 2, 4])
@pytest.mark.parametrize("stride", [64, 256])
def test_strides_and_ring_alignments(stride, shift):
    ifaces, table, headers, sf, force, ss = C.random_case(5, 520)
    _check(headers, stride, ifaces, table, sf=sf, force=force, ss=ss, shift=shift)


def test_odd_strides_take_every_alignment():
    """Strides that are no multiple of 4: consecutive slots take every residue; a stride below 34
    resolves nothing, and a header longer than its slot is left alone."""
    for stride in (61, 54, 35):
        _check(C.placed_batch(300, "sent"), stride, C.LAN, C.lan_table(), shift=1)
    headers = [C.header(C.LAN[0]["addr"], C.PEER_SENT, length=34)] * 40
    e = _check(headers, 33, C.LAN, C.lan_table())
    assert (e.status == C.NONE).all() and (e.send_len == 34).all()


@pytest.mark.parametrize("which", range(8))
def test_optional_pointers(which):
    ifaces, table, headers, sf, force, ss = C.random_case(9, 300)
    _check(headers, 64, ifaces, table, sf=sf if which & 1 else None, force=force if which & 2 else None,
           ss=ss if which & 4 else None)


def test_random_segments():
    ifaces, table, headers, sf, force, ss = C.random_case(20261021, 2048)
    e = _check(headers, 64, ifaces, table, sf=sf, force=force, ss=ss, device_tables=True)
    assert set(e.status.tolist()) == set(range(41, 48))


# ---- replay from a graph ---------------------------------------------------------------------------

def test_graph_replay():
    ifaces, table, first, sf, force, ss = C.random_case(77, 700)
    second = first[1:] + first[:1]
    n = len(first)
    b = Buffers(n, 64, len(table))
    it, at = _dev(C.iface_table(ifaces).view(np.uint8)), _dev(table.view(np.uint8))
    lens = torch.zeros(n, dtype=torch.int32, device=DEV)
    dsf, dss, dforce = _dev(sf), _dev(ss), _dev(force.view(np.int16))

    def call():
        return A.tx_resolve(b.ring, 64, lens, it, at, seg_status=dss, send_flags=dsf, force_iface=dforce,
                            workspace=b.workspace, **b.out)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                                  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = call()
    for headers in (first, second, first):
        ring, hl = C.ring_of(headers, 64)
        b.ring.copy_(torch.from_numpy(ring))
        lens.copy_(torch.from_numpy(hl.view(np.int32)))
        for t in list(b.out.values()) + [b.workspace]:
            t.view(torch.uint8).fill_(POISON)
        g.replay()
        _compare(C.expected(ring, 64, hl, ifaces, table, seg_status=ss, send_flags=sf, force=force), got, b, n)


# ---- the argument list, through the wrapper -------------------------------------------------------

def test_einval_paths_and_no_segments():
    """What the wrapper lets through to the library with device tensors; null pointers and
    n > 2^40 are covered on host buffers in test_tx_resolve_host.py."""
    ring, lens = C.ring_of(C.placed_batch(8, "sent"), 64)
    dr, dl = _dev(ring), _dev(lens.view(np.int32))
    it = C.iface_table(C.LAN)
    with pytest.raises(A.ChksumError):
        A.tx_resolve(dr, 64, dl, np.concatenate([it] * 17))
    with pytest.raises(A.ChksumError):
        A.tx_resolve(dr, 64, dl, it, workspace=torch.zeros(A.tx_resolve_workspace_bytes(8) - 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(A.ChksumError):
        A.tx_resolve(dr, 64, dl, it, workspace=torch.zeros(256, dtype=torch.uint8, device=DEV)[4:])
    for name, nbytes in (("held_seg", 8), ("failed_seg", 8), ("counts", 8)):
        odd = torch.zeros(nbytes * 9 + 8, dtype=torch.uint8, device=DEV)[4:4 + nbytes * 9].view(torch.int32)
        with pytest.raises((A.ChksumError, ValueError)):
            A.tx_resolve(dr, 64, dl, it, **{name: odd})
    with pytest.raises(A.ChksumError):
        A.tx_resolve(dr, 64, dl, it, routes=torch.zeros(16 * 8 + 4, dtype=torch.uint8, device=DEV)[2:])
    with pytest.raises(ValueError):
        A.tx_resolve(dr, 128, dl, it)
    assert _lib.load().aipstack_chksum_last_hip_error() == 0
    torch.cuda.synchronize()
    assert np.array_equal(dr.cpu().numpy(), ring)
    none = A.tx_resolve(dr[:0], 64, dl[:0], it, C.lan_table())
    torch.cuda.synchronize()
    assert none.n == 0 and none.counts.tolist() == [0, 0] and none.arp_used.tolist() == [0, 0, 0]


# ---- end to end: responders, resolve, linearise ---------------------------------------------------

def test_responders_then_resolve_then_linearise():
    """Echo requests through icmp_rx_respond and SYNs to a closed port through tcp_rx_respond, from
    a peer the ARP table holds under another MAC than the frames' Ethernet source and from a peer
    it lacks. The answers' slots go through tx_resolve naming the receive interface, then through
    tx_linearise_slotted with send_lens: the frames to the first peer carry the table's MAC, the
    second peer yields no frame and one held entry per answer."""
    import frame_cases as F
    import icmp_ref as IR
    import tcp_rsp_cases as TC
    import test_gpu_icmp as TI
    local, known, missing = C.LAN[0]["addr"], C.PEER_SENT, C.PEER_NEW
    mac = C.LAN[0]["mac"]
    assert local == TC.LOCAL and mac == F.LOCAL_MAC and R.peer_mac(known) != F.peer_mac(0)
    f = A.icmp_iface(local, C.bcast_of(C.LAN[0]), mac)
    echo = [mac + F.peer_mac(0) + b"\x08\x00" + IR.echo(IR.pattern(9 + k, k), src=src, dst=local)
            for k, src in enumerate((known, missing, known))]
    syn = [TC.rst_due(6 * k, src=src) for k, src in enumerate((missing, known, known))]
    for frames, peers, respond, answered, hdr in (
            (echo, (known, missing, known), A.icmp_rx_respond, A.AIPSTACK_ICMP_ECHO_REPLY, 42),
            (syn, (missing, known, known), A.tcp_rx_respond, A.AIPSTACK_TCP_RSP_RST, 54)):
        n = len(frames)
        lay = TI.Layout(frames, False)
        rsp = respond(lay.dev, lay.offsets, f)
        torch.cuda.synchronize()
        assert rsp.status.cpu().tolist() == [answered] * n and rsp.hdr_lens.cpu().tolist() == [hdr] * n
        before = rsp.headers.cpu().numpy().reshape(n, -1).copy()
        assert all(before[i, :6].tobytes() == frames[i][6:12] != R.peer_mac(known) for i in range(n))
        force = torch.zeros(n, dtype=torch.int16, device=DEV)                  # the receive interface
        res = A.tx_resolve(rsp.headers, rsp.hdr_stride, rsp.hdr_lens, C.iface_table(C.LAN), C.lan_table(),
                           force_iface=force)
        torch.cuda.synchronize()
        held = [i for i in range(n) if peers[i] == missing]
        assert res.status.cpu().tolist() == [C.ARP_QUERY if p == missing else C.SENT for p in peers]
        assert res.held_seg.cpu().tolist() == held + [-1] * (n - 1) and res.counts.cpu().tolist() == [1, 0]
        routes = res.routes_numpy()
        assert routes["flags"].tolist() == [C.FORCED | (C.NEW_ENTRY if p == missing else 0) for p in peers]
        assert routes["next_hop"].tolist() == list(peers)
        used = res.arp_used.cpu().numpy()
        assert used.sum() == 1 and C.lan_table()["addr"][int(np.flatnonzero(used)[0])] == known
        ring = torch.full((n * 128,), POISON, dtype=torch.uint8, device=DEV)
        lin = A.tx_linearise_slotted(ring, 128, headers=rsp.headers, hdr_stride=rsp.hdr_stride,
                                     hdr_lens=res.send_lens, chunk_addr=rsp.chunk_addr, chunk_len=rsp.chunk_len,
                                     chunk_index=rsp.chunk_index, frame_max=128)
        torch.cuda.synchronize()
        assert lin.status.cpu().tolist() == [A.AIPSTACK_TX_LIN_SKIPPED if p == missing else A.AIPSTACK_TX_LIN_WRITTEN
                                             for p in peers]
        out, lens = ring.cpu().numpy().reshape(n, 128), lin.lens.cpu().numpy()
        want = R.peer_mac(known) + mac + b"\x08\x00"
        for i, p in enumerate(peers):
            if p == missing:                                                   # no frame, nothing stored
                assert lens[i] == 0 and (out[i] == POISON).all()
                continue
            assert out[i, :14].tobytes() == want and lens[i] >= hdr
            assert out[i, 14:hdr].tobytes() == before[i, 14:hdr].tobytes()     # the answer as emitted
            assert int.from_bytes(out[i, 30:34].tobytes(), "big") == known
        assert rsp.hdr_lens.cpu().tolist() == [hdr] * n                        # intact for the retry
