"""aipstack_tcp_tx_control on the GPU against the model of tcp_ctl_cases.py: the frames recorded
from the reference stack rebuilt from their descriptors and carried through tx_resolve and
tx_linearise_slotted; the edge set at the wave and tile edges with invalid descriptors at them;
header rings of every stride class and base alignment over a canary; the call repeated and
replayed from a captured graph; a ring spanning more than 4 GiB; and the Tx fill of header-split
segments as a cross-check of both checksums."""
import numpy as np
import pytest

import aipstack_amd as A

import tcp_ctl_cases as C
import tcp_ctl_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = 0xA5
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 1025)


@pytest.fixture(autouse=True)
def _no_contract_violation():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


def _iface(mac=C.MAC, ip_id=0):
    return A.icmp_iface(C.LOCAL, C.LOCAL | 0xFF, mac, ip_id=ip_id)


def _invalid_places(n):
    at = {i for i in (0, 63, 64, 255, 256, n - 1) if i < n}
    if n >= 1025:
        at |= set(range(512, 768))                      # a whole tile
    return sorted(at)


def _run(cs, ip_id, ttl, stride=64, shift=0, fill=CANARY):
    """The call on descriptors `cs` into a ring of `stride`-byte slots that starts `shift` bytes
    behind a 64-byte boundary and is pre-filled with `fill`; (result, ring tensor)."""
    n = len(cs)
    arena = torch.full((256 + n * stride,), fill, dtype=torch.uint8, device=DEV)
    off = (-arena.data_ptr()) % 64 + shift
    ring = arena[off:off + n * stride]
    assert ring.data_ptr() % 64 == shift % 64
    res = A.tcp_tx_control(C.to_array(cs), _iface(ip_id=ip_id), tcp_ttl=ttl, hdr_stride=stride, headers=ring)
    torch.cuda.synchronize()
    return res, ring, arena, off


def _want_ring(e, n, stride, fill=CANARY):
    want = np.full((n, stride), fill, dtype=np.uint8)
    for i, h in e.headers.items():
        want[i, :len(h)] = np.frombuffer(h, dtype=np.uint8)
        want[i, len(h):min(stride, 64)] = 0
    return want


def _compare(res, ring, e, n, stride, fill=CANARY):
    assert res.counts.cpu().numpy().tolist() == e.counts.tolist()
    assert np.array_equal(res.status.cpu().numpy(), e.status)
    assert np.array_equal(res.hdr_lens.cpu().numpy(), e.hdr_len)
    ci = res.chunk_index.cpu().numpy()
    assert ci.size == n + 1 and not ci.any()
    got = ring.cpu().numpy().reshape(n, stride)
    want = _want_ring(e, n, stride, fill)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[0]].tobytes().hex(), want[bad[0]].tobytes().hex())


def test_reference_frames_through_resolve_and_linearise():
    """Each session of the fixture as one batch with its first Ident; after tx_resolve (the
    interface and an ARP snapshot that holds the peer) and tx_linearise_slotted the linear frames
    are the recorded ones in full."""
    total = 0
    for s in R.load():
        fr = [f for _, f in R.frames(s)]
        cs = [C.from_frame(f)[0] for f in fr]
        n, mac, first = len(fr), bytes.fromhex(s["mac"]), C.from_frame(fr[0])[3]
        ifc = A.icmp_iface(s["addr"], s["addr"] | (0xFFFFFFFF >> s["prefix"]), mac, ip_id=first)
        res = A.tcp_tx_control(C.to_array(cs), ifc)
        assert res.counts.cpu().numpy().tolist() == [n, 0]
        arp = np.zeros(1, dtype=A.ARP_ENTRY_DTYPE)
        arp[0]["addr"], arp[0]["iface"], arp[0]["state"] = s["peer"], 0, A.AIPSTACK_ARP_STATE_VALID
        arp[0]["mac"] = np.frombuffer(bytes.fromhex(s["peer_mac"]), dtype=np.uint8)
        rs = A.tx_resolve(res.headers, res.hdr_stride, res.hdr_lens,
                          A.tx_ifaces([(s["addr"], s["prefix"], s["gateway"], mac)]), A.arp_table_sort(arp))
        assert (rs.status.cpu().numpy() == A.AIPSTACK_TX_RES_SENT).all()
        ring = torch.full((n * 128,), CANARY, dtype=torch.uint8, device=DEV)
        lin = A.tx_linearise_slotted(ring, 128, res, frame_max=128)
        torch.cuda.synchronize()
        assert (lin.status.cpu().numpy() == A.AIPSTACK_TX_LIN_WRITTEN).all()
        got, lens = ring.cpu().numpy().reshape(n, 128), lin.lens.cpu().numpy()
        for i, f in enumerate(fr):
            assert lens[i] == len(f) and got[i, :len(f)].tobytes() == f, (s["name"], i)
            assert (got[i, len(f):] == CANARY).all()
        # the peer's view: every frame is a valid TCP frame
        assert (A.rx_verify_slotted(ring, 128, lin.lens).cpu().numpy() == 6).all()   # AIPSTACK_RX_ACCEPT
        total += n
    assert total >= 150


@pytest.mark.parametrize("n", SIZES)
def test_edge_set_at_wave_and_tile_edges(n):
    """The Ident is the rank among the valid descriptors, across 0xFFFF -> 0 inside the batch."""
    at = _invalid_places(n)
    cs = C.batch(n, invalid_at=at)
    ip_id = (0x10000 - max((n - len(at)) // 2, 1)) & 0xFFFF
    e = C.Expected(cs, dict(mac=C.MAC, ip_id=ip_id), 77)
    assert e.counts.tolist() == [n - len(at), len(at)]
    if n - len(at) >= 2:
        ids = {int.from_bytes(h[18:20], "big") for h in e.headers.values()}
        assert {0xFFFF, 0} <= ids
    if n >= 63:
        # the batch holds the edge set whole: the TCP checksums 0000, 0001 and fffe as the model
        # computes them, and seq and ack at both ends
        assert C.covers_the_ends(cs)
        assert {"0000", "0001", "fffe"} <= {h[50:52].hex() for h in e.headers.values()}
        ends = {(h[38:42].hex(), h[42:46].hex()) for h in e.headers.values()}
        assert {(a, b) for a in ("00000000", "ffffffff") for b in ("00000000", "ffffffff")} <= ends
    res, ring, _, _ = _run(cs, ip_id, 77)
    _compare(res, ring, e, n, 64)


@pytest.mark.parametrize("k", [0, 35, 45, 50])
def test_single_valid_descriptor(k):
    """n = 1 with a valid descriptor: 54 bytes, 62 bytes with seq = ack = 0xFFFFFFFF, and the
    TCP checksums 0x0000 and 0xFFFE, each alone in its batch."""
    c = C.edge_set()[k]
    e = C.Expected([c], dict(mac=C.MAC, ip_id=0xFFFF), 64)
    assert e.counts.tolist() == [1, 0]
    res, ring, _, _ = _run([c], 0xFFFF, 64)
    _compare(res, ring, e, 1, 64)


def test_all_valid_and_all_invalid():
    for cs in (C.batch(513), [C.invalid_set()[k % 6] for k in range(513)]):
        e = C.Expected(cs, dict(mac=C.MAC, ip_id=5), 64)
        res, ring, _, _ = _run(cs, 5, 64)
        _compare(res, ring, e, 513, 64)


def test_ip_checksum_ends():
    c = C.edge_set()[0]
    for want in (0x0000, 0x0001, 0xFFFE):
        ident = C.ident_for_ip_checksum(want, c)
        res, ring, _, _ = _run([c], ident, 64)
        assert ring.cpu().numpy()[24:26].tobytes() == want.to_bytes(2, "big")
        _compare(res, ring, C.Expected([c], dict(mac=C.MAC, ip_id=ident), 64), 1, 64)


@pytest.mark.parametrize("stride", [62, 64, 66, 72, 128, 4096])
@pytest.mark.parametrize("shift", [0, 2, 4, 8, 16])
def test_strides_and_bases_over_a_canary(stride, shift):
    """Every byte outside [0, min(stride, 64)) of a valid slot is unchanged, an invalid slot
    whole, the arena around the ring too; the slack behind the header is zero."""
    n = 321
    cs = C.batch(n, invalid_at=(0, 63, 64, 255, 256, n - 1))
    e = C.Expected(cs, dict(mac=C.MAC, ip_id=0xFFF0), 64)
    res, ring, arena, off = _run(cs, 0xFFF0, 64, stride=stride, shift=shift)
    _compare(res, ring, e, n, stride)
    a = arena.cpu().numpy()
    assert (a[:off] == CANARY).all() and (a[off + n * stride:] == CANARY).all()


def test_repeat_and_graph_replay():
    n = 700
    cs = C.batch(n, invalid_at=(0, 64, 300, n - 1))
    e = C.Expected(cs, dict(mac=C.MAC, ip_id=9), 64)
    ctl = torch.from_numpy(C.to_array(cs).view(np.uint8).copy()).to(DEV)
    ring = torch.full((n * 64,), CANARY, dtype=torch.uint8, device=DEV)
    ws = torch.empty(A.tcp_tx_control_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    ifc = _iface(ip_id=9)
    first = A.tcp_tx_control(ctl, ifc, headers=ring, workspace=ws)
    torch.cuda.synchronize()
    _compare(first, ring, e, n, 64)
    ring.bitwise_not_()                                  # the canary becomes 0x5A, the slots garbage
    second = A.tcp_tx_control(ctl, ifc, headers=ring, workspace=ws)
    torch.cuda.synchronize()
    _compare(second, ring, e, n, 64, fill=CANARY ^ 0xFF)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.tcp_tx_control(ctl, ifc, headers=ring, workspace=ws)     # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = A.tcp_tx_control(ctl, ifc, headers=ring, workspace=ws)
    for _ in range(2):
        ring.fill_(CANARY)
        captured.status.zero_()
        captured.hdr_lens.zero_()
        captured.counts.zero_()
        captured.chunk_index.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        _compare(captured, ring, e, n, 64)


def test_header_ring_past_4gib():
    """70 descriptors in slots of 64 MiB: slot 64 starts at byte offset 2^32. Only the first 64
    bytes of a valid slot are written; the rest of the ring stays zero."""
    n, stride = 70, 1 << 26
    need = n * stride + (1 << 28)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %d MiB of free device memory" % (need >> 20))
    cs = C.batch(n, invalid_at=(0, 63, 65))
    e = C.Expected(cs, dict(mac=C.MAC, ip_id=0xFFE0), 64)
    for shift in (0, 2):
        arena = torch.zeros(shift + n * stride, dtype=torch.uint8, device=DEV)
        ring = arena[shift:]
        res = A.tcp_tx_control(C.to_array(cs), _iface(ip_id=0xFFE0), hdr_stride=stride, headers=ring)
        torch.cuda.synchronize()
        slots = ring.view(n, stride)
        got = slots[:, :64].cpu().numpy()
        assert np.array_equal(got, _want_ring(e, n, 64, fill=0)), shift
        assert res.counts.cpu().numpy().tolist() == e.counts.tolist()
        assert np.array_equal(res.hdr_lens.cpu().numpy(), e.hdr_len)
        slots[:, :64] = 0
        assert not bool(arena.any()), "bytes outside the first 64 of a slot"
        del slots, ring, arena, res
        torch.cuda.empty_cache()


def test_tx_fill_header_split_changes_nothing():
    """Both checksums again by the Tx fill of header-split segments, zero chunks: no byte of an
    emitted slot changes (54-, 58- and 62-byte headers), each valid one is ACCEPT."""
    n = 300
    cs = C.batch(n, invalid_at=(3, 64))
    assert C.covers_the_ends(cs)                                    # the checksum 0x0000 among them
    res, ring, _, _ = _run(cs, 0xFFFA, 64)
    assert set(np.unique(res.hdr_lens.cpu().numpy()).tolist()) == {0, 54, 58, 62}
    before = ring.clone()
    st = A.tx_fill_header_split(res.headers, res.hdr_stride, res.hdr_lens, res.chunk_addr, res.chunk_len,
                                res.chunk_index)
    torch.cuda.synchronize()
    assert torch.equal(ring, before)
    ok = res.status.cpu().numpy() == C.EMITTED
    assert (st.cpu().numpy()[ok] == 6).all()                       # AIPSTACK_RX_ACCEPT
