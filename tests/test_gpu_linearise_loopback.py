"""From what we send to what we receive: the Tx builders' output, linearised on the GPU
(tx_linearise_slotted / tx_linearise with the builder's own result object, its `status` as
d_seg_status and its `hdr_lens`), goes through our own Rx calls and the linear Tx fill.
Expectations come from the builders' models (tcpseg_cases, ipfrag_cases) and the CPU oracle."""
import numpy as np
import pytest

import aipstack_amd as A

import hsplit_cases as H
import ipfrag_cases as I
import linearise_cases as LC
import tcpseg_cases as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOT = 2048


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ring(n):
    return torch.full((n * SLOT,), LC.SENTINEL, dtype=torch.uint8, device=DEV)


def test_tcp_segments_to_rx_parse(oracle):
    """tcp_tx_segment -> linearise into 2048-byte slots -> rx_verify_slotted and
    tcp_rx_parse_slotted: every frame accepted, seq / flags / data_len the burst plan's, the data
    bytes at data_off the send ring's. Bursts whose range wraps (two pieces), an mss of 1, FINs,
    one invalid burst in the middle (its segments skipped)."""
    rng = np.random.default_rng(31)
    payload = T.payload_bytes(1 << 16, seed=31)
    cases = [T.burst((5, 300), mss=1, seq=0xFFFFFF00, flags=T.FIN)]
    for b in range(160):
        mss = (7, 100, 536, 1460)[b % 4]
        d = int(rng.integers(1, 40 * mss)) if mss < 536 else int(rng.integers(1, 30000))
        o = int(rng.integers(0, 30000))
        if b % 3 == 0:                              # the range wraps: two pieces
            a = int(rng.integers(1, d + 1))
            p0, p1 = (o, a), (int(rng.integers(0, 30000)), d - a)
        else:
            p0, p1 = (o, d), (0, 0)
        cases.append(T.burst(p0, p1, mss=mss, seq=int(rng.integers(0, 1 << 32)), psh_offset=d,
                             ip_id=int(rng.integers(0, 1 << 16)), flags=b % 2))
    cases.insert(20, T.burst((0, 50), mss=0, give=(3, 3)))      # breaks the contract
    batch = T.Batch(cases, payload)
    si, cb = T.caller_index(cases)
    e = T.expected(oracle, batch, si, cb)
    n = len(e.status)
    ok = e.status == T.ACCEPT
    assert 2000 <= n <= 8000 and (~ok).sum() == 3
    assert sum(len(ch) == 2 for ch in e.seg_chunks) >= 10
    dpay = _d(payload)
    seg = A.tcp_tx_segment(T.descriptors(batch, dpay.data_ptr(), A.TCP_BURST_DTYPE), si, cb)
    ring = _ring(n)
    lin = A.tx_linearise_slotted(ring, SLOT, seg, frame_max=1514)
    st = lin.status.cpu().numpy()
    assert np.array_equal(st, np.where(ok, LC.WRITTEN, LC.SKIPPED))
    want_len = np.array([54 + sum(l for _, l in ch) for ch in e.seg_chunks]) * ok
    assert np.array_equal(lin.lens.cpu().numpy(), want_len)
    verdict = A.rx_verify_slotted(ring, SLOT, lin.lens).cpu().numpy()
    assert (verdict[ok] == T.ACCEPT).all() and (verdict[~ok] == 0).all()
    parsed = A.tcp_rx_parse_slotted(ring, SLOT, lin.lens)
    assert np.array_equal(parsed.verdict.cpu().numpy(), verdict)
    rec = parsed.segs_numpy()
    got = ring.cpu().numpy().reshape(n, SLOT)
    start = 0
    for i in range(n):
        c = cases[int(e.seg_case[i])]
        if e.seg_k[i] == 0:
            start = 0
        if not ok[i]:
            assert (got[i] == LC.SENTINEL).all() and rec[i]["opts"] == 0
            continue
        ln = int(want_len[i]) - 54
        assert rec[i]["opts"] & A.AIPSTACK_TCP_SEG_VALID
        assert rec[i]["seq_num"] == (c["seq"] + start) & 0xFFFFFFFF
        assert rec[i]["flags"] == e.seg_flags[i] and rec[i]["data_len"] == ln
        off = int(rec[i]["data_off"])
        data = b"".join(payload[o:o + l].tobytes() for o, l in e.seg_chunks[i])
        assert off == 54 and got[i, off:off + ln].tobytes() == data
        assert (got[i, 54 + ln:] == LC.SENTINEL).all()
        start += ln


@pytest.mark.parametrize("mtu", [256, 576, 1500])
def test_udp_fragments_to_reassembly(oracle, mtu):
    """udp_tx_fragment -> linearise -> ip4_rx_reassemble_slotted: every valid datagram comes
    back complete with a good UDP checksum, and its chunk list, read back from the ring, is the
    original payload. D of 0, M mod 8 != 0 (mtu 1006 is not asked for; 256 - 20 and 576 - 20 are
    no multiples of 8), two-piece payloads, one invalid datagram (nothing emitted)."""
    rng = np.random.default_rng(40 + mtu)
    payload = I.payload_bytes(1 << 16, seed=mtu)
    assert mtu == 1500 or (mtu - 20) % 8 != 0
    cases = [I.dgram((0, 0), mtu=mtu, ip_id=0)]
    for d in range(1, 90):
        D = int(rng.integers(1, 12 * mtu)) if d % 5 else int(rng.integers(1, mtu - 28))
        D = min(D, 20000)
        o = int(rng.integers(0, 30000))
        if d % 3 == 0:
            a = int(rng.integers(1, D + 1))
            p0, p1 = (o, a), (int(rng.integers(0, 30000)), D - a)
        else:
            p0, p1 = (o, D), (0, 0)
        cases.append(I.dgram(p0, p1, mtu=mtu, ip_id=d))
    cases.insert(30, I.dgram((0, 100), mtu=100, ip_id=999, give=(2, 2)))    # mtu below the minimum
    batch = I.Batch(cases, payload)
    fi, cb = I.caller_index(cases)
    e = I.expected(oracle, batch, fi, cb)
    n = len(e.status)
    ok = e.status == I.ACCEPT
    assert (~ok).sum() == 2 and 300 <= n <= 8000
    dpay = _d(payload)
    frags = A.udp_tx_fragment(I.descriptors(batch, dpay.data_ptr(), A.UDP_DGRAM_DTYPE), fi, cb)
    ring = _ring(n)
    lin = A.tx_linearise_slotted(ring, SLOT, frags, frame_max=14 + mtu)
    assert np.array_equal(lin.status.cpu().numpy(), np.where(ok, LC.WRITTEN, LC.SKIPPED))
    lens = lin.lens.cpu().numpy()
    assert np.array_equal(lens, [len(I.frame_of(e, payload, i)) if ok[i] else 0 for i in range(n)])
    r = A.ip4_rx_reassemble_slotted(ring, SLOT, lin.lens)
    verdict = r.verdict.cpu().numpy()
    nxt, head, dg = r.next_numpy(), r.head_numpy(), r.dgram_numpy()
    ca = r.chunk_addr.cpu().numpy().view(np.uint64)
    cl = r.chunk_len.cpu().numpy().view(np.uint32)
    got = ring.cpu().numpy()
    base = ring.data_ptr()
    whole = fragmented = 0
    for d, c in enumerate(cases):
        ids = np.nonzero((e.frag_case == d) & ok)[0]
        if ids.size == 0:
            continue
        (o0, l0), (o1, l1) = c["pieces"]
        data = payload[o0:o0 + l0].tobytes() + payload[o1:o1 + l1].tobytes()
        first = int(ids[0])
        if ids.size == 1:                           # not fragmented: Rx verify's own verdict
            assert verdict[first] == I.ACCEPT
            f = got[first * SLOT:first * SLOT + lens[first]]
            assert f[42:].tobytes() == data
            whole += 1
            continue
        assert (verdict[ids] == A.AIPSTACK_RX_FRAG_MEMBER).all() and (head[ids] == first).all()
        assert dg[first]["verdict"] == I.ACCEPT and dg[first]["n_frags"] == ids.size
        assert dg[first]["data_len"] == 8 + len(data) and dg[first]["proto"] == 17
        body, i, steps = b"", first, 0
        while i != A.AIPSTACK_REASS_NONE:
            at = int(ca[i]) - base
            assert i * SLOT + 34 == at
            body += got[at:at + int(cl[i])].tobytes()
            i, steps = int(nxt[i]), steps + 1
        assert steps == ids.size and body[8:] == data
        fragmented += 1
    assert whole >= 10 and fragmented >= 50
    assert (got.reshape(n, SLOT)[~ok] == LC.SENTINEL).all()


def test_split_layout_segments_to_the_linear_fill(oracle):
    """Segments the header-split fill answers with AIPSTACK_TX_SPLIT_LAYOUT (and the ones it
    fills) -> linearise (offsets form, the fill's status as d_seg_status) -> tx_fill on the linear
    frames: the bytes and statuses the frame oracle gives on the original frames."""
    frs = [f for f in H.golden_frames() if len(f) >= 14]
    buf, off = H.pack(frs)
    n = len(frs)
    classes = ("short4", "l4_fixed", "l4_plus1", "whole")
    points = [H.split_points(frs, cls, 128) for cls in classes]
    at = [points[i % 4][i] for i in range(n)]
    assert min(at) >= 14
    sp = A.split_frames(buf, off, at, hdr_stride=128, payload_pieces=[[7, 33]] * n, payload_gap=3)
    headers, hdr_lens, dpay = _d(sp.headers), _d(sp.hdr_lens.view(np.int32)), _d(sp.payload)
    addr, lens, index = sp.chunk_table(dpay.data_ptr())
    tab = dict(headers=headers, hdr_stride=128, hdr_lens=hdr_lens, chunk_addr=_d(addr.view(np.int64)),
               chunk_len=_d(lens.view(np.int32)), chunk_index=_d(index.view(np.int64)))
    st = A.tx_fill_header_split(headers, 128, hdr_lens, tab["chunk_addr"], tab["chunk_len"],
                                tab["chunk_index"])
    assert (st.cpu().numpy() == H.SPLIT_LAYOUT).sum() >= 300
    dest = torch.full((buf.size,), LC.SENTINEL, dtype=torch.uint8, device=DEV)
    doff = _d(off.view(np.int64))
    lin = A.tx_linearise(dest, doff, seg_status=st, frame_max=65535, **tab)
    assert (lin.status.cpu().numpy() == LC.WRITTEN).all()
    assert np.array_equal(lin.lens.cpu().numpy(), np.diff(off.astype(np.int64)))
    got_st = A.tx_fill(dest, doff).cpu().numpy()
    want = buf.copy()
    want_st = oracle.tx_fill_batch(want, off)
    assert np.array_equal(got_st, want_st)
    assert np.array_equal(dest.cpu().numpy(), want)
