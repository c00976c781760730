"""The two Tx kernels held to what the reference stack puts on the wire: every burst and datagram
of tests/golden/stack_tx_ref_cases.json (recorded from the reference's IpStack with its TCP and UDP
protocols on a capture driver) goes through aipstack_tcp_tx_segment / aipstack_udp_tx_fragment as
one batch, then through tx_linearise_slotted and rx_verify_slotted. Only the fixture is read.

Every comparison is bit-exact or a hash of exact bytes: statuses, the header bytes behind the
Ethernet header against the recorded ones, the bytes the chunk table names against the recorded
FNV, the segment and fragment counts (the host layout's, which the kernels check against their
own plan)."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import ipfrag_cases as U
import stack_ref_batches as S
import tcpseg_cases as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOT = 2048
SENTINEL = 0xC3
RX_FRAGMENT, RX_ACCEPT = 3, 6        # AIPSTACK_RX_FRAGMENT, AIPSTACK_RX_ACCEPT (chksum.h)


def _tune(key, value):
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == A.AIPSTACK_CHKSUM_OK


def _check(res, want, index, hdr_of, dpay, payload):
    """Statuses, counts, header bytes from byte 14 on and the chunk table's bytes of a result
    against the recorded packets."""
    n = len(want)
    assert int(index[-1]) == n
    st = res.status.cpu().numpy()
    assert st.size == n and (st == RX_ACCEPT).all(), np.nonzero(st != RX_ACCEPT)[0][:8]
    hdr = res.headers.cpu().numpy().reshape(n, res.hdr_stride)
    lens = res.hdr_lens.cpu().numpy()
    ci = res.chunk_index.cpu().numpy().view(np.uint64).astype(np.int64)
    ca = res.chunk_addr.cpu().numpy().view(np.uint64).astype(np.int64) - dpay.data_ptr()
    cl = res.chunk_len.cpu().numpy().view(np.uint32).astype(np.int64)
    assert ci[0] == 0 and (np.diff(ci) >= 0).all() and ci[n] == ca.size == cl.size
    assert ((ca >= 0) & (ca + cl <= payload.size) & (cl > 0)).all()
    for i, p in enumerate(want):
        assert int(lens[i]) == hdr_of(p), i
        assert hdr[i, 14:int(lens[i])].tobytes() == p.ip + p.l4, i
        data = S.chunk_bytes(payload, [(int(ca[j]), int(cl[j])) for j in range(ci[i], ci[i + 1])])
        assert (len(data), S.fnv(data)) == (p.length, p.fnv), i
    assert np.array_equal(dpay.cpu().numpy(), payload)


def _linear_frames(res, want, hdr_of, frame_max):
    """tx_linearise_slotted then rx_verify_slotted: the frames from byte 14 on are the recorded
    header and data; returns the verdicts."""
    n = len(want)
    ring = torch.full((n * SLOT,), SENTINEL, dtype=torch.uint8, device=DEV)
    lin = A.tx_linearise_slotted(ring, SLOT, res, frame_max=frame_max)
    lens = lin.lens.cpu().numpy()
    assert np.array_equal(lens, [hdr_of(p) + p.length for p in want])
    verdict = A.rx_verify_slotted(ring, SLOT, lin.lens).cpu().numpy()
    got = ring.cpu().numpy().reshape(n, SLOT)
    for i, p in enumerate(want):
        h = hdr_of(p)
        assert got[i, 14:h].tobytes() == p.ip + p.l4, i
        assert S.fnv(got[i, h:h + p.length].tobytes()) == p.fnv, i
        assert (got[i, h + p.length:] == SENTINEL).all(), i
    return verdict


def test_tcp_segments_are_the_reference_stack_s():
    batch, records = S.tcp_batch()
    want, index = S.flat(records)
    assert 1000 <= len(want) <= 5000
    dpay = torch.from_numpy(batch.payload.copy()).to(DEV)
    desc = T.descriptors(batch, dpay.data_ptr(), A.TCP_BURST_DTYPE)
    si, cb = A.tcp_burst_layout(desc)
    assert np.array_equal(si.astype(np.int64), index), "segment counts per burst"
    hdr_of = lambda p: T.HDR                                              # noqa: E731
    seg = A.tcp_tx_segment(desc, si, cb)
    _check(seg, want, index, hdr_of, dpay, batch.payload)
    _tune("aux_blocks", 1)
    try:
        capped = A.tcp_tx_segment(desc, si, cb)
        torch.cuda.synchronize()
    finally:
        _tune("aux_blocks", -1)
    _check(capped, want, index, hdr_of, dpay, batch.payload)
    _check(A.tcp_tx_segment(desc, si, cb, just_written=True), want, index, hdr_of, dpay, batch.payload)
    verdict = _linear_frames(seg, want, hdr_of, 1514)
    assert (verdict == RX_ACCEPT).all()


def test_udp_fragments_are_the_reference_stack_s():
    batch, records = S.udp_batch()
    want, index = S.flat(records)
    assert 300 <= len(want) <= 5000
    dpay = torch.from_numpy(batch.payload.copy()).to(DEV)
    desc = U.descriptors(batch, dpay.data_ptr(), A.UDP_DGRAM_DTYPE)
    fi, cb, st = A.udp_dgram_layout(desc)
    assert np.array_equal(fi.astype(np.int64), index), "fragment counts per datagram"
    assert (st == RX_ACCEPT).all()
    hdr_of = lambda p: U.HDR0 if p.l4 else U.HDRK                         # noqa: E731
    frags = A.udp_tx_fragment(desc, fi, cb)
    assert (frags.dgram_status.cpu().numpy() == RX_ACCEPT).all()
    _check(frags, want, index, hdr_of, dpay, batch.payload)
    _tune("aux_blocks", 1)
    try:
        capped = A.udp_tx_fragment(desc, fi, cb)
        torch.cuda.synchronize()
    finally:
        _tune("aux_blocks", -1)
    _check(capped, want, index, hdr_of, dpay, batch.payload)
    _check(A.udp_tx_fragment(desc, fi, cb, just_written=True), want, index, hdr_of, dpay, batch.payload)
    verdict = _linear_frames(frags, want, hdr_of, 1514)
    # a whole datagram is accepted with its checksums verified; a fragment whose header verifies
    # gets rx_verify's "fragment" verdict (the datagram's checksum is reassembly's to verify)
    # (the scenarios craft 6 unfragmented datagrams per MTU; the random ones add some)
    whole = np.array([len(r) == 1 for r in records for _ in r])
    assert (verdict[whole] == RX_ACCEPT).all() and whole.sum() >= 24
    assert (verdict[~whole] == RX_FRAGMENT).all() and (~whole).sum() >= 300
