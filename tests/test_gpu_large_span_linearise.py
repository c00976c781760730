"""aipstack_tx_linearise / _slotted beyond 4 GiB (large_span_linearise_cases.py, on the arena of
large_span_cases.py): a destination ring whose slots 32768 and 65536 start 2^31 and 2^32 bytes
from d_frames, CSR offsets on both sides of 2^32, source chunks and header slots below, above and
across a device address that is a multiple of 2^32. A 32-bit-truncated offset or address lands in
the zero arena or in another slot, so a truncation shows as a wrong byte."""
import numpy as np
import pytest

import aipstack_amd as A

import large_span_cases as L
import large_span_linearise_cases as C
import linearise_cases as LC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def arena():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    a = torch.zeros(L.ARENA_BYTES, dtype=torch.uint8, device=DEV)
    A.contract_violations(clear=True)
    yield a
    del a
    torch.cuda.empty_cache()


def _tables(c, headers):
    return dict(headers=headers, hdr_stride=C.HDR_STRIDE, hdr_lens=_d(c.hdr_lens.view(np.int32)),
                chunk_addr=_d(c.chunk_addr.view(np.int64)), chunk_len=_d(c.chunk_len.view(np.int32)),
                chunk_index=_d(c.index.view(np.int64)), frame_max=c.frame_max)


def _outcome(c, res):
    lens, status = c.plan()
    assert np.array_equal(res.status.cpu().numpy(), status)
    assert np.array_equal(res.lens.cpu().numpy(), lens)
    return lens, status


def test_ring_of_65538_slots(arena):
    for shift in (0, 15):
        pool = torch.empty(C.POOL, dtype=torch.uint8, device=DEV)
        c = C.ring_case(pool.data_ptr(), shift)
        pool.copy_(_d(c.pool))
        ring = arena[shift:shift + c.n * C.STRIDE]
        rows = ring.view(c.n, C.STRIDE)[:, :C.ROW]
        try:
            res = A.tx_linearise_slotted(ring, C.STRIDE, **_tables(c, _d(c.hdr)))
            lens, _ = _outcome(c, res)
            got = rows.cpu().numpy()
            for i in C.ring_rows():
                assert np.array_equal(got[i, :lens[i]], c.frame(i)), i
            # every row: nothing behind its frame
            assert not (got * (np.arange(C.ROW)[None, :] >= lens[:, None])).any()
            assert (got[:, :6] != 0).any(axis=1).all()      # and every frame arrived in its own slot
        finally:
            rows.zero_()
        assert not bool(arena.view(torch.int64).any()), "bytes outside the frames' slots"
        assert np.array_equal(pool.cpu().numpy(), c.pool)
    assert A.contract_violations(clear=True) == 0


@pytest.mark.parametrize("distance", C.DISTANCES)
def test_csr_offsets_on_both_sides_of_4gib(arena, distance):
    for shift in (0, 15):
        pool = torch.empty(C.POOL, dtype=torch.uint8, device=DEV)
        c = C.csr_case(pool.data_ptr(), shift, distance)
        pool.copy_(_d(c.pool))
        off = c.offsets.astype(np.int64)
        spans = [(shift + int(off[f]), shift + int(off[f + k])) for f, k in c.runs]
        try:
            res = A.tx_linearise(arena[shift:], _d(off), **_tables(c, _d(c.hdr)))
            lens, _ = _outcome(c, res)
            for (f, k), (lo, hi) in zip(c.runs, spans):
                want = np.concatenate([c.frame(i) for i in range(f, f + k)])
                assert np.array_equal(arena[lo:hi].cpu().numpy(), want), (f, lo)
        finally:
            for lo, hi in spans:
                arena[lo:hi].zero_()
        assert not bool(arena.view(torch.int64).any()), "bytes outside the frames' rooms"
    assert A.contract_violations(clear=True) == 0


@pytest.mark.parametrize("what", ["payload", "headers"])
def test_sources_round_a_4gib_aligned_address(arena, what):
    P = arena.data_ptr()
    pool = torch.empty(C.POOL, dtype=torch.uint8, device=DEV)
    c = C.source_case(P, what)
    L.check_windows(c.windows)
    if what == "headers":
        c.chunk_addr = c.chunk_addr + np.uint64(pool.data_ptr())
        pool.copy_(_d(c.pool))
        headers = arena[c.hdr_off:c.hdr_off + c.hdr.size]
    else:
        headers = _d(c.hdr)
    dest = torch.full((c.n * c.slot_stride,), LC.SENTINEL, dtype=torch.uint8, device=DEV)
    try:
        for w in c.windows:
            arena[w.start:w.end].copy_(_d(w.data))
        res = A.tx_linearise_slotted(dest, c.slot_stride, **_tables(c, headers))
        lens, _ = _outcome(c, res)
        got = dest.cpu().numpy().reshape(c.n, c.slot_stride)
        for i in range(c.n):
            assert np.array_equal(got[i, :lens[i]], c.frame(i)), i
            assert (got[i, lens[i]:] == LC.SENTINEL).all(), i
        for w in c.windows:                                  # the sources are only read
            assert np.array_equal(arena[w.start:w.end].cpu().numpy(), w.data)
    finally:
        for w in c.windows:
            arena[w.start:w.end].zero_()
    assert not bool(arena.view(torch.int64).any())
    assert A.contract_violations(clear=True) == 0
