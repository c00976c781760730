"""What the large-span linearise cases cover, for fake base pointers (no GPU): ring slots that
start 2^31 and 2^32 bytes from the base, CSR frames across both offsets, source chunks and header
slots below, above and across a 4 GiB-aligned address; windows disjoint and small; everything
inside the arena."""
import numpy as np
import pytest

import large_span_cases as L
import large_span_linearise_cases as C
import linearise_cases as LC

POINTERS = [0x7F3A_4020_0000, 0x7000_0000_0000, 0x7F00_FFF0_0000, 0x7F00_8000_0000]


def test_ring_case_reaches_both_edges():
    for shift in (0, 15):
        c = C.ring_case(0x1000, shift)
        assert c.n * c.slot_stride > L.E32 and shift + c.n * c.slot_stride <= L.ARENA_BYTES
        assert c.frame_start(32768) == L.E31 and c.frame_start(65536) == L.E32
        lens, status = c.plan()
        assert (status == LC.WRITTEN).all() and lens.max() < C.ROW and lens.min() == 54
        rows = C.ring_rows()
        assert {32767, 32768, 65535, 65536, c.n - 1} <= set(rows) and len(rows) > 1000
        for i in (32768, 65536):
            assert c.frame(i).size == lens[i]


@pytest.mark.parametrize("distance", C.DISTANCES)
def test_csr_case_crosses_both_edges(distance):
    for shift in (0, 15):
        c = C.csr_case(0x1000, shift, distance)
        lens, status = c.plan()
        off = c.offsets.astype(np.int64)
        assert (np.diff(off) >= 0).all() and shift + off[-1] <= L.ARENA_BYTES
        assert (status[c.fillers] == LC.SKIPPED).all()
        assert (np.delete(status, c.fillers) == LC.WRITTEN).all()
        for edge, j in zip(L.EDGES, c.across):
            d = int(lens[j]) - 1 if distance == "len-1" else distance
            assert off[j] == edge - d and off[j] < edge < off[j + 1]
        first, count = c.runs[-1]
        assert off[first] > L.E32 and first + count == c.n
        for f in c.fillers:
            assert off[f + 1] - off[f] > 1 << 28


@pytest.mark.parametrize("P", POINTERS)
def test_source_cases_lie_round_an_aligned_address(P):
    e = C.address_edge(P)
    assert (P + e) % L.E32 == 0
    c = C.source_case(P, "payload")
    L.check_windows(c.windows)
    lens, status = c.plan()
    assert (status == LC.WRITTEN).all()
    A4 = P + e
    ends = c.chunk_addr + c.chunk_len
    live = c.chunk_len > 0
    assert (live & (ends <= A4)).sum() > 100 and (live & (c.chunk_addr >= A4)).sum() > 100
    assert len(c.across) >= 2 * len(C.DISTANCES)
    for k in c.across:
        assert c.chunk_addr[k] < A4 < ends[k]
    assert {int(A4 - c.chunk_addr[k]) for k in c.across} >= {1, 15, 16, 17}
    for k in range(c.chunk_len.size):       # the model's bytes are the window's
        o = int(c.chunk_addr[k] - P) - c.windows[0].start
        assert np.array_equal(c.chunk_bytes(k), c.windows[0].data[o:o + int(c.chunk_len[k])])
    h = C.source_case(P, "headers")
    L.check_windows(h.windows)
    assert P + h.hdr_off + (h.n // 2) * C.HDR_STRIDE == A4
    assert h.hdr_off > 0 and h.hdr_off + h.hdr.size < L.ARENA_BYTES
