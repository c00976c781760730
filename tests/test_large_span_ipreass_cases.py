"""What the large-span reassembly case covers, for fake base pointers (no GPU): the frame that
holds each edge byte is a fragment of a complete datagram whose list goes on to the other side of
the edge; offsets cross 2^31 and 2^32, an address crosses a multiple of 2^32; 64 frames span at
most 4 MiB; windows are disjoint and small."""
import numpy as np
import pytest

import ipreass_cases as R
import large_span_cases as L
import large_span_ipreass_cases as C


@pytest.mark.parametrize("P", [0x7F3A_4020_0000, 0x7000_0000_0000, 0x7F00_FFF0_0000, 0x7F00_8000_0000])
@pytest.mark.parametrize("distance", C.DISTANCES)
def test_case_covers_the_edges(oracle, P, distance):
    for shift in (0, 15):
        c = C.case(P, shift, distance)
        L.check_windows(c.windows)
        assert L.span_of_64(c.offsets) <= 4 * L.MiB
        e = C.expected(oracle, c, 0)
        assert L.E31 in c.edges and L.E32 in c.edges
        if shift == 0:                                  # an edge at a 4 GiB-aligned address
            assert any((P + x) % L.E32 == 0 for x in c.edges)
        verdicts = {int(e.dgram[o[0]]["verdict"]) for o in e.complete.values()}
        assert {R.ACCEPT, R.L4_CHKSUM} <= verdicts and len(e.complete) >= 15
        assert (e.verdict == R.FRAGMENT).any()
        for edge, i in zip(c.edges, c.across):
            lo, hi = int(c.offsets[i]), int(c.offsets[i + 1])
            assert lo < edge < hi and e.verdict[i] == R.MEMBER
            order = next(o for o in e.complete.values() if i in o)
            k = order.index(i)
            # its neighbours in the list lie on the two sides of the edge
            assert int(c.offsets[order[k - 1] + 1]) <= edge <= int(c.offsets[order[k + 1]])
            assert e.next[i] == order[k + 1] and e.head[i] == order[0]
        for o in e.complete.values():                   # every datagram has members past 2^32
            ends = c.offsets[np.array(o) + 1]
            assert ends.min() < L.E31 < L.E32 < ends.max()
