"""The scenario generators of test_gpu_random_tcp.py, checked on the CPU: over the full seed
range, with the oracle, the scenarios cover what the GPU tests rely on them to cover."""
import numpy as np
import pytest

import hsplit_cases as H
import random_tcp_cases as G
import tcprx_cases as R
import tcpseg_cases as S


def _accepted_and_not(accepted, seed):
    """At least one element accepted; from 8 elements on, at least one not."""
    assert accepted.any(), seed
    if accepted.size >= 8:
        assert not accepted.all(), seed


@pytest.fixture(scope="module")
def hsplit(oracle):
    return [G.hsplit_scenario(oracle, s) for s in range(G.SEEDS)]


@pytest.fixture(scope="module")
def tcpseg(oracle):
    return [G.tcpseg_scenario(oracle, s) for s in range(G.SEEDS)]


@pytest.fixture(scope="module")
def tcprx(oracle):
    return [G.tcprx_scenario(oracle, s) for s in range(G.SEEDS)]


def test_hsplit_scenarios(hsplit):
    statuses, cells, strides, empty, above = set(), set(), set(), 0, 0
    for sc in hsplit:
        assert 1 <= sc.n <= G.MAX_ELEMENTS and sc.want_st.size == sc.n
        _accepted_and_not(sc.want_st == H.ACCEPT, sc.seed)
        statuses |= set(sc.want_st.tolist())
        strides.add(sc.stride)
        for i in np.nonzero(sc.want_st == H.ACCEPT)[0]:
            cells.add((bool(sc.swapped[i]), (sc.shift + int(i) * sc.stride) % 16))
        empty += sum(1 for seg in sc.sp.chunks for _, ln in seg if ln == 0)
        above += int((sc.sp.hdr_lens > min(sc.stride, H.MAX_SPLIT_HEADER)).sum())
        assert (sc.want_st[sc.sp.hdr_lens > min(sc.stride, H.MAX_SPLIT_HEADER)] == H.SPLIT_LAYOUT).all()
    # every status a Tx fill can return: 2, 5 and 7 are verdicts of Rx verify alone (a bad or an
    # absent checksum is what the fill overwrites)
    assert statuses == {0, 1, 3, 4, 6, 8, H.SPLIT_LAYOUT}
    # the swapped (odd in-slot L4 length) and the unswapped case at every slot residue mod 16
    assert cells == {(s, r) for s in (False, True) for r in range(16)}
    assert {sc.shift % 16 for sc in hsplit} == set(range(16))
    assert strides == set(G.HS_STRIDES) and empty >= 100 and above >= 40
    assert any(sc.n < 8 for sc in hsplit) and any(sc.n > 1024 for sc in hsplit)


def test_tcpseg_scenarios(tcpseg):
    ident = seq = odd = zero = mismatch = 0
    classes = set()
    for sc in tcpseg:
        n = len(sc.e.status)
        assert 1 <= n <= G.MAX_ELEMENTS + 2 and 1 <= len(sc.batch.cases) <= 120
        assert set(sc.e.status.tolist()) <= {S.ACCEPT, S.BURST_INVALID}
        _accepted_and_not(sc.e.status == S.ACCEPT, sc.seed)
        i, q = G.tcpseg_wraps(sc)
        ident, seq = ident + i, seq + q
        odd += S.count_straddle_odd_first(sc.e)
        d = np.diff(sc.si.astype(np.int64))
        zero += int(((d[1:-1] == 0) & (d[:-2] > 0)).sum())
        for c in sc.batch.cases:
            if not S.descriptor_ok(c):
                classes.add((c["mss"], tuple(c["reserved"]), c["flags"] & ~S.FIN, c["hdr"][12:15],
                             c["hdr"][23], c["pieces"][0][1]))
            elif "give" in c:
                mismatch += 1
    assert ident >= 1 and seq >= 1          # each wrap inside a burst of 3 or more segments
    assert odd >= 1                         # a straddling segment with an odd first part
    assert zero >= 10 and mismatch >= 20 and len(classes) == len(S.INVALID_CLASSES)
    assert {sc.stride for sc in tcpseg} == set(G.TS_STRIDES)
    lines = [sc.stride == 64 and sc.shift == 0 for sc in tcpseg]        # both emit forms
    assert sum(lines) >= 3 and len(lines) - sum(lines) >= 20


def test_tcprx_scenarios(tcprx):
    verdicts, branches, wave = set(), set(), 0
    for sc in tcprx:
        assert 1 <= sc.n <= G.MAX_ELEMENTS
        verdicts |= set(sc.e.verdict.tolist())
        _accepted_and_not(sc.e.verdict == R.ACCEPT, sc.seed)
        assert sc.e.segs["opts"][0] & R.SEG_VALID
        branches |= G.tcprx_option_branches(sc)
        wave += G.tcprx_hit_and_miss_in_a_wave(sc)
    assert verdicts == set(range(9)) | {R.DROP_TCP_OFFSET}
    assert branches == set(R.STOP_SKIP_BRANCHES) | {"mss", "wnd_scale"}
    assert wave >= 10                       # a table hit and a miss in the same wave
    assert {sc.seg_shift for sc in tcprx} == {0, 8} and len({sc.lead for sc in tcprx}) >= 12
    # the slotted form meets both store forms, lengths above the stride and bad offsets
    assert {(sc.stride, sc.seg_shift) for sc in tcprx} >= {(s, h) for s in (192, 2048) for h in (0, 8)}
    assert sum(int((sc.lens > sc.stride).sum()) for sc in tcprx) >= 10
    assert sum(int((sc.slot_e.verdict == R.DROP_TCP_OFFSET).sum()) for sc in tcprx) >= 10
