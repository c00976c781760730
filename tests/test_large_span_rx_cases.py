"""The case generators of test_gpu_large_span_rx.py, checked on the CPU for fake base pointers
(one of them a multiple of 2^32): the cases reach the edges they claim, with the frames and the
model's answers that the GPU tests rely on."""
import numpy as np
import pytest

import icmp_cases as IC
import large_span_cases as L
import large_span_rx_cases as C
import udp_rx_cases as UC

BASES = (7 << 32, 0x7F1234567000, 0x7E00C0001000)


@pytest.mark.parametrize("P", BASES)
def test_csr_cases(oracle, P):
    met, splits = set(), set()
    for shift in L.SHIFTS:
        for kind in C.DISTANCES:
            c = C.csr_case(P, shift, kind)
            L.check_windows(c.windows)
            assert {L.E31, L.E32} <= set(c.edges) and len(c.edges) == (2 if P % L.E32 == 0 else 3)
            if shift == 0 or len(c.edges) == 3:      # (an aligned P: offset 2^32 is that address for shift 0)
                assert any((P + shift + e) % L.E32 == 0 for e in c.edges)
            assert L.span_of_64(c.offsets) <= 4 * L.MiB and c.n > 65536       # the scan's second step
            fv = C.filler_verdicts(oracle, [L.FILL])
            assert fv == {L.FILL: 0}                                          # NOT_IP4
            for (i, name), e in zip(c.across, c.edges):
                f = c.frames[i]
                d = e - int(c.offsets[i])
                assert f == C.pool()[0][name] and 0 < d < len(f) and int(c.offsets[i + 1]) > e
                assert d == (len(f) - 1 if kind == "len-1" else kind)
                met.add((name, kind))
                hl = (f[14] & 0xF) * 4
                splits.add("eth" if d < 14 else "ip" if d < 14 + hl else "l4" if d < 14 + hl + 8 else "data")
            # the windows hold exactly the frames, at their offsets
            for w in c.windows:
                i = int(np.searchsorted(c.offsets, np.uint64(w.start - shift)))
                assert int(c.offsets[i]) == w.start - shift
                assert w.data[:len(c.frames[i])].tobytes() == c.frames[i]
            eu = C.expected_udp(oracle, c.n, c.lens, c.frames)
            codes = dict(zip(sorted(c.frames), C.host_codes([c.frames[i] for i in sorted(c.frames)])))
            ei = C.expected_icmp(oracle, c.n, c.lens, c.frames, codes)
            for (i, name), e in zip(c.across, c.edges):
                rec = eu.dgrams[i]
                if name == "udp_hit":
                    assert rec["assoc"] == 3 and rec["listeners"] == 1 and i in eu.deliver_frame
                elif name in ("udp_closed", "udp_code3"):
                    assert eu.unreach[i] == UC.PORT_UNREACH and ei.status[i] == IC.UNREACH
                else:
                    assert ei.status[i] == IC.ECHO_REPLY and not rec["flags"]
                # responders and non-responders on either side, and a chunk beyond the edge
                lo, hi = i - 9, i + 12
                assert (ei.status[lo:i] == IC.NONE).any() and (ei.hdr_len[lo:i] != 0).any()
                assert (ei.status[i + 1:hi] == IC.NONE).any() and (ei.hdr_len[i + 1:hi] != 0).any()
                assert any(fi > i and fi < hi for fi, _, _ in ei.chunks)
                assert (eu.dgrams["flags"][i + 1:hi] != 0).any() and (eu.unreach[lo:i] != UC.NO_UNREACH).any()
            fill = np.ones(c.n, dtype=bool)
            fill[sorted(c.frames)] = False
            assert not eu.dgrams[fill].tobytes().strip(b"\0") and (eu.unreach[fill] == UC.NO_UNREACH).all()
            assert (ei.status[fill] == IC.NONE).all() and not ei.hdr_len[fill].any()
            assert int(eu.counts[0]) >= 6 and int(eu.counts[1]) >= 6 and int(ei.counts[0]) >= 20
    assert met == {(s, k) for s in C.STRADDLERS for k in C.DISTANCES}
    assert splits == {"eth", "ip", "l4", "data"}


def test_slotted_cases(oracle):
    for stride, n in C.SLOTTED:
        assert n == 65600 and (n - 1) * stride > L.E32 and n > 256 * 256
        for shift in L.SHIFTS:
            c = C.slotted_case(stride, n, shift)
            L.check_windows(c.windows)
            assert {0, n - 1} < set(c.frames) and (c.lens != 0).sum() == len(c.frames)
            for e in L.EDGES:
                assert any(s * stride < e for s in c.frames if s) and any(e <= s * stride for s in c.frames if s < n - 1)
                assert {e // stride - 1, e // stride, e // stride + 1} < set(c.frames)
            eu = C.expected_udp(oracle, n, c.lens, c.frames)
            ei = C.expected_icmp(oracle, n, c.lens, c.frames, None)
            assert int(eu.counts[0]) >= 3 and int(eu.counts[1]) >= 3 and int(ei.counts[0]) >= 4
            # deliveries, unreach requests and responses on the far side of 2^32
            far = L.E32 // stride
            assert (eu.deliver_frame[:int(eu.counts[0])] > far).any() and (eu.unreach[far:] != UC.NO_UNREACH).any()
            assert (ei.response_frame[:int(ei.counts[0])] > far).any()


def test_ring_case(oracle):
    c = C.ring_case(oracle)
    assert c.n == 65600 and C.RING_STRIDE * 32768 == L.E31 and C.RING_STRIDE * 65536 == L.E32
    assert {32767, 32768, 32769, 65535, 65536, 65537, 0, 61} < set(c.rows.tolist())
    assert np.array_equal(np.flatnonzero(c.e.hdr_len), c.rows) and int(c.e.counts[0]) == c.rows.size
    assert sorted(c.e.headers) == c.rows.tolist() and (c.e.status[c.rows] == IC.ECHO_REPLY).all()
    assert L.RING_STRIDE * (c.n - 1) + 64 <= L.ARENA_BYTES - max(L.SHIFTS)
    # the Ident wraps within the batch
    assert C.IFACE["ip_id"] + c.rows.size > 0x10000
