"""The conditions the inputs of test_gpu_tx_fill_cut.py are built to hold (tx_fill_cut_cases.py),
checked on the CPU."""
import numpy as np
import pytest

import tx_fill_cut_cases as T


def test_every_tx_fill_status_occurs(oracle):
    seen = set()
    for name in T.STAGES:
        for family in ("A", "C"):
            for variant in T.VARIANTS:
                seen |= set(T.cached(oracle, name, family, "csr", False, variant)[3].tolist())
    assert seen == T.TX_STATUSES, seen


@pytest.mark.parametrize("name", T.STAGES)
def test_variants_differ_as_meant(oracle, name):
    """Zeroed frames have both fields 0 and the fill changes them; a filled buffer is its own
    expectation; the inverted layout of family C expects inverted surroundings."""
    lay, host, want, st = T.cached(oracle, name, "A", "csr", False, "zeroed")
    assert (st == 6).any() and not np.array_equal(host, want)
    _, host, want, _ = T.cached(oracle, name, "A", "csr", False, "filled")
    assert np.array_equal(host, want)
    plain = T.cached(oracle, name, "C", "slots2048", False, "raw")
    other = T.cached(oracle, name, "C", "slots2048", True, "raw")
    assert np.array_equal(plain[3], other[3]) and plain[0].stride % 128 == 0
    diff = plain[2] != other[2]
    assert diff.any() and (plain[2][diff] ^ other[2][diff] == 0xFF).all()


@pytest.mark.parametrize("layout", list(T.LAYOUTS))
def test_checksum_field_positions(oracle, layout):
    """Both checksum fields at every position within a 32-byte sector (31: across two), and in a
    sector that reaches behind the frame's end, over the shifts of the CSR form (frames back to
    back) and of the 256-byte slots; the other two strides add slot grids, not positions."""
    ip, l4, behind = set(), set(), set()
    for name in T.STAGES:
        lay = T.cached(oracle, name, "A", layout, False, "raw")[0]
        for shift in T.SHIFTS[layout]:
            for s, f in zip((lay.start + shift).tolist(), lay.frames):
                at = T.l4_field(f)
                if T.is_ip(f):
                    ip.add((s + 24) % 32)
                    if (s + 24) // 32 * 32 + 32 > s + len(f):
                        behind.add("ip")
                if at is not None:
                    l4.add((s + at) % 32)
                    if (s + at + 1) // 32 * 32 + 32 > s + len(f):
                        behind.add("l4")
    if layout in ("csr", "slots256"):
        want = set(range(32))
        assert ip >= want and l4 >= want, (sorted(want - ip), sorted(want - l4))
        assert behind == {"ip", "l4"}
    assert len(ip) >= 3 and len(l4) >= 3
    assert T.LAYOUTS["slots2048"] % 128 == 0 and T.LAYOUTS["slots264"] % 128
