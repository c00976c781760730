"""The scenario generator of test_gpu_random_ipfrag.py, checked on the CPU: over the full seed
range, from the model alone, the scenarios take every branch of the fragmentation loop that the
GPU test relies on them to take."""
import numpy as np
import pytest

import ipfrag_cases as T
import random_ipfrag_cases as G


@pytest.fixture(scope="module")
def scenarios(oracle):
    return [G.scenario(oracle, s) for s in range(G.SEEDS)]


def test_scenarios_take_every_branch(scenarios):
    got, invalid, mismatch, classes = set(), 0, 0, set()
    for sc in scenarios:
        n = len(sc.e.status)
        assert 1 <= n <= G.MAX_FRAGS and 1 <= len(sc.batch.cases) <= 70
        assert set(sc.e.status.tolist()) <= {T.ACCEPT, T.DGRAM_INVALID}
        assert (sc.e.status == T.ACCEPT).any(), sc.seed
        got |= T.branches(sc.batch, sc.e)
        for c in sc.batch.cases:
            if not T.descriptor_ok(c):
                invalid += 1
                classes.add((c["mtu"], c["reserved"], c["hdr"][12:15], c["hdr"][20:22], c["hdr"][23],
                             c["pieces"][0][1]))
            elif "give" in c:
                mismatch += 1
    assert got >= {"S=0", "S=1", "S>1", "S>64", "straddle", "no_straddle", "edge", "clamped",
                   "last>F", "0xFFFF"}, got
    assert invalid >= 10 and mismatch >= 10 and len(classes) >= 6
    assert {sc.stride for sc in scenarios} == set(G.STRIDES)
    lines = [sc.stride == 64 and sc.shift == 0 for sc in scenarios]        # both emit forms
    assert sum(lines) >= 3 and len(lines) - sum(lines) >= 20
    assert any(sc.just_written for sc in scenarios) and not all(sc.just_written for sc in scenarios)


def test_scenarios_are_reproducible(oracle, scenarios):
    again = G.scenario(oracle, 7)
    assert np.array_equal(again.e.headers, scenarios[7].e.headers)
    assert np.array_equal(again.fi, scenarios[7].fi) and np.array_equal(again.batch.payload,
                                                                        scenarios[7].batch.payload)
