"""IPv4 reassembly on receive, 40 seeded scenarios (ipreass_cases.scenario: complete groups of
every protocol and datagram verdict, incomplete groups of every cause, empty fragments, whole
frames, shuffled) on the GPU against the model; test_random_ipreass_cases.py asserts what the
generator covers."""
import pytest

import aipstack_amd as A

import ipreass_cases as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ipreass_gpu as H  # noqa: E402


@pytest.mark.parametrize("seed", R.SEEDS)
def test_scenario(oracle, seed):
    A.contract_violations(clear=True)
    s = R.scenario(oracle, seed)
    e, out, (dbuf, doff, addr) = H.run(oracle, s.batch, s.max_reass)
    first = out.bytes()
    out.poison()
    A.ip4_rx_reassemble(dbuf, doff, max_reass_size=s.max_reass, **out.kw())
    assert out.bytes() == first
    assert A.contract_violations(clear=True) == 0
