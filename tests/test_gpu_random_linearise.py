"""The seeded linearise scenarios of linearise_cases on the GPU: TCP-shaped, UDP-fragment-shaped
and adversarial, slotted and offsets forms alternating (tests/test_linearise_host.py counts what
the set covers)."""
import pytest

import linearise_cases as LC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import linearise_gpu as G  # noqa: E402


@pytest.mark.parametrize("seed", range(LC.N_SCENARIOS))
def test_seeded_scenario(seed):
    sc = LC.scenario(seed)
    assert sc.form == ("slots" if seed % 2 == 0 else "csr")
    G.check(sc, just_written=bool(seed & 4))
