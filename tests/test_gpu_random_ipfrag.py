"""Randomised GPU parity for the UDP send with IPv4 fragmentation (udp_tx_fragment): the seeded
scenarios of random_ipfrag_cases.py, bit-exact against the model of ipfrag_cases.py and the CPU
oracle, with every output poisoned first and guard bytes round it. test_random_ipfrag_cases.py
checks on the CPU which branches the scenarios take.

The model rests on tests/golden/ip_frag_ref_cases.json, which test_ipfrag_host.py pins to the
reference's own Ip4RoundFragLen, IpChksum and UDP accumulator sequence."""
import numpy as np
import pytest

import aipstack_amd as A

import ipfrag_cases as T
import random_ipfrag_cases as G
import test_gpu_ipfrag as GF

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield


@pytest.mark.parametrize("seed", range(G.SEEDS))
def test_random_udp_fragmentation(oracle, seed):
    sc = G.scenario(oracle, seed)
    batch, e = sc.batch, sc.e
    n, nc = int(sc.fi[-1]), int(sc.cb[-1])
    dpay = torch.from_numpy(batch.payload.copy()).to(DEV)
    desc = T.descriptors(batch, dpay.data_ptr(), A.UDP_DGRAM_DTYPE)
    out = GF.Outputs(n, nc, len(batch.cases), sc.stride, sc.shift)
    A.udp_tx_fragment(desc, sc.fi, sc.cb, out=out.frags, just_written=sc.just_written)
    GF._compare(e, out, sc.stride, dpay, batch.payload)
    if seed % 4 == 0:
        # linearised from what the GPU left: fragments verify as FRAGMENT, whole datagrams ACCEPT
        ok = np.nonzero(e.status == T.ACCEPT)[0]
        got = out.frags.headers.cpu().numpy().reshape(n, sc.stride)
        buf, offs, ids = T.linearise(e, batch.payload, headers=got)
        assert ids == ok.tolist()
        v = A.rx_verify(torch.from_numpy(buf).to(DEV),
                        torch.from_numpy(offs.view(np.int64)).to(DEV)).cpu().numpy()
        S = np.diff(sc.fi.astype(np.int64))[e.frag_case[ok]]
        assert (v[S == 1] == T.ACCEPT).all() and (v[S > 1] == 3).all()
    assert A.contract_violations(clear=True) == 0
