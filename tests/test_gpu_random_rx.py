"""Seeded random scenarios for the UDP Rx demux and the ICMP responder on the GPU
(random_rx_cases.py; test_random_rx_cases.py checks on the CPU what the scenarios cover). Every
output byte between the guards is compared with the models of udp_rx_cases.py and icmp_cases.py,
the call runs a second time into re-poisoned outputs and must leave identical bytes, and the ICMP
responses are linearised and compared with the packets the model builds."""
import numpy as np
import pytest

import aipstack_amd as A

import icmp_cases as IC
import random_rx_cases as G

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_icmp as TI  # noqa: E402
import test_gpu_udprx as TU  # noqa: E402

DEV = "cuda"
SLOT = 2048


@pytest.fixture(autouse=True)
def _no_contract_violation():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


@pytest.mark.parametrize("seed", range(G.SEEDS))
def test_udp_rx_demux(oracle, seed):
    sc = G.udp_scenario(oracle, seed)
    lay = TU.Layout(sc.frames, sc.slotted, slot=sc.slot, lead=sc.lead)
    TU._tune("aux_blocks", sc.aux_blocks)
    try:
        seen = []
        for _ in range(2):
            out = TU.Guarded(sc.n, sc.dgram_shift)                  # poisoned afresh
            got = lay.call(sc.ifc, sc.assocs, sc.listeners, out)
            assert got.n == sc.n and got.dgrams.data_ptr() % 16 == sc.dgram_shift
            TU._compare(sc.e, out, lay)
            seen.append(out.bytes())
    finally:
        TU._tune("aux_blocks", -1)
    assert seen[0] == seen[1]


def _icmp_bytes(got):
    torch.cuda.synchronize()
    return b"".join(getattr(got, k).cpu().numpy().tobytes() for k in (
        "headers", "hdr_lens", "chunk_addr", "chunk_len", "chunk_index", "status", "verdict",
        "response_frame", "counts"))


@pytest.mark.parametrize("seed", range(G.SEEDS))
def test_icmp_rx_respond(oracle, seed):
    sc = G.icmp_scenario(oracle, seed)
    TI._tune("aux_blocks", sc.aux_blocks)
    try:
        for start, end, ifc, e in sc.batches:
            frames = sc.frames[start:end]
            codes = None if sc.codes is None else sc.codes[start:end]
            n = end - start
            lay = TI.Layout(frames, sc.slotted)
            seen = []
            for _ in range(2):
                out = TI._dirty(n, sc.hdr_stride, sc.shift)         # poisoned afresh
                got = lay.call(ifc, codes, out=out)
                assert got.headers is out.headers and got.n == n
                TI._compare(e, got, lay, frames, sc.hdr_stride)
                seen.append(_icmp_bytes(got))
            assert seen[0] == seen[1]
            # the responses as frames of a send ring: the model's packet, nothing else written
            ring = torch.full((n * SLOT,), TI.POISON, dtype=torch.uint8, device=DEV)
            lin = A.tx_linearise_slotted(ring, SLOT, got)
            h, lens = ring.cpu().numpy().reshape(n, SLOT), lin.lens.cpu().numpy()
            ls = lin.status.cpu().numpy()
            for i in range(n):
                if i in e.headers:
                    pkt = IC.response_packet(e, frames, i)
                    assert ls[i] == A.AIPSTACK_TX_LIN_WRITTEN and lens[i] == 14 + len(pkt), (start, i)
                    assert h[i, :14].tobytes() == e.headers[i][:14]
                    assert h[i, 14:lens[i]].tobytes() == pkt, (start, i)
                    assert (h[i, lens[i]:] == TI.POISON).all()
                else:
                    assert ls[i] == A.AIPSTACK_TX_LIN_SKIPPED and lens[i] == 0 and (h[i] == TI.POISON).all()
    finally:
        TI._tune("aux_blocks", -1)
