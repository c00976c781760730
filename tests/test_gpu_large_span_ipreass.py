"""aipstack_ip4_rx_reassemble with fragments of one datagram on both sides of a 2^31 and a 2^32
byte offset from its base and of a device address that is a multiple of 2^32
(large_span_ipreass_cases.py, on the arena and windows of large_span_cases.py): all six outputs
byte for byte against the model, guard bytes round them and the workspace. A 32-bit-truncated
offset or address lands inside the zero arena, so a truncation shows as a wrong value."""
import numpy as np
import pytest

import aipstack_amd as A

import ipreass_cases as R
import large_span_cases as L
import large_span_ipreass_cases as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ipreass_gpu as H  # noqa: E402


@pytest.fixture(scope="module")
def arena():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    a = torch.zeros(L.ARENA_BYTES, dtype=torch.uint8, device=H.DEV)
    A.contract_violations(clear=True)
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("distance", C.DISTANCES)
def test_datagrams_across_4gib_offsets_and_addresses(arena, oracle, distance):
    P = arena.data_ptr()
    for shift in (0, 15):
        c = C.case(P, shift, distance)
        L.check_windows(c.windows)
        fill = {int(ln) for i, ln in enumerate(np.diff(c.offsets.astype(np.int64))) if i not in c.frames}
        fv = {int(oracle.rx_verify_batch(np.zeros(max(ln, 1), dtype=np.uint8), [0, ln])[0]) for ln in fill}
        assert fv == {R.NOT_IP4}
        e = C.expected(oracle, c, R.NOT_IP4)
        if shift == 0:
            assert any((P + x) % L.E32 == 0 for x in c.edges)
        for i in c.across:
            assert e.verdict[i] == R.MEMBER
        base = arena[shift:]
        doff = torch.from_numpy(c.offsets.view(np.int64)).to(H.DEV)
        addr = np.uint64(P + shift) + c.offsets[:-1]
        out = H.Outputs(c.n)
        try:
            for w in c.windows:
                arena[w.start:w.end].copy_(torch.from_numpy(w.data))
            res = A.ip4_rx_reassemble(base, doff, **out.kw())
            H.compare(e, out, addr)
            # the chunk addresses of a datagram's list lie on both sides of a multiple of 2^32
            ca = res.chunk_addr.cpu().numpy().view(np.uint64)
            for o in e.complete.values():
                assert len({int(ca[i]) >> 32 for i in o}) >= 2
            for w in c.windows:                          # the frames are only read
                assert np.array_equal(arena[w.start:w.end].cpu().numpy(), w.data)
        finally:
            for w in c.windows:
                arena[w.start:w.end].zero_()
        assert A.contract_violations(clear=True) == 0
    assert not bool(arena.view(torch.int64).any()), "the test left bytes in the arena"
