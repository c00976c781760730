"""aipstack_tx_resolve on a batch that takes the scan of the tile counts into its second step, and
on a header ring of 65536-byte slots whose slots 32768 and 65536 start at byte offsets 2^31 and
2^32: every output whole against the model of tx_resolve_cases.py; a 32-bit-truncated slot offset
lands in another slot, whose bytes are compared too."""
import numpy as np
import pytest

import aipstack_amd as A

import large_span_cases as L
import tx_resolve_cases as C
import test_gpu_tx_resolve as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"


def test_scan_over_several_steps():
    """65,600 segments are 257 tiles: the one-workgroup scan runs its loop twice. Held and failed
    segments lie in every tile, in the last one too."""
    n = 65600
    base = C.placed_batch(1000, "query") + C.placed_batch(1000, "error")
    headers = [base[i % 2000] for i in range(n)]
    headers[n - 2] = C.header(C.LAN[0]["addr"], C.ALL_ONES)                  # _BCAST_REJECTED
    headers[n - 1] = C.header(C.LAN[0]["addr"], C.PEER_QUERY)
    e = T._check(headers, 64, C.LAN, C.lan_table(60))
    assert int(e.counts[0]) > 5000 and int(e.counts[1]) > 5000
    assert int(e.held[int(e.counts[0]) - 1]) == n - 1 and int(e.failed[int(e.counts[1]) - 1]) == n - 2


def test_header_ring_past_4gib():
    """Slots on both sides of the 2^31 and 2^32 byte offsets of the ring resolve; every other slot
    has length 0. The ring's first 64 bytes of every slot are compared, and the ring beyond them
    stays zero."""
    n, stride = L.RING_SLOTS, L.RING_STRIDE
    need = n * stride + (1 << 28)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %d MiB of free device memory" % (need >> 20))
    near, rows = L.ring_rows(n)
    assert {32767, 32768, 65535, 65536} <= set(near.tolist())
    kinds = C.placed_batch(rows.size, "sent")
    lens = np.zeros(n, dtype=np.uint32)
    small = np.zeros((n, 64), dtype=np.uint8)
    for j, r in enumerate(rows):
        h = kinds[j]
        lens[r] = len(h)
        small[r, :len(h)] = np.frombuffer(h, dtype=np.uint8)
    table = C.lan_table(20)
    e = C.expected(small.reshape(-1), 64, lens, C.LAN, table)
    assert {C.SENT, C.ARP_QUERY} <= set(e.status[near].tolist())
    drows = torch.from_numpy(rows).to(DEV)
    for shift in (0, 1):
        arena = torch.zeros(shift + n * stride, dtype=torch.uint8, device=DEV)
        ring = arena[shift:]
        slots = ring.view(n, stride)
        slots[drows, :64] = torch.from_numpy(small[rows]).to(DEV)
        b = T.Buffers(n, 1, len(table))
        got = A.tx_resolve(ring, stride, torch.from_numpy(lens.view(np.int32)).to(DEV), C.iface_table(C.LAN), table,
                           workspace=b.workspace, **b.out)
        torch.cuda.synchronize()
        for name, w in (("status", e.status), ("routes", e.routes), ("send_lens", e.send_len),
                        ("arp_used", e.arp_used), ("held_seg", e.held), ("failed_seg", e.failed),
                        ("counts", e.counts)):
            assert getattr(got, name).cpu().numpy().tobytes() == w.tobytes(), (name, shift)
        assert np.array_equal(slots[drows, :64].cpu().numpy(), e.ring.reshape(n, 64)[rows]), shift
        b.guards_intact()
        slots[drows, :64] = 0
        assert not bool(arena.any()), "bytes outside the first 64 of the resolved slots"
        del slots, ring, arena, b, got
        torch.cuda.empty_cache()
    assert A.contract_violations(clear=True) == 0
