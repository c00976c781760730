"""Randomised GPU parity for the three TCP send / receive operations: seeded scenarios of
random_tcp_cases.py for the header-split Tx fill (tx_fill_header_split), the burst segmentation
(tcp_tx_segment) and the Rx parse (tcp_rx_parse / _slotted), each bit-exact against the models of
hsplit_cases.py, tcpseg_cases.py and tcprx_cases.py and the CPU oracle, with every output
poisoned first and guard bytes round it. test_random_tcp_cases.py checks on the CPU what the
scenarios cover.

The random option bytes of the Rx scenarios rest on tcprx_cases.parse_options, which
test_tcprx_host.py pins to the reference's own ParseTcpOptions by the 2,000+ recorded buffers of
tests/golden/tcp_rx_ref_cases.json; the key order of the tables on the same fixture.
"""
import numpy as np
import pytest

import aipstack_amd as A

import frame_cases as F
import random_tcp_cases as G
import tcprx_cases as R
import tcpseg_cases as S
import test_gpu_tcprx as GR
import test_gpu_tcpseg as GS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield


@pytest.mark.parametrize("seed", range(G.SEEDS))
def test_random_header_split_fill(oracle, seed):
    sc = G.hsplit_scenario(oracle, seed)
    sp, n, stride = sc.sp, sc.n, sc.stride
    lo = GUARD + sc.shift
    ring = torch.full((lo + sp.headers.size + GUARD,), G.GUARD_BYTE, dtype=torch.uint8, device=DEV)
    ring[lo:lo + sp.headers.size] = _d(sp.headers)
    headers = ring[lo:lo + n * stride]
    assert headers.data_ptr() % 16 == seed % 16
    pay = torch.full((GUARD + sp.payload.size + GUARD,), G.GUARD_BYTE, dtype=torch.uint8, device=DEV)
    pay[GUARD:GUARD + sp.payload.size] = _d(sp.payload)
    addr, lens, index = sp.chunk_table(pay.data_ptr() + GUARD)
    if addr.size == 0:
        addr, lens = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
    status = torch.full((GUARD + n + GUARD,), G.GUARD_BYTE, dtype=torch.uint8, device=DEV)
    st = A.tx_fill_header_split(headers, stride, _d(sp.hdr_lens.view(np.int32)),
                                _d(addr.view(np.int64)), _d(lens.view(np.int32)),
                                _d(index.view(np.int64)), out=status[GUARD:GUARD + n],
                                just_written=sc.just_written).cpu().numpy()
    bad = np.nonzero(st != sc.want_st)[0]
    assert bad.size == 0, (seed, bad[:8], st[bad[:8]], sc.want_st[bad[:8]], sp.hdr_lens[bad[:8]])
    got = ring.cpu().numpy()
    body = got[lo:lo + sp.headers.size]
    rows = np.nonzero((body[:n * stride] != sc.want_h[:n * stride]).reshape(n, stride).any(axis=1))[0]
    assert rows.size == 0, (seed, stride, sc.shift, rows[:8], sc.want_st[rows[:8]], sp.hdr_lens[rows[:8]])
    assert (got[:lo] == G.GUARD_BYTE).all() and (got[lo + n * stride:] == G.GUARD_BYTE).all()
    hp = pay.cpu().numpy()
    assert np.array_equal(hp[GUARD:GUARD + sp.payload.size], sp.payload)
    assert (hp[:GUARD] == G.GUARD_BYTE).all() and (hp[GUARD + sp.payload.size:] == G.GUARD_BYTE).all()
    hs = status.cpu().numpy()
    assert (hs[:GUARD] == G.GUARD_BYTE).all() and (hs[GUARD + n:] == G.GUARD_BYTE).all()
    assert A.contract_violations(clear=True) == 0


@pytest.mark.parametrize("seed", range(G.SEEDS))
def test_random_burst_segmentation(oracle, seed):
    sc = G.tcpseg_scenario(oracle, seed)
    batch, e = sc.batch, sc.e
    n, nc = int(sc.si[-1]), int(sc.cb[-1])
    dpay = _d(batch.payload.copy())
    desc = S.descriptors(batch, dpay.data_ptr(), A.TCP_BURST_DTYPE)
    out = GS.Outputs(n, nc, sc.stride, sc.shift)
    A.tcp_tx_segment(desc, sc.si, sc.cb, out=out.seg, just_written=sc.just_written)
    GS._compare(e, out, sc.stride, dpay, batch.payload)
    if seed % 4 == 0:
        # linearised from what the GPU left: every accepted segment verifies
        ok = np.nonzero(e.status == S.ACCEPT)[0]
        got = out.seg.headers.cpu().numpy().reshape(n, sc.stride)
        addr = out.seg.chunk_addr.cpu().numpy().view(np.uint64).astype(np.int64) - dpay.data_ptr()
        ln = out.seg.chunk_len.cpu().numpy().astype(np.int64)
        idx = out.seg.chunk_index.cpu().numpy().astype(np.int64)
        parts, offs = [], [0]
        for i in ok:
            parts.append(got[i, :S.HDR])
            parts += [batch.payload[addr[k]:addr[k] + ln[k]] for k in range(idx[i], idx[i + 1])]
            offs.append(offs[-1] + S.HDR + int(ln[idx[i]:idx[i + 1]].sum()))
        v = A.rx_verify(_d(np.concatenate(parts)), _d(np.array(offs, dtype=np.int64)))
        assert (v.cpu().numpy() == S.ACCEPT).all()
    assert A.contract_violations(clear=True) == 0


@pytest.mark.parametrize("seed", range(G.SEEDS))
def test_random_rx_parse(oracle, seed):
    sc = G.tcprx_scenario(oracle, seed)
    buf, off = F.pack(sc.frames)
    dbuf = _d(np.concatenate([np.full(sc.lead, 0x99, dtype=np.uint8), buf]))
    doff = _d((off + np.uint64(sc.lead)).view(np.int64))
    out = GR.Outputs(sc.n, sc.seg_shift)
    A.tcp_rx_parse(dbuf, doff, sc.tbl, **out.kw())
    GR._compare(sc.e, out)
    assert A.contract_violations(clear=True) == 0
    # the slotted form over the frames that fit, with the same alignment of the records
    m = len(sc.slot_frames)
    if m:
        out = GR.Outputs(m, sc.seg_shift)
        A.tcp_rx_parse_slotted(_d(sc.ring), sc.stride, _d(sc.lens.view(np.int32)), sc.tbl, **out.kw())
        GR._compare(sc.slot_e, out)
        over = bool((sc.lens > sc.stride).any())
        assert (A.contract_violations(clear=True) != 0) == over   # lengths above the stride
