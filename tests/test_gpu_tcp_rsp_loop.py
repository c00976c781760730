"""aipstack_tcp_rx_respond in the receive loop of INTEGRATION.md section 2, on two of the mixed
batches of rx_loop_cases.py (used as they are: one in ring slots, one CSR, both with a start Ident
just below 2^16): udp_rx_demux, icmp_rx_respond fed the demux's codes, then tcp_rx_respond with the
scenario's PCB table, listeners on ports the batch's own PCB-less segments go to, and the ICMP
call's Ident plus its response count. The TCP frames without a PCB, which the loop test leaves to
the host, get exactly the model's answers; the status codes of the three responders do not
collide; no frame gets two answers; the Idents of the two calls follow each other without a gap or
a repeat; and the ICMP responses and the RSTs linearise into ONE send ring."""
import numpy as np
import pytest

import aipstack_amd as A

import arp_cases as AC
import icmp_cases as IC
import rx_loop_cases as G
import tcp_rsp_cases as C
import tcprx_cases as TC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_icmp as TI  # noqa: E402
import test_gpu_tcp_rsp as TT  # noqa: E402
import test_gpu_udprx as TU  # noqa: E402

DEV = "cuda"
SLOT = G.SLOT
POISON = TT.POISON
SEEDS = (0, 3)
TCP_TTL = 77


@pytest.fixture(autouse=True)
def _no_contract_violation():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


def _dev(table):
    return None if table is None else torch.from_numpy(table.view(np.uint8).copy()).to(DEV)


def listeners_of(sc):
    """Listeners on the ports the batch's PCB-less segments to the interface's address go to: a
    wildcard on the lowest, a specific one on the highest, and both on one port in between."""
    t = sc.e_tcp
    free = ((t.segs["opts"] & TC.SEG_VALID) != 0) & (t.pcb == TC.NO_PCB) & (t.segs["local_addr"] == G.LOCAL)
    ports = sorted(set(int(p) for p in t.segs["local_port"][free]))
    assert len(ports) >= 3
    mid = ports[len(ports) // 2]
    return [(0, ports[0], 11), (G.LOCAL, ports[-1], 12), (G.LOCAL, mid, 13), (0, mid, 14)], free


@pytest.mark.parametrize("seed", SEEDS)
def test_tcp_responder_in_the_receive_loop(oracle, seed):
    sc = G.cached(oracle, seed)
    assert sc.slotted == (seed == 0) and sc.ifc["ip_id"] > 0x10000 - 200
    n = sc.n
    lay = TU.Layout(sc.frames, sc.slotted, slot=SLOT, lead=sc.lead)
    s = "_slotted" if sc.slotted else ""
    where = (lay.dev, lay.slot, lay.lens) if sc.slotted else (lay.dev, lay.offsets)
    lis, free = listeners_of(sc)
    icmp_if = TI._np_iface(sc.ifc)
    o = TT.Outputs(n, 64, sc.hdr_shift, sc.rec_shift)
    TI._tune("aux_blocks", sc.aux_blocks)
    try:
        udp = getattr(A, "udp_rx_demux" + s)(*where, icmp_if, _dev(sc.assocs), _dev(sc.listeners))
        icmp = getattr(A, "icmp_rx_respond" + s)(*where, icmp_if, udp.unreach_code)
        n_icmp = int(icmp.counts.cpu()[0])                       # the hand-over: the host reads the count
        ifc = dict(local=sc.ifc["local"], bcast=sc.ifc["bcast"], mac=sc.ifc["mac"], mtu=sc.ifc["mtu"],
                   ip_id=(sc.ifc["ip_id"] + n_icmp) & 0xFFFF, ttl=TCP_TTL)
        getattr(A, "tcp_rx_respond" + s)(*where, TT._np_iface(ifc), _dev(sc.pcbs), A.tcp_listeners(lis),
                                         tcp_ttl=TCP_TTL, out=o.res, workspace=o.workspace)
        e = C.respond(sc.frames, sc.verdicts, ifc, sc.pcbs, lis)
        TT._compare(e, o, lay, n, 64)
    finally:
        TI._tune("aux_blocks", -1)
    assert n_icmp == int(sc.e_icmp.counts[0]) >= 40
    assert np.array_equal(icmp.status.cpu().numpy(), sc.e_icmp.status)

    # what the TCP Rx parse of the loop gives, and the frames it left to the host
    assert np.array_equal(e.verdict, sc.e_tcp.verdict) and np.array_equal(e.pcb, sc.e_tcp.pcb)
    assert e.segs.tobytes() == sc.e_tcp.segs.tobytes()
    st = o.res.status.cpu().numpy()
    assert free.sum() >= 10 and np.isin(st[free], (C.DROP, C.SYN, C.RST)).all()
    assert (st[free] == C.RST).sum() >= 8 and (st == C.PCB).sum() >= 14 and (st == C.SYN).sum() >= 1
    assert (st[(sc.e_tcp.segs["opts"] & TC.SEG_VALID) == 0] == C.NONE).all()

    # one space of status codes, one answer per frame
    arp_codes, icmp_codes = {AC.NONE, AC.MALFORMED, AC.SEEN, AC.REPLY}, set(np.unique(sc.e_icmp.status).tolist())
    assert set(np.unique(st).tolist()) <= set(range(31, 37))
    assert not (set(range(31, 37)) & (arp_codes | icmp_codes | set(range(24))))
    rst = e.hdr_len != 0
    assert not (rst & (sc.e_icmp.hdr_len != 0)).any() and not (rst & (sc.e_arp.hdr_len != 0)).any()

    # the Idents: ICMP's from ip_id, the RSTs' behind them, each value once, across 2^16
    icmp_ids = [int.from_bytes(sc.e_icmp.headers[i][18:20], "big") for i in sorted(sc.e_icmp.headers)]
    rst_ids = [int.from_bytes(e.headers[i][18:20], "big") for i in sorted(e.headers)]
    first = sc.ifc["ip_id"]
    assert icmp_ids + rst_ids == [(first + j) & 0xFFFF for j in range(len(icmp_ids) + len(rst_ids))]
    assert min(icmp_ids + rst_ids) < 300 and max(icmp_ids + rst_ids) > 0xFF00

    # one send ring for both kinds of answer
    ring = torch.full((n * SLOT,), POISON, dtype=torch.uint8, device=DEV)
    A.tx_linearise_slotted(ring, SLOT, icmp)
    lin = A.tx_linearise_slotted(ring, SLOT, o.res)
    torch.cuda.synchronize()
    want = np.full((n, SLOT), POISON, dtype=np.uint8)
    for i in sc.e_icmp.headers:
        w = sc.wire[i]
        want[i, :len(w)] = np.frombuffer(w, dtype=np.uint8)
    for i, h in e.headers.items():
        want[i, :54] = np.frombuffer(h, dtype=np.uint8)
    assert ring.cpu().numpy().tobytes() == want.tobytes()
    ls = lin.status.cpu().numpy()
    assert (ls[rst] == A.AIPSTACK_TX_LIN_WRITTEN).all() and (ls[~rst] == A.AIPSTACK_TX_LIN_SKIPPED).all()
    # the peer's view: every RST in the ring is a valid TCP frame
    dl = torch.from_numpy(np.where(rst, 54, 0).astype(np.int32)).to(DEV)
    pv = A.rx_verify_slotted(ring, SLOT, dl).cpu().numpy()
    assert (pv[rst] == IC.ACCEPT).all()
