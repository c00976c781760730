"""The passive open on the device: the SYNs the reference stack was fed (tests/golden/
tcp_ctl_ref.py), mixed with SYNs for closed ports, go through tcp_rx_respond_slotted; for the
_RSP_SYN list a host model of the rest of listen_input makes the descriptors (the ISS and the
window from the recorded answer, the MSS from the interface, the window scale from the record's
options); tcp_tx_control builds the SYN-ACKs with the responder's Ident plus its count; both
producers go through tx_resolve and tx_linearise into ONE send ring. The SYN-ACKs are the frames
the reference sent; the RSTs are the responder model's; the Idents follow each other."""
import numpy as np
import pytest

import aipstack_amd as A

import tcp_ctl_cases as C
import tcp_ctl_ref as R
import tcp_rsp_ref as RR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOT, POISON, TTL = 128, 0xEE, 64
RCV_WND_SHIFT = 6                      # Constants::RcvWndShift


@pytest.mark.parametrize("which", [0, 1])
def test_syn_acks_of_a_received_batch(which):
    s = [x for x in R.load() if x["name"].startswith("passive")][which]
    local, peer, mac = s["addr"], s["peer"], bytes.fromhex(s["mac"])
    pairs = R.syn_frames(s)
    frames, answer = [], {}
    for k, (syn, synack) in enumerate(pairs):               # a closed port in front of every SYN
        frames.append(RR.frame(RR.SYN, src=peer, dst=local, sport=50000 + k, dport=81, seq=77 * k))
        answer[len(frames)] = synack
        frames.append(syn)
    n, m = len(frames), len(pairs)
    host = np.full((n, SLOT), 0x5A, dtype=np.uint8)
    for i, f in enumerate(frames):
        host[i, :len(f)] = np.frombuffer(f, dtype=np.uint8)
    dev = torch.from_numpy(host.reshape(-1)).to(DEV)
    lens = torch.tensor([len(f) for f in frames], dtype=torch.int32, device=DEV)
    bcast = local | (0xFFFFFFFF >> s["prefix"])
    first = (0x10000 - m) & 0xFFFF                          # the RSTs end at 0xFFFF
    rsp = A.tcp_rx_respond_slotted(dev, SLOT, lens, A.icmp_iface(local, bcast, mac, ip_id=first), None,
                                   A.tcp_listeners([(local, R.SMALL, 1), (local, R.LARGE, 2)]), tcp_ttl=TTL)
    counts = rsp.counts.cpu().numpy()                       # the hand-over: the host reads the counts
    assert counts.tolist() == [m, m]
    syn_at = rsp.syn_frame.cpu().numpy()[:m]
    assert syn_at.tolist() == sorted(answer)
    segs, lis = rsp.segs_numpy(), rsp.listener_numpy()

    # the rest of listen_input, on the host
    cs = []
    for i in syn_at:
        r, want = segs[i], C.from_frame(answer[int(i)])[0]
        assert int(lis[i]) == (1 if r["local_port"] == R.SMALL else 2)
        ws = bool(r["opts"] & A.AIPSTACK_TCP_OPT_WND_SCALE)
        cs.append(C.ctl(local_addr=int(r["local_addr"]), remote_addr=int(r["remote_addr"]),
                        local_port=int(r["local_port"]), remote_port=int(r["remote_port"]),
                        seq=want["seq"], ack=(int(r["seq_num"]) + 1) & 0xFFFFFFFF, window=want["window"],
                        flags=0x12, mss=1500 - 40, options=A.AIPSTACK_TCP_OPT_MSS | (2 if ws else 0),
                        wnd_scale=RCV_WND_SHIFT if ws else 0))
    ctl = A.tcp_tx_control(A.tcp_ctl(cs), A.icmp_iface(local, bcast, mac, ip_id=first + int(counts[0])),
                           tcp_ttl=TTL)
    assert ctl.counts.cpu().numpy().tolist() == [m, 0]

    # both producers: resolve, then one send ring (the responder's slots, then the SYN-ACKs')
    ifaces = A.tx_ifaces([(local, s["prefix"], s["gateway"], mac)])
    arp = np.zeros(1, dtype=A.ARP_ENTRY_DTYPE)
    arp[0]["addr"], arp[0]["state"] = peer, A.AIPSTACK_ARP_STATE_VALID
    arp[0]["mac"] = np.frombuffer(bytes.fromhex(s["peer_mac"]), dtype=np.uint8)
    arp = A.arp_table_sort(arp)
    ring = torch.full(((n + m) * SLOT,), POISON, dtype=torch.uint8, device=DEV)
    for prod, part in ((rsp, ring[:n * SLOT]), (ctl, ring[n * SLOT:])):
        rs = A.tx_resolve(prod.headers, prod.hdr_stride, prod.hdr_lens, ifaces, arp)
        assert int(rs.counts.cpu().numpy().sum()) == 0
        A.tx_linearise_slotted(part, SLOT, prod, frame_max=SLOT)
    torch.cuda.synchronize()
    got = ring.cpu().numpy().reshape(n + m, SLOT)

    # the SYN-ACKs are the reference's, Ident included (0 .. m-1, behind the RSTs' 0xFFFx)
    for k, i in enumerate(syn_at):
        f = answer[int(i)]
        assert got[n + k, :len(f)].tobytes() == f, (k, got[n + k, :64].tobytes().hex(), f.hex())
        assert (got[n + k, len(f):] == POISON).all()
    assert [int.from_bytes(got[n + k, 18:20].tobytes(), "big") for k in range(m)] == list(range(m))
    # the RSTs: one per closed-port SYN, Idents first .. 0xFFFF, each a valid frame for the peer
    rst_at = rsp.response_frame.cpu().numpy()[:m]
    assert rst_at.tolist() == [i for i in range(n) if i not in answer]
    assert [int.from_bytes(got[i, 18:20].tobytes(), "big") for i in rst_at] == \
        [(first + j) & 0xFFFF for j in range(m)]
    for i in rst_at:
        assert got[i, :6].tobytes() == bytes.fromhex(s["peer_mac"]) and got[i, 47] == 0x14
        assert (got[i, 54:] == POISON).all()
    for i in syn_at:
        assert (got[i] == POISON).all()
    out_lens = np.zeros(n + m, dtype=np.int32)
    out_lens[rst_at] = 54
    out_lens[n:] = [len(answer[int(i)]) for i in syn_at]
    v = A.rx_verify_slotted(ring, SLOT, torch.from_numpy(out_lens).to(DEV)).cpu().numpy()
    assert (v[out_lens != 0] == 6).all()                    # AIPSTACK_RX_ACCEPT
