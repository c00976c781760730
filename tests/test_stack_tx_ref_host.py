"""The two Tx models and the host layout functions held to what the reference stack puts on the
wire (tests/golden/stack_tx_ref_cases.json: the reference's IpStack with its TCP and UDP protocols
run by oracle/stack_ref_gen.cpp on a capture driver). No GPU is needed.

Every comparison is bit-exact or a hash of exact bytes: the model's 40 header bytes behind the
Ethernet header against the recorded ones, the bytes its chunk lists name against the recorded
FNV, the segment and fragment counts. Where the generator binary exists the fixture is
regenerated and compared byte for byte, and the frames ipfrag_cases builds are handed to the
reference's own receive path (reassembly, UDP checksum, listener)."""
import os
import struct

import numpy as np
import pytest

import aipstack_amd as A

import ipfrag_cases as U
import stack_ref_batches as S
import stack_tx_ref as R
import tcpseg_cases as T

needs_generator = pytest.mark.skipif(not os.path.exists(R.GEN_BIN),
                                     reason="reference generator not built here")


# ---- the fixture ----------------------------------------------------------------------------

def test_fixture_udp_coverage():
    udp, _, _ = S.fixture()
    assert 150 <= len(udp) <= 400
    assert {d["mtu"] for d in udp} == set(R.UDP_MTUS)
    assert {(m - 20) % 8 == 0 for m in R.UDP_MTUS} == {True, False}
    two_piece = {"inside": 0, "boundary": 0, "first8": 0}
    zero = 0
    for mtu in R.UDP_MTUS:
        M = mtu - 20
        F = M // 8 * 8
        mine = [d for d in udp if d["mtu"] == mtu]
        Ds = {d["len0"] + d["len1"] for d in mine}
        assert {0, 1, mtu - 29, mtu - 28, mtu - 27} <= Ds
        by_D = {d["len0"] + d["len1"]: d for d in mine}
        assert len(by_D[mtu - 28]["frags"]) == 1 and len(by_D[mtu - 27]["frags"]) == 2
        # the shortest last fragment there is: 1 byte where M % 8 == 0 (stack_tx_ref.py)
        assert any(len(d["frags"]) > 1 and d["frags"][-1].length == M % 8 + 1 for d in mine)
        assert any(len(d["frags"]) > 1 and (8 + d["len0"] + d["len1"]) % F == 0 for d in mine)
        assert any(D >= 20000 for D in Ds)
        if M % 8:
            assert any(len(d["frags"]) > 1 and d["frags"][-1].length > F for d in mine)
        for d in mine:
            if d["len0"] and d["len1"] and len(d["frags"]) > 1:
                at = (8 + d["len0"]) % F
                two_piece["boundary" if at == 0 else "first8" if at < 8 else "inside"] += 1
            if d["fix"] >= 0:
                assert d["frags"][0].l4[6:8] == b"\xff\xff"
                zero += 1
    assert 65507 in {d["len0"] + d["len1"] for d in udp if d["mtu"] == 1500}
    assert sum(two_piece.values()) >= 20 and min(two_piece.values()) >= 4, two_piece
    assert zero >= 3
    # the ident is one per datagram, and the next datagram of a stack has the next one
    for a, b in zip(udp, udp[1:]):
        ia, ib = (struct.unpack_from(">H", x["frags"][0].ip, 4)[0] for x in (a, b))
        assert ib == (ia + 1 if a["mtu"] == b["mtu"] else 0)


def test_fixture_tcp_coverage():
    _, tcp, min_mss = S.fixture()
    assert min_mss == [(215, 0), (216, 1)]            # 216 = MinMTU - 40 is the smallest accepted
    assert {c["snd_mss"] for c in tcp} >= {216, 536, 1460}
    bursts = [(c, b) for c in tcp for b in c["bursts"]]
    assert 100 <= len(bursts) <= 300
    assert all(p.kind == "D" for _, b in bursts for p in b["packets"])
    assert all(b["mss"] == c["snd_mss"] for c, b in bursts)
    n = [len(b["packets"]) for _, b in bursts]
    assert 1 in n and max(n) >= 20
    data = [(c, b) for c, b in bursts if b["len0"] + b["len1"]]
    assert any(b["packets"][-1].length == 1 for _, b in data)
    assert any(b["packets"][-1].length == b["mss"] for _, b in data)
    wraps = [b for _, b in bursts if b["len1"]]
    assert len(wraps) >= 10 and any(b["len0"] % b["mss"] == 0 for b in wraps)
    assert any(b["len0"] % b["mss"] for b in wraps)
    D = lambda b: b["len0"] + b["len1"]                                    # noqa: E731
    inner = [b for _, b in data if not b["fin"]]
    assert any(0 < b["push"] < D(b) and b["push"] % b["mss"] == 0 for b in inner)       # a last byte
    assert any(b["push"] % b["mss"] == 1 and b["push"] > 1 for b in inner)              # a first byte
    assert any(1 < b["push"] % b["mss"] < b["mss"] - 1 and b["push"] < D(b) for b in inner)
    assert any(b["push"] == 0 for b in inner) and any(b["push"] == D(b) for b in inner)
    assert any(b["fin"] and D(b) for _, b in bursts) and any(b["fin"] and not D(b) for _, b in bursts)
    assert any(b["seq"] + D(b) > 1 << 32 for _, b in bursts)               # sequence numbers wrap
    assert any(b["seq"] + D(b) == 1 << 32 for _, b in bursts)              # a segment ends at 2^32
    assert any(b["seq"] == 0 for _, b in bursts)                           # and the next begins at 0
    # the handshake: our SYN, then the pure ACK of the peer's SYN-ACK, neither in a burst
    for c in tcp:
        assert [p.kind for p in c["handshake"]] == ["S", "A"]
    # the ident advances by one per packet of a connection's stack
    for c in tcp:
        ids = [struct.unpack_from(">H", p.ip, 4)[0] for p in c["handshake"]]
        ids += [struct.unpack_from(">H", p.ip, 4)[0] for b in c["bursts"] for p in b["packets"]]
        assert ids == list(range(len(ids)))


def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(R.FIXTURE) < 512 * 1024
    with open(R.FIXTURE) as f:
        text = f.read()
    assert set(text) <= set("0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ_ -|;:,.[]{}\"\n")


@needs_generator
def test_fixture_regenerates_byte_for_byte():
    with open(R.FIXTURE) as f:
        assert R.generate() == f.read()


# ---- the models -----------------------------------------------------------------------------

def test_burst_model_matches_the_reference_stack(oracle):
    batch, records = S.tcp_batch()
    e = T.expected(oracle, batch)
    want, index = S.flat(records)
    si, _ = T.caller_index(batch.cases)
    assert np.array_equal(si.astype(np.int64), index), "segment counts"
    assert (e.status == T.ACCEPT).all()
    for i, p in enumerate(want):
        assert e.headers[i, 14:54].tobytes() == p.ip + p.l4, (i, int(e.seg_case[i]), int(e.seg_k[i]))
        data = S.chunk_bytes(batch.payload, e.seg_chunks[i])
        assert (len(data), S.fnv(data)) == (p.length, p.fnv), (i, int(e.seg_case[i]))


def test_fragment_model_matches_the_reference_stack(oracle):
    batch, records = S.udp_batch()
    e = U.expected(oracle, batch)
    want, index = S.flat(records)
    fi, _ = U.caller_index(batch.cases)
    assert np.array_equal(fi.astype(np.int64), index), "fragment counts"
    assert (e.status == U.ACCEPT).all() and (e.dgram_status == U.ACCEPT).all()
    for i, p in enumerate(want):
        first = bool(p.l4)
        assert int(e.hdr_len[i]) == (U.HDR0 if first else U.HDRK), i
        assert e.headers[i, 14:int(e.hdr_len[i])].tobytes() == p.ip + p.l4, (i, int(e.frag_case[i]))
        data = S.chunk_bytes(batch.payload, e.frag_chunks[i])
        assert (len(data), S.fnv(data)) == (p.length, p.fnv), (i, int(e.frag_case[i]))


def test_layout_functions_give_the_recorded_counts():
    batch, records = S.tcp_batch()
    si, _ = A.tcp_burst_layout(T.descriptors(batch, 1 << 20, A.TCP_BURST_DTYPE))
    assert np.diff(si.astype(np.int64)).tolist() == [len(r) for r in records]
    batch, records = S.udp_batch()
    fi, _, st = A.udp_dgram_layout(U.descriptors(batch, 1 << 20, A.UDP_DGRAM_DTYPE))
    assert np.diff(fi.astype(np.int64)).tolist() == [len(r) for r in records]
    assert (st == U.ACCEPT).all()


# ---- our frames into the reference's receive path -------------------------------------------

def _receive_batch(oracle):
    """Three dozen datagrams to 10.0.0.2:53 over the four MTUs: unfragmented, fragmented, two
    pieces, a last fragment of 1 byte, a zero UDP sum (sent as 0xFFFF)."""
    cs = []
    for mtu in (256, 576, 1006, 1500):
        M = mtu - 20
        F = M // 8 * 8
        for D, l0 in ((0, 0), (1, 1), (mtu - 28, 7), (mtu - 27, mtu - 27), (2 * F + 1 - 8, F - 8),
                      (3 * F - 8, F - 5), (F + M - 8, 0), (5 * M + 3, 2 * M)):
            cs.append(U.dgram((1 + len(cs), l0), (70000 + 3 * len(cs), D - l0), mtu=mtu, ip_id=len(cs)))
    cs.append(U.dgram((9, 30000), (60001, 20000), mtu=1500, ip_id=999))
    return U.Batch(cs + U.zero_udp_checksum_batch(oracle).cases, None)


@needs_generator
def test_reference_stack_receives_our_frames(oracle):
    batch = _receive_batch(oracle)
    batch.payload = U.zero_udp_checksum_batch(oracle).payload
    e = U.expected(oracle, batch)
    assert (e.status == U.ACCEPT).all() and "0xFFFF" in U.branches(batch, e)
    packets, want = [], []
    for d, c in enumerate(batch.cases):
        ids = [int(i) for i in np.nonzero(e.frag_case == d)[0]]
        packets.append([U.frame_of(e, batch.payload, i)[14:] for i in ids])
        (o0, l0), (o1, l1) = c["pieces"]
        data = batch.payload[o0:o0 + l0].tobytes() + batch.payload[o1:o1 + l1].tobytes()
        want.append([(len(data), S.fnv(data))])
    assert len(packets) >= 36 and sum(len(p) > 1 for p in packets) >= 20
    assert R.receive(0x0A000002, 53, packets) == want
    assert R.receive(0x0A000002, 53, [p[::-1] for p in packets]) == want
    # one payload byte changed: the datagram's checksum no longer holds, nothing is delivered
    for d in (3, len(packets) - 1):
        bad = [bytearray(p) for p in packets[d]]
        assert len(bad) > 1 and len(bad[-1]) > 20
        bad[-1][-1] ^= 0x10
        assert R.receive(0x0A000002, 53, [bad]) == [[]]
