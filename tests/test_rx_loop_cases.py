"""The scenarios of test_gpu_rx_loop.py (rx_loop_cases.py), checked on the CPU over every seed with
the oracle and the models: what they cover, that the models give every frame exactly one owner,
that the models' verdict arrays agree with the oracle's Rx verify but for the documented rewrites,
and that the generator is stable. And the CPU half of the reference sessions
(tests/golden/rx_loop_ref_cases.json): run batch by batch with the Ident carried over, the models
send exactly the frames the reference's own stack sent and name the handler calls it made."""
import os

import numpy as np
import pytest

import arp_cases as AC
import icmp_cases as IC
import ipreass_cases as RC
import rx_loop_cases as G
import rx_loop_ref as LR
import tcprx_cases as TC
import udp_rx_cases as UC

REFERENCE = "/root/reference"
SEED0_DIGEST = "7a0c4f90c01b5133627dee5701849bd0593949cce2437da91ec45959fd067e50"


@pytest.fixture(scope="module")
def scenarios(oracle):
    return [G.cached(oracle, s) for s in range(G.SEEDS)]


def test_coverage(scenarios):
    """The conditions the GPU tests rely on, from the models alone."""
    layouts = {k: [] for k in ("slotted", "lead", "hdr_shift", "rec_shift", "aux_blocks")}
    all_tile = none_tile = 0
    n_lis, last_kinds = set(), set()
    for sc in scenarios:
        n = sc.n
        assert 1100 <= n <= 1400 and len(sc.frames) == n == len(sc.kinds)
        assert 5 <= -(-n // G.TILE) <= 6 and n % G.TILE                    # a ragged last tile
        counts = np.bincount(sc.owner, minlength=len(G.OWNERS))
        assert (counts >= 20).all(), (sc.seed, dict(zip(G.OWNERS, counts.tolist())))
        sorts = np.bincount(sc.host_sort[sc.owner == G.HOST], minlength=len(G.HOST_SORTS))
        assert (sorts >= 1).all(), (sc.seed, dict(zip(G.HOST_SORTS, sorts.tolist())))
        for k in layouts:
            layouts[k].append(getattr(sc, k))
        n_lis.add(0 if sc.listeners is None else len(sc.listeners))
        # every list's edges: each responding kind at lanes 0, 63, 64, 255 of a tile, one at the end
        want = {"arp_req": G.ARP, "echo": G.ICMP_ECHO, "udp_closed": G.UDP_UNREACH, "udp_assoc": G.UDP_DELIVER}
        for j, kind in enumerate(G.RESPONDING):
            tile = (j + sc.seed) % 4
            for lane in G.PLACES:
                assert sc.owner[tile * G.TILE + lane] == want[kind], (sc.seed, kind, lane)
        assert sc.owner[n - 1] == want[G.RESPONDING[sc.seed % 4]]
        last_kinds.add(int(sc.owner[n - 1]))
        assert sc.e_arp.status[[t * G.TILE + lane for t in range(4) for lane in G.PLACES
                                if sc.owner[t * G.TILE + lane] == G.ARP]].tolist() == [AC.REPLY] * 4
        tiles = [sc.responds[t:t + G.TILE] for t in range(0, n - n % G.TILE, G.TILE)]
        all_tile += any(t.all() for t in tiles)
        none_tile += any(not t.any() for t in tiles)
        # the kinds the issue lists, by what the models made of them
        st, e = sc.e_arp.status, sc.e_udp
        assert (st == AC.REPLY).sum() >= 8 and (st == AC.SEEN).sum() >= 8 and (st == AC.MALFORMED).sum() >= 8
        assert any(len(f) == 41 and s == AC.MALFORMED for f, s in zip(sc.frames, st))
        assert any(len(f) == 42 and s == AC.REPLY for f, s in zip(sc.frames, st))
        assert any(len(f) == 60 and s == AC.REPLY for f, s in zip(sc.frames, st))
        valid = (e.dgrams["flags"] & UC.VALID) != 0
        delivered = G.delivered_mask(e.deliver_frame, e.counts[0], n)
        bcast = (e.dgrams["flags"] & UC.DST_BCAST) != 0
        assert (valid & (e.dgrams["assoc"] != UC.NO_ASSOC)).sum() >= 20
        assert (valid & bcast & ~delivered).sum() >= 4 and (e.unreach[bcast] == UC.NO_UNREACH).all()
        assert (valid & (e.dgrams["flags"] & UC.HAS_CHKSUM == 0)).sum() >= 4
        if sc.listeners is not None and len(sc.listeners) >= 8:
            masks = e.dgrams["listeners"][valid]
            assert (masks != 0).sum() >= 5 and any(bin(int(m)).count("1") >= 2 for m in masks)
        t = sc.e_tcp
        seg = (t.segs["opts"] & TC.SEG_VALID) != 0
        assert (seg & (t.pcb != TC.NO_PCB)).sum() >= 10 and (seg & (t.pcb == TC.NO_PCB)).sum() >= 10
        assert (t.verdict == TC.DROP_TCP_OFFSET).sum() >= 8
        r = sc.e_reass
        assert len(r.complete) >= 8 and len(r.groups) - len(r.complete) >= 6
        assert (r.dgram["n_frags"] != 0).sum() == len(r.complete)
        i = sc.e_icmp
        assert (i.status == IC.TOO_LARGE).sum() >= 1 and (i.status == IC.UNREACH).sum() >= 20
        assert any(f[14] & 0xF > 5 for f, s in zip(sc.frames, i.status) if s == IC.ECHO_REPLY)
        assert set(np.unique(sc.verdicts)) == set(range(9))
        assert sum(1 for f in sc.frames if 0 < len(f) < 14) >= 4 and sum(1 for f in sc.frames if not f) >= 1
        assert sc.ifc["ip_id"] + int(i.counts[0]) < 0x10000 + 2000
    for k, vals in layouts.items():
        choices = {"slotted": (False, True), "lead": (0, 1, 2, 3), "hdr_shift": (0, 8), "rec_shift": (0, 8),
                   "aux_blocks": G.AUX_BLOCKS}[k]
        if k == "lead":
            vals = [v for v, s in zip(vals, layouts["slotted"]) if not s]
        assert all(vals.count(c) >= 2 for c in choices), (k, vals)
    assert all_tile >= 1 and none_tile >= 1
    assert {0, 64} <= n_lis and last_kinds == {G.ARP, G.ICMP_ECHO, G.UDP_UNREACH, G.UDP_DELIVER}
    # the Ident passes 0xFFFF inside a batch somewhere
    assert any(sc.ifc["ip_id"] + int(sc.e_icmp.counts[0]) > 0x10000 for sc in scenarios)
    assert {sc.ifc["allow"] for sc in scenarios} == {False, True}


def test_exactly_one_owner_in_the_models(scenarios):
    """Read as the host loop reads them, the models' outputs give every frame at most one stage,
    and a frame without one is the host's or dropped; no frame is left out."""
    for sc in scenarios:
        assert len(sc.owner) == sc.n == len(sc.claims)
        assert (sc.claims <= 1).all(), (sc.seed, np.flatnonzero(sc.claims > 1)[:8])
        none = sc.claims == 0
        assert np.isin(sc.owner[none], (G.HOST, G.DROP)).all() and (sc.owner[~none] < G.HOST).all()
        assert ((sc.host_sort >= 0) == (sc.owner == G.HOST)).all()
        # the unreach the responder makes is one the demux asked for, and nothing it delivered
        un = sc.e_icmp.status == IC.UNREACH
        delivered = G.delivered_mask(sc.e_udp.deliver_frame, sc.e_udp.counts[0], sc.n)
        assert (sc.e_udp.unreach[un] == UC.PORT_UNREACH).all() and not (un & delivered).any()
        # what leaves for the wire: exactly the frames of the three responding owners
        resp = np.isin(sc.owner, (G.ICMP_ECHO, G.UDP_UNREACH)) | (sc.e_arp.status == AC.REPLY)
        assert np.array_equal(resp, sc.responds) and len(sc.wire) == int(resp.sum())
        assert ((sc.e_arp.status == AC.REPLY) <= (sc.owner == G.ARP)).all()


def test_verdicts_agree_in_the_models(scenarios):
    tcp = reass = 0
    for sc in scenarios:
        t, r = G.verdicts_agree(sc.verdicts, sc.e_icmp.verdict, sc.e_udp.verdict, sc.e_tcp.verdict,
                                sc.e_reass.verdict)
        assert t >= 8 and r >= 20
        tcp, reass = tcp + t, reass + r
        assert (sc.verdicts[sc.e_arp.status != AC.NONE] == RC.NOT_IP4).all()
    assert tcp >= 100 and reass >= 300


def test_idents_run_in_frame_order(scenarios):
    """Echo replies and unreachables share one count: response j in frame order carries the Ident
    ip_id + j, in the expected send ring too."""
    for sc in scenarios:
        ring, lens = G.send_ring(sc)
        j = 0
        for i in range(sc.n):
            if sc.owner[i] in (G.ICMP_ECHO, G.UDP_UNREACH):
                assert int.from_bytes(ring[i, 18:20].tobytes(), "big") == (sc.ifc["ip_id"] + j) & 0xFFFF
                assert lens[i] == 14 + int.from_bytes(ring[i, 16:18].tobytes(), "big")
                j += 1
            elif sc.owner[i] == G.ARP and lens[i]:
                assert lens[i] == 42
            else:
                assert lens[i] == 0 and (ring[i] == 0xC3).all()
        assert j == int(sc.e_icmp.counts[0]) >= 40


def test_generator_is_stable(oracle, scenarios):
    again = G.scenario(oracle, 3)
    assert again.frames == scenarios[3].frames and np.array_equal(again.owner, scenarios[3].owner)
    other = G.cached(oracle, 3, 1)
    assert other.n == again.n and other.frames != again.frames
    assert other.ifc == again.ifc and other.pcbs.tobytes() == again.pcbs.tobytes()
    assert (other.slotted, other.lead, other.aux_blocks) == (again.slotted, again.lead, again.aux_blocks)
    assert G.digest(scenarios[0].frames) == SEED0_DIGEST


# ---- the sessions recorded from the reference ------------------------------------------------------

def test_models_equal_the_reference_sessions(oracle):
    """Each session in two or three batches with next_ip_id += counts[0] between them: the ARP and
    ICMP models' responses, merged by frame index, are the frames the reference sent, in order and
    byte for byte (so the Ident runs over echo replies and port unreachables as its m_next_id
    did), and the delivery list and the records name its handler calls."""
    for s in LR.load():
        ip_id, sent, calls, idents = 0, 0, 0, []
        cuts = G.session_cuts(s)
        assert 3 <= len(cuts) <= 4 and cuts[0][0] == 0 and cuts[-1][1] == len(s["frames"])
        for start, end in cuts:
            sc = G.session_batch(oracle, s, start, end, ip_id, False)
            want = G.session_sent(s, start, end)
            assert sc.wire == want, (s["seed"], start, sorted(set(sc.wire) ^ set(want))[:8])
            calls += G.session_calls_match(s, start, sc, sc.e_udp.dgrams, sc.e_udp.deliver_frame,
                                           sc.e_udp.counts[0])
            assert not (sc.e_icmp.status == IC.TOO_LARGE).any()
            assert not np.isin(sc.owner, (G.TCP, G.REASS_MEMBER, G.HOST)).any() or \
                set(sc.host_sort[sc.owner == G.HOST]) == {3}          # other ICMP types only
            assert not np.isin(sc.owner, (G.TCP, G.REASS_MEMBER)).any()
            idents += [int.from_bytes(w[18:20], "big") for _, w in sorted(want.items()) if w[12:14] == b"\x08\x00"]
            ip_id += int(sc.e_icmp.counts[0])
            sent += len(want)
        assert idents == list(range(len(idents))) and len(idents) == ip_id >= 100
        assert sent >= 150 and calls >= 100


def test_sessions_hold_only_what_the_loop_answers():
    kinds = set()
    for s in LR.load():
        assert 300 <= len(s["frames"]) <= 400
        macs = {}
        for row in s["frames"]:
            f = bytes.fromhex(row[0])
            assert all(len(bytes.fromhex(o)) <= 1514 for o in row[1]) and len(row[1]) <= 1
            if len(f) >= 34 and f[12:14] == b"\x08\x00":
                assert f[23] in (1, 17) and not int.from_bytes(f[20:22], "big") & 0x3FFF      # no TCP, no fragment
                assert f[6:12] == macs[f[26:30]]              # the peer's ARP request came first
                kinds.add((f[23], bool(row[1]), bool(row[2])))
            elif len(f) >= 42 and f[12:14] == b"\x08\x06" and f[6:12] == f[22:28]:
                macs.setdefault(f[28:32], f[22:28])
            for o in row[1]:
                assert bytes.fromhex(o)[:6] == f[6:12]        # every response leaves for the frame's source
        assert len(macs) == 4
    assert kinds == {(p, a, b) for p in (1, 17) for a in (0, 1) for b in (0, 1)} - {(1, 0, 1), (1, 1, 1), (17, 1, 1)}
    assert {s["allow"] for s in LR.load()} == {0, 1}


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "aipstack")),
                    reason="reference tree not present")
def test_generator_reproduces_the_fixture():
    with open(LR.FIXTURE) as f:
        assert LR.generate(REFERENCE) == f.read()


def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(LR.FIXTURE) < 512 * 1024
    for s in LR.load():
        assert set(s) == {"allow", "addr", "prefix", "mac", "seed", "listeners", "assocs", "frames"}
        for fin, sent, calls in s["frames"]:
            bytes.fromhex(fin)
            for o in sent:
                bytes.fromhex(o)
            for c in calls:
                who, ln = c.split()
                assert who[0] in "LA" and int(who[1:]) >= 0 and int(ln) >= 0


# ---- the shared C++ demux on the scenarios, as a stand-alone program under ASan + UBSan ------------

def test_udp_demux_of_the_scenarios_through_the_shared_builder(scenarios):
    """The first two scenarios through tests/cpp/udprx_table_test.cpp, which runs the demux of
    udprx_common.h that the kernels run: record, unreach code and delivery of every frame are the
    model's."""
    from test_random_rx_cases import _run
    lines, cases = [], 0
    for sc in scenarios[:2]:
        a, l, e = sc.assocs, sc.listeners, sc.e_udp
        lines.append("T %d %d %s %s" % (sc.ifc["local"], sc.ifc["bcast"], a.tobytes().hex(),
                                         l.tobytes().hex() if l is not None else "-"))
        delivered = G.delivered_mask(e.deliver_frame, e.counts[0], sc.n)
        for i, f in enumerate(sc.frames):
            lines.append("F %d %s %s %d %d" % (int(sc.verdicts[i]), f.hex() or "-", e.dgrams[i].tobytes().hex(),
                                               int(e.unreach[i]), int(delivered[i])))
            cases += 1
    assert cases >= 2200
    _run("udprx.mk", "udprx_table_test", "rx_loop_udprx_cases.txt", lines, cases)
