"""The scenario generators of test_gpu_random_rx.py, checked on the CPU: over the full seed range,
with the oracle and the models, the scenarios cover what the GPU tests rely on them to cover; and
the scenarios of the first seeds go through the stand-alone ASan/UBSan builds of the shared C++
builders (tests/cpp/udprx_table_test.cpp, icmp_build_test.cpp), which must agree with the models
on every frame."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import icmp_cases as IC
import random_rx_cases as G
import udp_rx_cases as UC

PROGRAM_SEEDS = 10


@pytest.fixture(scope="module")
def udp(oracle):
    return [G.udp_scenario(oracle, s) for s in range(G.SEEDS)]


@pytest.fixture(scope="module")
def icmp(oracle):
    return [G.icmp_scenario(oracle, s) for s in range(G.SEEDS)]


# ---- UDP Rx demux -----------------------------------------------------------------------------

def test_udp_scenarios(udp):
    verdicts, flags, layouts, sizes = set(), set(), set(), set()
    first = last = below = above = refused = nonlocal_taken = cut = padded = dirty = 0
    near_miss, near_hit = [0] * 4, [0] * 4
    bits, data_lens, ihls, special_ports, ttls = set(), set(), set(), set(), set()
    delivered = unreach = both_causes = high_bit_scenarios = 0
    dsts = set()
    for sc in udp:
        e = sc.e
        assert 1 <= sc.n <= G.MAX_ELEMENTS and len(e.dgrams) == sc.n
        verdicts |= set(e.verdict.tolist())
        keys = G.udp_table_keys(sc)
        assert keys == sorted(keys, key=G.sort_key) and len(set(keys)) == len(keys)
        held = set(keys)
        sizes.add(len(keys))
        n_lis = 0 if sc.listeners is None else len(sc.listeners)
        layouts.add((sc.slotted, sc.lead if not sc.slotted else sc.slot, sc.dgram_shift, sc.aux_blocks))
        dirty += bool(sc.dirty and n_lis)
        if sc.dirty and n_lis:
            assert (sc.listeners["flags"] & 0xFC == 0xFC).all() and sc.listeners["reserved1"].all()
        valid = np.nonzero(e.dgrams["flags"] & UC.VALID)[0]
        delivered += int(e.counts[0])
        unreach += int(e.counts[1])
        seen_bits = set()
        for i in valid:
            f, rec = sc.frames[i], e.dgrams[i]
            k = G.udp_key(f)
            flags.add(int(rec["flags"]))
            ttls.add(int(rec["ttl"]))
            ihls.add(f[14] & 0xF)
            data_lens.add(int(rec["data_len"]))
            special_ports |= {int(rec["local_port"]), int(rec["remote_port"])} & set(G.SPECIAL_PORTS)
            hl = (f[14] & 0xF) * 4
            total = struct.unpack_from(">H", f, 16)[0]
            cut += int(rec["data_len"]) + 8 < total - hl
            padded += 14 + total < len(f)
            dsts.add("local" if k[0] == sc.ifc["local"] else "bcast" if k[0] == sc.ifc["bcast"]
                     else "ones" if k[0] == G.ALL_ONES else "other")
            m = int(rec["listeners"])
            seen_bits |= {b for b in range(64) if m >> b & 1}
            both_causes += bool(m) and rec["assoc"] != UC.NO_ASSOC
            if k in held:
                first += k == keys[0]
                last += k == keys[-1]
                cookie = int(sc.assocs["cookie"][keys.index(k)])
                local = k[0] == sc.ifc["local"]
                refused += not local and not cookie & UC.ASSOC_NONLOCAL
                nonlocal_taken += not local and bool(cookie & UC.ASSOC_NONLOCAL)
                assert (rec["assoc"] == UC.NO_ASSOC) == (not local and not cookie & UC.ASSOC_NONLOCAL)
            elif keys:
                assert rec["assoc"] == UC.NO_ASSOC
                below += G.sort_key(k) < G.sort_key(keys[0])
                above += G.sort_key(k) > G.sort_key(keys[-1])
            for fld in range(4):
                if any(q in held for q in G.neighbours(k, fld)):
                    if k in held:
                        near_hit[fld] += 1
                    else:
                        near_miss[fld] += 1
        bits |= seen_bits
        high_bit_scenarios += {31, 32, 63} <= seen_bits
        if sc.edge is not None:                          # the pinned ends: hit, and missed on both sides
            got = {G.udp_key(sc.frames[i]): e.dgrams[i] for i in valid}
            assert sc.edge[0] == keys[0] and sc.edge[1] == keys[-1]
            assert all(k in got for k in sc.edge)
            assert got[sc.edge[0]]["assoc"] != UC.NO_ASSOC and got[sc.edge[1]]["assoc"] != UC.NO_ASSOC
            assert got[sc.edge[2]]["assoc"] == got[sc.edge[3]]["assoc"] == UC.NO_ASSOC
    assert verdicts == set(range(9))
    # every flag combination: the checksum field zero or not, and the destination the interface's
    # address, a broadcast address or neither (it cannot be both)
    assert flags == {UC.VALID | c | d for c in (0, UC.HAS_CHKSUM) for d in (0, UC.DST_LOCAL, UC.DST_BCAST)}
    assert dsts == {"local", "bcast", "ones", "other"}
    assert first >= 10 and last >= 10 and below >= 10 and above >= 10
    assert sum(sc.edge is not None for sc in udp) >= 10
    assert min(near_miss) >= 20 and min(near_hit) >= 20       # per field: one-field neighbours in the table
    assert refused >= 10 and nonlocal_taken >= 10             # cookie bit 31 decides
    # listener bits in both halves of the mask, and 31, 32 and 63 together in one scenario
    assert {0, 31, 32, 63} <= bits and len([b for b in bits if b >= 32]) >= 16 and high_bit_scenarios >= 3
    assert {0, 1, 2, 3} <= sizes and max(sizes) >= 1500
    assert any(s >= 4 and s & (s - 1) == 0 for s in sizes)
    assert any(s >= 4 and (s + 1) & s == 0 for s in sizes) and any(s >= 5 and (s - 1) & (s - 2) == 0 for s in sizes)
    n_lis = {0 if sc.listeners is None else len(sc.listeners) for sc in udp}
    assert {0, 64} <= n_lis and len(n_lis) >= 10 and dirty >= 5
    assert {0, 1} <= data_lens and any(d & 1 and d > 1 for d in data_lens) and max(data_lens) >= 1400
    assert ihls == set(range(5, 16)) and special_ports == set(G.SPECIAL_PORTS) and {0, 255} <= ttls
    assert cut >= 100 and padded >= 100
    assert delivered >= 1000 and unreach >= 1000 and both_causes >= 50
    assert {(s, d) for s, _, d, _ in layouts} == {(s, d) for s in (False, True) for d in (0, 8)}
    assert {l for s, l, _, _ in layouts if not s} == {0, 1, 2, 3}
    assert {l for s, l, _, _ in layouts if s} >= {2048, 2049} and len({l for s, l, _, _ in layouts if s}) >= 4
    assert {a for _, _, _, a in layouts} == set(G.AUX_BLOCKS)
    assert any(sc.n < 8 for sc in udp) and any(sc.n > 1024 for sc in udp)
    short = sum(1 for sc in udp for f in sc.frames if len(f) < 42)
    assert short >= 100


# ---- ICMP responder ---------------------------------------------------------------------------

def test_icmp_scenarios(icmp):
    statuses, verdicts, classes, layouts, mtus, unreach_codes = {}, set(), {}, set(), set(), set()
    wraps = multi = no_codes = code_on_rejected = reply_cks = 0
    data_kinds, echo_dsts, refused_src, allow = set(), set(), 0, set()
    reply_fields = set()
    for sc in icmp:
        assert 1 <= sc.n <= G.MAX_ELEMENTS
        assert [b[0] for b in sc.batches] == [0] + [b[1] for b in sc.batches[:-1]] and sc.batches[-1][1] == sc.n
        verdicts |= set(sc.verdicts.tolist())
        layouts.add((sc.slotted, sc.hdr_stride, sc.shift, sc.aux_blocks))
        mtus.add(sc.ifc["mtu"])
        allow.add(sc.ifc["allow"])
        multi += len(sc.batches) > 1
        no_codes += sc.codes is None
        if sc.codes is not None:
            rejected = ~np.isin(sc.verdicts, (IC.ACCEPT, IC.ACCEPT_NO_CHKSUM, IC.ACCEPT_OTHER))
            code_on_rejected += int((rejected & (np.array(sc.codes) != IC.NO_UNREACH)).sum())
        for start, end, ifc, e in sc.batches:
            assert (e.status[:-1] != IC.TOO_LARGE).all()            # only a batch's last frame
            wraps += ifc["ip_id"] + int(e.counts[0]) > 0x10000      # an Ident 0xFFFF and an Ident 0
            for st, cnt in zip(*np.unique(e.status, return_counts=True)):
                statuses[int(st)] = statuses.get(int(st), 0) + int(cnt)
            for i in e.headers:
                f = sc.frames[start + i]
                ck = struct.unpack_from(">H", e.headers[i], 36)[0]
                if e.status[i] == IC.UNREACH:
                    unreach_codes.add(sc.codes[start + i])
                    continue
                c = G.echo_class(f)
                classes[c] = classes.get(c, 0) + 1
                if c == "zero_class":
                    reply_fields.add(ck)
                t = 14 + (f[14] & 0xF) * 4
                total = struct.unpack_from(">H", f, 16)[0]
                data = f[t + 8:14 + total]
                data_kinds.add("empty" if not data else "one" if len(data) == 1 else
                               "zero" if not any(data) else "ones" if all(b == 0xFF for b in data) else
                               "odd" if len(data) & 1 else "even")
                if 28 + len(data) == ifc["mtu"]:
                    data_kinds.add("mtu")
                dst = struct.unpack_from(">I", f, 30)[0]
                echo_dsts.add("local" if dst == ifc["local"] else "bcast" if dst == ifc["bcast"] else "ones")
        # a request from a source the reference does not answer
        for i, f in enumerate(sc.frames):
            if len(f) >= 42 and sc.verdicts[i] == IC.ACCEPT and f[23] == 1:
                src = struct.unpack_from(">I", f, 26)[0]
                refused_src += src in (G.ALL_ONES, sc.ifc["bcast"]) or src >> 28 == 0xE
    assert verdicts == set(range(9))
    assert set(statuses) == {IC.NONE, IC.ECHO_REPLY, IC.UNREACH, IC.TOO_LARGE}
    assert statuses[IC.ECHO_REPLY] >= 2000 and statuses[IC.UNREACH] >= 300 and statuses[IC.TOO_LARGE] >= 20
    assert multi >= 10 and no_codes >= 3 and code_on_rejected >= 300
    assert wraps >= 5
    # each class of the echo checksum update, and both outcomes of the one that reads the data
    assert set(classes) == set(G.ECHO_CLASSES) | {"plain"} and min(classes.values()) >= 40
    assert reply_fields == {0x0000, 0xFFFF}
    assert unreach_codes == set(range(16))
    assert data_kinds == {"empty", "one", "zero", "ones", "odd", "even", "mtu"}
    assert echo_dsts == {"local", "bcast", "ones"} and allow == {False, True} and refused_src >= 50
    assert set(G.MTUS) <= mtus and len(mtus) > len(G.MTUS)
    assert {(s, h) for s, h, _, _ in layouts} >= {(s, h) for s in (False, True) for h in (42, 64)}
    assert {h for _, h, _, _ in layouts} == set(G.HDR_STRIDES)
    assert {(h, s) for _, h, s, _ in layouts} >= {(64, 0), (64, 8)}      # whole lines and plain stores
    assert {a for _, _, _, a in layouts} == set(G.AUX_BLOCKS)
    assert any(sc.n < 8 for sc in icmp) and any(sc.n > 1024 for sc in icmp)


# ---- the shared C++ builders on the scenarios, under ASan + UBSan -----------------------------

_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
            UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def _run(mk, program, name, lines, cases):
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", mk], check=True, stdout=subprocess.DEVNULL)
    path = os.path.join(cpp, "build", name)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([os.path.join(cpp, "build", "asan", program), path], env=_ENV,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK %d cases" % cases in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_udp_scenarios_through_the_shared_builder(udp):
    lines, cases = [], 0
    for sc in udp[:PROGRAM_SEEDS]:
        a, l, e = sc.assocs, sc.listeners, sc.e
        lines.append("T %d %d %s %s" % (sc.ifc["local"], sc.ifc["bcast"],
                                         a.tobytes().hex() if a is not None else "-",
                                         l.tobytes().hex() if l is not None else "-"))
        delivered = set(e.deliver_frame[:int(e.counts[0])].tolist())
        for i, f in enumerate(sc.frames):
            lines.append("F %d %s %s %d %d" % (int(sc.verdicts[i]), f.hex() or "-", e.dgrams[i].tobytes().hex(),
                                               int(e.unreach[i]), int(i in delivered)))
            cases += 1
    assert cases >= 2000
    _run("udprx.mk", "udprx_table_test", "random_udprx_cases.txt", lines, cases)


def test_icmp_scenarios_through_the_shared_builder(icmp):
    lines = []
    for sc in icmp[:PROGRAM_SEEDS]:
        for start, end, ifc, e in sc.batches:
            by_frame = {fi: (off, ln) for fi, off, ln in e.chunks}
            j = 0
            for i in range(end - start):
                f, st = sc.frames[start + i], int(e.status[i])
                code = IC.NO_UNREACH if sc.codes is None else sc.codes[start + i]
                off, ln = IC.plan(f, int(sc.verdicts[start + i]), code, ifc)[1:] if st != IC.NONE else (0, 0)
                if i in e.headers:
                    assert by_frame.get(i, (off, 0)) == (off, ln)
                lines.append("%d %d %d %d %d %s %d %d %d %d %d %d %s %s" % (
                    ifc["local"], ifc["bcast"], ifc["mtu"], ifc["ttl"], int(ifc["allow"]), ifc["mac"].hex(),
                    int(sc.verdicts[start + i]), code, ifc["ip_id"] + j, st, off, ln, f.hex() or "-",
                    e.headers[i].hex() if i in e.headers else "-"))
                j += i in e.headers
    assert len(lines) >= 2000 and any(len(sc.batches) > 1 for sc in icmp[:PROGRAM_SEEDS])
    _run("icmp.mk", "icmp_build_test", "random_icmp_cases.txt", lines, len(lines))
