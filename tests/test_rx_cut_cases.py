"""The inputs of test_gpu_rx_cut.py are not vacuous: properties of rx_cut_cases.py's batches and of
the models alone, checked without a GPU; and the same family-A frames through the stand-alone host
programs of tests/cpp that take their cases from a file (ARP, ICMP respond, UDP demux, TCP respond,
ICMP Destination Unreachable), which run the *_common.h functions the kernels are built from under
ASan and UBSan. tcprx_table_test and ipreass_table_test carry their cases in their own text and
take none from outside; Rx verify has no host program (its reference is the frame oracle)."""
import os
import subprocess

import numpy as np
import pytest

import aipstack_amd as A
from conftest import ROOT

import rx_cut_cases as X

NAMES = list(X.STAGES)
PASSES = {"ip4_rx_reassemble": (3,)}          # what Rx verify hands this stage; elsewhere 6, 7, 8

_e = {}


def _expected(oracle, name, family):
    """(batch, the model's Expected for the cases as the slotted form sees them, outcome codes)."""
    if (name, family) not in _e:
        b = X.cached(oracle, name, family)
        e = X.STAGES[name].expect(oracle, [f for f, _ in b.cases])
        _e[(name, family)] = (b, e, list(X.STAGES[name].outcome(e)))
    return _e[(name, family)]


@pytest.mark.parametrize("name", NAMES)
def test_family_a_has_every_length_of_every_seed(oracle, name):
    b, _, _ = _expected(oracle, name, "A")
    assert len(b.seeds) >= 4 and max(len(s) for s in b.seeds) <= 160
    for j, s in enumerate(b.seeds):
        for variant in (0, 1):
            rows = np.flatnonzero((b.seed == j) & (b.variant == variant))
            assert sorted(b.k[rows].tolist()) == list(range(len(s) + 1)), (j, variant)
            assert all(b.cases[i][0] == s[:int(b.k[i])] or name == "ip4_rx_reassemble" for i in rows)
            assert all(len(b.cases[i][0]) == b.k[i] for i in rows)
    assert len(b.cases) < 2200                                       # a few thousand frames, not more


@pytest.mark.parametrize("name", NAMES)
def test_family_a_has_three_verdicts(oracle, name):
    """Rx verify's verdicts, from the frame oracle; ARP runs no verify: its statuses."""
    b, e, out = _expected(oracle, name, "A")
    if X.STAGES[name].has_verdict:
        assert len(set(X.verdicts_of(oracle, [f for f, _ in b.cases]).tolist())) >= 3
    else:
        assert len(set(out)) >= 3


@pytest.mark.parametrize("name", NAMES)
def test_uncut_seeds_take_the_interesting_path_and_a_cut_changes_it(oracle, name):
    b, _, out = _expected(oracle, name, "A")
    st = X.STAGES[name]
    for j in range(b.n_seeds):
        s = b.seeds[j]
        rows = np.flatnonzero(b.seed == j)
        full = [i for i in rows if b.k[i] == len(s)]
        assert len(full) == 2 and all(out[i] in st.interesting for i in full), (j, [out[i] for i in full])
        assert any(out[i] not in st.interesting for i in rows), j


@pytest.mark.parametrize("name", NAMES)
def test_seeds_have_the_shapes_that_go_wrong(oracle, name):
    """IHL 6 or more, padding to 60 bytes (a Destination Unreachable has at least 62: padding
    behind the total length), TCP options that end on the frame's last byte, a quoted IHL above 5
    and a quoted total length on both sides of the quoted bytes present."""
    st = X.STAGES[name]
    seeds = st.seeds(oracle)
    if name == "arp_rx_respond":
        assert {len(s) for s in seeds} >= {42, 60}
        return
    assert any(s[14] & 0xF >= 6 for s in seeds)
    total = [int.from_bytes(s[16:18], "big") for s in seeds]
    if name == "icmp_rx_unreach":
        assert any(len(s) > 14 + t for s, t in zip(seeds, total))
        q = [s[14 + (s[14] & 0xF) * 4 + 8:14 + t] for s, t in zip(seeds, total)]
        assert any(d[0] & 0xF > 5 for d in q)
        sides = {(int.from_bytes(d[2:4], "big") > len(d)) - (int.from_bytes(d[2:4], "big") < len(d)) for d in q}
        assert sides == {-1, 0, 1}
    else:
        assert any(len(s) == 60 and 14 + t < 60 for s, t in zip(seeds, total))
    if name in ("tcp_rx_parse", "tcp_rx_respond", "rx_verify"):
        def ends_on_options(s):
            T = 14 + (s[14] & 0xF) * 4
            return s[23] == 6 and s[T + 12] >> 4 > 5 and T + (s[T + 12] >> 4) * 4 == len(s)
        assert any(ends_on_options(s) for s in seeds)


@pytest.mark.parametrize("name", NAMES)
def test_families_a_and_b_reach_every_code(oracle, name):
    st = X.STAGES[name]
    seen = set(_expected(oracle, name, "A")[2]) | set(_expected(oracle, name, "B")[2])
    seen = {int(c) if not isinstance(c, str) else c for c in seen}
    assert set(st.codes) - seen == set(st.exempt), (set(st.codes) - seen, st.exempt)
    # the exemptions, by name
    assert set(st.exempt) == ({X.IC.TOO_LARGE} if name == "icmp_rx_respond" else set())


@pytest.mark.parametrize("name", NAMES)
def test_tails_differ_and_the_models_do_not_see_them(oracle, name):
    b, _, out = _expected(oracle, name, "A")
    for i, p in enumerate(b.partner):
        (f, t), (g, u) = b.cases[i], b.cases[p]
        assert len(t) == len(u) and (not t or t != u), i
        assert len(f) + len(t) >= len(b.seeds[b.seed[i]]) + X.EXTRA or b.seed[i] < 0
        assert out[i] == out[p]
        if name != "ip4_rx_reassemble":       # there the two variants are two trains: other Idents
            assert f == g
    assert sum(1 for f, t in b.cases if t) >= len(b.cases) - 0
    # family C: every byte outside the frames differs between the two layouts, none inside
    c = X.cached(oracle, name, "C")
    assert len(c.cases) == X.C_FRAMES
    for slotted in (False, True):
        one, two = X.lay_out(c, slotted), X.lay_out(c, slotted, alt=True)
        m = X.outside(c, one)
        assert one.host.size == two.host.size and (one.host[m] != two.host[m]).all()
        assert np.array_equal(one.host[~m], two.host[~m]) and m.sum() > 2 * X.GUARD
        assert [f for f in one.frames[::1 if slotted else 2]] == [f for f, _ in c.cases]
        if not slotted:
            assert {len(g) for g in one.frames[1::2]} == set(range(8))
            e1, e2 = (X.STAGES[name].expect(oracle, lay.frames) for lay in (one, two))
            assert list(X.STAGES[name].outcome(e1)) == list(X.STAGES[name].outcome(e2))


@pytest.mark.parametrize("name", NAMES)
def test_family_b_gets_past_rx_verify(oracle, name):
    """At least a fifth of family B reaches the stage (for reassembly: as a fragment). ARP runs no
    Rx verify; there a tenth of its field sweep must still be well-formed ARP."""
    b, e, out = _expected(oracle, name, "B")
    if name == "arp_rx_respond":
        assert np.isin(e.status, (X.AC.SEEN, X.AC.REPLY)).mean() >= 0.1
        return
    v = X.verdicts_of(oracle, [f for f, _ in b.cases])
    assert np.isin(v, PASSES.get(name, (6, 7, 8))).mean() >= 0.2
    assert set(b.what) == set(X.STAGES[name].sweeps)


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("name", NAMES)
def test_every_frame_has_room_inside_the_buffer(oracle, name, family):
    b = X.cached(oracle, name, family)
    leads = set()
    for slotted in (False, True):
        lay = X.lay_out(b, slotted)
        start = lay.start[lay.index]
        reach = np.maximum(np.array([len(f) for f, _ in b.cases]), b.room)
        if family != "C":
            seed_len = np.array([len(b.seeds[j]) if j >= 0 else 0 for j in b.seed])
            reach = np.maximum(reach, seed_len)
        assert (start - X.GUARD >= 0).all() and (start + reach + X.GUARD <= lay.host.size).all()
        if slotted:
            assert lay.stride == (2048 if name == "ip4_rx_reassemble" or family == "C" and lay.stride != 256
                                  else 256)
            assert (reach <= lay.stride).all()
        else:
            leads.add(int(lay.offsets[0]) - X.GUARD)
    assert leads <= {0, 1, 2, 3}


def test_csr_leads_vary():
    leads = {(list(X.STAGES).index(n) + k) % 4 for n in NAMES for k in range(3)}
    assert leads == {0, 1, 2, 3}


# ---- the host path: the *_common.h functions, through the stand-alone programs ------------------

def _run(mk, prog, lines, count=None):
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", mk], check=True, stdout=subprocess.DEVNULL)
    path = os.path.join(cpp, "build", "rx_cut_" + prog + ".txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", prog), path], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "OK %d cases" % (len(lines) if count is None else count) in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _ab(oracle, name):
    """Families A and B of a stage as one list of frames with the model's answer."""
    frames = [f for fam in "AB" for f, _ in X.cached(oracle, name, fam).cases]
    return frames, X.verdicts_of(oracle, frames), X.STAGES[name].expect(oracle, frames)


def test_host_arp(oracle):
    st = X.STAGES["arp_rx_respond"]
    frames, _, e = _ab(oracle, st.name)
    ifc = st.ifc
    _run("arp.mk", "arp_build_test", ["%d %d %d %s %s %s %s" % (
        ifc["local"], ifc["netmask"], int(ifc["have"]), ifc["mac"].hex(), e.records[i].tobytes().hex(),
        f.hex() or "-", e.headers[i].hex() if i in e.headers else "-") for i, f in enumerate(frames)])


def test_host_icmp(oracle):
    st = X.STAGES["icmp_rx_respond"]
    frames, v, e = _ab(oracle, st.name)
    ifc, codes = st.ifc, st.codes_of(frames)
    lines, j = [], 0
    for i, f in enumerate(frames):
        status = int(e.status[i])
        off, ln = X.IC.plan(f, int(v[i]), codes[i], ifc)[1:] if status != X.IC.NONE else (0, 0)
        lines.append("%d %d %d %d %d %s %d %d %d %d %d %d %s %s" % (
            ifc["local"], ifc["bcast"], ifc["mtu"], ifc["ttl"], int(ifc["allow"]), ifc["mac"].hex(), int(v[i]),
            codes[i], ifc["ip_id"] + j, status, off, ln, f.hex(), e.headers[i].hex() if i in e.headers else "-"))
        j += i in e.headers
    _run("icmp.mk", "icmp_build_test", [ln for ln, f in zip(lines, frames) if f])    # its format has no empty frame


def test_host_udp(oracle):
    st = X.STAGES["udp_rx_demux"]
    frames, v, e = _ab(oracle, st.name)
    delivered = set(e.deliver_frame[:int(e.counts[0])].tolist())
    lines = ["T %d %d %s %s" % (st.ifc["local"], st.ifc["bcast"], st.assocs.tobytes().hex(),
                                st.listeners.tobytes().hex())]
    lines += ["F %d %s %s %d %d" % (int(v[i]), f.hex() or "-", e.dgrams[i].tobytes().hex(), int(e.unreach[i]),
                                    int(i in delivered)) for i, f in enumerate(frames)]
    _run("udprx.mk", "udprx_table_test", lines, len(frames))


def test_host_tcp_rsp(oracle):
    st = X.STAGES["tcp_rx_respond"]
    frames, v, e = _ab(oracle, st.name)
    ifc, lis = st.ifc, st.lis
    tail = "%d %s" % (len(lis), " ".join("%d %d %d" % l for l in lis))
    place = {int(i): j for j, i in enumerate(e.response_frame[:int(e.counts[0])])}
    _run("tcp_rsp.mk", "tcp_rsp_build_test", ["%d %d %d %d %d %s %d %d %d %d %d %d %s %s %s %s" % (
        ifc["local"], ifc["bcast"], ifc["mtu"], ifc["ip_id"], ifc["ttl"], ifc["mac"].hex(), int(v[i] == 6),
        int(e.pcb[i] != 0xFFFFFFFF), 0, place.get(i, 0), int(e.status[i]), int(e.listener[i]),
        e.segs[i].tobytes().hex() if e.segs["opts"][i] & 0x80 else "-", f.hex() or "-",
        e.headers[i].hex() if i in e.headers else "-", tail) for i, f in enumerate(frames)])


def test_host_icmp_du(oracle):
    st = X.STAGES["icmp_rx_unreach"]
    frames, v, e = _ab(oracle, st.name)
    s = A.tcp_pcb_table_sort(st.pcbs)
    lines = ["T %d" % len(s)] + ["%d %d %d %d %d" % tuple(int(x) for x in k) for k in s]
    lines += ["%d %d %d %d %s %s" % (st.ifc["local"], st.ifc["bcast"], int(v[i] == 6), int(e.status[i]),
                                     e.records[i].tobytes().hex() if e.status[i] != X.DU.NONE else "-",
                                     f.hex() or "-") for i, f in enumerate(frames)]
    _run("icmp_du.mk", "icmp_du_build_test", lines, len(frames))
