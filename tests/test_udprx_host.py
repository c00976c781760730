"""The UDP Rx demux, the parts that need no GPU: the model of udp_rx_cases.py pinned against the
handler calls and the port unreachables recorded from the reference's own stack
(tests/golden/udp_rx_ref_cases.json), the fixture's coverage, the structs and the constants, the
argument validation of the two batch calls (rejected before any HIP call), and the shared record
builder, table search and listener match under ASan/UBSan as a stand-alone program
(tests/cpp/udprx_table_test.cpp)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib
from conftest import ROOT

import frame_cases as F
import udp_rx_cases as C
import udp_rx_ref as R

REFERENCE = "/root/reference"
KEY, LIS, DGRAM = A.TCP_PCB_KEY_DTYPE, A.UDP_LISTENER_DTYPE, A.UDP_RX_DGRAM_DTYPE


def _verdicts(oracle, frames):
    buf, off = F.pack(frames)
    return oracle.rx_verify_batch(buf, off)


@pytest.fixture(scope="module")
def replayed(oracle):
    """[(stack, frames, verdicts, iface, association table, listener table, Expected)]"""
    out = []
    for s in R.load():
        frames = C.stack_frames(s)
        v = _verdicts(oracle, frames)
        a, l = C.stack_tables(s, KEY, LIS)
        ifc = C.stack_iface(s)
        out.append((s, frames, v, ifc, a, l, C.expected(frames, v, ifc, a, l, DGRAM)))
    return out


# ---- the model against the reference's recorded calls and packets ------------------------------

def _is_port_unreach(pkt, case):
    p, q = bytes.fromhex(pkt), bytes.fromhex(case["in"])
    hl = (q[0] & 0xF) * 4
    return p[9] == 1 and p[20:22] == b"\x03\x03" and p[28:28 + hl + 8] == q[:hl + 8]


def test_model_equals_the_reference(replayed):
    """Every case: the record's association and listener mask name exactly the handlers the
    reference called, in its order, with the data it gave them (length, FNV-1a, has_checksum);
    unreach code 3 exactly where the reference sent a port unreachable with no handler called
    (but for the marked sources checkSendIp4Allowed refuses); and with every handler rejecting,
    a port unreachable exactly for the records with DST_LOCAL (:611)."""
    seen = 0
    for s, frames, v, ifc, a, l, e in replayed:
        for i, case in enumerate(s["cases"]):
            name = case["name"]
            assert C.calls_of(e, i, frames[i], l) == case["calls"], name
            rec = e.dgrams[i]
            valid = bool(rec["flags"] & C.VALID)
            local = bool(rec["flags"] & C.DST_LOCAL)
            assert all(_is_port_unreach(p, case) for p in case["out"] + case["reject_out"]), name
            if not valid:
                assert case["calls"] == [] and case["out"] == [] and case["reject_out"] == [], name
                assert e.unreach[i] == C.NO_UNREACH and not rec.tobytes().strip(b"\0"), name
                continue
            sent = 0 if case["src_rejected"] else 1
            if case["calls"]:
                assert case["out"] == [] and e.unreach[i] == C.NO_UNREACH, name
                assert len(case["reject_out"]) == (sent if local else 0), name
                assert i in e.deliver_frame[:int(e.counts[0])], name
            else:
                want = C.PORT_UNREACH if local else C.NO_UNREACH
                assert e.unreach[i] == want, name
                assert len(case["out"]) == len(case["reject_out"]) == (sent if local else 0), name
                assert i not in e.deliver_frame[:int(e.counts[0])], name
            seen += 1
        assert int(e.counts[1]) == int((e.unreach == C.PORT_UNREACH).sum())
    assert seen >= 80


def test_fixture_covers_the_branches(replayed):
    by = {}
    for s, frames, v, ifc, a, l, e in replayed:
        for i, case in enumerate(s["cases"]):
            by[case["name"]] = (case, frames[i], int(v[i]), e.dgrams[i], int(e.unreach[i]),
                                [c.split()[0] for c in case["calls"]])
    ports = next(s for s, *_ in replayed if s["name"] == "ports")
    # listener port: 0 (stack "any"), equal, different
    assert by["any_port1_dst_local"][5] == ["L2", "L1", "L0"]
    assert by["lis_port5001_dst_local"][5] == ["L1"] and by["lis_port7_dst_local"][5] == []
    # accept_broadcast on and off against all-ones, the subnet broadcast and unicast
    for dst in ("bcast", "allones"):
        assert by["lis_port5001_dst_" + dst][5] == ["L1"]                  # on
        assert "L0" not in by["lis_port5000_dst_" + dst][5]                # off
        assert by["lis_port5000_dst_" + dst][5] == ["L7"]
        assert by["lis_port5002_dst_" + dst][5] == []                      # nonlocal alone is not enough
        assert by["lis_port5003_dst_" + dst][5] == ["L3"]
    assert by["lis_port5000_dst_bcast"][3]["flags"] & C.DST_BCAST
    assert struct.unpack_from(">I", by["lis_port5000_dst_allones"][1], 30)[0] == 0xFFFFFFFF
    # accept_nonlocal_dst on and off against local and non-local unicast
    assert by["lis_port5002_dst_nonlocal"][5] == ["L2"] and by["lis_port5002_dst_local"][5] == ["L2"]
    assert by["lis_port5000_dst_nonlocal"][5] == [] and by["lis_port5001_dst_nonlocal"][5] == []
    assert by["lis_port5003_dst_nonlocal"][5] == ["L3"]
    # iface_addr zero, equal, different
    assert ports["listeners"][5][0] == R.LOCAL and by["lis_port5004_dst_local"][5] == ["L5"]
    assert ports["listeners"][6][0] not in (0, R.LOCAL)
    assert all(by["lis_port5005_dst_" + d][5] == [] for d, _ in R.DSTS)
    # several listeners, and an association with them
    assert by["assoc_and_listeners"][5] == ["A3", "L7", "L4", "L0"]
    assert by["assoc_and_listeners_miss_remote_port"][5] == ["L7", "L4", "L0"]
    # associations
    assert by["assoc_hit"][5] == ["A0"] and by["assoc_nonlocal_accepted"][5] == ["A1"]
    assert by["assoc_nonlocal_refused"][5] == [] and by["assoc_nonlocal_refused"][4] == C.NO_UNREACH
    assert by["assoc_bcast_dst"][5] == ["A4"] and by["assoc_hit_nonlocal_flag_local_dst"][5] == ["A5"]
    base = F_key(by["assoc_hit"][1])
    for name, field in (("assoc_miss_remote_addr", 1), ("assoc_miss_remote_port", 3),
                        ("assoc_miss_local_port", 2), ("assoc_miss_local_addr", 0)):
        k = F_key(by[name][1])
        assert [x != y for x, y in zip(k, base)] == [j == field for j in range(4)], name
        assert by[name][5] == []
        assert by[name][4] == (C.NO_UNREACH if field == 0 else C.PORT_UNREACH), name
    # the UDP length
    for pn, calls in (("open", ["A3", "L7", "L4", "L0"]), ("closed", []), ("assoc", ["A0"])):
        assert by["len_8_" + pn][3]["data_len"] == 0 and by["len_8_" + pn][5] == calls
        c, f, v, rec, u, got = by["len_truncates_" + pn]
        ip_payload = struct.unpack_from(">H", f, 16)[0] - 20
        assert rec["data_len"] == 6 and ip_payload == 8 + 6 + 9 and got == calls and v == C.ACCEPT
        assert by["len_truncates_to_8_" + pn][3]["data_len"] == 0
        assert by["len_equal_" + pn][3]["data_len"] == 20
        for name in ("len_above_ip_", "len_7_", "len_0_"):
            assert by[name + pn][2] == 4 and by[name + pn][5] == [] and not by[name + pn][3]["flags"]
        # the checksum: field 0, good, bad
        assert by["chksum_zero_" + pn][2] == C.ACCEPT_NO_CHKSUM
        assert not by["chksum_zero_" + pn][3]["flags"] & C.HAS_CHKSUM
        assert by["chksum_good_" + pn][2] == C.ACCEPT and by["chksum_good_" + pn][3]["flags"] & C.HAS_CHKSUM
        assert by["chksum_bad_" + pn][2] == 5 and by["chksum_bad_" + pn][5] == []
        assert by["chksum_bad_" + pn][0]["out"] == []
        assert by["chksum_zero_truncated_" + pn][3]["data_len"] == 5
        # IHL 5 and 15
        assert by["ihl5_" + pn][1][14] == 0x45 and by["ihl15_" + pn][1][14] == 0x4F
        assert by["ihl15_" + pn][3]["data_off"] == 14 + 60 + 8 and by["ihl15_" + pn][3]["ttl"] == 22
        assert by["ihl15_" + pn][5] == calls
    assert by["len_8_closed"][4] == by["ihl15_closed"][4] == C.PORT_UNREACH
    # the sources the reference refuses an unreach: marked, and the code is still 3
    for name in ("src_all_ones_closed", "src_bcast_closed"):
        assert by[name][0]["src_rejected"] == 1 and by[name][0]["out"] == [] and by[name][4] == C.PORT_UNREACH
    assert by["src_multicast_closed"][0]["src_rejected"] == 0 and len(by["src_multicast_closed"][0]["out"]) == 1
    assert by["none_dst_local"][4] == C.PORT_UNREACH and by["none_dst_bcast"][4] == C.NO_UNREACH


def F_key(frame):
    T = 14 + (frame[14] & 0xF) * 4
    src, dst = struct.unpack_from(">II", frame, 26)
    sport, dport = struct.unpack_from(">HH", frame, T)
    return dst, src, dport, sport


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "aipstack")),
                    reason="reference tree not present")
def test_generator_reproduces_the_fixture():
    with open(R.FIXTURE) as f:
        assert R.generate(REFERENCE) == f.read()


def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(R.FIXTURE) < 256 * 1024
    for s in R.load():
        assert set(s) == {"name", "addr", "prefix", "gateway", "listeners", "assocs", "cases"}
        assert all(len(l) == 4 and all(isinstance(x, int) for x in l) for l in s["listeners"])
        assert all(len(a) == 5 and all(isinstance(x, int) for x in a) for a in s["assocs"])
        for c in s["cases"]:
            assert set(c) == {"name", "in", "calls", "out", "reject_out", "src_rejected"}
            bytes.fromhex(c["in"])
            for p in c["out"] + c["reject_out"]:
                bytes.fromhex(p)
            for call in c["calls"]:
                k, ln, h, hc = call.split()
                assert k[0] in "AL" and int(k[1:]) >= 0 and int(ln) >= 0 and len(h) == 16 and hc in "01"


# ---- the structs and the constants --------------------------------------------------------------

class _CListener(ctypes.Structure):
    _fields_ = [("iface_addr", ctypes.c_uint32), ("port", ctypes.c_uint16), ("flags", ctypes.c_uint8),
                ("reserved0", ctypes.c_uint8), ("cookie", ctypes.c_uint32), ("reserved1", ctypes.c_uint32)]


class _CDgram(ctypes.Structure):
    _fields_ = [("remote_addr", ctypes.c_uint32), ("local_addr", ctypes.c_uint32),
                ("remote_port", ctypes.c_uint16), ("local_port", ctypes.c_uint16),
                ("data_off", ctypes.c_uint16), ("data_len", ctypes.c_uint16),
                ("listeners", ctypes.c_uint64), ("assoc", ctypes.c_uint32), ("flags", ctypes.c_uint8),
                ("ttl", ctypes.c_uint8), ("reserved", ctypes.c_uint16)]


@pytest.mark.parametrize("d,c,size", [(LIS, _CListener, 16), (DGRAM, _CDgram, 32)])
def test_dtypes_match_the_c_structs(d, c, size):
    assert d.itemsize == size == ctypes.sizeof(c)
    assert list(d.names) == [n for n, _ in c._fields_]
    for name, ct in c._fields_:
        assert d.fields[name][1] == getattr(c, name).offset, name
        assert d.fields[name][0].itemsize == ctypes.sizeof(ct), name


def test_constants():
    assert (A.AIPSTACK_UDP_NO_ASSOC, A.AIPSTACK_UDP_ASSOC_NONLOCAL, A.AIPSTACK_UDP_MAX_LISTENERS) == (
        0xFFFFFFFF, 0x80000000, 64) == (C.NO_ASSOC, C.ASSOC_NONLOCAL, 64)
    assert (A.AIPSTACK_UDP_LIS_BROADCAST, A.AIPSTACK_UDP_LIS_NONLOCAL) == (1, 2) == (C.LIS_BROADCAST, C.LIS_NONLOCAL)
    assert (A.AIPSTACK_UDP_DGRAM_VALID, A.AIPSTACK_UDP_DGRAM_HAS_CHKSUM, A.AIPSTACK_UDP_DGRAM_DST_LOCAL,
            A.AIPSTACK_UDP_DGRAM_DST_BCAST) == (0x80, 1, 2, 4) == (C.VALID, C.HAS_CHKSUM, C.DST_LOCAL, C.DST_BCAST)
    assert A.AIPSTACK_ICMP_NO_UNREACH == C.NO_UNREACH
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for line in ("#define AIPSTACK_UDP_NO_ASSOC        0xFFFFFFFFu", "#define AIPSTACK_UDP_ASSOC_NONLOCAL  0x80000000u ",
                 "#define AIPSTACK_UDP_MAX_LISTENERS   64u", "#define AIPSTACK_UDP_LIS_BROADCAST   1u ",
                 "#define AIPSTACK_UDP_LIS_NONLOCAL    2u ", "#define AIPSTACK_UDP_DGRAM_VALID        0x80u",
                 "#define AIPSTACK_UDP_DGRAM_HAS_CHKSUM   1u ", "#define AIPSTACK_UDP_DGRAM_DST_LOCAL    2u ",
                 "#define AIPSTACK_UDP_DGRAM_DST_BCAST    4u ", "#define AIPSTACK_CHKSUM_ABI_VERSION 1"):
        assert line in text, line
    assert A.udp_rx_demux_workspace_bytes(1 << 20) == 16 * (4096 + 1) + 32 * 4096
    assert A.udp_rx_demux_workspace_bytes(257) == 16 * 3 + 32 * 2


# ---- argument validation of the batch calls -----------------------------------------------------

_OUT = ("iface", "assocs", "n_assocs", "listeners", "n_listeners", "verdict", "dgrams", "unreach",
        "deliver_frame", "counts", "workspace", "workspace_bytes", "stream")
_CSR = ("base", "offsets", "n") + _OUT
_SLOT = ("base", "stride", "lens", "n") + _OUT


def _args(names, fields=None, **over):
    """A well-formed argument list for 4 frames (host buffers standing in for device ones: a
    rejected call must return before touching them)."""
    bufs = {k: ctypes.create_string_buffer(512 + 16) for k in
            ("base", "offsets", "lens", "assocs", "listeners", "verdict", "dgrams", "unreach",
             "deliver_frame", "counts", "workspace")}
    a = {k: (ctypes.addressof(v) + 15) & ~15 for k, v in bufs.items()}
    f = A.icmp_iface(R.LOCAL, R.BCAST, C.IC.LOCAL_MAC)
    for k, v in (fields or {}).items():
        f[k] = v
    bufs["iface"] = f
    a.update(n=4, stride=128, n_assocs=2, n_listeners=3, workspace_bytes=64, stream=None,
             iface=f.ctypes.data)
    for k, v in over.items():
        a[k] = a[k] + int(v[1:]) if isinstance(v, str) else v
    return bufs, [a[k] for k in names]


_BAD = [{k: None} for k in ("base", "iface", "assocs", "listeners", "verdict", "dgrams", "unreach",
                            "deliver_frame", "counts", "workspace")] + [
    {"n": (1 << 40) + 1, "workspace_bytes": 1 << 62}, {"n_assocs": (1 << 40) + 1}, {"n_listeners": 65},
    {"workspace_bytes": 63}, {"workspace": "+4"}, {"dgrams": "+4"}, {"deliver_frame": "+4"},
    {"counts": "+4"}, {"assocs": "+4"}, {"listeners": "+4"}]
_BAD_IFACE = [{"mtu": 255}, {"flags": 2}, {"flags": 3}, {"reserved": 1}]


@pytest.mark.parametrize("over", _BAD + [{"offsets": None}])
def test_csr_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_CSR, **over)
    assert lib.aipstack_udp_rx_demux(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("over", _BAD + [{"lens": None}, {"stride": 0}, {"stride": 65537}])
def test_slotted_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_SLOT, **over)
    assert lib.aipstack_udp_rx_demux_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("iface", _BAD_IFACE)
def test_iface_einval_before_any_hip_call(iface):
    lib = _lib.load()
    keep, args = _args(_CSR, fields=iface)
    assert lib.aipstack_udp_rx_demux(*args) == A.AIPSTACK_CHKSUM_EINVAL
    keep, args = _args(_SLOT, fields=iface)
    assert lib.aipstack_udp_rx_demux_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_no_frames_is_a_noop():
    lib = _lib.load()
    keep, args = _args(_CSR, n=0)
    assert lib.aipstack_udp_rx_demux(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_CSR, n=0, base=None, iface=None, workspace=None, n_listeners=99)
    assert lib.aipstack_udp_rx_demux(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_SLOT, n=0, stride=0)
    assert lib.aipstack_udp_rx_demux_slotted(*args) == A.AIPSTACK_CHKSUM_OK
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_wrappers_reject_host_tensors():
    torch = pytest.importorskip("torch")
    fr, off = torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    f = A.icmp_iface(R.LOCAL, R.BCAST, C.IC.LOCAL_MAC)
    with pytest.raises(ValueError):
        A.udp_rx_demux(fr, off, f)
    with pytest.raises(ValueError):
        A.udp_rx_demux_slotted(fr, 64, torch.zeros(1, dtype=torch.int32), f)


# ---- the frame sets of the GPU tests are not vacuous (from the model and the oracle alone) -----

def test_crafted_frames_contain_their_classes(oracle):
    ifc = C.iface()
    # the 64 listeners, bit by bit
    fr = C.bit_frames()
    e = C.expected(fr, _verdicts(oracle, fr), ifc, None, C.bit_listeners(LIS, dirty=True), DGRAM)
    assert [int(m) for m in e.dgrams["listeners"][:64]] == [1 << k for k in range(64)]
    assert int(e.counts[0]) == 64 and int(e.counts[1]) == 2 and not e.dgrams["listeners"][64:].any()
    # the associations
    tbl = C.many_assocs(KEY, 1000)
    fr = C.assoc_frames(1000, 7)
    e = C.expected(fr, _verdicts(oracle, fr), ifc, tbl, None, DGRAM)
    hit = e.dgrams["assoc"] != C.NO_ASSOC
    assert hit[0::2].all() and not hit[1::2].any() and len(set(e.dgrams["assoc"][0::2].tolist())) == len(fr) // 2
    assert (e.unreach[1::2] == C.PORT_UNREACH).any() and (e.unreach[1::2] == C.NO_UNREACH).any()
    assert np.all(np.diff(tbl["remote_port"].astype(np.int64)) >= 0)
    # floods
    fr = C.flood(513)
    e = C.expected(fr, _verdicts(oracle, fr), ifc, None, C.bit_listeners(LIS, 8), DGRAM)
    assert int(e.counts[0]) == 0 and int(e.counts[1]) == 513 and {6, 7} == set(np.unique(e.verdict))
    fr = C.flood(513, open_port=7003)
    e = C.expected(fr, _verdicts(oracle, fr), ifc, None, C.bit_listeners(LIS, 8), DGRAM)
    assert int(e.counts[0]) == 513 and int(e.counts[1]) == 0
    assert {int(f[14]) for f in fr} >= {0x45, 0x46, 0x4E}
    # mixed traffic and traffic without UDP
    fr = C.mixed(700)
    v = _verdicts(oracle, fr)
    e = C.expected(fr, v, ifc, None, C.listeners([(0, 5000, 0, 0, 1)], LIS), DGRAM)
    assert set(np.unique(v)) >= {0, 1, 2, 3, 4, 5, 6, 7, 8}
    assert int(e.counts[0]) >= 60 and int(e.counts[1]) >= 60
    fr = C.without_udp(600)
    v = _verdicts(oracle, fr)
    e = C.expected(fr, v, ifc, None, C.listeners([(0, 0, 1, 1, 1)], LIS), DGRAM)
    assert set(np.unique(v)) >= {0, 1, 2, 3, 4, 5, 6, 8} and 7 not in v
    assert not e.dgrams.tobytes().strip(b"\0") and (e.unreach == C.NO_UNREACH).all() and not e.counts.any()


# ---- the shared builder under ASan + UBSan, as a stand-alone program ---------------------------

def test_builder_under_asan_ubsan(replayed, oracle):
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "udprx.mk"], check=True, stdout=subprocess.DEVNULL)
    lines, cases = [], 0

    def add(frames, v, ifc, a, l, e):
        nonlocal cases
        lines.append("T %d %d %s %s" % (ifc["local"], ifc["bcast"],
                                         a.tobytes().hex() if a is not None and len(a) else "-",
                                         l.tobytes().hex() if l is not None and len(l) else "-"))
        delivered = set(e.deliver_frame[:int(e.counts[0])].tolist())
        for i, f in enumerate(frames):
            lines.append("F %d %s %s %d %d" % (int(v[i]), f.hex() or "-", e.dgrams[i].tobytes().hex(),
                                               int(e.unreach[i]), int(i in delivered)))
            cases += 1

    for s, frames, v, ifc, a, l, e in replayed:
        add(frames, v, ifc, a, l, e)
    ifc = C.iface()
    fr = C.bit_frames()
    v, l = _verdicts(oracle, fr), C.bit_listeners(LIS, dirty=True)
    add(fr, v, ifc, None, l, C.expected(fr, v, ifc, None, l, DGRAM))
    fr, a = C.assoc_frames(1000, 13), C.many_assocs(KEY, 1000)
    v = _verdicts(oracle, fr)
    add(fr, v, ifc, a, None, C.expected(fr, v, ifc, a, None, DGRAM))
    fr = C.mixed(300)
    v, l = _verdicts(oracle, fr), C.listeners([(0, 5000, 0, 0, 1)], LIS)
    add(fr, v, ifc, None, l, C.expected(fr, v, ifc, None, l, DGRAM))
    path = os.path.join(cpp, "build", "udprx_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "udprx_table_test"), path], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK %d cases" % cases in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-4000:])
