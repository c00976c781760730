"""Received ICMP Destination Unreachable, the parts that need no GPU: the model of
icmp_du_cases.py pinned against the handler calls the reference's own stack made for every frame
of tests/golden/icmp_du_ref_cases.json, the fixture's coverage, the struct and the constants, the
argument validation of the two batch calls (rejected before any HIP call), and the shared decision
and record builder under ASan/UBSan as a stand-alone program (tests/cpp/icmp_du_build_test.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib
from conftest import ROOT

import icmp_du_cases as C
import icmp_du_ref as R

REFERENCE = "/root/reference"


@pytest.fixture(scope="module")
def replayed(oracle):
    """[(stack, interface, frames, verdicts, Expected)] of the fixture, a stack's cases as one
    batch without a PCB table."""
    out = []
    for s in R.load():
        ifc, frames = C.stack_iface(s), C.stack_frames(s)
        v = C.verdicts_of(oracle, frames)
        out.append((s, ifc, frames, v, C.expected(frames, v, ifc)))
    return out


# ---- the model against the reference's recorded behaviour ---------------------------------------

def test_model_equals_the_reference(replayed):
    """The reference called a handler iff the model's record is valid and its protocol is 6 or
    17; every recorded argument is the record's field, and dgram_initial is the frame's bytes
    [ip_off + hl, ip_off + hl + l4_len). No case is left out."""
    seen = total = 0
    for stack, ifc, frames, v, e in replayed:
        total += len(stack["cases"])
        for i, case in enumerate(stack["cases"]):
            name = (case["name"], stack["prefix"])
            calls = C.handler_calls(case["out"])
            r, f = e.records[i], frames[i]
            valid = int(r["hl"]) != 0
            assert valid == (int(e.status[i]) != C.NONE), name
            assert len(calls) == (1 if valid and int(r["proto"]) in (6, 17) else 0), name
            if not valid:
                assert r.tobytes() == bytes(32), name
            for handler, code, rest, src, dst, ttl, proto, hl, dgram in calls:
                assert handler == proto == int(r["proto"]), name
                assert (code, rest, src, dst, ttl, hl) == (int(r["code"]), int(r["rest"]), int(r["local_addr"]),
                                                           int(r["remote_addr"]), int(r["ttl"]), int(r["hl"])), name
                at = int(r["ip_off"]) + hl
                assert dgram == f[at:at + int(r["l4_len"])] and len(dgram) == int(r["l4_len"]), name
                if len(dgram) >= 8:
                    assert (int(r["local_port"]), int(r["remote_port"]), int(r["seq"])) == \
                        (C.be16(dgram, 0), C.be16(dgram, 2), C.be32(dgram, 4)), name
                else:
                    assert (int(r["local_port"]), int(r["remote_port"]), int(r["seq"])) == (0, 0, 0), name
            # a message is never also handed over as a datagram of the quoted protocol
            assert not (calls and any(ev.startswith("R ") for ev in case["out"])), name
            seen += 1
    assert seen == total == sum(len(R.cases(*s)) for s in R.STACKS) and seen >= 180


def test_fixture_covers_the_cases(replayed):
    for stack, ifc, frames, v, e in replayed:
        by = {c["name"]: (frames[i], int(e.status[i]), e.records[i], C.handler_calls(c["out"]))
              for i, c in enumerate(stack["cases"])}
        assert len(by) == len(stack["cases"])

        def st(name):
            return by[name][1]

        def rec(name, field):
            return int(by[name][2][field])
        assert {x[1] for x in by.values()} == {C.NONE, C.PARSED, C.TCP_NO_PCB}
        for code in R.CODES:
            assert st("tcp_code_%d" % code) == (C.TCP_NO_PCB if code == 4 else C.PARSED)
            assert st("udp_code_%d" % code) == C.PARSED and rec("udp_code_%d" % code, "code") == code
        assert [rec("tcp_rest_%08x" % r, "rest") for r in R.RESTS] == list(R.RESTS)
        assert [rec("tcp_rest_%08x" % r, "rest") & 0xFFFF for r in R.RESTS] == [0, 1500, 0x0100, 0]
        for ihl in (5, 6, 15):
            assert rec("outer_ihl_%d" % ihl, "ip_off") == 14 + 4 * ihl + 8 and rec("outer_ihl_%d" % ihl, "hl") == 20
            assert rec("quoted_ihl_%d" % ihl, "hl") == 4 * ihl and rec("quoted_ihl_%d" % ihl, "ip_off") == 42
            assert rec("both_ihl_%d" % ihl, "l4_len") == 20 and st("both_ihl_%d" % ihl) == C.TCP_NO_PCB
        assert len(by["both_ihl_15"][0]) == 14 + 60 + 8 + 60 + 20
        for name in ("quoted_ihl_4", "quoted_ihl_0", "quoted_version_6", "quoted_version_5",
                     "quoted_ihl_6_only_20_bytes", "quoted_ihl_6_only_23_bytes", "quoted_ihl_15_only_59_bytes",
                     "quoted_total_below_header", "quoted_total_below_header_ihl_6", "icmp_data_19", "icmp_data_0"):
            assert st(name) == C.NONE and v[list(by).index(name)] == 6, name
        assert st("quoted_total_equals_header") == st("quoted_total_equals_header_ihl_6") == C.PARSED
        assert [rec("quoted_total_cuts_l4_to_%s" % k, "l4_len") for k in ("12", "8", "7", "5_udp")] == [12, 8, 7, 5]
        assert [st("quoted_total_cuts_l4_to_%s" % k) for k in ("12", "8", "7")] == \
            [C.TCP_NO_PCB, C.TCP_NO_PCB, C.PARSED]
        for n in (0, 3, 4, 7, 8, 9, 28):
            assert rec("tcp_l4_%d" % n, "l4_len") == rec("udp_l4_%d" % n, "l4_len") == n
            assert st("tcp_l4_%d" % n) == (C.TCP_NO_PCB if n >= 8 else C.PARSED) and st("udp_l4_%d" % n) == C.PARSED
            assert (rec("udp_l4_%d" % n, "local_port"), rec("udp_l4_%d" % n, "seq") != 0) == \
                ((5000, True) if n >= 8 else (0, False))
        assert st("icmp_data_20") == C.PARSED and rec("icmp_data_20", "l4_len") == 0
        # a protocol without a handler: a valid record, nobody called
        for proto in (1, 47):
            assert st("quoted_proto_%d" % proto) == C.PARSED and not by["quoted_proto_%d" % proto][3]
            assert rec("quoted_proto_%d" % proto, "proto") == proto and rec("quoted_proto_%d" % proto, "seq")
        assert st("quoted_src_not_ours") == C.TCP_NO_PCB and rec("quoted_src_not_ours", "local_addr") == 0xC0A80909
        assert st("quoted_fragment_offset") == st("quoted_more_fragments") == C.TCP_NO_PCB
        assert [st("src_%s" % k) for k in ("all_ones", "224_0_0_1", "subnet_bcast")] == [C.NONE] * 3
        assert [st("src_%s" % k) for k in ("240_0_0_1", "zero", "outside")] == [C.TCP_NO_PCB] * 3
        assert [st("dst_%s" % k) for k in ("subnet_bcast", "all_ones", "other_host")] == \
            [C.TCP_NO_PCB, C.TCP_NO_PCB, C.NONE]
        for name in ("bad_icmp_checksum", "type_3_in_a_fragment", "type_3_in_a_later_fragment",
                     "type_11_good_quote", "type_8", "type_0", "cut_to_74_bytes_stale_icmp_checksum",
                     "cut_without_the_total_length", "tcp_segment", "udp_datagram"):
            assert st(name) == C.NONE, name
        # (a message with a whole quoted header has 62 bytes: padding to 60 meets shorter ones only)
        assert len(by["padded_to_60"][0]) == len(by["padded_to_60_no_data"][0]) == 60
        assert st("padded_to_60") == st("padded_to_60_no_data") == st("icmp_data_19_padded_by_5") == C.NONE
        assert rec("tcp_l4_4_padded_by_5", "l4_len") == 4 and rec("padded_by_5", "l4_len") == 8
        assert rec("padded_by_5_tcp_7", "l4_len") == 7 and st("padded_by_5_tcp_7") == C.PARSED
        assert st("cut_to_64_bytes") == C.NONE
        assert (st("cut_to_71_bytes"), rec("cut_to_71_bytes", "l4_len")) == (C.PARSED, 5)
        assert (st("cut_to_74_bytes"), rec("cut_to_74_bytes", "l4_len")) == (C.TCP_NO_PCB, 8)
    assert {s["prefix"] for s, *_ in replayed} == {24, 30}


def test_model_finds_the_pcb(replayed):
    """Step 3, on the fixture's own frames: with the quoted connection in the table the frames
    whose handler goes on to find_pcb, and only those, get its cookie."""
    for stack, ifc, frames, v, e in replayed:
        t = np.array([(stack["addr"], R.FAR, 5000, 80, 77), (0xC0A80909, R.FAR, 5000, 80, 78)], dtype=C.KEY)
        w = C.expected(frames, v, ifc, t)
        looked = e.status == C.TCP_NO_PCB
        assert looked.sum() >= 25 and (w.status[looked] == C.TCP_PCB).all()
        assert np.array_equal(w.status[~looked], e.status[~looked])
        assert set(w.records["pcb"][looked].tolist()) == {77, 78}
        assert (w.records["pcb"][~looked] == np.where(e.status[~looked] == C.NONE, 0, C.NO_PCB)).all()
        assert w.counts.tolist() == [int(looked.sum()), int(e.counts[1])]
        assert np.array_equal(w.pcb_frame[:int(w.counts[0])], np.flatnonzero(looked).astype(np.uint64))
        assert (w.pcb_frame[int(w.counts[0]):] == C.NO_FRAME).all()


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "aipstack")),
                    reason="reference tree not present")
def test_generator_reproduces_the_fixture():
    with open(R.FIXTURE) as f:
        assert R.generate(REFERENCE) == f.read()


def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(R.FIXTURE) < 100 * 1024
    for s in R.load():
        assert set(s) == {"addr", "prefix", "gateway", "mac", "cases"}
        assert 90 <= len(s["cases"]) <= 200
        for c in s["cases"]:
            assert set(c) == {"name", "in", "out"} and len(c["out"]) <= 1
            assert len(bytes.fromhex(c["in"])) <= 14 + 60 + 8 + 60 + 28
            for e in c["out"]:
                p = e.split(" ")
                assert (p[0] == "D" and len(p) == 10) or (p[0] == "R" and len(p) == 2)
                assert all(x == "-" or int(x, 16) >= 0 for x in p[1:])


# ---- the struct and the constants ----------------------------------------------------------------

class _CRecord(ctypes.Structure):
    _fields_ = [("local_addr", ctypes.c_uint32), ("remote_addr", ctypes.c_uint32),
                ("local_port", ctypes.c_uint16), ("remote_port", ctypes.c_uint16), ("seq", ctypes.c_uint32),
                ("rest", ctypes.c_uint32), ("pcb", ctypes.c_uint32), ("ip_off", ctypes.c_uint16),
                ("l4_len", ctypes.c_uint16), ("code", ctypes.c_uint8), ("proto", ctypes.c_uint8),
                ("ttl", ctypes.c_uint8), ("hl", ctypes.c_uint8)]


def test_dtype_matches_the_c_struct():
    d = A.ICMP_DU_RECORD_DTYPE
    assert d.itemsize == 32 == ctypes.sizeof(_CRecord)
    assert list(d.names) == [n for n, _ in _CRecord._fields_]
    for name, ct in _CRecord._fields_:
        assert d.fields[name][1] == getattr(_CRecord, name).offset, name
        assert d.fields[name][0].itemsize == ctypes.sizeof(ct), name
    assert d == C.RECORD and A.TCP_PCB_KEY_DTYPE == C.KEY


def test_constants_and_workspace():
    assert (A.AIPSTACK_ICMP_DU_NONE, A.AIPSTACK_ICMP_DU_PARSED, A.AIPSTACK_ICMP_DU_TCP_NO_PCB,
            A.AIPSTACK_ICMP_DU_TCP_PCB) == (37, 38, 39, 40) == (C.NONE, C.PARSED, C.TCP_NO_PCB, C.TCP_PCB)
    assert A.AIPSTACK_TCP_NO_PCB == C.NO_PCB
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for line in ("#define AIPSTACK_ICMP_DU_NONE        37 ", "#define AIPSTACK_ICMP_DU_PARSED      38 ",
                 "#define AIPSTACK_ICMP_DU_TCP_NO_PCB  39 ", "#define AIPSTACK_ICMP_DU_TCP_PCB     40 ",
                 "#define AIPSTACK_TCP_RSP_RST        36 ", "#define AIPSTACK_CHKSUM_ABI_VERSION 1"):
        assert line in text, line
    assert text.index("AIPSTACK_ICMP_DU_NONE") > text.index("aipstack_tcp_rx_respond_slotted")
    assert A.icmp_rx_unreach_workspace_bytes(1 << 20) == 16 * (4096 + 1) + 32 * 4096
    for n in (1, 63, 64, 65, 255, 256, 257, 513, 65836):
        tiles = (n + 255) // 256
        assert A.icmp_rx_unreach_workspace_bytes(n) == 16 * (tiles + 1) + 32 * tiles


# ---- argument validation of the batch calls -----------------------------------------------------

_OUT = ("iface", "pcbs", "n_pcbs", "verdict", "status", "records", "pcb_frame", "counts", "workspace",
        "workspace_bytes", "stream")
_CSR = ("base", "offsets", "n") + _OUT
_SLOT = ("base", "stride", "lens", "n") + _OUT
_PTRS = ("base", "offsets", "lens", "pcbs", "verdict", "status", "records", "pcb_frame", "counts", "workspace")


def _args(names, fields=None, **over):
    """A well-formed argument list for 4 frames (host buffers standing in for device ones: a
    rejected call must return before touching them)."""
    bufs = {k: ctypes.create_string_buffer(512 + 16) for k in _PTRS}
    a = {k: (ctypes.addressof(v) + 15) & ~15 for k, v in bufs.items()}
    f = A.icmp_iface(0x0A141E28, 0x0A141EFF, R.LOCAL_MAC)
    for k, v in (fields or {}).items():
        f[k] = v
    bufs["iface"] = f
    a.update(n=4, stride=128, workspace_bytes=64, stream=None, iface=f.ctypes.data, n_pcbs=3)
    for k, v in over.items():
        a[k] = a[k] + int(v[1:]) if isinstance(v, str) else v
    return bufs, [a[k] for k in names]


_BAD = [{k: None} for k in ("base", "iface", "pcbs", "verdict", "status", "records", "pcb_frame", "counts",
                            "workspace")] + [
    {"n": (1 << 40) + 1, "workspace_bytes": 1 << 62}, {"n_pcbs": (1 << 40) + 1}, {"workspace_bytes": 63},
    {"workspace": "+4"}, {"records": "+4"}, {"pcbs": "+4"}, {"pcb_frame": "+4"}, {"counts": "+4"}]
_BAD_IFACE = [{"mtu": 255}, {"flags": 2}, {"flags": 0x80}, {"reserved": 1}]


@pytest.mark.parametrize("over", _BAD + [{"offsets": None}])
def test_csr_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_CSR, **over)
    assert lib.aipstack_icmp_rx_unreach(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("over", _BAD + [{"lens": None}, {"stride": 0}, {"stride": 65537}])
def test_slotted_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_SLOT, **over)
    assert lib.aipstack_icmp_rx_unreach_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("iface", _BAD_IFACE)
def test_iface_einval_before_any_hip_call(iface):
    lib = _lib.load()
    keep, args = _args(_CSR, fields=iface)
    assert lib.aipstack_icmp_rx_unreach(*args) == A.AIPSTACK_CHKSUM_EINVAL
    keep, args = _args(_SLOT, fields=iface)
    assert lib.aipstack_icmp_rx_unreach_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_no_frames_is_a_noop():
    lib = _lib.load()
    keep, args = _args(_CSR, n=0)
    assert lib.aipstack_icmp_rx_unreach(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_CSR, n=0, base=None, iface=None, workspace=None, workspace_bytes=0)
    assert lib.aipstack_icmp_rx_unreach(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_SLOT, n=0, stride=0)
    assert lib.aipstack_icmp_rx_unreach_slotted(*args) == A.AIPSTACK_CHKSUM_OK


def test_wrappers_reject_host_tensors():
    torch = pytest.importorskip("torch")
    fr, off = torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    f = A.icmp_iface(0x0A141E28, 0x0A141EFF, R.LOCAL_MAC)
    with pytest.raises(ValueError):
        A.icmp_rx_unreach(fr, off, f)
    with pytest.raises(ValueError):
        A.icmp_rx_unreach_slotted(fr, 64, torch.zeros(1, dtype=torch.int32), f)


# ---- CHECKS OF THE TEST INFRASTRUCTURE, not of the feature: the frame sets of the GPU tests are
# ---- not vacuous. They run the Python model and the frame generators alone and pass without the
# ---- library's new entry points.

@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_infrastructure_sized_batches_hit_where_they_say(oracle, n):
    table = C.pcb_table(64)
    hits = sorted({i for i in (0, 255, 256, n - 1) if i < n})
    frames = C.sized_batch(n, table, hits)
    e = C.expected(frames, C.verdicts_of(oracle, frames), C.iface(), table)
    assert e.pcb_frame[:len(hits)].tolist() == hits and int(e.counts[0]) == len(hits)
    if n > 2:
        assert {C.NONE, C.PARSED, C.TCP_NO_PCB, C.TCP_PCB} == set(np.unique(e.status))


def test_infrastructure_random_batch_contains_every_status(oracle):
    table = C.pcb_table(64)
    frames = C.random_batch(20261021, 2048, table)
    v = C.verdicts_of(oracle, frames)
    e = C.expected(frames, v, C.iface(), table)
    assert set(np.unique(e.status)) == {C.NONE, C.PARSED, C.TCP_NO_PCB, C.TCP_PCB}
    assert 300 < sum(1 for f in frames if len(f) > 34 and f[12:14] == b"\x08\x00" and f[23] == 1 and
                     f[14 + (f[14] & 0xF) * 4] == 3) < 700
    assert int(e.counts[0]) >= 10 and int(e.counts[1]) >= 100 and set(np.unique(v)) >= {0, 5, 6}
    for name in ("l4_len", "hl", "code", "proto"):
        assert len(set(e.records[name].tolist())) >= 4, name


def test_infrastructure_table_has_the_neighbours():
    """Entries that differ only in remote_port, only in local_port and only in remote_addr, and
    near misses that differ from an entry in one field alone."""
    t = C.pcb_table(4096)
    keys = [C.key_of(t, i) for i in range(len(t))]
    assert len(set(keys)) == 4096
    for i in (0, 1, 2, 3, 4095):
        for bit, field in ((1, 3), (2, 2), (4, 1)):
            assert [a != b for a, b in zip(keys[i], keys[i ^ bit])] == [k == field for k in range(4)]
        for k in range(4):
            miss = C.near_miss(t, i, k)
            assert miss not in keys and sum(a != b for a, b in zip(miss, keys[i])) == 1
    s = A.tcp_pcb_table_sort(t)
    assert {int(s["cookie"][0]), int(s["cookie"][-1])} <= set(range(1000, 1000 + 4096))


# ---- the shared builder under ASan + UBSan, as a stand-alone program ---------------------------

def test_builder_under_asan_ubsan(replayed, oracle):
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "icmp_du.mk"], check=True, stdout=subprocess.DEVNULL)
    lines = []

    def add(frames, v, ifc, table, e):
        s = A.tcp_pcb_table_sort(table)
        lines.append("T %d" % len(s))
        lines.extend("%d %d %d %d %d" % tuple(int(x) for x in k) for k in s)
        for i, f in enumerate(frames):
            lines.append("%d %d %d %d %s %s" % (
                ifc["local"], ifc["bcast"], int(v[i] == 6), int(e.status[i]),
                e.records[i].tobytes().hex() if e.status[i] != C.NONE else "-", f.hex() or "-"))
        return len(frames)

    count = 0
    for stack, ifc, frames, v, _ in replayed:
        for t in (np.zeros(0, dtype=C.KEY),
                  np.array([(stack["addr"], R.FAR, 5000, 80, 77), (0xC0A80909, R.FAR, 5000, 80, 78)], dtype=C.KEY)):
            count += add(frames, v, ifc, t, C.expected(frames, v, ifc, t))
    table = C.pcb_table(64)
    frames = C.random_batch(7, 600, table) + C.sized_batch(257, table, (0, 255, 256))
    v = C.verdicts_of(oracle, frames)
    count += add(frames, v, C.iface(), table, C.expected(frames, v, C.iface(), table))
    path = os.path.join(cpp, "build", "icmp_du_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "icmp_du_build_test"), path], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK %d cases" % count in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-4000:])
