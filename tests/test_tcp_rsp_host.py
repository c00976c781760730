"""TCP segments without a connection, the parts that need no GPU: the model of tcp_rsp_cases.py
pinned against what the reference's own stack sent for every frame of
tests/golden/tcp_rsp_ref_cases.json (status, and the sent frame byte for byte), the fixture's
coverage, the struct and the constants, the argument validation of the two batch calls (rejected
before any HIP call), and the shared decision and RST builder under ASan/UBSan as a stand-alone
program (tests/cpp/tcp_rsp_build_test.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib
from conftest import ROOT

import tcp_rsp_cases as C
import tcp_rsp_ref as R

REFERENCE = "/root/reference"


@pytest.fixture(scope="module")
def replayed(oracle):
    """[(stack, interface, listeners, frames, verdicts, Expected)] of the fixture: a stack's cases
    as one batch with ip_id 0, then as (..., session frames, Expected) its session."""
    out = []
    for s in R.load():
        ifc, lis, frames = C.stack_iface(s), C.stack_listeners(s), C.stack_frames(s)
        v = C.verdicts_of(oracle, frames)
        sess = [bytes.fromhex(f) for f in s["session"]["in"]]
        sv = C.verdicts_of(oracle, sess)
        out.append((s, ifc, lis, frames, v, C.respond(frames, v, ifc, None, lis), sess, sv,
                    C.respond(sess, sv, ifc, None, lis)))
    return out


# ---- the model against the reference's recorded behaviour ---------------------------------------

def test_model_equals_the_reference(replayed):
    """Every case ran on a fresh stack: the model's RST with Ident 0 is the one frame the
    reference sent, byte for byte; where the reference sent a SYN-ACK the model says _SYN; where
    it sent nothing the model says anything else."""
    seen = 0
    for stack, ifc, lis, frames, v, e, _, _, _ in replayed:
        for i, case in enumerate(stack["cases"]):
            name = (case["name"], stack["prefix"])
            st = int(e.status[i])
            if case["out"] == ["SYNACK"]:
                assert st == C.SYN and int(e.listener[i]) != C.NO_LISTENER, name
                continue
            assert st != C.SYN, name
            one = C.respond([frames[i]], v[i:i + 1], ifc, None, lis)          # Ident 0
            assert C.sent(case["out"]) == ([one.headers[0]] if st == C.RST else []), name
            assert (int(one.status[0]), int(one.listener[0])) == (st, int(e.listener[i])), name
            seen += 1
    assert seen >= 250


def test_model_equals_the_reference_session(replayed):
    """One stack over 50 frames: RST j carries Ident j, in frame order."""
    for stack, ifc, lis, _, _, _, sess, sv, e in replayed:
        assert len(sess) >= 50 and int(e.counts[0]) >= 25 and int(e.counts[1]) == 0
        for i, out in enumerate(stack["session"]["out"]):
            assert C.sent(out) == ([e.headers[i]] if i in e.headers else []), (i, stack["prefix"])
        idents = [int.from_bytes(e.headers[i][18:20], "big") for i in sorted(e.headers)]
        assert idents == list(range(len(idents)))


def test_fixture_covers_the_cases(replayed):
    for stack, ifc, lis, frames, v, e, _, _, _ in replayed:
        by = {c["name"]: (frames[i], int(e.status[i]), int(e.listener[i]), e.headers.get(i))
              for i, c in enumerate(stack["cases"])}

        def st(name):
            return by[name][1]
        assert {x[1] for x in by.values()} == {C.NONE, C.NOT_LOCAL, C.DROP, C.SYN, C.RST}
        # the sixteen flag combinations at a closed, a listening and a wildcard port
        for flags in range(0x18):
            if flags & 0x08:
                continue
            assert st("flags_%02x_port_81" % flags) == (C.DROP if flags & 4 else C.RST)
            for port in (80, 8080):
                want = C.SYN if flags == 2 else C.RST if flags & 0x14 == 0x10 else C.DROP
                assert st("flags_%02x_port_%d" % (flags, port)) == want, (flags, port)
        assert st("flags_03_port_80") == C.DROP                       # SYN+FIN
        assert st("syn_psh_port_80") == st("syn_ece_cwr_port_80") == st("syn_urg_port_80") == C.SYN
        # two listeners on one port: the one opened later is found first
        cookies = {tuple(l): 100 + k for k, l in enumerate(stack["listeners"])}
        assert by["syn_port_443"][2] == cookies[(0, 443)]
        assert by["syn_port_444"][2] == cookies[(stack["addr"], 444)]
        assert by["flags_02_port_8080"][2] == cookies[(0, 8080)]
        assert by["flags_10_port_80"][2] == cookies[(stack["addr"], 80)]  # consulted, then RST
        assert by["flags_02_port_81"][2] == C.NO_LISTENER
        # data lengths with padding: the acknowledgement counts the data, not the frame
        for n in (0, 1, 1460):
            f, s, _, h = by["data_%d_psh_padded" % n]
            assert s == C.RST and len(f) > 54 + n
            assert int.from_bytes(h[42:46], "big") == 0x11223344 + n and h[47] == 0x14
            assert int.from_bytes(by["data_%d_syn_padded" % n][3][42:46], "big") == 0x11223344 + n + 1
        assert int.from_bytes(by["data_1_syn_fin_padded"][3][42:46], "big") == 0x11223344 + 2
        h = by["data_1_ack_padded"][3]
        assert h[38:42] == bytes.fromhex("55667788") and h[42:46] == bytes(4) and h[47] == 0x04
        assert [st("ihl_%d_syn" % k) for k in (6, 15)] == [C.RST] * 2
        assert [st("doff_%d_syn" % k) for k in (5, 6, 15)] == [C.RST] * 3
        assert [st("doff_%d_syn_listening" % k) for k in (5, 6, 15)] == [C.SYN] * 3
        assert st("doff_4") == st("doff_4_data") == st("doff_above_datagram") == st("doff_6_no_room") == C.NONE
        assert [st("mss_%d_listening" % k) for k in (215, 216, 536, 1460)] == [C.RST, C.SYN, C.SYN, C.SYN]
        assert [st("mss_%d_wildcard" % k) for k in (215, 216)] == [C.RST, C.SYN]
        assert st("mss_0_listening") == C.RST and st("mss_wrong_length_listening") == C.SYN
        assert st("mss_215_behind_end_listening") == C.SYN and st("mss_twice_listening") == C.RST
        assert st("mss_215_syn_ack_listening") == C.RST and st("wnd_scale_listening") == C.SYN
        assert by["seq_ffffffff_syn"][3][42:46] == bytes(4)
        assert by["seq_fffffff0_32_bytes"][3][42:46] == bytes.fromhex("00000010")
        assert by["seq_ffffffff_fin_1_byte"][3][42:46] == bytes.fromhex("00000001")
        for src in ("all_ones", "224_0_0_1", "239_255_255_255", "subnet_bcast"):
            assert [st("src_%s_%s" % (src, k)) for k in ("syn_closed", "syn_listening", "ack_listening")] == \
                [C.DROP] * 3, src
        for src in ("240_0_0_1", "zero", "outside", "223_255_255_255"):
            assert [st("src_%s_%s" % (src, k)) for k in ("syn_closed", "syn_listening", "ack_listening")] == \
                [C.RST, C.SYN, C.RST], src
        for dst in ("subnet_bcast", "all_ones", "other_host"):
            assert [st("dst_%s_%s" % (dst, k)) for k in ("syn_closed", "syn_listening", "syn_wildcard")] == \
                [C.NOT_LOCAL] * 3, dst
        assert st("bad_tcp_checksum") == st("udp_closed_port") == st("short_tcp") == C.NONE
        assert [by["rst_checksum_%04x" % k][3][50:52].hex() for k in (0, 1, 0xFFFE, 0x8000)] == \
            ["0000", "0001", "fffe", "8000"]
    assert {s["prefix"] for s, *_ in replayed} == {24, 30}


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "aipstack")),
                    reason="reference tree not present")
def test_generator_reproduces_the_fixture():
    with open(R.FIXTURE) as f:
        assert R.generate(REFERENCE) == f.read()


def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(R.FIXTURE) < 200 * 1024
    for s in R.load():
        assert set(s) == {"addr", "prefix", "gateway", "mac", "listeners", "cases", "session"}
        assert 100 <= len(s["cases"]) <= 400 and set(s["session"]) == {"in", "out"}
        outs = [c["out"] for c in s["cases"]] + s["session"]["out"]
        for c in s["cases"]:
            assert set(c) == {"name", "in", "out"}
            bytes.fromhex(c["in"])
        for out in outs:
            assert len(out) <= 1
            for e in out:
                assert e == "SYNACK" or (e[:2] == "T " and len(bytes.fromhex(e[2:])) == 54)


# ---- the struct and the constants ----------------------------------------------------------------

class _CListener(ctypes.Structure):
    _fields_ = [("addr", ctypes.c_uint32), ("port", ctypes.c_uint16), ("reserved0", ctypes.c_uint16),
                ("cookie", ctypes.c_uint32), ("reserved1", ctypes.c_uint32)]


def test_dtype_matches_the_c_struct():
    d = A.TCP_LISTENER_DTYPE
    assert d.itemsize == 16 == ctypes.sizeof(_CListener)
    assert list(d.names) == [n for n, _ in _CListener._fields_]
    for name, ct in _CListener._fields_:
        assert d.fields[name][1] == getattr(_CListener, name).offset, name
        assert d.fields[name][0].itemsize == ctypes.sizeof(ct), name
    t = A.tcp_listeners([(0x0A141E28, 80, 7), (0, 8080, 0xFFFFFFFE)])
    assert t.dtype == d and t.tobytes().hex() == "281e140a5000000007000000000000000000000" \
        "0901f0000feffffff00000000"
    assert A.TCP_RX_SEG_DTYPE == C.SEG and A.TCP_PCB_KEY_DTYPE == C.KEY


def test_constants_and_workspace():
    assert (A.AIPSTACK_TCP_RSP_NONE, A.AIPSTACK_TCP_RSP_NOT_LOCAL, A.AIPSTACK_TCP_RSP_PCB,
            A.AIPSTACK_TCP_RSP_DROP, A.AIPSTACK_TCP_RSP_SYN, A.AIPSTACK_TCP_RSP_RST) == \
        (31, 32, 33, 34, 35, 36) == (C.NONE, C.NOT_LOCAL, C.PCB, C.DROP, C.SYN, C.RST)
    assert A.AIPSTACK_TCP_RSP_HEADER == 54 == A.AIPSTACK_TCP_SEGMENT_HEADER == C.HEADER
    assert A.AIPSTACK_TCP_NO_LISTENER == 0xFFFFFFFF and A.AIPSTACK_TCP_MAX_LISTENERS == 256
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for line in ("#define AIPSTACK_TCP_RSP_HEADER 54u", "#define AIPSTACK_TCP_RSP_NONE       31 ",
                 "#define AIPSTACK_TCP_RSP_NOT_LOCAL  32 ", "#define AIPSTACK_TCP_RSP_PCB        33 ",
                 "#define AIPSTACK_TCP_RSP_DROP       34 ", "#define AIPSTACK_TCP_RSP_SYN        35 ",
                 "#define AIPSTACK_TCP_RSP_RST        36 ", "#define AIPSTACK_TCP_NO_LISTENER 0xFFFFFFFFu",
                 "#define AIPSTACK_TCP_MAX_LISTENERS 256u", "#define AIPSTACK_ARP_REPLY      30 ",
                 "#define AIPSTACK_CHKSUM_ABI_VERSION 1"):
        assert line in text, line
    assert text.index("AIPSTACK_TCP_RSP_HEADER") > text.index("aipstack_arp_rx_respond_slotted")
    assert A.tcp_rx_respond_workspace_bytes(1 << 20) == 16 * (4096 + 1) + 64 * 4096
    assert A.tcp_rx_respond_workspace_bytes(1) == 32 + 64
    for n in (1, 63, 64, 65, 255, 256, 257, 513, 65836):
        tiles = (n + 255) // 256
        assert A.tcp_rx_respond_workspace_bytes(n) == 16 * (tiles + 1) + 64 * tiles


# ---- argument validation of the batch calls -----------------------------------------------------

_OUT = ("iface", "ttl", "pcbs", "n_pcbs", "listeners", "n_listeners", "rst_request", "verdict", "segs",
        "pcb", "status", "listener", "hdr", "hdr_stride", "hdr_len", "chunk_index", "response_frame",
        "syn_frame", "counts", "workspace", "workspace_bytes", "stream")
_CSR = ("base", "offsets", "n") + _OUT
_SLOT = ("base", "stride", "lens", "n") + _OUT
_PTRS = ("base", "offsets", "lens", "pcbs", "listeners", "rst_request", "verdict", "segs", "pcb", "status",
         "listener", "hdr", "hdr_len", "chunk_index", "response_frame", "syn_frame", "counts", "workspace")


def _args(names, fields=None, **over):
    """A well-formed argument list for 4 frames (host buffers standing in for device ones: a
    rejected call must return before touching them)."""
    bufs = {k: ctypes.create_string_buffer(512 + 16) for k in _PTRS}
    a = {k: (ctypes.addressof(v) + 15) & ~15 for k, v in bufs.items()}
    f = A.icmp_iface(0x0A141E28, 0x0A141EFF, R.LOCAL_MAC)
    for k, v in (fields or {}).items():
        f[k] = v
    bufs["iface"] = f
    a.update(n=4, stride=128, hdr_stride=64, workspace_bytes=96, stream=None, iface=f.ctypes.data, ttl=64,
             n_pcbs=3, n_listeners=2)
    for k, v in over.items():
        a[k] = a[k] + int(v[1:]) if isinstance(v, str) else v
    return bufs, [a[k] for k in names]


_BAD = [{k: None} for k in ("base", "iface", "pcbs", "listeners", "verdict", "segs", "pcb", "status",
                            "listener", "hdr", "hdr_len", "chunk_index", "response_frame", "syn_frame",
                            "counts", "workspace")] + [
    {"hdr_stride": 53}, {"hdr_stride": 0}, {"n": (1 << 40) + 1, "workspace_bytes": 1 << 62},
    {"n_pcbs": (1 << 40) + 1}, {"n_listeners": 257}, {"ttl": 0}, {"ttl": 256},
    {"workspace_bytes": 95}, {"workspace": "+4"}, {"segs": "+4"}, {"pcbs": "+4"}, {"listeners": "+4"},
    {"chunk_index": "+4"}, {"response_frame": "+4"}, {"syn_frame": "+4"}, {"counts": "+4"},
    {"hdr_len": "+2"}, {"pcb": "+2"}, {"listener": "+2"}]
_BAD_IFACE = [{"mtu": 255}, {"flags": 2}, {"flags": 0x80}, {"reserved": 1}]


@pytest.mark.parametrize("over", _BAD + [{"offsets": None}])
def test_csr_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_CSR, **over)
    assert lib.aipstack_tcp_rx_respond(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("over", _BAD + [{"lens": None}, {"stride": 0}, {"stride": 65537}])
def test_slotted_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_SLOT, **over)
    assert lib.aipstack_tcp_rx_respond_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("iface", _BAD_IFACE)
def test_iface_einval_before_any_hip_call(iface):
    lib = _lib.load()
    keep, args = _args(_CSR, fields=iface)
    assert lib.aipstack_tcp_rx_respond(*args) == A.AIPSTACK_CHKSUM_EINVAL
    keep, args = _args(_SLOT, fields=iface)
    assert lib.aipstack_tcp_rx_respond_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_no_frames_is_a_noop():
    lib = _lib.load()
    keep, args = _args(_CSR, n=0)
    assert lib.aipstack_tcp_rx_respond(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_CSR, n=0, base=None, iface=None, workspace=None, hdr_stride=0, ttl=0)
    assert lib.aipstack_tcp_rx_respond(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_SLOT, n=0, stride=0)
    assert lib.aipstack_tcp_rx_respond_slotted(*args) == A.AIPSTACK_CHKSUM_OK


def test_wrappers_reject_host_tensors():
    torch = pytest.importorskip("torch")
    fr, off = torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    f = A.icmp_iface(0x0A141E28, 0x0A141EFF, R.LOCAL_MAC)
    with pytest.raises(ValueError):
        A.tcp_rx_respond(fr, off, f)
    with pytest.raises(ValueError):
        A.tcp_rx_respond_slotted(fr, 64, torch.zeros(1, dtype=torch.int32), f)


# ---- CHECKS OF THE TEST INFRASTRUCTURE, not of the feature: the frame sets of the GPU tests are
# ---- not vacuous. They run the Python model and the frame generators alone and pass without the
# ---- library's new entry points.

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_infrastructure_sized_batches_contain_their_classes(oracle, n):
    ifc = C.iface()

    def run(kind):
        frames = C.sized_batch(n, kind)
        return C.respond(frames, C.verdicts_of(oracle, frames), ifc, None, C.LISTENERS)
    e = run("all")
    assert e.counts.tolist() == [n, 0] and (e.status == C.RST).all()
    e = run("none")
    assert int(e.counts[0]) == 0 and C.RST not in set(np.unique(e.status))
    e = run("mixed")
    assert e.status[0] == e.status[n - 1] == C.RST
    if n == 513:
        assert set(np.unique(e.status)) == {C.NONE, C.NOT_LOCAL, C.DROP, C.SYN, C.RST}
        assert e.hdr_len[512] and not e.hdr_len[257:512].any() and int(e.counts[1]) > 0


def test_infrastructure_random_batches_contain_every_status(oracle):
    table = C.pcb_table(64)
    frames, req = C.random_batch(1, 1000, table)
    e = C.respond(frames, C.verdicts_of(oracle, frames), C.iface(), table, C.LISTENERS, req)
    assert set(np.unique(e.status)) == {C.NONE, C.NOT_LOCAL, C.PCB, C.DROP, C.SYN, C.RST}
    pcb = e.pcb != 0xFFFFFFFF
    assert (e.status[pcb & (req != 0)] == C.RST).all() and (e.status[pcb & (req == 0)] == C.PCB).all()


# ---- the shared builder under ASan + UBSan, as a stand-alone program ---------------------------

def test_builder_under_asan_ubsan(replayed, oracle):
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "tcp_rsp.mk"], check=True, stdout=subprocess.DEVNULL)
    lines = []

    def add(frames, v, ifc, lis, e, req=None):
        tail = "%d %s" % (len(lis), " ".join("%d %d %d" % l for l in lis))
        place = {int(i): j for j, i in enumerate(e.response_frame[:int(e.counts[0])])}
        for i, f in enumerate(frames):
            valid = bool(e.segs["opts"][i] & 0x80)
            lines.append("%d %d %d %d %d %s %d %d %d %d %d %d %s %s %s %s" % (
                ifc["local"], ifc["bcast"], ifc["mtu"], ifc["ip_id"], ifc["ttl"], ifc["mac"].hex(),
                int(v[i] == 6), int(e.pcb[i] != 0xFFFFFFFF), int(req is not None and req[i]),
                place.get(i, 0), int(e.status[i]), int(e.listener[i]),
                e.segs[i].tobytes().hex() if valid else "-", f.hex() or "-",
                e.headers[i].hex() if i in e.headers else "-", tail))

    for _, ifc, lis, frames, v, e, sess, sv, se in replayed:
        add(frames, v, ifc, lis, e)
        add(sess, sv, ifc, lis, se)
    table = C.pcb_table(64)
    for ifc in (C.iface(ip_id=0xFFFE, ttl=255), C.iface(prefix=30, local=0x0A141E29, ttl=1, mtu=256)):
        frames, req = C.random_batch(7, 600, table)
        frames += C.sized_batch(513, "mixed")
        req = np.concatenate([req, np.zeros(513, dtype=np.uint8)])
        v = C.verdicts_of(oracle, frames)
        add(frames, v, ifc, C.LISTENERS, C.respond(frames, v, ifc, table, C.LISTENERS, req), req)
    path = os.path.join(cpp, "build", "tcp_rsp_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "tcp_rsp_build_test"), path], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK %d cases" % len(lines) in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-4000:])
