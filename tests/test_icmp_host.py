"""The ICMP responder, the parts that need no GPU: the model of icmp_cases.py pinned byte for byte
(Ident included) against the packets recorded from the reference's own stack
(tests/golden/icmp_ref_cases.json), the fixture's coverage, the struct and the constants, the
argument validation of the two batch calls (rejected before any HIP call), and the shared decision
and slot builder under ASan/UBSan as a stand-alone program (tests/cpp/icmp_build_test.cpp)."""
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
import icmp_cases as C
import icmp_ref as R

REFERENCE = "/root/reference"


def _verdicts(oracle, frames):
    buf, off = F.pack(frames)
    return oracle.rx_verify_batch(buf, off)


@pytest.fixture(scope="module")
def replayed(oracle):
    """[(stack, [batch of icmp_cases.stack_batches])] of the fixture."""
    return [(s, C.stack_batches(s, _verdicts(oracle, C.stack_frames(s)))) for s in R.load()]


# ---- the model against the reference's recorded packets ----------------------------------------

def test_model_equals_the_reference(replayed):
    """Every case: the model's response is the one packet the reference sent, byte for byte, and
    nothing where it sent nothing. A TOO_LARGE case: the reference sent fragments, all under the
    one Ident that the model's next batch skips -- the host that takes the slow path consumes it."""
    seen = 0
    for stack, batches in replayed:
        assert len(batches) == (2 if stack["mtu"] < 1500 else 1)
        for start, frames, _, _, ifc, e in batches:
            for i in range(len(frames)):
                case = stack["cases"][start + i]
                out = [bytes.fromhex(o) for o in case["out"]]
                if e.status[i] == C.TOO_LARGE:
                    assert i == len(frames) - 1 and len(out) >= 2, case["name"]
                    used = (ifc["ip_id"] + int(e.counts[0])) & 0xFFFF
                    assert all(struct.unpack_from(">H", o, 4)[0] == used for o in out), case["name"]
                    assert struct.unpack_from(">H", out[0], 6)[0] & 0x2000
                elif e.status[i] == C.NONE:
                    assert out == [], case["name"]
                else:
                    assert out == [C.response_packet(e, frames, i)], case["name"]
                    assert e.headers[i][:6] == C.PEER_MAC and e.headers[i][6:14] == C.LOCAL_MAC + b"\x08\x00"
                seen += 1
    assert seen == sum(len(s["cases"]) for s, _ in replayed) >= 150


def test_fixture_covers_the_cases(replayed):
    by = {}
    for stack, batches in replayed:
        for start, frames, verdicts, _, ifc, e in batches:
            for i, f in enumerate(frames):
                name = stack["cases"][start + i]["name"]
                by[(name, stack["mtu"], stack["allow"])] = (f, int(verdicts[i]), int(e.status[i]), e, i)
    mtus = {m for _, m, _ in by}
    assert mtus == {576, 1500}

    def st(name, mtu=576, allow=0):
        return by[(name, mtu, allow)][2]

    for mtu in (576, 1500):
        for n in ("0", "1", "2", "17", "18", "19", "mtu-28"):
            assert st("echo_data_" + n, mtu) == C.ECHO_REPLY
        f = by[("echo_data_mtu-28", mtu, 0)][0]
        assert len(f) == 14 + mtu
    f, _, s, e, i = by[("echo_pad60", 576, 0)]
    assert len(f) == 60 and struct.unpack_from(">H", f, 16)[0] == 60 - 14 - 18 and s == C.ECHO_REPLY
    assert int(e.chunk_index[i + 1]) == int(e.chunk_index[i])                # padding is not data
    assert by[("echo_ihl6", 576, 0)][0][14] == 0x46 and by[("echo_ihl15", 576, 0)][0][14] == 0x4F
    assert st("echo_ihl6") == st("echo_ihl15") == C.ECHO_REPLY
    assert by[("echo_code", 576, 0)][0][35] == 5 and st("echo_code") == C.ECHO_REPLY
    assert by[("echo_rest_0", 576, 0)][0][38:42] == bytes(4)
    assert by[("echo_rest_ones", 576, 0)][0][38:42] == b"\xff" * 4
    # both members of the zero class: the request's field is what a sum of 0 mod 0xFFFF gives
    for name, want in (("echo_zero_class_all_zero", 0xFFFF), ("echo_zero_class_all_zero_odd", 0xFFFF),
                       ("echo_zero_class_nonzero", 0), ("echo_zero_class_nonzero_rest_0", 0),
                       ("echo_zero_class_nonzero_tail", 0)):
        f, _, s, e, i = by[(name, 576, 0)]
        assert struct.unpack_from(">H", f, 36)[0] == 0xF7FF and s == C.ECHO_REPLY, name
        assert struct.unpack_from(">H", e.headers[i], 36)[0] == want, name
    assert by[("echo_bad_chksum", 576, 0)][1] == 5 and st("echo_bad_chksum") == C.NONE
    for name in ("icmp_type0", "icmp_type3", "echo_src_all_ones", "echo_src_multicast", "echo_src_bcast",
                 "echo_dst_not_local"):
        assert by[(name, 576, 0)][1] == C.ACCEPT and st(name) == C.NONE, name
    assert by[("icmp_type0", 576, 0)][0][34] == 0 and by[("icmp_type3", 576, 0)][0][34] == 3
    assert by[("echo_src_multicast", 576, 0)][0][26:30] == bytes([224, 0, 0, 1])
    for name in ("echo_dst_bcast", "echo_dst_all_ones"):
        assert st(name + "_clear", 1500, 0) == C.NONE and st(name + "_set", 1500, 1) == C.ECHO_REPLY
    assert by[("echo_fragment", 576, 0)][1] == C.FRAGMENT and st("echo_fragment") == C.NONE
    f = by[("echo_too_large", 576, 0)][0]
    assert len(f) == 14 + 20 + 8 + 576 - 27 and st("echo_too_large") == C.TOO_LARGE
    assert st("echo_after_too_large") == C.ECHO_REPLY
    # the Ident passes 0xFFFF within the stack that was warmed up to it
    ids = [struct.unpack_from(">H", e.headers[i], 18)[0] for (n, m, a), (_, _, s, e, i) in by.items()
           if m == 1500 and a == 0 and s in (C.ECHO_REPLY, C.UNREACH)]
    assert 0xFFFF in ids and 0 in ids
    for ihl in (5, 7):
        for n in (0, 100):
            for k, v in (("chksum", C.ACCEPT), ("nochksum", C.ACCEPT_NO_CHKSUM)):
                f, vd, s, e, i = by[("udp_closed_ihl%d_data%d_%s" % (ihl, n, k), 576, 0)]
                assert (vd, s) == (v, C.UNREACH) and f[14] == 0x40 | ihl
                assert e.chunks[int(e.chunk_index[i])][1:] == (14, 4 * ihl + 8)
    assert st("udp_dst_not_local") == C.NONE and by[("udp_dst_not_local", 576, 0)][1] == C.ACCEPT
    assert st("udp_src_multicast") == C.UNREACH


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "aipstack")),
                    reason="reference tree not present")
def test_generator_reproduces_the_fixture():
    with open(R.FIXTURE) as f:
        assert R.generate(REFERENCE) == f.read()


def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(R.FIXTURE) < 256 * 1024
    for s in R.load():
        assert set(s) == {"allow", "mtu", "addr", "prefix", "gateway", "warm", "cases"}
        for c in s["cases"]:
            assert set(c) == {"name", "in", "out"}
            bytes.fromhex(c["in"])


# ---- the struct and the constants ---------------------------------------------------------------

class _CIface(ctypes.Structure):
    _fields_ = [("local_addr", ctypes.c_uint32), ("bcast_addr", ctypes.c_uint32),
                ("mtu", ctypes.c_uint16), ("ip_id", ctypes.c_uint16), ("ttl", ctypes.c_uint8),
                ("flags", ctypes.c_uint8), ("mac", ctypes.c_uint8 * 6), ("reserved", ctypes.c_uint8 * 12)]


def test_dtype_matches_the_c_struct():
    d = A.ICMP_IFACE_DTYPE
    assert d.itemsize == 32 == ctypes.sizeof(_CIface)
    assert list(d.names) == [n for n, _ in _CIface._fields_]
    for name, ct in _CIface._fields_:
        assert d.fields[name][1] == getattr(_CIface, name).offset, name
        assert d.fields[name][0].itemsize == ctypes.sizeof(ct), name
    f = A.icmp_iface(R.LOCAL, R.BCAST, C.LOCAL_MAC, mtu=576, ip_id=0x1FFFE, allow_broadcast_ping=True)
    assert (int(f["mtu"][0]), int(f["ip_id"][0]), int(f["ttl"][0]), int(f["flags"][0])) == (576, 0xFFFE, 64, 1)
    assert f["mac"][0].tobytes() == C.LOCAL_MAC and not f["reserved"].any()


def test_constants():
    assert (A.AIPSTACK_ICMP_NONE, A.AIPSTACK_ICMP_ECHO_REPLY, A.AIPSTACK_ICMP_UNREACH,
            A.AIPSTACK_ICMP_TOO_LARGE) == (23, 24, 25, 26) == (C.NONE, C.ECHO_REPLY, C.UNREACH, C.TOO_LARGE)
    assert A.AIPSTACK_ICMP_RESPONSE_HEADER == 42 and A.AIPSTACK_ICMP_NO_UNREACH == 0xFF
    assert A.AIPSTACK_ICMP_ALLOW_BROADCAST_PING == 1
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for line in ("#define AIPSTACK_ICMP_RESPONSE_HEADER 42u", "#define AIPSTACK_ICMP_NONE        23 ",
                 "#define AIPSTACK_ICMP_ECHO_REPLY  24", "#define AIPSTACK_ICMP_UNREACH     25",
                 "#define AIPSTACK_ICMP_TOO_LARGE   26 ", "#define AIPSTACK_ICMP_NO_UNREACH  0xFF ",
                 "#define AIPSTACK_ICMP_ALLOW_BROADCAST_PING 1u", "#define AIPSTACK_TX_LIN_WRONG_ROOM 22 ",
                 "#define AIPSTACK_CHKSUM_ABI_VERSION 1"):
        assert line in text, line
    assert A.icmp_rx_respond_workspace_bytes(1 << 20) == 16 * (4096 + 1)


# ---- argument validation of the batch calls -----------------------------------------------------

_OUT = ("verdict", "status", "hdr", "hdr_stride", "hdr_len", "chunk_addr", "chunk_len", "chunk_index",
        "response_frame", "counts", "workspace", "workspace_bytes", "stream")
_CSR = ("base", "offsets", "n", "iface", "unreach") + _OUT
_SLOT = ("base", "stride", "lens", "n", "iface", "unreach") + _OUT


def _args(names, fields=None, **over):
    """A well-formed argument list for 4 frames (host buffers standing in for device ones: a
    rejected call must return before touching them)."""
    bufs = {k: ctypes.create_string_buffer(512 + 16) for k in
            ("base", "offsets", "lens", "unreach", "verdict", "status", "hdr", "hdr_len", "chunk_addr",
             "chunk_len", "chunk_index", "response_frame", "counts", "workspace")}
    a = {k: (ctypes.addressof(v) + 15) & ~15 for k, v in bufs.items()}
    f = A.icmp_iface(R.LOCAL, R.BCAST, C.LOCAL_MAC)
    for k, v in (fields or {}).items():
        f[k] = v
    bufs["iface"] = f
    a.update(n=4, stride=128, hdr_stride=64, workspace_bytes=32, stream=None, iface=f.ctypes.data)
    for k, v in over.items():
        a[k] = a[k] + int(v[1:]) if isinstance(v, str) else v
    return bufs, [a[k] for k in names]


_BAD = [{k: None} for k in ("base", "iface", "verdict", "status", "hdr", "hdr_len", "chunk_addr",
                            "chunk_len", "chunk_index", "response_frame", "counts", "workspace")] + [
    {"hdr_stride": 41}, {"hdr_stride": 0}, {"n": (1 << 40) + 1, "workspace_bytes": 1 << 62},
    {"workspace_bytes": 31}, {"workspace": "+4"}, {"chunk_addr": "+4"}, {"chunk_index": "+4"},
    {"response_frame": "+4"}, {"counts": "+4"}, {"hdr_len": "+2"}, {"chunk_len": "+1"}]
_BAD_IFACE = [{"mtu": 255}, {"flags": 2}, {"flags": 3}, {"reserved": 1}]


@pytest.mark.parametrize("over", _BAD + [{"offsets": None}])
def test_csr_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_CSR, **over)
    assert lib.aipstack_icmp_rx_respond(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("over", _BAD + [{"lens": None}, {"stride": 0}, {"stride": 65537}])
def test_slotted_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_SLOT, **over)
    assert lib.aipstack_icmp_rx_respond_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("iface", _BAD_IFACE)
def test_iface_einval_before_any_hip_call(iface):
    lib = _lib.load()
    keep, args = _args(_CSR, fields=iface)
    assert lib.aipstack_icmp_rx_respond(*args) == A.AIPSTACK_CHKSUM_EINVAL
    keep, args = _args(_SLOT, fields=iface)
    assert lib.aipstack_icmp_rx_respond_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_no_frames_is_a_noop():
    lib = _lib.load()
    keep, args = _args(_CSR, n=0)
    assert lib.aipstack_icmp_rx_respond(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_CSR, n=0, base=None, iface=None, workspace=None, hdr_stride=0)
    assert lib.aipstack_icmp_rx_respond(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_SLOT, n=0, stride=0)
    assert lib.aipstack_icmp_rx_respond_slotted(*args) == A.AIPSTACK_CHKSUM_OK


def test_wrappers_reject_host_tensors():
    torch = pytest.importorskip("torch")
    fr, off = torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    f = A.icmp_iface(R.LOCAL, R.BCAST, C.LOCAL_MAC)
    with pytest.raises(ValueError):
        A.icmp_rx_respond(fr, off, f)
    with pytest.raises(ValueError):
        A.icmp_rx_respond_slotted(fr, 64, torch.zeros(1, dtype=torch.int32), f)


# ---- the frame sets of the GPU tests are not vacuous (from the model and the oracle alone) -----

def test_crafted_frames_contain_their_classes(oracle):
    frames = C.crafted_frames()
    v = _verdicts(oracle, frames)
    e = C.respond(frames, v, C.crafted_codes(frames), C.iface())
    n_echo, n_unr = int((e.status == C.ECHO_REPLY).sum()), int((e.status == C.UNREACH).sum())
    assert n_echo >= 44 + 20 and n_unr >= 44 + 1 and (e.status == C.NONE).sum() >= 2
    ck = {struct.unpack_from(">H", h, 36)[0] for h in e.headers.values()}
    assert {0, 0xFFFF} <= ck
    assert int(e.counts[1]) < int(e.counts[0])                         # replies without a chunk
    fr = C.mixed_batch(700, {0, 63, 64, 255, 256, 699})
    v = _verdicts(oracle, fr)
    assert set(np.unique(v)) >= {0, 1, 2, 3, 4, 5, 6, 7, 8}
    e = C.respond(fr, v, C.host_codes(fr), C.iface())
    assert all(e.status[i] == C.ECHO_REPLY for i in (0, 63, 64, 255, 256, 699))


# ---- the shared builder under ASan + UBSan, as a stand-alone program ---------------------------

def test_builder_under_asan_ubsan(replayed, oracle):
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "icmp.mk"], check=True, stdout=subprocess.DEVNULL)
    lines = []

    def add(frames, verdicts, codes, ifc, e):
        j = 0
        by_frame = {fi: (off, ln) for fi, off, ln in e.chunks}
        for i, f in enumerate(frames):
            st = int(e.status[i])
            code = C.NO_UNREACH if codes is None else codes[i]
            off, ln = C.plan(f, int(verdicts[i]), code, ifc)[1:] if st != C.NONE else (0, 0)
            if i in e.headers:
                assert by_frame.get(i, (off, 0)) == (off, ln)
            lines.append("%d %d %d %d %d %s %d %d %d %d %d %d %s %s" % (
                ifc["local"], ifc["bcast"], ifc["mtu"], ifc["ttl"], int(ifc["allow"]), ifc["mac"].hex(),
                int(verdicts[i]), code, ifc["ip_id"] + j, st, off, ln, f.hex(),
                e.headers[i].hex() if i in e.headers else "-"))
            j += i in e.headers

    for _, batches in replayed:
        for _, frames, verdicts, codes, ifc, e in batches:
            add(frames, verdicts, codes, ifc, e)
    frames = C.crafted_frames()
    v = _verdicts(oracle, frames)
    ifc = C.iface(ip_id=0xFFF0, ttl=17, mtu=1400)
    add(frames, v, C.crafted_codes(frames), ifc, C.respond(frames, v, C.crafted_codes(frames), ifc))
    path = os.path.join(cpp, "build", "icmp_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "icmp_build_test"), path], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK %d cases" % len(lines) in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-4000:])
