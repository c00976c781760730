"""aipstack_tcp_tx_control on the CPU: the Python model (tcp_ctl_cases.py) against the frames
recorded from the reference stack (tests/golden/tcp_ctl_ref_cases.json), the fixture's coverage,
the descriptor dtype and the constants, the argument checks of the entry point, and the shared
builder (tcpctl_common.h) under ASan + UBSan in a stand-alone program."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib
from conftest import ROOT

import tcp_ctl_cases as C
import tcp_ctl_ref as R

REFERENCE = "/root/reference"
FIN, SYN, RST, PSH, ACK = R.FIN, R.SYN, R.RST, R.PSH, R.ACK


@pytest.fixture(scope="module")
def sessions():
    return [(s, R.frames(s)) for s in R.load()]


# ---- the model against the reference's recorded frames ------------------------------------------

def test_model_equals_the_reference(sessions):
    """Every recorded frame, rebuilt from the descriptor read out of it, byte for byte; bytes
    0..5 after copying the recorded destination MAC (the resolve step supplies it)."""
    seen = 0
    for s, fr in sessions:
        for step, f in fr:
            c, ifc, ttl, ident = C.from_frame(f)
            assert C.valid(c) and ifc["mac"] == bytes.fromhex(s["mac"]) and ttl == 64
            assert f[:6] == bytes.fromhex(s["peer_mac"])
            h = C.build(c, dict(mac=ifc["mac"], ip_id=0), ttl, ident)
            assert h[:6] == bytes(6) and f[:6] + h[6:] == f, (s["name"], step)
            seen += 1
    assert 150 <= seen <= 400


def test_model_equals_the_reference_session(sessions):
    """A session as one batch with its first Ident: frame j carries Ident first + j."""
    for s, fr in sessions:
        cs = [C.from_frame(f)[0] for _, f in fr]
        first = C.from_frame(fr[0][1])[3]
        e = C.Expected(cs, dict(mac=bytes.fromhex(s["mac"]), ip_id=first), 64)
        assert e.counts.tolist() == [len(fr), 0]
        for i, (_, f) in enumerate(fr):
            assert e.headers[i][6:] == f[6:], (s["name"], i)
    assert max(len(fr) for _, fr in sessions) >= 40


def test_fixture_covers_the_scenarios(sessions):
    kinds = set()
    for s, fr in sessions:
        by_step = {st["step"]: [bytes.fromhex(h) for h in st["out"]] for st in s["steps"]}
        for step, f in fr:
            c = C.from_frame(f)[0]
            kinds.add((c["flags"], c["options"]))
        if s["name"].startswith("passive"):
            def synack(what, pname):
                (f,) = by_step["SYN with %s to the %s-buffer listener" % (what, pname)]
                return C.from_frame(f)[0]
            for pname, wnd in (("small", 4096), ("large", 65535)):
                for what in ("no option", "MSS 216", "MSS 536", "MSS 1460"):
                    c = synack(what, pname)
                    assert (c["flags"], c["options"], c["window"]) == (SYN | ACK, C.OPT_MSS, wnd)
                for what in ("MSS 1460 + window scale 7", "window scale alone"):
                    c = synack(what, pname)
                    assert (c["flags"], c["options"], c["wnd_scale"]) == (SYN | ACK, 3, 6)
            again = by_step["1 s later: every SYN-ACK is retransmitted"]
            first = [f for st in s["steps"][:12] for f in (bytes.fromhex(h) for h in st["out"])]
            assert len(again) == len(first) == 12
            assert sorted(f[34:54] for f in again) == sorted(f[34:54] for f in first)
            assert not {f[18:20] for f in again} & {f[18:20] for f in first}
            upd = [by_step[k] for k in by_step if "window update" in k]
            assert len(upd) == 4 and all(len(u) == 1 and C.from_frame(u[0])[0]["flags"] == ACK for u in upd)
            assert sum("beyond the window" in k and len(v) == 1 for k, v in by_step.items()) == 8
            assert sum("in order" in k and len(v) == 1 for k, v in by_step.items()) == 8
        else:
            syn = [by_step[k][0] for k in by_step if k.startswith("startConnection")]
            again = by_step["1 s later: every SYN is retransmitted"]
            assert len(syn) == len(again) == 3
            for f in syn + again:
                c = C.from_frame(f)[0]
                assert (c["flags"], c["options"], c["wnd_scale"], c["ack"]) == (SYN, 3, 6, 0)
            assert sorted(f[34:62] for f in syn) == sorted(f[34:62] for f in again)
            assert not {f[18:20] for f in syn} & {f[18:20] for f in again}
            (f,) = [v[0] for k, v in by_step.items() if "RST without ACK" in k]
            assert C.from_frame(f)[0]["flags"] == RST
    assert {(SYN | ACK, 1), (SYN | ACK, 3), (SYN, 3), (ACK, 0), (RST | ACK, 0), (RST, 0),
            (FIN | PSH | ACK, 0)} <= kinds
    assert {s["prefix"] for s, _ in sessions} == {24, 30}
    # the second stack's sequence numbers (the ISS is the clock) cross 2^32
    seqs = [C.from_frame(f)[0]["seq"] for s, fr in sessions if s["prefix"] == 30 for _, f in fr]
    assert min(seqs) < 0x1000 and max(seqs) > 0xFFFFFF00


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "aipstack")),
                    reason="reference tree not present")
def test_generator_reproduces_the_fixture():
    with open(R.FIXTURE) as f:
        assert R.generate(REFERENCE) == f.read()


def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(R.FIXTURE) < 200 * 1024
    for s in R.load():
        assert set(s) == {"name", "addr", "prefix", "gateway", "mac", "peer", "peer_mac", "steps"}
        for st in s["steps"]:
            assert set(st) == {"step", "out"}
            for h in st["out"]:
                assert len(bytes.fromhex(h)) in (54, 58, 62)


# ---- the model's edge set ------------------------------------------------------------------------

def test_model_edge_set():
    edge = C.edge_set()
    ifc = dict(mac=C.MAC, ip_id=0)
    assert {(c["options"], c["flags"]) for c in edge} >= {(o, f) for o in range(4) for f in C.FLAGS}
    cks = set()
    for c in edge:
        h = C.build(c, ifc, 64, 7)
        assert len(h) == 54 + 4 * bin(c["options"]).count("1") and C.valid(c)
        # what a receiver computes: both checksums verify
        assert C.chksum(h[14:34]) == 0
        seg = h[34:]
        pseudo = h[26:34] + bytes([0, 6]) + len(seg).to_bytes(2, "big")
        assert C.chksum(pseudo + seg) == 0 or seg[16:18] == b"\x00\x00"
        cks.add(h[50:52].hex())
        assert h[50:52] != b"\xff\xff"      # the summed words are never all zero
    assert {"0000", "0001", "fffe"} <= cks
    for c in C.invalid_set():
        assert not C.valid(c)
    # the IPv4 header checksum at its ends, by a search over the Ident
    c = edge[0]
    for want in (0x0000, 0x0001, 0xFFFE):
        ident = C.ident_for_ip_checksum(want, c)
        assert ident is not None and C.build(c, ifc, 64, ident)[24:26] == want.to_bytes(2, "big")
    assert C.ident_for_ip_checksum(0xFFFF, c) is None


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 300, 321, 513, 700, 1025])
def test_batches_keep_the_edge_set_whole(n):
    """The batches of the GPU tests hold the searched TCP checksums and the ends of seq and ack,
    with the invalid descriptors of the GPU tests in place."""
    at = [i for i in (0, 63, 64, 255, 256, n - 1) if i < n]
    cs = C.batch(n, invalid_at=at)
    assert C.covers_the_ends(cs) and sum(not C.valid(c) for c in cs) == len(set(at))
    edge = C.edge_set()
    assert all(cs[k] == edge[k] for k in range(len(edge)) if k not in at)
    assert [C.pinned(c) for c in edge].count(True) >= 10


def test_model_ident_wraps():
    cs = C.batch(40, invalid_at=(0, 5))
    e = C.Expected(cs, dict(mac=C.MAC, ip_id=0xFFF0), 64)
    ids = [int.from_bytes(e.headers[i][18:20], "big") for i in sorted(e.headers)]
    assert ids == [(0xFFF0 + j) & 0xFFFF for j in range(38)] and 0 in ids and 0xFFFF in ids
    assert e.counts.tolist() == [38, 2] and e.hdr_len[0] == 0 and e.status[5] == C.INVALID


# ---- the struct and the constants ----------------------------------------------------------------

class _CCtl(ctypes.Structure):
    _fields_ = [("local_addr", ctypes.c_uint32), ("remote_addr", ctypes.c_uint32),
                ("local_port", ctypes.c_uint16), ("remote_port", ctypes.c_uint16),
                ("seq", ctypes.c_uint32), ("ack", ctypes.c_uint32), ("window", ctypes.c_uint16),
                ("mss", ctypes.c_uint16), ("flags", ctypes.c_uint8), ("options", ctypes.c_uint8),
                ("wnd_scale", ctypes.c_uint8), ("reserved0", ctypes.c_uint8),
                ("reserved1", ctypes.c_uint32)]


def test_dtype_matches_the_c_struct():
    d = A.TCP_CTL_DTYPE
    assert d.itemsize == 32 == ctypes.sizeof(_CCtl) and d == C.CTL
    assert list(d.names) == [n for n, _ in _CCtl._fields_]
    for name, ct in _CCtl._fields_:
        assert d.fields[name][1] == getattr(_CCtl, name).offset, name
        assert d.fields[name][0].itemsize == ctypes.sizeof(ct), name
    t = A.tcp_ctl([dict(local_addr=0x0A141E28, remote_addr=0x0A141E64, local_port=80, remote_port=40000,
                        seq=1, ack=2, window=4096, mss=1460, flags=0x12, options=3, wnd_scale=6)])
    assert t.dtype == d and t.tobytes().hex() == \
        "281e140a641e140a5000409c01000000020000000010b405120306" + "00" * 5
    assert t.tobytes() == C.to_array([dict(C.ctl(), seq=1, ack=2, mss=1460, flags=0x12, options=3,
                                           wnd_scale=6)]).tobytes()
    with pytest.raises(ValueError):
        A.tcp_ctl([dict(urgent=1)])


def test_constants_and_workspace():
    assert (A.AIPSTACK_TCP_CTL_EMITTED, A.AIPSTACK_TCP_CTL_INVALID, A.AIPSTACK_TCP_CTL_MAX_HEADER) == \
        (48, 49, 62) == (C.EMITTED, C.INVALID, C.MAX_HEADER)
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for line in ("#define AIPSTACK_TCP_CTL_MAX_HEADER 62u", "#define AIPSTACK_TCP_CTL_EMITTED  48 ",
                 "#define AIPSTACK_TCP_CTL_INVALID  49 ", "#define AIPSTACK_TX_RES_ARP_QUERY      47 ",
                 "#define AIPSTACK_CHKSUM_ABI_VERSION 1"):
        assert line in text, line
    assert text.index("AIPSTACK_TCP_CTL_MAX_HEADER") > text.index("aipstack_chksum_source_digest(void)")
    for n in (1, 63, 64, 65, 255, 256, 257, 513, 1 << 20):
        tiles = (n + 255) // 256
        assert A.tcp_tx_control_workspace_bytes(n) == 16 * (tiles + 1) + 32 * tiles


# ---- argument validation -------------------------------------------------------------------------

_NAMES = ("ctl", "n", "iface", "ttl", "hdr", "hdr_stride", "hdr_len", "chunk_index", "status", "counts",
          "workspace", "workspace_bytes", "stream")
_PTRS = ("ctl", "hdr", "hdr_len", "chunk_index", "status", "counts", "workspace")


def _args(fields=None, **over):
    """A well-formed argument list for 4 descriptors (host buffers standing in for device ones: a
    rejected call must return before touching them)."""
    bufs = {k: ctypes.create_string_buffer(512 + 16) for k in _PTRS}
    a = {k: (ctypes.addressof(v) + 15) & ~15 for k, v in bufs.items()}
    f = A.icmp_iface(0x0A141E28, 0x0A141EFF, R.LOCAL_MAC)
    for k, v in (fields or {}).items():
        f[k] = v
    bufs["iface"] = f
    a.update(n=4, hdr_stride=64, workspace_bytes=64, stream=None, iface=f.ctypes.data, ttl=64)
    for k, v in over.items():
        a[k] = a[k] + int(v[1:]) if isinstance(v, str) else v
    return bufs, [a[k] for k in _NAMES]


_BAD = [{k: None} for k in _PTRS + ("iface",)] + [
    {"hdr_stride": 61}, {"hdr_stride": 54}, {"hdr_stride": 0}, {"n": (1 << 40) + 1, "workspace_bytes": 1 << 62},
    {"ttl": 0}, {"ttl": 256}, {"workspace_bytes": 63}, {"workspace": "+4"}, {"ctl": "+4"},
    {"chunk_index": "+4"}, {"counts": "+4"}, {"hdr_len": "+2"}]


@pytest.mark.parametrize("over", _BAD)
def test_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(**over)
    assert lib.aipstack_tcp_tx_control(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("iface", [{"mtu": 255}, {"flags": 2}, {"flags": 0x80}, {"reserved": 1}])
def test_iface_einval_before_any_hip_call(iface):
    lib = _lib.load()
    keep, args = _args(fields=iface)
    assert lib.aipstack_tcp_tx_control(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_no_descriptors_is_a_noop():
    lib = _lib.load()
    keep, args = _args(n=0)
    assert lib.aipstack_tcp_tx_control(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(n=0, ctl=None, iface=None, workspace=None, hdr_stride=0, ttl=0)
    assert lib.aipstack_tcp_tx_control(*args) == A.AIPSTACK_CHKSUM_OK


# ---- the shared builder under ASan + UBSan, as a stand-alone program ---------------------------

def test_builder_under_asan_ubsan(sessions):
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "tcp_ctl.mk"], check=True, stdout=subprocess.DEVNULL)
    lines = []

    def add(cs, ifc, ttl):
        e = C.Expected(cs, ifc, ttl)
        arr, j = C.to_array(cs), 0
        for i in range(len(cs)):
            ok = i in e.headers
            lines.append("%s %d %d %d %s %d %s" % (bytes(ifc["mac"]).hex(), ifc["ip_id"], ttl, j,
                                                   arr[i].tobytes().hex(), int(ok),
                                                   e.headers[i].hex() if ok else "-"))
            j += ok

    for s, fr in sessions:
        add([C.from_frame(f)[0] for _, f in fr],
            dict(mac=bytes.fromhex(s["mac"]), ip_id=C.from_frame(fr[0][1])[3]), 64)
    add(C.batch(600, invalid_at=(0, 63, 64, 255, 256, 599)), dict(mac=C.MAC, ip_id=0xFF00), 255)
    add(C.edge_set() + C.invalid_set(), dict(mac=bytes([0xFF] * 6), ip_id=0xFFFF), 1)
    c = C.edge_set()[0]
    for want in (0x0000, 0x0001, 0xFFFE):
        add([c], dict(mac=C.MAC, ip_id=C.ident_for_ip_checksum(want, c)), 64)
    path = os.path.join(cpp, "build", "tcp_ctl_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "tcp_ctl_build_test"), path], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK %d cases" % len(lines) in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert len(lines) >= 800
