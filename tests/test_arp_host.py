"""ARP on receive, the parts that need no GPU: the model of arp_cases.py pinned against what the
reference's own EthIpIface did with every frame of tests/golden/arp_ref_cases.json (the frames it
sent byte for byte, its observer notifications, and what a probe showed of its ARP table), the
fixture's coverage, the structs and the constants, the argument validation of the two batch
calls (rejected before any HIP call), and the shared record and reply builder under ASan/UBSan
as a stand-alone program (tests/cpp/arp_build_test.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib
from conftest import ROOT

import arp_cases as C
import arp_ref as R

REFERENCE = "/root/reference"


@pytest.fixture(scope="module")
def replayed():
    """[(stack, interface, frames, Expected)] of the fixture: a stack's cases as one batch."""
    out = []
    for s in R.load():
        ifc, frames = C.stack_iface(s), C.stack_frames(s)
        out.append((s, ifc, frames, C.respond(frames, ifc)))
    return out


# ---- the model against the reference's recorded behaviour ---------------------------------------

def test_model_equals_the_reference(replayed):
    """Every case: the model's reply is the one frame the reference sent, byte for byte, and
    nothing where it sent nothing; a NOTIFY record is the reference's one observer call with the
    record's address and MAC, and there is no call without it; the probe found the sender's MAC
    learned exactly for a LEARN record with NEW_OK (the stack was fresh: no entry to find), an ARP
    query where an entry could have been made and none was, and nothing for every other address."""
    seen = 0
    for stack, ifc, frames, e in replayed:
        for i, case in enumerate(stack["cases"]):
            name = (case["name"], stack["have"], stack["prefix"])
            rec = e.records[i]
            status, flags = int(e.status[i]), int(rec["flags"])
            assert C.sent(case["out"]) == ([e.headers[i]] if status == C.REPLY else []), name
            mac = rec["sender_mac"].tobytes()
            want_obs = [(int(rec["sender_addr"]), mac)] if flags & C.NOTIFY else []
            assert C.observed(case["out"]) == want_obs, name
            if status == C.REPLY and want_obs:
                assert case["out"][0].startswith("O ")           # save_hw_addr runs first (:497)
            if status in (C.NONE, C.MALFORMED):
                assert flags == 0 and not rec["sender_addr"] and not rec["sender_mac"].any(), name
            # the probe: an echo request from the frame's sender address
            probe = bytes.fromhex(case["probe"])
            sender = int.from_bytes(probe[26:30], "big")
            if status in (C.SEEN, C.REPLY):
                assert sender == int(rec["sender_addr"]), name
            learned = status in (C.SEEN, C.REPLY) and flags & C.LEARN and flags & C.NEW_OK
            outcome, to = C.probe_outcome(case["probe_out"], ifc)
            if learned:
                assert (outcome, to) == ("learned", mac), name
                assert probe[6:12] != mac or case["name"] == "arp_then_echo_one_peer"
            elif C.new_ok(sender, ifc):
                assert outcome == "query", name
            else:
                assert outcome == "none", name
            seen += 1
    assert seen == sum(len(s["cases"]) for s, _, _, _ in replayed) >= 120


def test_fixture_covers_the_cases(replayed):
    by = {}
    for stack, ifc, frames, e in replayed:
        key = "none" if not stack["have"] else "/%d" % stack["prefix"]
        for i, case in enumerate(stack["cases"]):
            by[(case["name"], key)] = (frames[i], int(e.status[i]), int(e.records[i]["flags"]), e, i)
    assert {k for _, k in by} == {"/24", "/30", "none"}
    # every status, and every combination of flags the rules allow, occurs
    assert {v[1] for v in by.values()} == {C.NONE, C.MALFORMED, C.SEEN, C.REPLY}
    combos = {v[2] for v in by.values() if v[1] in (C.SEEN, C.REPLY)}
    base = (0, C.NEW_OK, C.LEARN, C.LEARN | C.NOTIFY, C.LEARN | C.NOTIFY | C.NEW_OK)
    assert combos == {b | r for b in base for r in (0, C.REC_REPLY)}
    for key in ("/24", "/30"):
        def st(name):
            return by[(name, key)][1]

        def fl(name):
            return by[(name, key)][2]
        assert st("request_for_us") == st("request_unicast") == C.REPLY
        assert st("request_for_other") == st("reply_to_us") == st("op0") == st("op3") == C.SEEN
        for field in ("hwtype", "ptype", "hlen", "plen"):
            assert st(field + "_minus_1") == st(field + "_plus_1") == C.MALFORMED
        assert [len(by[(n, key)][0]) for n in ("len0", "len13", "len14_arp", "len41", "len42", "len60")] == \
            [0, 13, 14, 41, 42, 60]
        assert [st(n) for n in ("len0", "len13", "len14_arp", "len41", "len42", "len60")] == \
            [C.NONE, C.NONE, C.MALFORMED, C.MALFORMED, C.REPLY, C.REPLY]
        assert st("ethertype_ip4") == st("ethertype_ip6") == C.NONE
        # a reply is due whatever LEARN says, and goes to the ARP sender, not the Ethernet source
        assert st("sender_mac_bcast_request") == C.REPLY and not fl("sender_mac_bcast_request") & C.LEARN
        f, _, _, e, i = by[("request_for_us", key)]
        assert f[6:12] == R.ETH_SRC != f[22:28] == R.SENDER_MAC == e.headers[i][:6]
        assert fl("sender_zero_request") == C.LEARN | C.REC_REPLY
        assert fl("sender_all_ones_reply") == C.LEARN
        assert fl("sender_subnet_bcast_reply") == fl("sender_outside_reply") == C.LEARN | C.NOTIFY
        assert fl("gratuitous_request_peer") == C.LEARN | C.NOTIFY | C.NEW_OK
        assert st("gratuitous_request_own_addr") == C.REPLY and st("target_mac_garbage") == C.REPLY
    # no address: nothing replies, nothing may be created, the observers still hear (DHCP's case)
    none = [v for (_, k), v in by.items() if k == "none"]
    assert not any(v[1] == C.REPLY or v[2] & C.NEW_OK for v in none)
    assert by[("request_for_us", "none")][2] == C.LEARN | C.NOTIFY
    assert by[("sender_outside_request", "none")][2] == C.LEARN | C.NOTIFY


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "aipstack")),
                    reason="reference tree not present")
def test_generator_reproduces_the_fixture():
    with open(R.FIXTURE) as f:
        assert R.generate(REFERENCE) == f.read()


def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(R.FIXTURE) < 100 * 1024
    for s in R.load():
        assert set(s) == {"have", "addr", "prefix", "mac", "cases"}
        for c in s["cases"]:
            assert set(c) == {"name", "in", "out", "probe", "probe_out"}
            bytes.fromhex(c["in"]), bytes.fromhex(c["probe"])
            for e in c["out"] + c["probe_out"]:
                assert e[:2] in ("T ", "O ")
                [bytes.fromhex(w) if k or e[0] == "T" else int(w) for k, w in enumerate(e[2:].split())]


# ---- the structs and the constants ---------------------------------------------------------------

class _CIface(ctypes.Structure):
    _fields_ = [("local_addr", ctypes.c_uint32), ("netmask", ctypes.c_uint32), ("mac", ctypes.c_uint8 * 6),
                ("flags", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 17)]


class _CRecord(ctypes.Structure):
    _fields_ = [("sender_addr", ctypes.c_uint32), ("sender_mac", ctypes.c_uint8 * 6),
                ("op", ctypes.c_uint16), ("flags", ctypes.c_uint8), ("status", ctypes.c_uint8),
                ("reserved", ctypes.c_uint16)]


@pytest.mark.parametrize("dtype,cstruct,size", [("ARP_IFACE_DTYPE", _CIface, 32),
                                                ("ARP_RECORD_DTYPE", _CRecord, 16)])
def test_dtypes_match_the_c_structs(dtype, cstruct, size):
    d = getattr(A, dtype)
    assert d.itemsize == size == ctypes.sizeof(cstruct)
    assert list(d.names) == [n for n, _ in cstruct._fields_]
    for name, ct in cstruct._fields_:
        assert d.fields[name][1] == getattr(cstruct, name).offset, name
        assert d.fields[name][0].itemsize == ctypes.sizeof(ct), name
    assert A.ARP_RECORD_DTYPE == C.RECORD


def test_iface_and_constants():
    f = A.arp_iface(0x0A141E28, 0xFFFFFF00, R.LOCAL_MAC)
    assert (int(f["local_addr"][0]), int(f["netmask"][0]), int(f["flags"][0])) == (0x0A141E28, 0xFFFFFF00, 1)
    assert f["mac"][0].tobytes() == R.LOCAL_MAC and not f["reserved"].any()
    assert int(A.arp_iface(0, 0, R.LOCAL_MAC, have_addr=False)["flags"][0]) == 0
    assert (A.AIPSTACK_ARP_NONE, A.AIPSTACK_ARP_MALFORMED, A.AIPSTACK_ARP_SEEN, A.AIPSTACK_ARP_REPLY) == \
        (27, 28, 29, 30) == (C.NONE, C.MALFORMED, C.SEEN, C.REPLY)
    assert (A.AIPSTACK_ARP_REC_LEARN, A.AIPSTACK_ARP_REC_NEW_OK, A.AIPSTACK_ARP_REC_NOTIFY,
            A.AIPSTACK_ARP_REC_REPLY) == (1, 2, 4, 8) == (C.LEARN, C.NEW_OK, C.NOTIFY, C.REC_REPLY)
    assert A.AIPSTACK_ARP_REPLY_HEADER == 42 and A.AIPSTACK_ARP_HAVE_ADDR == 1
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for line in ("#define AIPSTACK_ARP_REPLY_HEADER 42u", "#define AIPSTACK_ARP_NONE       27 ",
                 "#define AIPSTACK_ARP_MALFORMED  28 ", "#define AIPSTACK_ARP_SEEN       29 ",
                 "#define AIPSTACK_ARP_REPLY      30 ", "#define AIPSTACK_ARP_HAVE_ADDR  1u ",
                 "#define AIPSTACK_ARP_REC_LEARN  1u ", "#define AIPSTACK_ARP_REC_NEW_OK 2u ",
                 "#define AIPSTACK_ARP_REC_NOTIFY 4u ", "#define AIPSTACK_ARP_REC_REPLY  8u ",
                 "#define AIPSTACK_ICMP_TOO_LARGE   26 ", "#define AIPSTACK_CHKSUM_ABI_VERSION 1"):
        assert line in text, line
    assert A.arp_rx_respond_workspace_bytes(1 << 20) == 16 * (4096 + 1) + 64 * 4096
    assert A.arp_rx_respond_workspace_bytes(1) == 32 + 64


# ---- argument validation of the batch calls -----------------------------------------------------

_OUT = ("status", "arp", "hdr", "hdr_stride", "hdr_len", "chunk_index", "reply_frame", "seen_frame",
        "counts", "workspace", "workspace_bytes", "stream")
_CSR = ("base", "offsets", "n", "iface") + _OUT
_SLOT = ("base", "stride", "lens", "n", "iface") + _OUT


def _args(names, fields=None, **over):
    """A well-formed argument list for 4 frames (host buffers standing in for device ones: a
    rejected call must return before touching them)."""
    bufs = {k: ctypes.create_string_buffer(512 + 16) for k in
            ("base", "offsets", "lens", "status", "arp", "hdr", "hdr_len", "chunk_index", "reply_frame",
             "seen_frame", "counts", "workspace")}
    a = {k: (ctypes.addressof(v) + 15) & ~15 for k, v in bufs.items()}
    f = A.arp_iface(0x0A141E28, 0xFFFFFF00, R.LOCAL_MAC)
    for k, v in (fields or {}).items():
        f[k] = v
    bufs["iface"] = f
    a.update(n=4, stride=128, hdr_stride=64, workspace_bytes=96, stream=None, iface=f.ctypes.data)
    for k, v in over.items():
        a[k] = a[k] + int(v[1:]) if isinstance(v, str) else v
    return bufs, [a[k] for k in names]


_BAD = [{k: None} for k in ("base", "iface", "status", "arp", "hdr", "hdr_len", "chunk_index",
                            "reply_frame", "seen_frame", "counts", "workspace")] + [
    {"hdr_stride": 41}, {"hdr_stride": 0}, {"n": (1 << 40) + 1, "workspace_bytes": 1 << 62},
    {"workspace_bytes": 95}, {"workspace": "+4"}, {"chunk_index": "+4"}, {"reply_frame": "+4"},
    {"seen_frame": "+4"}, {"counts": "+4"}, {"hdr_len": "+2"}, {"arp": "+2"}, {"arp": "+1"}]
_BAD_IFACE = [{"flags": 2}, {"flags": 3}, {"flags": 0x80}, {"reserved": 1}]


@pytest.mark.parametrize("over", _BAD + [{"offsets": None}])
def test_csr_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_CSR, **over)
    assert lib.aipstack_arp_rx_respond(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("over", _BAD + [{"lens": None}, {"stride": 0}, {"stride": 65537}])
def test_slotted_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_SLOT, **over)
    assert lib.aipstack_arp_rx_respond_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("iface", _BAD_IFACE)
def test_iface_einval_before_any_hip_call(iface):
    lib = _lib.load()
    keep, args = _args(_CSR, fields=iface)
    assert lib.aipstack_arp_rx_respond(*args) == A.AIPSTACK_CHKSUM_EINVAL
    keep, args = _args(_SLOT, fields=iface)
    assert lib.aipstack_arp_rx_respond_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_no_frames_is_a_noop():
    lib = _lib.load()
    keep, args = _args(_CSR, n=0)
    assert lib.aipstack_arp_rx_respond(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_CSR, n=0, base=None, iface=None, workspace=None, hdr_stride=0)
    assert lib.aipstack_arp_rx_respond(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_SLOT, n=0, stride=0)
    assert lib.aipstack_arp_rx_respond_slotted(*args) == A.AIPSTACK_CHKSUM_OK


def test_wrappers_reject_host_tensors():
    torch = pytest.importorskip("torch")
    fr, off = torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    f = A.arp_iface(0x0A141E28, 0xFFFFFF00, R.LOCAL_MAC)
    with pytest.raises(ValueError):
        A.arp_rx_respond(fr, off, f)
    with pytest.raises(ValueError):
        A.arp_rx_respond_slotted(fr, 64, torch.zeros(1, dtype=torch.int32), f)


# ---- the frame sets of the GPU tests are not vacuous (from the model alone) ----------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_sized_batches_contain_their_classes(n):
    """The batches of test_gpu_arp.py hold what their names say, and the workspace the library
    asks for them is a pair of counts per 256-frame tile and the totals, then four ballot pairs
    per tile."""
    tiles = (n + 255) // 256
    assert A.arp_rx_respond_workspace_bytes(n) == 16 * (tiles + 1) + 64 * tiles
    ifc = C.iface()
    e = C.respond(C.sized_batch(n, "all"), ifc)
    assert e.counts.tolist() == [n, n] and (e.status == C.REPLY).all()
    assert len(set(e.headers.values())) == n                            # every reply differs
    e = C.respond(C.sized_batch(n, "none"), ifc)
    assert int(e.counts[0]) == 0 and set(np.unique(e.status)) <= {C.SEEN, C.MALFORMED}
    e = C.respond(C.sized_batch(n, "no_arp"), ifc)
    assert e.counts.tolist() == [0, 0] and (e.status == C.NONE).all()
    e = C.respond(C.sized_batch(n, "mixed"), ifc)
    assert e.status[0] == e.status[n - 1] == C.REPLY
    if n == 513:
        assert set(np.unique(e.status)) == {C.NONE, C.MALFORMED, C.SEEN, C.REPLY}
        assert e.hdr_len[512] and not e.hdr_len[257:512].any() and int(e.counts[1]) > int(e.counts[0])


# ---- the shared builder under ASan + UBSan, as a stand-alone program ---------------------------

def test_builder_under_asan_ubsan(replayed):
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "arp.mk"], check=True, stdout=subprocess.DEVNULL)
    lines = []

    def add(frames, ifc, e):
        for i, f in enumerate(frames):
            lines.append("%d %d %d %s %s %s %s" % (
                ifc["local"], ifc["netmask"], int(ifc["have"]), ifc["mac"].hex(),
                e.records[i].tobytes().hex(), f.hex() or "-",
                e.headers[i].hex() if i in e.headers else "-"))

    for _, ifc, frames, e in replayed:
        add(frames, ifc, e)
    for ifc in (C.iface(), C.iface(prefix=30, local=0x0A141E29), C.iface(have=False)):
        frames = C.sized_batch(513, "mixed") + C.sized_batch(40, "none") + C.sized_batch(40, "no_arp")
        add(frames, ifc, C.respond(frames, ifc))
    path = os.path.join(cpp, "build", "arp_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "arp_build_test"), path], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK %d cases" % len(lines) in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-4000:])
