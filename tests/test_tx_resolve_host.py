"""Tx resolve, the parts that need no GPU: the model of tx_resolve_cases.py and a table keeper that
plays the host, pinned against what the reference's own IpStack and EthIpIface did for every send
of tests/golden/tx_resolve_ref_cases.json; the fixture's coverage; the structs and the constants;
aipstack_arp_table_sort; the argument validation of aipstack_tx_resolve (rejected before any HIP
call); and the shared decision with the host code under ASan/UBSan as a stand-alone program
(tests/cpp/tx_resolve_build_test.cpp)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib
from conftest import ROOT

import tx_resolve_cases as C
import tx_resolve_ref as R

REFERENCE = "/root/reference"


def replay(stack):
    """Yields (step, table, decision) for every send of a fixture stack, the keeper following
    the steps in order; for an injected frame (step, None, None)."""
    ifaces = C.stack_ifaces(stack)
    n = len(ifaces)
    keeper = C.Keeper(ifaces)
    for step in stack["steps"]:
        if step["op"] == "F":
            keeper.heard(n - 1 - step["iface"], bytes.fromhex(step["in"]))
            yield step, None, None
            continue
        table = keeper.table()
        force = C.ROUTE_ANY if step["iface"] < 0 else n - 1 - step["iface"]
        d = C.decide(step["src"], step["dst"], step["flags"], force, ifaces, C.table_lookup(table))
        yield step, table, d
        if d[0] == C.ARP_QUERY:
            keeper.held(d[3], d[1], d[4])


# ---- the model against the reference's recorded behaviour ---------------------------------------

def test_model_equals_the_reference():
    """Every recorded send: the IpErr, which interface's driver was handed a frame, the frame's 14
    bytes, and whether a broadcast ARP request left (exactly when the model says the host makes a
    new entry). No send is left out."""
    seen = 0
    statuses = set()
    for stack in R.load():
        ifaces = C.stack_ifaces(stack)
        n = len(ifaces)
        for step, table, d in replay(stack):
            if d is None:
                continue
            name = (stack["name"], step["name"])
            st, hop, index, k, flags, header, used = d
            assert step["err"] == C.IP_ERR[st], name
            sent = [e.split() for e in step["out"] if e.startswith("T ")]
            asked = [e.split() for e in step["out"] if e.startswith("Q ")]
            assert len(sent) + len(asked) == len(step["out"])
            if st == C.SENT:
                assert sent == [["T", str(n - 1 - k), header.hex()]], name
                assert (used is None) == bool(flags & C.BROADCAST) == (header[:6] == b"\xff" * 6), name
            else:
                assert not sent, name
            if st == C.ARP_QUERY and flags & C.NEW_ENTRY:
                assert len(asked) == 1 and int(asked[0][1]) == n - 1 - k, name
                q = bytes.fromhex(asked[0][2])
                f = ifaces[k]
                assert q[:6] == b"\xff" * 6 and q[6:12] == f["mac"] and q[12:14] == b"\x08\x06", name
                assert struct.unpack_from(">H", q, 20)[0] == 1, name
                assert struct.unpack_from(">I", q, 28)[0] == f["addr"] and struct.unpack_from(">I", q, 38)[0] == hop, name
            else:
                assert not asked, name
            statuses.add(st)
            seen += 1
    assert seen == sum(1 for s in R.load() for x in s["steps"] if x["op"] == "D") and seen >= 600
    assert statuses == {C.SENT, C.NO_ROUTE, C.BCAST_REJECTED, C.NONLOCAL_SRC, C.NO_HW_ROUTE, C.ARP_QUERY}


def test_fixture_covers_the_cases():
    by = {}
    for stack in R.load():
        for step, table, d in replay(stack):
            if d is not None:
                by[(stack["name"], step["name"])] = d
    n_three = 3

    def st(stack, name):
        return by[(stack, name)][0]

    def field(stack, name, j):
        return by[(stack, name)][j]
    # one interface, a /24 with a gateway: the four rounds
    assert [st("one_24_gw", "%s_if0_peer" % r) for r in ("empty", "query", "valid", "changed")] == \
        [C.ARP_QUERY, C.ARP_QUERY, C.SENT, C.SENT]
    assert field("one_24_gw", "empty_if0_peer", 4) & C.NEW_ENTRY and not field("one_24_gw", "query_if0_peer", 4) & C.NEW_ENTRY
    assert field("one_24_gw", "valid_if0_peer", 5)[:6] != field("one_24_gw", "changed_if0_peer", 5)[:6]
    assert st("one_24_gw", "valid_outside") == C.SENT and field("one_24_gw", "valid_outside", 4) & C.GATEWAY
    assert field("one_24_gw", "valid_outside", 1) == R.ip(10, 20, 30, 1)
    # the order of the error returns: NoIpRoute, BroadcastRejected, NonLocalSrc, then the hardware
    assert st("one_30", "empty_outside") == C.NO_ROUTE and st("one_30", "empty_all_ones") == C.NO_ROUTE
    assert st("one_30", "empty_force0_all_ones") == C.BCAST_REJECTED
    assert st("one_24_gw", "empty_if0_subnet_bcast_nonlocal_src") == C.BCAST_REJECTED
    assert st("one_24_gw", "empty_if0_subnet_bcast_allowed_nonlocal_src") == C.NONLOCAL_SRC
    assert st("one_24_gw", "empty_if0_subnet_bcast_allowed") == C.SENT
    assert st("one_24_gw", "empty_force0_all_ones_both_flags") == C.SENT
    assert st("one_24_gw", "empty_all_ones_both_flags") == C.ARP_QUERY          # unnamed: all-ones is not local,
    assert field("one_24_gw", "empty_all_ones_both_flags", 4) & C.GATEWAY      # so it goes to the gateway
    assert st("one_no_addr_gw", "empty_outside") == C.NONLOCAL_SRC
    assert st("one_no_addr_gw", "empty_outside_both_flags") == C.NO_HW_ROUTE
    assert st("one_no_addr", "empty_force0_all_ones_both_flags") == C.SENT
    assert st("one_24_gw", "empty_zero_both_flags") == C.ARP_QUERY             # 0.0.0.0 goes to the gateway
    assert st("one_24_gw", "empty_force0_zero_both_flags") == C.ARP_QUERY
    assert st("one_24_gw", "empty_if0_network_addr") == C.ARP_QUERY
    # the longest prefix wins whatever the list order; equal prefixes: the first in list order
    assert field("three_nested", "valid_if2_peer", 3) == n_three - 1 - 2
    assert field("three_nested", "valid_if1_peer", 3) == n_three - 1 - 2      # .41 lies in the /30 too
    assert field("three_nested", "valid_if0_peer", 3) == n_three - 1 - 0
    assert field("two_same_24", "valid_if0_peer", 3) == 0 == field("two_same_24", "valid_outside", 3)
    assert st("two_same_24", "valid_if0_peer") == C.NONLOCAL_SRC             # routed to the other interface
    assert st("two_same_24", "valid_force0_if0_peer") == C.SENT
    # a gateway interface met first gives way to a subnet behind it
    assert field("three_mixed", "valid_if0_peer", 3) == n_three - 1 - 0
    assert field("three_mixed", "valid_outside", 3) == 0 and field("three_mixed", "valid_outside", 4) & C.GATEWAY
    assert st("three_mixed", "empty_force1_outside_both_flags") == C.NO_HW_ROUTE   # no address: no ARP
    assert st("three_mixed", "empty_force0_outside") == C.NO_ROUTE
    assert {len(s["ifaces"]) for s in R.load()} == {1, 2, 3}


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "aipstack")),
                    reason="reference tree not present")
def test_generator_reproduces_the_fixture():
    with open(R.FIXTURE) as f:
        assert R.generate(REFERENCE) == f.read()


def test_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(R.FIXTURE) < 256 * 1024
    for s in R.load():
        assert set(s) == {"name", "ifaces", "steps"} and 1 <= len(s["ifaces"]) <= 3
        for f in s["ifaces"]:
            assert set(f) == {"have", "addr", "prefix", "have_gw", "gateway", "mac"}
            assert len(bytes.fromhex(f["mac"])) == 6
        for c in s["steps"]:
            if c["op"] == "F":
                assert set(c) == {"op", "iface", "in", "out"} and len(bytes.fromhex(c["in"])) == 42
            else:
                assert set(c) == {"op", "name", "src", "dst", "flags", "iface", "err", "out"}
                assert 0 <= c["err"] <= 15 and 0 <= c["flags"] <= 3
            assert len(c["out"]) <= 1
            for e in c["out"]:
                p = e.split(" ")
                assert p[0] in ("T", "Q") and len(p) == 3 and int(p[1]) < 3
                assert len(bytes.fromhex(p[2])) == (14 if p[0] == "T" else 42)


# ---- the structs, the constants, the sort ----------------------------------------------------------

class _CIface(ctypes.Structure):
    _fields_ = [("addr", ctypes.c_uint32), ("netmask", ctypes.c_uint32), ("gateway", ctypes.c_uint32),
                ("prefix", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("mac", ctypes.c_uint8 * 6),
                ("reserved", ctypes.c_uint8 * 12)]


class _CEntry(ctypes.Structure):
    _fields_ = [("addr", ctypes.c_uint32), ("iface", ctypes.c_uint16), ("state", ctypes.c_uint8),
                ("mac", ctypes.c_uint8 * 6), ("reserved", ctypes.c_uint8 * 3)]


class _CRoute(ctypes.Structure):
    _fields_ = [("next_hop", ctypes.c_uint32), ("arp_index", ctypes.c_uint32), ("iface", ctypes.c_uint16),
                ("status", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 4)]


@pytest.mark.parametrize("dtype,cstruct,model", [(A.TX_IFACE_DTYPE, _CIface, C.IFACE),
                                                 (A.ARP_ENTRY_DTYPE, _CEntry, C.ENTRY),
                                                 (A.TX_ROUTE_DTYPE, _CRoute, C.ROUTE)])
def test_dtypes_match_the_c_structs(dtype, cstruct, model):
    assert dtype.itemsize == ctypes.sizeof(cstruct) and dtype == model
    assert list(dtype.names) == [n for n, _ in cstruct._fields_]
    for name, ct in cstruct._fields_:
        assert dtype.fields[name][1] == getattr(cstruct, name).offset, name
        assert dtype.fields[name][0].itemsize == ctypes.sizeof(ct), name


def test_constants_and_workspace():
    assert (A.AIPSTACK_TX_RES_NONE, A.AIPSTACK_TX_RES_SENT, A.AIPSTACK_TX_RES_NO_ROUTE,
            A.AIPSTACK_TX_RES_BCAST_REJECTED, A.AIPSTACK_TX_RES_NONLOCAL_SRC, A.AIPSTACK_TX_RES_NO_HW_ROUTE,
            A.AIPSTACK_TX_RES_ARP_QUERY) == (41, 42, 43, 44, 45, 46, 47) == \
        (C.NONE, C.SENT, C.NO_ROUTE, C.BCAST_REJECTED, C.NONLOCAL_SRC, C.NO_HW_ROUTE, C.ARP_QUERY)
    assert (A.AIPSTACK_TX_ALLOW_BROADCAST, A.AIPSTACK_TX_ALLOW_NONLOCAL_SRC) == (1, 2) == \
        (R.ALLOW_BROADCAST, R.ALLOW_NONLOCAL_SRC)
    assert (A.AIPSTACK_TX_ROUTE_ANY, A.AIPSTACK_TX_MAX_IFACES, A.AIPSTACK_TX_NO_ARP_ENTRY) == (0xFFFF, 16, C.NO_ENTRY)
    assert (A.AIPSTACK_ARP_STATE_QUERY, A.AIPSTACK_ARP_STATE_VALID, A.AIPSTACK_ARP_STATE_REFRESHING) == (1, 2, 3)
    assert (A.AIPSTACK_TX_ROUTE_GATEWAY, A.AIPSTACK_TX_ROUTE_BROADCAST, A.AIPSTACK_TX_ROUTE_NEW_ENTRY,
            A.AIPSTACK_TX_ROUTE_FORCED) == (C.GATEWAY, C.BROADCAST, C.NEW_ENTRY, C.FORCED)
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for line in ("#define AIPSTACK_TX_RES_NONE           41 ", "#define AIPSTACK_TX_RES_SENT           42 ",
                 "#define AIPSTACK_TX_RES_NO_ROUTE       43 ", "#define AIPSTACK_TX_RES_BCAST_REJECTED 44 ",
                 "#define AIPSTACK_TX_RES_NONLOCAL_SRC   45 ", "#define AIPSTACK_TX_RES_NO_HW_ROUTE    46 ",
                 "#define AIPSTACK_TX_RES_ARP_QUERY      47 ", "#define AIPSTACK_ICMP_DU_TCP_PCB     40 ",
                 "#define AIPSTACK_TX_ROUTE_ANY 0xFFFFu", "#define AIPSTACK_CHKSUM_ABI_VERSION 1"):
        assert line in text, line
    assert text.index("AIPSTACK_TX_RES_NONE") > text.index("aipstack_icmp_rx_unreach_slotted")
    assert A.tx_resolve_workspace_bytes(1 << 20) == 16 * (4096 + 1) + 64 * 4096
    for n in (1, 63, 64, 65, 255, 256, 257, 513, 65600):
        tiles = (n + 255) // 256
        assert A.tx_resolve_workspace_bytes(n) == 16 * (tiles + 1) + 64 * tiles


def test_tx_ifaces_builds_the_table():
    ifaces = C.stack_ifaces(R.load()[4])
    t = A.tx_ifaces([(f["addr"] if f["have"] else None, f["prefix"], f["gateway"] if f["have_gw"] else None,
                      f["mac"]) for f in ifaces])
    assert t.tobytes() == C.iface_table(ifaces).tobytes()
    t = A.tx_ifaces([(None, 0, 0x0A090909, R.mac_of(1)), (5, 0, None, R.mac_of(2)), (7, 32, None, R.mac_of(3))])
    assert t["flags"].tolist() == [2, 1, 1] and t["netmask"].tolist() == [0, 0, 0xFFFFFFFF]
    with pytest.raises(ValueError):
        A.tx_ifaces([(1, 33, None, bytes(6))])


def test_arp_table_sort():
    t = C.lan_table(500)
    rng = np.random.default_rng(3)
    shuffled = t[rng.permutation(len(t))]
    assert A.arp_table_sort(shuffled).tobytes() == t.tobytes()
    assert A.arp_table_sort(np.zeros(0, dtype=C.ENTRY)).size == 0
    dup = np.concatenate([t[:5], t[2:3]])
    with pytest.raises(A.ChksumError):
        A.arp_table_sort(dup)
    for field, value in (("state", 0), ("state", 4), ("iface", 16)):
        bad = t[:4].copy()
        bad[field][1] = value
        with pytest.raises(A.ChksumError):
            A.arp_table_sort(bad)
    lib = _lib.load()
    assert lib.aipstack_arp_table_sort(None, 1) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_arp_table_sort(None, 0) == A.AIPSTACK_CHKSUM_OK


# ---- argument validation ---------------------------------------------------------------------------

_NAMES = ("hdr", "stride", "hdr_len", "n", "seg_status", "send_flags", "force", "ifaces", "n_ifaces", "arp",
          "n_arp", "status", "route", "send_len", "arp_used", "held", "failed", "counts", "workspace",
          "workspace_bytes", "flags", "stream")
_PTRS = ("hdr", "hdr_len", "seg_status", "send_flags", "force", "ifaces", "arp", "status", "route", "send_len",
         "arp_used", "held", "failed", "counts", "workspace")


def _args(**over):
    """A well-formed argument list for 4 segments (host buffers standing in for device ones: a
    rejected call must return before touching them)."""
    bufs = {k: ctypes.create_string_buffer(512 + 16) for k in _PTRS}
    a = {k: (ctypes.addressof(v) + 15) & ~15 for k, v in bufs.items()}
    a.update(stride=64, n=4, n_ifaces=2, n_arp=3, workspace_bytes=96, flags=0, stream=None)
    for k, v in over.items():
        a[k] = a[k] + int(v[1:]) if isinstance(v, str) else v
    return bufs, [a[k] for k in _NAMES]


_BAD = [{k: None} for k in ("hdr", "hdr_len", "ifaces", "arp", "arp_used", "status", "route", "send_len", "held",
                            "failed", "counts", "workspace")] + [
    {"n_ifaces": 17}, {"stride": 0}, {"n": (1 << 40) + 1, "workspace_bytes": 1 << 62}, {"n_arp": 0xFFFFFFFF},
    {"workspace_bytes": 95}, {"workspace": "+4"}, {"held": "+4"}, {"failed": "+4"}, {"counts": "+4"},
    {"hdr_len": "+2"}, {"send_len": "+2"}, {"route": "+2"}, {"ifaces": "+2"}, {"arp": "+2"}, {"force": "+1"}]


@pytest.mark.parametrize("over", _BAD)
def test_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(**over)
    assert lib.aipstack_tx_resolve(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_no_segments_is_a_noop():
    lib = _lib.load()
    keep, args = _args(n=0)
    assert lib.aipstack_tx_resolve(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(n=0, hdr=None, ifaces=None, workspace=None, workspace_bytes=0, stride=0, n_ifaces=99)
    assert lib.aipstack_tx_resolve(*args) == A.AIPSTACK_CHKSUM_OK


def test_wrapper_rejects_host_tensors():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        A.tx_resolve(torch.zeros(64, dtype=torch.uint8), 64, torch.zeros(1, dtype=torch.int32),
                     C.iface_table(C.LAN))


# ---- CHECKS OF THE TEST INFRASTRUCTURE, not of the feature: the batches of the GPU tests are not
# ---- vacuous. They run the Python model and the builders alone.

@pytest.mark.parametrize("kind", ["sent", "query", "error"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_infrastructure_placed_batches_hit_where_they_say(n, kind):
    ring, lens = C.ring_of(C.placed_batch(n, kind), 64)
    e = C.expected(ring, 64, lens, C.LAN, C.lan_table())
    want = {"sent": (C.SENT,), "query": (C.ARP_QUERY,), "error": C.FAILED}[kind]
    places = sorted({i for i in C.PLACES + (n - 1,) if i < n})
    assert all(int(e.status[i]) in want for i in places)
    listed = {"sent": None, "query": e.held, "error": e.failed}[kind]
    if listed is not None:
        assert set(places) <= set(listed.tolist())
    if n >= 63:
        assert set(e.status.tolist()) >= {C.NONE, C.SENT, C.BCAST_REJECTED, C.ARP_QUERY}
        assert e.arp_used.sum() == 2 and (e.routes["flags"] & C.NEW_ENTRY).any()


def test_infrastructure_random_case_contains_every_status():
    ifaces, table, headers, sf, force, ss = C.random_case(20261021, 2048)
    ring, lens = C.ring_of(headers, 64)
    e = C.expected(ring, 64, lens, ifaces, table, seg_status=ss, send_flags=sf, force=force)
    assert set(e.status.tolist()) == set(range(41, 48))
    assert e.arp_used.sum() >= 20 and int(e.counts[0]) >= 20 and int(e.counts[1]) >= 100
    assert len(set(e.routes["iface"].tolist())) >= 4 and len(set(e.routes["flags"].tolist())) >= 6


# ---- the shared decision under ASan + UBSan, as a stand-alone program ----------------------------

def _tables(lines, ifaces, table):
    t = C.iface_table(ifaces)
    lines.append("I %d" % len(t))
    lines.extend("%d %d %d %d %d %s" % (f["addr"], f["netmask"], f["gateway"], f["prefix"], f["flags"],
                                        f["mac"].tobytes().hex()) for f in t)
    lines.append("T %d" % len(table))
    lines.extend("%d %d %d %s" % (e["addr"], e["iface"], e["state"], e["mac"].tobytes().hex()) for e in table)


def _cases(lines, headers, stride, ifaces, table, *, sf=None, force=None, ss=None, specified=True):
    ring, lens = C.ring_of(headers, stride)
    e = C.expected(ring, stride, lens, ifaces, table, seg_status=ss, send_flags=sf, force=force)
    for i, h in enumerate(headers):
        sent = int(e.status[i]) == C.SENT
        lines.append("C %d %d %d %d %d %s %s %s" % (
            stride, ss[i] if ss is not None else 0, sf[i] if sf is not None else 0,
            force[i] if force is not None else C.ROUTE_ANY, int(e.status[i]) if specified else 0,
            e.routes[i].tobytes().hex(), e.ring[i * stride:i * stride + 14].tobytes().hex() if sent else "-",
            h.hex() or "-"))
    return len(headers)


def test_decision_under_asan_ubsan():
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "tx_resolve.mk"], check=True, stdout=subprocess.DEVNULL)
    lines, count = [], 0
    for stack in R.load():                      # the fixture's sends, each against the table of its moment
        ifaces, last = C.stack_ifaces(stack), None
        n = len(ifaces)
        for step, table, d in replay(stack):
            if d is None:
                continue
            if last is None or table.tobytes() != last:
                _tables(lines, ifaces, table)
                last = table.tobytes()
            force = C.ROUTE_ANY if step["iface"] < 0 else n - 1 - step["iface"]
            count += _cases(lines, [C.header(step["src"], step["dst"], length=64)], 64, ifaces, table,
                            sf=[step["flags"]], force=[force])
    ifaces, table, headers, sf, force, ss = C.random_case(7, 600)
    _tables(lines, ifaces, table)
    count += _cases(lines, headers, 64, ifaces, table, sf=sf, force=force, ss=ss)
    _tables(lines, C.LAN, C.lan_table(40))
    count += _cases(lines, C.placed_batch(257), 256, C.LAN, C.lan_table(40))
    count += _cases(lines, [C.header(C.LAN[0]["addr"], C.PEER_SENT, length=40)], 36, C.LAN, C.lan_table(40))
    # an unsorted table and one with duplicate keys: outcomes unspecified, every index inside
    t = C.lan_table(40)
    for bad in (t[::-1].copy(), np.concatenate([t, t[5:30], t[:3]])):
        _tables(lines, C.LAN, bad)
        count += _cases(lines, C.placed_batch(130), 64, C.LAN, t, specified=False)
    _tables(lines, C.LAN, np.zeros(0, dtype=C.ENTRY))
    count += _cases(lines, C.placed_batch(70), 64, C.LAN, np.zeros(0, dtype=C.ENTRY))
    path = os.path.join(cpp, "build", "tx_resolve_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "tx_resolve_build_test"), path], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "OK %d cases" % count in r.stdout, (
        r.returncode, r.stdout[-2000:], r.stderr[-4000:])
