"""IPv4 reassembly on receive, the parts that need no GPU: the hole model pinned against answers
recorded from code compiled from the reference (tests/golden/ip_reass_ref_cases.json); the record's layout and the constants,
the argument validation of aipstack_ip4_rx_reassemble / _slotted (rejected before any HIP call),
the workspace size, the two models of ipreass_cases.py against each other and against the frame
oracle on every generated batch, the crafted groups' expected outcomes, and the shared host /
device text run serially under ASan/UBSan as a stand-alone program
(tests/cpp/ipreass_table_test.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib
from conftest import ROOT

import ip_reass_ref
import ipreass_cases as R

REFERENCE = "/root/reference"


class _CDgram(ctypes.Structure):
    _fields_ = [("n_frags", ctypes.c_uint32), ("last_frame", ctypes.c_uint32),
                ("data_len", ctypes.c_uint16), ("proto", ctypes.c_uint8), ("verdict", ctypes.c_uint8),
                ("reserved", ctypes.c_uint32)]


def test_dgram_dtype_matches_the_c_struct():
    assert A.IP4_DGRAM_DTYPE.itemsize == 16 == ctypes.sizeof(_CDgram)
    for name, _ in _CDgram._fields_:
        assert A.IP4_DGRAM_DTYPE.fields[name][1] == getattr(_CDgram, name).offset, name
    assert A.IP4_DGRAM_DTYPE == R.DGRAM_DTYPE


def test_constants():
    assert (A.AIPSTACK_RX_FRAG_MEMBER, A.AIPSTACK_RX_DROP_FRAG, A.AIPSTACK_RX_REASS_TRUNCATED) == (14, 15, 16)
    assert A.AIPSTACK_REASS_NONE == 0xFFFFFFFF and A.RX_VERDICTS[14] == "FRAG_MEMBER"
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for line in ("#define AIPSTACK_RX_FRAG_MEMBER      14 ", "#define AIPSTACK_RX_DROP_FRAG        15 ",
                 "#define AIPSTACK_RX_REASS_TRUNCATED  16 ", "#define AIPSTACK_REASS_NONE 0xFFFFFFFFu",
                 "#define AIPSTACK_CHKSUM_ABI_VERSION 1"):
        assert line in text


# ---- argument validation ------------------------------------------------------------------

_NAMES = ("base", "frames", "n", "max", "verdict", "chunk_addr", "chunk_len", "next", "head", "dgram",
          "ws", "ws_bytes", "stream")
_POINTERS = ("base", "frames", "verdict", "chunk_addr", "chunk_len", "next", "head", "dgram")


def _args(slotted=False, **over):
    lib = _lib.load()
    n = 4
    need = int(lib.aipstack_ip4_reass_workspace_bytes(n))
    bufs = {k: ctypes.create_string_buffer(512) for k in _POINTERS}
    ws = ctypes.create_string_buffer(need + 16)
    wsp = (ctypes.addressof(ws) + 7) & ~7
    a = {k: (ctypes.addressof(v) + 7) & ~7 for k, v in bufs.items()}
    a.update(n=n, max=65531, ws=wsp, ws_bytes=need, stream=None, stride=2048)
    for k, v in over.items():
        a[k] = a[k] + int(v[1:]) if isinstance(v, str) and v.startswith("+") else v
    if a["ws_bytes"] == "short":
        a["ws_bytes"] = need - 1
    names = _NAMES if not slotted else ("base", "stride") + _NAMES[1:]
    return lib, (bufs, ws), [a[k] for k in names]


@pytest.mark.parametrize("over", [{k: None} for k in _POINTERS] + [
    {"ws": None}, {"ws_bytes": 0}, {"ws_bytes": "short"}, {"ws": "+4"}, {"max": 0}, {"max": 65532},
    {"n": (1 << 32) - 1, "ws_bytes": 1 << 62}, {"chunk_addr": "+4"}, {"chunk_len": "+2"},
    {"next": "+1"}, {"head": "+2"}, {"dgram": "+1"},
])
def test_einval_before_any_hip_call(over):
    for slotted in (False, True):
        lib, keep, args = _args(slotted, **over)
        f = lib.aipstack_ip4_rx_reassemble_slotted if slotted else lib.aipstack_ip4_rx_reassemble
        assert f(*args) == A.AIPSTACK_CHKSUM_EINVAL
        assert lib.aipstack_chksum_last_hip_error() == 0


def test_slot_stride_and_the_empty_batch():
    lib, keep, args = _args(True, stride=0)
    assert lib.aipstack_ip4_rx_reassemble_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    lib, keep, args = _args(True, stride=65537)
    assert lib.aipstack_ip4_rx_reassemble_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    lib, keep, args = _args(n=0)
    assert lib.aipstack_ip4_rx_reassemble(*args) == A.AIPSTACK_CHKSUM_OK
    lib, keep, args = _args(n=0, max=0)
    assert lib.aipstack_ip4_rx_reassemble(*args) == A.AIPSTACK_CHKSUM_EINVAL


def test_workspace_holds_two_tables_of_a_power_of_two():
    prev = 0
    for n in list(range(0, 40)) + [255, 256, 257, 4096, 4097, 1 << 20, (1 << 32) - 2]:
        b = A.ip4_reass_workspace_bytes(n)
        slots = R.table_slots(n)
        assert slots & (slots - 1) == 0 and slots >= 4 * n
        assert b % 8 == 0 and b >= prev and 16 * slots + 30 * n + 8 <= b <= 16 * slots + 30 * n + 24, n
        prev = b
    assert A.ip4_reass_workspace_bytes(1 << 40) == A.ip4_reass_workspace_bytes((1 << 32) - 2)


def test_wrapper_rejects_host_tensors():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        A.ip4_rx_reassemble(torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64))


# ---- the models ----------------------------------------------------------------------------

def _batches(oracle):
    rng = np.random.default_rng(1)
    out = [("crafted", R.Batch([f for _, fr, _ in R.crafted() for f in fr]), R.MAX_REASS),
           ("small", R.Batch([f for _, fr, _ in R.crafted_small_max() for f in fr]), R.SMALL_MAX),
           ("round_trip", R.Batch(R.round_trip_batch(oracle)[0]), R.MAX_REASS),
           ("collide", R.Batch(R.colliding_batch()[0]), R.MAX_REASS),
           ("align", R.Batch(R.alignment_batch()), R.MAX_REASS)]
    big, over, tiny = R.big_datagrams(oracle)
    fr = big + over + tiny
    out.append(("big", R.Batch([fr[int(p)] for p in rng.permutation(len(fr))]), R.MAX_REASS))
    return out


def test_the_hole_algorithm_completes_what_the_model_completes(oracle):
    """Fed every batch in batch order, the restated reassembleIp4 returns true for every group
    the declarative model completes, at the arrival of the group's last-arriving fragment and
    with byte-identical payload; the frame oracle, given the linearised datagram, agrees with the
    datagram verdict (it knows no TRUNCATED: it then verifies the UDP length's bytes)."""
    seen = lin = 0
    for name, batch, max_reass in _batches(oracle):
        e = R.model(oracle, batch, max_reass)
        hole = R.feed_batch(batch, e, max_reass)
        for key, order in e.complete.items():
            assert hole.get(key) == [(max(order), e.body[key])], (name, key)
            assert [e.frags[i]["off"] for i in order] == sorted(e.frags[i]["off"] for i in order)
            f = R.linearised(batch, e, key)
            v = int(e.dgram[order[0]]["verdict"])
            if f is not None:
                arr = np.frombuffer(f, dtype=np.uint8).copy()
                ov = int(oracle.rx_verify_batch(arr, [0, arr.size])[0])
                assert ov == v or (v == R.TRUNCATED and ov in (R.ACCEPT, R.L4_CHKSUM)), (name, key, v, ov)
                lin += 1
            seen += 1
        for key, members in e.groups.items():                     # left whole
            if key not in e.complete:
                assert all(e.verdict[i] in (R.FRAGMENT, R.DROP_FRAG) and e.next[i] == R.NONE
                           and e.head[i] == R.NONE for i in members)
    assert seen >= 150 and lin >= 150


def test_crafted_groups_take_their_branches(oracle):
    names = set()
    for groups, max_reass in ((R.crafted(), R.MAX_REASS), (R.crafted_small_max(), R.SMALL_MAX)):
        for name, frames, what in groups:
            e = R.model(oracle, R.Batch(frames), max_reass)
            heads = np.nonzero(e.dgram["n_frags"])[0]
            assert (int(e.dgram[heads[0]]["verdict"]) if heads.size else None) == what, name
            names.add(name)
    assert len(names) >= 35
    e = R.model(oracle, R.Batch(next(fr for nm, fr, _ in R.crafted() if nm == "ends_past_max")))
    assert (e.verdict == R.DROP_FRAG).sum() == 1 and not e.complete
    e = R.model(oracle, R.Batch(next(fr for nm, fr, _ in R.crafted() if nm == "empty_fragment")))
    assert (e.verdict == R.DROP_FRAG).sum() == 1 and len(e.complete) == 1


def test_hole_algorithm_corners():
    """What the restatement does by itself: duplicates are accepted, a hole below 4 bytes and a
    second last fragment with another end invalidate, MaxReassHoles bounds the holes."""
    h = R.HoleReassembler(1000)
    k = (1, 2, 3, 17)
    assert h.feed(k, True, 0, b"a" * 8) is None and h.feed(k, True, 0, b"a" * 8) is None
    assert h.feed(k, False, 8, b"b" * 3) == b"a" * 8 + b"b" * 3
    assert h.feed(k, True, 0, b"a" * 6) is None and h.feed(k, False, 8, b"b") is None   # hole of 2
    assert k not in h.entries
    assert h.feed(k, False, 8, b"b" * 4) is None and h.feed(k, False, 8, b"b" * 5) is None
    assert k not in h.entries
    assert h.feed(k, False, 1000, b"x") is None and k not in h.entries                  # oversize
    assert h.feed(k, True, 0, b"") is None and k not in h.entries                       # empty
    h = R.HoleReassembler(1000, max_holes=2)
    assert h.feed(k, True, 16, b"a" * 8) is None and k in h.entries
    assert h.feed(k, True, 48, b"a" * 8) is None and k not in h.entries                 # three holes


# ---- the hole model against the reference ------------------------------------------------------

def test_hole_model_equals_the_recorded_reference_answers():
    """tests/golden/ip_reass_ref_cases.json, recorded from the reference's own reassembleIp4
    (ip_reass_ref_gen.cpp: IpReassembly.h alone on a stub platform): call by call, the restatement
    returns a datagram exactly when the reference does, of the same length and bytes (duplicates
    with other bytes show which copy stays), under every MaxReassSize / MaxReassHoles recorded."""
    seqs = ip_reass_ref.load()
    calls = done = 0
    cfgs = set()
    for cfg, frs, res in seqs:
        size, holes = ip_reass_ref.CONFIGS[cfg]
        h = R.HoleReassembler(size, holes)
        cfgs.add(cfg)
        for (ident, src, dst, ttl, proto, mf, off, ln, salt), want in zip(frs, res):
            got = h.feed((src, dst, ident, proto), bool(mf), off, ip_reass_ref.payload(off, ln, salt))
            g = None if got is None else (len(got), ip_reass_ref.fnv(got))
            assert g == want, (cfg, ident, mf, off, ln, g, want)
            calls += 1
            done += want is not None
    assert len(seqs) >= 300 and calls >= 2500 and done >= 300 and cfgs == {0, 1, 2, 3}


def test_declarative_model_agrees_with_the_recorded_reference_answers(oracle):
    """The recorded sequences as frames: every group the declarative model completes, the
    reference completed at the group's last-arriving fragment with the same bytes."""
    seen = 0
    for cfg, frs, res in ip_reass_ref.load():
        size, holes = ip_reass_ref.CONFIGS[cfg]
        if holes < 250:
            continue          # the call knows no hole bound: that state is the host's
        frames = [R.ip_frame(src, dst, ident, proto, (0x2000 if mf else 0) | off // 8,
                             ip_reass_ref.payload(off, ln, salt), ttl=ttl)
                  for ident, src, dst, ttl, proto, mf, off, ln, salt in frs]
        if any(len(f) > 65535 for f in frames):
            continue
        batch = R.Batch(frames)
        e = R.model(oracle, batch, size)
        assert sorted(e.frags) == list(range(len(frs)))
        for key, order in e.complete.items():
            want = res[max(order)]
            assert want == (len(e.body[key]), ip_reass_ref.fnv(e.body[key])), (cfg, key)
            seen += 1
    assert seen >= 100


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "aipstack")),
                    reason="reference tree not present")
def test_generator_reproduces_the_fixture():
    with open(ip_reass_ref.FIXTURE) as f:
        assert ip_reass_ref.generate(REFERENCE) == f.read()


def test_fixture_is_small():
    assert os.path.getsize(ip_reass_ref.FIXTURE) < 256 * 1024


# ---- the shared text under ASan + UBSan, as a stand-alone program ---------------------------

def _table_test():
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "ipreass.mk"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(cpp, "build", "asan", "ipreass_table_test")


def test_shared_text_under_asan_ubsan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([_table_test()], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_the_models_hash_is_the_librarys():
    """The collisions of colliding_batch are crafted from the Python restatement of the hash; the
    stand-alone program prints the shared text's values for the same keys."""
    exe = _table_test()
    for src, dst, ident, proto, off in ((0x0A010203, 0x0A040506, 1, 47, 0), (1, 2, 65535, 253, 4088),
                                        (0xFFFFFFFF, 0, 77, 17, 65528)):
        r = subprocess.run([exe, "--hash", str(src), str(dst), str(ident), str(proto), str(off)],
                           capture_output=True, text=True, timeout=60, check=True)
        assert [int(x) for x in r.stdout.split()] == [R.hash_key(src, dst, ident, proto),
                                                      R.hash_key_off(src, dst, ident, proto, off)]
