"""TCP burst segmentation, the parts that need no GPU: aipstack_tcp_burst_layout against the
model, the argument validation of aipstack_tcp_tx_segment (rejected before any HIP call), the
descriptor's layout, the model itself pinned against code compiled from the reference
(oracle/_ref/libref_chksum.so: the reference's own TCP Tx and IPv4 Tx checksum sequences) and
against the frame oracle's Rx verify, and the host code under ASan/UBSan as a stand-alone
program (tests/cpp/tcpseg_layout_test.cpp)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib
from conftest import ROOT

import call_sites
import tcpseg_cases as T

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libref_chksum.so")


def _generated(oracle):
    return [("sizes", T.sizes_batch()), ("ones65", T.one_segment_bursts(65)),
            ("zeros", T.zero_segment_batch()), ("boundary", T.boundary_batch()),
            ("psh", T.psh_batch()), ("zero_tcp", T.zero_tcp_checksum_batch(oracle)),
            ("zero_ip", T.zero_ip_checksum_batch(oracle))]


# ---- the descriptor ---------------------------------------------------------------------

class _CBurst(ctypes.Structure):
    _fields_ = [("data_addr", ctypes.c_uint64 * 2), ("data_len", ctypes.c_uint32 * 2),
                ("seq", ctypes.c_uint32), ("psh_offset", ctypes.c_uint32),
                ("mss", ctypes.c_uint16), ("ip_id", ctypes.c_uint16), ("flags", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 3), ("hdr", ctypes.c_uint8 * 56)]


def test_burst_dtype_matches_the_c_struct():
    assert A.TCP_BURST_DTYPE.itemsize == 96 == ctypes.sizeof(_CBurst)
    assert ctypes.alignment(_CBurst) == 8
    for name, _ in _CBurst._fields_:
        assert A.TCP_BURST_DTYPE.fields[name][1] == getattr(_CBurst, name).offset, name
    assert set(A.TCP_BURST_DTYPE.names) == {n for n, _ in _CBurst._fields_}


def test_constants():
    assert A.AIPSTACK_TCP_SEGMENT_HEADER == 54
    assert A.AIPSTACK_TCP_BURST_FIN == 1
    assert A.AIPSTACK_TX_BURST_INVALID == 10
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for line in ("#define AIPSTACK_TCP_SEGMENT_HEADER 54u", "#define AIPSTACK_TCP_BURST_FIN 1u",
                 "#define AIPSTACK_TX_BURST_INVALID 10"):
        assert line in text


# ---- layout -------------------------------------------------------------------------------

def test_layout_matches_the_model(oracle):
    for name, batch in _generated(oracle):
        want = T.model_layout(batch.cases)
        assert want is not None, name
        si, cb = A.tcp_burst_layout(T.descriptors(batch, 1 << 20, A.TCP_BURST_DTYPE))
        assert np.array_equal(si, want[0]) and np.array_equal(cb, want[1]), name
        assert si[-1] > 0
    # the shapes are there: 200 segments in one burst, two-chunk segments, FIN-only segments
    si, cb = A.tcp_burst_layout(T.descriptors(T.sizes_batch(), 0, A.TCP_BURST_DTYPE))
    assert 200 in np.diff(si.astype(np.int64))
    si, cb = A.tcp_burst_layout(T.descriptors(T.boundary_batch(), 0, A.TCP_BURST_DTYPE))
    extra = np.diff(cb.astype(np.int64)) - np.diff(si.astype(np.int64))
    assert set(extra) == {0, 1} and (extra == 1).sum() > 100 and (extra == 0).sum() >= 4


def test_layout_of_nothing():
    si, cb = A.tcp_burst_layout(np.zeros(0, dtype=A.TCP_BURST_DTYPE))
    assert list(si) == [0] and list(cb) == [0]


@pytest.mark.parametrize("cls", T.INVALID_CLASSES)
@pytest.mark.parametrize("where", [0, 1, 2])
def test_layout_rejects_every_invalid_class(cls, where):
    cases = [T.burst((1, 3000)), T.burst((5, 10), flags=T.FIN)]
    assert T.model_layout(cases) is not None
    cases.insert(where, T.invalid_case(cls))
    assert T.model_layout(cases) is None
    with pytest.raises(A.ChksumError) as e:
        A.tcp_burst_layout(T.descriptors(T.Batch(cases, None), 0, A.TCP_BURST_DTYPE))
    assert e.value.status == A.AIPSTACK_CHKSUM_EINVAL


def test_layout_null_pointers():
    lib = _lib.load()
    out = np.zeros(4, dtype=np.uint64)
    d = T.descriptors(T.Batch([T.burst((1, 10))], None), 0, A.TCP_BURST_DTYPE)
    f = lib.aipstack_tcp_burst_layout
    assert f(d.ctypes.data, 1, out.ctypes.data, out.ctypes.data) == A.AIPSTACK_CHKSUM_OK
    assert f(None, 1, out.ctypes.data, out.ctypes.data) == A.AIPSTACK_CHKSUM_EINVAL
    assert f(d.ctypes.data, 1, None, out.ctypes.data) == A.AIPSTACK_CHKSUM_EINVAL
    assert f(d.ctypes.data, 1, out.ctypes.data, None) == A.AIPSTACK_CHKSUM_EINVAL


# ---- argument validation of the batch call ----------------------------------------------

_NAMES = ("bursts", "seg_index", "chunk_base", "n_bursts", "n_segments", "n_chunks", "hdr",
          "stride", "chunk_addr", "chunk_len", "chunk_index", "status", "ws", "ws_bytes", "flags",
          "stream")


def _args(**over):
    """A well-formed argument list for 4 segments (host buffers standing in for device ones: a
    rejected call must return before touching them)."""
    lib = _lib.load()
    n = 4
    need = int(lib.aipstack_tcp_tx_segment_workspace_bytes(n))
    bufs = {k: ctypes.create_string_buffer(512) for k in
            ("bursts", "seg_index", "chunk_base", "hdr", "chunk_addr", "chunk_len", "chunk_index",
             "status")}
    ws = ctypes.create_string_buffer(need + 16)
    wsp = (ctypes.addressof(ws) + 7) & ~7
    a = {k: ctypes.addressof(v) for k, v in bufs.items()}
    a.update(n_bursts=1, n_segments=n, n_chunks=4, stride=64, ws=wsp, ws_bytes=need, flags=0,
             stream=None)
    a.update(over)
    if a["ws_bytes"] == "short":
        a["ws_bytes"] = need - 1
    if a["ws"] == "misaligned":
        a["ws"], a["ws_bytes"] = wsp + 4, need + 4
    return lib, (bufs, ws), [a[k] for k in _NAMES]


@pytest.mark.parametrize("over", [
    {"bursts": None}, {"seg_index": None}, {"chunk_base": None}, {"hdr": None},
    {"chunk_addr": None}, {"chunk_len": None}, {"chunk_index": None}, {"status": None},
    {"ws": None},
    {"stride": 53}, {"stride": 0},
    {"n_segments": (1 << 40) + 1, "ws_bytes": 1 << 62},
    {"n_chunks": (1 << 40) + 1},
    {"ws_bytes": 0}, {"ws_bytes": "short"},
    {"ws": "misaligned"},
])
def test_einval_before_any_hip_call(over):
    lib, keep, args = _args(**over)
    assert lib.aipstack_tcp_tx_segment(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_no_segments_is_a_noop():
    lib, keep, args = _args(n_segments=0)
    assert lib.aipstack_tcp_tx_segment(*args) == A.AIPSTACK_CHKSUM_OK
    lib, keep, args = _args(n_segments=0, ws=None, ws_bytes=0, hdr=None)
    assert lib.aipstack_tcp_tx_segment(*args) == A.AIPSTACK_CHKSUM_OK


def test_workspace_bound_and_monotonic():
    f = _lib.load().aipstack_tcp_tx_segment_workspace_bytes
    assert f(0) == 0
    prev = 0
    for n in list(range(0, 70)) + [255, 256, 257, 4095, 4096, 1 << 20, (1 << 20) + 1, 1 << 40]:
        b = int(f(n))
        assert b % 8 == 0 and 14 * n <= b <= 16 * n + 256 and b >= prev, n
        prev = b


def test_wrapper_rejects_bad_arguments():
    torch = pytest.importorskip("torch")
    b = T.descriptors(T.Batch([T.burst((1, 10))], None), 0, A.TCP_BURST_DTYPE)
    si, cb = A.tcp_burst_layout(b)
    with pytest.raises(ValueError):
        A.tcp_tx_segment(b, si[:-1], cb)
    with pytest.raises(ValueError):   # device index tensors need the counts; host tensors are not device ones
        A.tcp_tx_segment(torch.zeros(96, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64),
                         torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        A.tcp_tx_segment(torch.zeros(96, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64),
                         torch.zeros(2, dtype=torch.int64), n_segments=1, n_chunks=1)


# ---- the model against the reference ----------------------------------------------------

def _fields(c):
    h = c["hdr"]
    src, dst = struct.unpack_from(">II", h, 26)
    sport, dport = struct.unpack_from(">HH", h, 34)
    ack, = struct.unpack_from(">I", h, 42)
    window, = struct.unpack_from(">H", h, 48)
    frag, ttl, proto = struct.unpack_from(">HBB", h, 20)
    return src, dst, sport, dport, ack, window, frag, ttl, proto


@pytest.mark.skipif(not os.path.exists(REF_LIB), reason="reference library not built here")
def test_model_checksums_equal_the_reference_call_sites(oracle):
    """Every segment of the generated cases: the model's TCP checksum is what the reference's
    prepareCommon + sendSegment sequence computes (ref_cs_tcp_tx), its IPv4 header checksum what
    prepareSendIp4Dgram + sendIp4DgramFast compute (ref_cs_ip4_tx), from the burst's ports, ack,
    window, addresses, seq, offset/flags, ident and the data chunks."""
    ref = ctypes.CDLL(REF_LIB)
    n = 0
    for name, batch in _generated(oracle):
        e = T.expected(oracle, batch)
        assert (e.status == T.ACCEPT).all(), name
        for i in range(len(e.status)):
            c = batch.cases[e.seg_case[i]]
            src, dst, sport, dport, ack, window, frag, ttl, proto = _fields(c)
            h = e.headers[i].tobytes()
            seq, = struct.unpack_from(">I", h, 38)
            fl, = struct.unpack_from(">H", h, 46)
            tot, ident = struct.unpack_from(">HH", h, 16)
            chunks = [[int(o), int(l)] for o, l in e.seg_chunks[i]]
            ln = sum(l for _, l in chunks)
            assert tot == 40 + ln and fl == e.seg_flags[i]
            got = call_sites.evaluate(ref, "ref", {
                "site": "tcp_tx", "args": [sport, dport, ack, window, src, dst, seq, fl], "hdr": "",
                "chunks": chunks, "offset": 0, "tot_len": ln}, batch.payload)
            assert got[0] == struct.unpack_from(">H", h, 50)[0], (name, i)
            got = call_sites.evaluate(ref, "ref", {
                "site": "ip4_tx", "args": [frag, ttl, proto, src, dst, tot, ident], "hdr": "",
                "chunks": [], "offset": 0, "tot_len": 0}, batch.payload)
            assert got[0] == struct.unpack_from(">H", h, 24)[0], (name, i)
            n += 1
    assert n > 1000


def test_model_frames_pass_rx_verify(oracle):
    for name, batch in _generated(oracle) + [("invalid", T.invalid_batch()),
                                             ("mismatch", T.mismatch_batch())]:
        e = T.expected(oracle, batch)
        buf, off, ids = T.linearise(e, batch.payload)
        assert len(ids) > 0
        v = oracle.rx_verify_batch(buf, off)
        assert (v == T.ACCEPT).all(), (name, np.nonzero(v != T.ACCEPT)[0][:8])


def test_generated_batches_contain_their_classes(oracle):
    """Not vacuous, from the model alone (the GPU tests compare against these batches)."""
    e = T.expected(oracle, T.boundary_batch())
    assert T.count_straddle_odd_first(e) >= 1
    even = sum(1 for ch in e.seg_chunks if len(ch) == 2 and not ch[0][1] & 1)
    assert even >= 1 and sum(1 for ch in e.seg_chunks if len(ch) == 1) >= 1
    b = T.boundary_batch()
    assert any(c["pieces"][0][1] == 0 for c in b.cases) and any(c["pieces"][1][1] == 0 for c in b.cases)
    assert any(c["pieces"][0][1] % c["mss"] == 0 and c["pieces"][0][1] and c["pieces"][1][1]
               for c in b.cases)                                            # boundary on an edge
    assert any((c["pieces"][0][0] & 1) for c in b.cases) and any((c["pieces"][1][0] & 1) for c in b.cases)
    f = T.count_flags(T.expected(oracle, T.psh_batch()))
    assert f["psh_only"] >= 3 and f["fin_psh"] >= 3 and f["neither"] >= 3, f
    f = T.count_flags(T.expected(oracle, T.sizes_batch()))
    assert f["fin_psh"] == 3 and f["psh_only"] >= 1
    e = T.expected(oracle, T.sizes_batch())
    assert any(len(ch) == 0 for ch, s in zip(e.seg_chunks, e.status) if s == T.ACCEPT)   # FIN only
    ids = e.headers[:, 18].astype(int) << 8 | e.headers[:, 19]
    assert {0xFFFE, 0xFFFF, 0x0000} <= set(ids.tolist())                                 # ident wraps
    seqs = [struct.unpack_from(">I", h.tobytes(), 38)[0] for h in e.headers]
    assert 0xFFFFFF00 in seqs and (0xFFFFFF00 + 1460) & 0xFFFFFFFF in seqs              # seq wraps
    e = T.expected(oracle, T.zero_tcp_checksum_batch(oracle))
    tcp = e.headers[:, 50].astype(int) << 8 | e.headers[:, 51]
    assert (tcp == 0).sum() == 3 and (tcp == 0xFFFF).sum() == 0
    e = T.expected(oracle, T.zero_ip_checksum_batch(oracle))
    ip = e.headers[:, 24].astype(int) << 8 | e.headers[:, 25]
    assert (ip == 0).sum() == 3 and (ip == 0xFFFF).sum() == 0
    e = T.expected(oracle, T.invalid_batch())
    assert (e.status == T.BURST_INVALID).sum() == 2 * len(T.INVALID_CLASSES)
    assert (e.status == T.ACCEPT).sum() >= 2 * len(T.INVALID_CLASSES)
    e = T.expected(oracle, T.mismatch_batch())
    assert (e.status == T.BURST_INVALID).sum() == 2 + 5 + 3 + 3 and (e.status == T.ACCEPT).sum() == 6 * 4
    si, _ = T.caller_index(T.zero_segment_batch().cases)
    d = np.diff(si.astype(np.int64))
    assert d[0] == 0 and d[-1] == 0 and (d == 0).sum() >= 70 and (d > 0).sum() >= 40


# ---- the host code under ASan + UBSan, as a stand-alone program -------------------------

def test_host_code_under_asan_ubsan():
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "tcpseg.mk"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "tcpseg_layout_test")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
