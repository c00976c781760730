"""UDP send with IPv4 fragmentation, the parts that need no GPU: aipstack_udp_dgram_layout against
the model, the argument validation of aipstack_udp_tx_fragment (rejected before any HIP call), the
descriptor's layout, properties of the model that do not rest on restating the loop (reassembly,
offsets, MF, sizes, the frame oracle's Rx verify and Tx fill), the model pinned against answers
recorded from code compiled from the reference (tests/golden/ip_frag_ref_cases.json), and the host
code under ASan/UBSan as a stand-alone program (tests/cpp/ipfrag_layout_test.cpp)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib
from conftest import ROOT

import ip_frag_ref
import ipfrag_cases as T


def _layout(cases):
    return A.udp_dgram_layout(T.descriptors(T.Batch(cases, None), 1 << 20, A.UDP_DGRAM_DTYPE))


# ---- the descriptor ---------------------------------------------------------------------

class _CDgram(ctypes.Structure):
    _fields_ = [("data_addr", ctypes.c_uint64 * 2), ("data_len", ctypes.c_uint32 * 2),
                ("mtu", ctypes.c_uint16), ("ip_id", ctypes.c_uint16), ("reserved", ctypes.c_uint32),
                ("hdr", ctypes.c_uint8 * 48)]


def test_dgram_dtype_matches_the_c_struct():
    assert A.UDP_DGRAM_DTYPE.itemsize == 80 == ctypes.sizeof(_CDgram)
    assert ctypes.alignment(_CDgram) == 8
    for name, _ in _CDgram._fields_:
        assert A.UDP_DGRAM_DTYPE.fields[name][1] == getattr(_CDgram, name).offset, name
    assert set(A.UDP_DGRAM_DTYPE.names) == {n for n, _ in _CDgram._fields_}


def test_constants():
    assert (A.AIPSTACK_TX_FRAG_NEEDED, A.AIPSTACK_TX_DGRAM_INVALID) == (12, 13)
    assert (A.AIPSTACK_UDP_FIRST_FRAGMENT_HEADER, A.AIPSTACK_UDP_NEXT_FRAGMENT_HEADER) == (42, 34)
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for line in ("#define AIPSTACK_TX_FRAG_NEEDED   12", "#define AIPSTACK_TX_DGRAM_INVALID 13",
                 "#define AIPSTACK_UDP_FIRST_FRAGMENT_HEADER 42u", "#define AIPSTACK_UDP_MIN_MTU 256u",
                 "#define AIPSTACK_CHKSUM_ABI_VERSION 1"):
        assert line in text


# ---- layout -------------------------------------------------------------------------------

def _check_layout(cases, name=""):
    want = T.model_layout(cases)
    assert want is not None, name
    got = _layout(cases)
    for w, g in zip(want, got):
        assert np.array_equal(w, g), (name, w[:12], g[:12])
    return got


@pytest.mark.parametrize("mtu", [256, 576, 1006, 1500, 9000, 257, 263, 65535])
def test_layout_boundaries_of_the_sizes(mtu):
    """P = M, M + 1, M + F, M + F + 1 (1, 2, 2, 3 fragments when M % 8 == 0; the last fragment of
    F + 1 ... M bytes when it is not), D = 0."""
    M, F = mtu - 20, ((mtu - 20) // 8) * 8
    cases = [T.dgram((5, P - 8), mtu=mtu) for P in (8, M, M + 1, M + F, M + F + 1, M + 2 * F, M + 2 * F + 1)
             if P <= 65535]
    fi, _, st = _check_layout(cases, mtu)
    S = np.diff(fi.astype(np.int64)).tolist()
    assert S == [1, 1, 2, 2, 3, 3, 4][:len(S)] and (st == T.ACCEPT).all()
    if M % 8:
        c = T.dgram((5, M + F - 8), mtu=mtu)                  # last fragment of M > F bytes
        assert [ln for _, ln, _ in T.ip_packets_of(c)] == [F, M]


def test_layout_largest_datagram_on_the_smallest_mtu():
    fi, cb, _ = _check_layout([T.dgram((1, 65527), mtu=256), T.dgram((0, 0), mtu=256)])
    assert fi.tolist() == [0, 283, 284] and cb.tolist() == [0, 283, 283]
    pk = T.ip_packets_of(T.dgram((1, 65527), mtu=256))
    assert pk[-1][0] // 8 == 8178 < 1 << 13 and sum(ln for _, ln, _ in pk) == 65535


@pytest.mark.parametrize("mtu", [256, 1006, 1500])
def test_layout_piece_boundaries(mtu):
    M, F = mtu - 20, ((mtu - 20) // 8) * 8
    D = M + 2 * F + 3 - 8
    cases = [T.dgram((1, l0), (70000, D - l0), mtu=mtu)
             for l0 in (0, 1, F - 9, F - 8, F - 7, 2 * F - 9, 2 * F - 8, 2 * F - 7, D - 1, D)]
    fi, cb, _ = _check_layout(cases, mtu)
    extra = (np.diff(cb.astype(np.int64)) - np.diff(fi.astype(np.int64))).tolist()
    assert extra == [0, 1, 1, 0, 1, 1, 0, 1, 1, 0]            # on a fragment edge: no straddle
    if M % 8 >= 2:                                            # the clamp: (len0 + 8) // F == S
        for S in (2, 3, 7):
            c = T.clamp_case(mtu, S=S, back=1)
            assert T.counts_of(c) == (S, S + 1) and len(T.fragments_of(c)[-1][3]) == 2
            _check_layout([c, T.dgram((1, 10))], (mtu, S))


def test_layout_df_with_and_without_need():
    cases = [T.dgram((7, 1472), df=True), T.dgram((7, 1473), df=True), T.dgram((7, 1473)),
             T.dgram((7, 65527), mtu=256, df=True), T.dgram((0, 0), mtu=256, df=True)]
    fi, cb, st = _check_layout(cases)
    assert np.diff(fi.astype(np.int64)).tolist() == [1, 0, 2, 0, 1]
    assert st.tolist() == [T.ACCEPT, T.FRAG_NEEDED, T.ACCEPT, T.FRAG_NEEDED, T.ACCEPT]


def test_layout_of_generated_batches(oracle):
    for name, b in (("boundary", T.boundary_batch()), ("spanning", T.spanning_batch()),
                    ("zero_udp", T.zero_udp_checksum_batch(oracle))):
        _check_layout(b.cases, name)
    fi, cb, st = _layout([])
    assert list(fi) == [0] and list(cb) == [0] and st.size == 0


@pytest.mark.parametrize("cls", T.INVALID_CLASSES)
@pytest.mark.parametrize("where", [0, 1, 2])
def test_layout_rejects_every_contract_breach(cls, where):
    cases = [T.dgram((1, 3000)), T.dgram((5, 10), df=True)]
    assert T.model_layout(cases) is not None
    cases.insert(where, T.invalid_case(cls))
    assert T.model_layout(cases) is None
    with pytest.raises(A.ChksumError) as e:
        _layout(cases)
    assert e.value.status == A.AIPSTACK_CHKSUM_EINVAL


def test_layout_null_pointers():
    lib = _lib.load()
    out = np.zeros(4, dtype=np.uint64)
    st = np.zeros(4, dtype=np.uint8)
    d = T.descriptors(T.Batch([T.dgram((1, 10))], None), 0, A.UDP_DGRAM_DTYPE)
    f = lib.aipstack_udp_dgram_layout
    o = out.ctypes.data
    assert f(d.ctypes.data, 1, o, o, st.ctypes.data) == A.AIPSTACK_CHKSUM_OK and st[0] == T.ACCEPT
    assert f(d.ctypes.data, 1, o, o, None) == A.AIPSTACK_CHKSUM_OK       # the status is optional
    assert f(None, 1, o, o, None) == A.AIPSTACK_CHKSUM_EINVAL
    assert f(d.ctypes.data, 1, None, o, None) == A.AIPSTACK_CHKSUM_EINVAL
    assert f(d.ctypes.data, 1, o, None, None) == A.AIPSTACK_CHKSUM_EINVAL
    assert f(d.ctypes.data, (1 << 40) + 1, o, o, None) == A.AIPSTACK_CHKSUM_EINVAL


# ---- argument validation of the batch call ----------------------------------------------

_NAMES = ("dgrams", "frag_index", "chunk_base", "n_dgrams", "n_frags", "n_chunks", "hdr", "stride",
          "hdr_len", "chunk_addr", "chunk_len", "chunk_index", "status", "dgram_status", "ws",
          "ws_bytes", "flags", "stream")
_POINTERS = ("dgrams", "frag_index", "chunk_base", "hdr", "hdr_len", "chunk_addr", "chunk_len",
             "chunk_index", "status", "dgram_status")


def _args(**over):
    """A well-formed argument list for 4 fragments of 2 datagrams (host buffers standing in for
    device ones: a rejected call must return before touching them)."""
    lib = _lib.load()
    n, nd = 4, 2
    need = int(lib.aipstack_udp_tx_fragment_workspace_bytes(nd, n))
    bufs = {k: ctypes.create_string_buffer(512) for k in _POINTERS}
    ws = ctypes.create_string_buffer(need + 16)
    wsp = (ctypes.addressof(ws) + 7) & ~7
    a = {k: ctypes.addressof(v) for k, v in bufs.items()}
    a.update(n_dgrams=nd, n_frags=n, n_chunks=4, stride=64, ws=wsp, ws_bytes=need, flags=0, stream=None)
    a.update(over)
    if a["ws_bytes"] == "short":
        a["ws_bytes"] = need - 1
    if a["ws"] == "misaligned":
        a["ws"], a["ws_bytes"] = wsp + 4, need + 4
    return lib, (bufs, ws), [a[k] for k in _NAMES]


@pytest.mark.parametrize("over", [{k: None} for k in _POINTERS] + [
    {"ws": None}, {"stride": 41}, {"stride": 0},
    {"n_frags": (1 << 40) + 1, "ws_bytes": 1 << 62},
    {"n_chunks": (1 << 40) + 1},
    {"n_dgrams": (1 << 40) + 1, "ws_bytes": 1 << 62},
    {"ws_bytes": 0}, {"ws_bytes": "short"}, {"ws": "misaligned"},
])
def test_einval_before_any_hip_call(over):
    lib, keep, args = _args(**over)
    assert lib.aipstack_udp_tx_fragment(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_no_fragments_is_a_noop():
    lib, keep, args = _args(n_frags=0)
    assert lib.aipstack_udp_tx_fragment(*args) == A.AIPSTACK_CHKSUM_OK
    lib, keep, args = _args(n_frags=0, ws=None, ws_bytes=0, hdr=None)
    assert lib.aipstack_udp_tx_fragment(*args) == A.AIPSTACK_CHKSUM_OK


def test_workspace_bound_and_monotonic():
    f = _lib.load().aipstack_udp_tx_fragment_workspace_bytes
    for nd in (0, 1, 7, 1 << 10, 1 << 40):
        prev = 0
        for n in list(range(0, 70)) + [255, 256, 257, 4096, 1 << 20, (1 << 20) + 1, 1 << 40]:
            b = int(f(nd, n))
            assert b % 8 == 0 and 8 * n + 14 * nd + 8 <= b <= 16 * (n + nd) + 256 and b >= prev, (nd, n)
            prev = b
    assert int(f(1 << 50, 1 << 50)) == int(f(1 << 40, 1 << 40))


def test_wrapper_rejects_bad_arguments():
    torch = pytest.importorskip("torch")
    g = T.descriptors(T.Batch([T.dgram((1, 10))], None), 0, A.UDP_DGRAM_DTYPE)
    fi, cb, _ = A.udp_dgram_layout(g)
    with pytest.raises(ValueError):
        A.udp_tx_fragment(g, fi[:-1], cb)
    with pytest.raises(ValueError):   # device index tensors need the counts; host tensors are not device ones
        A.udp_tx_fragment(torch.zeros(80, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64),
                          torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        A.udp_tx_fragment(torch.zeros(80, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64),
                          torch.zeros(2, dtype=torch.int64), n_frags=1, n_chunks=1)


# ---- properties of the model that do not rest on restating the loop -------------------------

def _property_batches(oracle):
    import random_ipfrag_cases as G
    out = [("boundary", T.boundary_batch()), ("zero_udp", T.zero_udp_checksum_batch(oracle))]
    out += [("seed%d" % s, G.scenario(oracle, s).batch) for s in (0, 1, 2, 5, 8)]
    return out


def test_model_fragments_reassemble_and_verify(oracle):
    """A few hundred datagrams: the fragments, put together by their offset fields, give back the
    UDP header and payload byte for byte; offsets are multiples of 8; only the last fragment lacks
    MF; no fragment exceeds the mtu; every fragment but the last carries F bytes; every linearised
    fragment is FRAGMENT (IPv4 header checksum good) or, alone, ACCEPT for the frame oracle's Rx
    verify; the reassembled datagram is ACCEPT (UDP checksum good); for S = 1 the frame is what the
    oracle's Tx fill leaves on it with both fields zeroed."""
    seen = ones = 0
    for name, batch in _property_batches(oracle):
        e = T.expected(oracle, batch)
        buf, off, ids = T.linearise(e, batch.payload)
        v = oracle.rx_verify_batch(buf, off)
        verdict = dict(zip(ids, v.tolist()))
        for d, c in enumerate(batch.cases):
            if e.dgram_status[d] != T.ACCEPT:
                continue
            mine = [int(i) for i in np.nonzero(e.frag_case == d)[0]]
            S = len(mine)
            M, F = c["mtu"] - 20, ((c["mtu"] - 20) // 8) * 8
            body = b""
            for k, i in enumerate(mine):
                f = T.frame_of(e, batch.payload, i)
                tot, ident, fo = struct.unpack_from(">HHH", f, 16)
                assert ident == c["ip_id"] and tot == len(f) - 14 <= c["mtu"], (name, d, k)
                assert (fo & 0x1FFF) * 8 == len(body) and bool(fo & 0x2000) == (k < S - 1)
                assert (fo & 0x4000) == (c["hdr"][20] << 8 & 0x4000) and not fo & 0x8000
                assert k == S - 1 or tot - 20 == F
                assert verdict[i] == (T.ACCEPT if S == 1 else 3), (name, d, k, verdict[i])
                body += f[34:]
            (o0, l0), (o1, l1) = c["pieces"]
            data = batch.payload[o0:o0 + l0].tobytes() + batch.payload[o1:o1 + l1].tobytes()
            assert body[8:] == data and body[:4] == c["hdr"][34:38]
            assert struct.unpack_from(">H", body, 4)[0] == len(body) == 8 + len(data)
            if 34 + len(body) <= 65535:
                whole = np.frombuffer(T.reassemble(e, batch.payload, d), dtype=np.uint8).copy()
                assert oracle.rx_verify_batch(whole, [0, whole.size])[0] == T.ACCEPT, (name, d)
            if S == 1:
                frame = np.frombuffer(T.frame_of(e, batch.payload, mine[0]), dtype=np.uint8).copy()
                zeroed = frame.copy()
                zeroed[24:26] = 0
                zeroed[40:42] = 0
                assert oracle.tx_fill_batch(zeroed, [0, zeroed.size])[0] == T.ACCEPT
                assert np.array_equal(zeroed, frame), (name, d)
                ones += 1
            seen += 1
    assert seen >= 300 and ones >= 50


def test_model_corners(oracle):
    # the UDP sum comes out 0: the field is 0xFFFF
    b = T.zero_udp_checksum_batch(oracle)
    e = T.expected(oracle, b)
    first = e.hdr_len == T.HDR0
    udp = e.headers[:, 40].astype(int) << 8 | e.headers[:, 41]
    assert (udp[first] == 0xFFFF).sum() == 4 and (udp == 0)[first].sum() == 0
    assert "0xFFFF" in T.branches(b, e)
    # all-zero addresses, zero ports, D = 0: the sum is 17 + 8 + 8
    c = T.dgram((0, 0), src=0, dst=0, sport=0, dport=0)
    e = T.expected(oracle, T.Batch([c], T.payload_bytes()))
    assert e.headers[0, 38:42].tobytes() == struct.pack(">HH", 8, ~33 & 0xFFFF)
    assert T.branches(T.boundary_batch()) >= {"S=0", "S=1", "S>64", "straddle", "no_straddle",
                                              "edge", "clamped", "last>F"}


def test_invalid_and_mismatch_batches_contain_their_classes(oracle):
    e = T.expected(oracle, T.invalid_batch())
    assert (e.status == T.DGRAM_INVALID).sum() == 2 * len(T.INVALID_CLASSES)
    assert all(not T.descriptor_ok(T.invalid_case(c)) for c in T.INVALID_CLASSES)
    e = T.expected(oracle, T.mismatch_batch())
    assert (e.dgram_status == T.DGRAM_INVALID).sum() == 6 and (e.status == T.ACCEPT).sum() == 21


# ---- the model against the reference ----------------------------------------------------

def test_model_equals_the_recorded_reference_answers(oracle):
    """tests/golden/ip_frag_ref_cases.json, recorded from the reference's own Ip4RoundFragLen,
    IpChksum and IpChksumAccumulator (ip_frag_ref_gen.cpp): the model's rounding, its fragment
    header checksums and its UDP checksum agree with all of it."""
    rnd, hdrs, udps = ip_frag_ref.load()
    assert len(rnd) >= 250 and len(hdrs) >= 300 and len(udps) >= 300
    assert {m % 8 for m, _ in rnd} == set(range(8)) and {256, 65535} <= {m for m, _ in rnd}
    for mtu, want in rnd:
        assert T.round_frag_len(20, mtu) == want, mtu
        c = T.dgram((0, 65527), mtu=mtu)
        assert T.ip_packets_of(c)[0][1] == want - 20
    pay = T.payload_bytes()
    for h, want in hdrs:
        # the header as the model builds a fragment's: template fields from h, the rest written
        tot, ident, fo, ttl, proto = struct.unpack_from(">HHHBB", h, 2)
        arr = np.frombuffer(h, dtype=np.uint8).copy()
        assert oracle.final(arr, 0, 20) == want
        if h[0] == 0x45 and proto == 17 and tot >= 28 and fo & 0x2000 and (fo & 0x1FFF) == 0:
            c = T.dgram((0, 65527), mtu=max(256, tot), ip_id=ident, ttl=ttl, dscp=h[1],
                        src=struct.unpack_from(">I", h, 12)[0], dst=struct.unpack_from(">I", h, 16)[0])
            if T.ip_packets_of(c)[0][1] == tot - 20:
                got = T.fragment_header(oracle, c, 0, tot - 20, True, 0)
                assert got[14:24] == h[:10] and struct.unpack_from(">H", got, 24)[0] == want
    for src, dst, sport, dport, p, want in udps:
        buf = pay.copy()
        buf[:len(p)] = np.frombuffer(p, dtype=np.uint8)
        c = T.dgram((0, len(p)), src=src, dst=dst, sport=sport, dport=dport)
        assert T.udp_checksum(oracle, c, buf) == want, (src, dst, sport, dport, len(p))


# ---- the host code under ASan + UBSan, as a stand-alone program -------------------------

def test_host_code_under_asan_ubsan():
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "ipfrag.mk"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "ipfrag_layout_test")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
