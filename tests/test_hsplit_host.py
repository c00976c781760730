"""Header-split Tx fill, the parts that need no GPU: argument validation of
aipstack_chksum_tx_fill_hsplit (rejected before any HIP call), its workspace bound, the
split_frames host helper (split, then linearise back) and the Python wrapper's tensor checks."""
import ctypes

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import hsplit_cases as H


def _args(**over):
    """A well-formed argument list for n = 4 (host buffers standing in for device ones: a
    rejected call must return before touching them)."""
    lib = _lib.load()
    n = 4
    need = int(lib.aipstack_chksum_tx_fill_hsplit_workspace_bytes(n))
    bufs = {k: ctypes.create_string_buffer(512) for k in
            ("hdr", "hdr_len", "addr", "len", "index", "status")}
    ws = ctypes.create_string_buffer(need + 16)
    wsp = (ctypes.addressof(ws) + 7) & ~7
    a = dict(hdr=ctypes.addressof(bufs["hdr"]), stride=64, hdr_len=ctypes.addressof(bufs["hdr_len"]),
             addr=ctypes.addressof(bufs["addr"]), len=ctypes.addressof(bufs["len"]),
             index=ctypes.addressof(bufs["index"]), n=n, status=ctypes.addressof(bufs["status"]),
             ws=wsp, ws_bytes=need, flags=0, stream=None)
    a.update(over)
    if a["ws_bytes"] == "short":
        a["ws_bytes"] = need - 1
    if a["ws"] == "misaligned":
        a["ws"], a["ws_bytes"] = wsp + 4, need + 4
    keep = (bufs, ws)
    return lib, keep, [a[k] for k in ("hdr", "stride", "hdr_len", "addr", "len", "index", "n",
                                      "status", "ws", "ws_bytes", "flags", "stream")]


@pytest.mark.parametrize("over", [
    {"hdr": None}, {"hdr_len": None}, {"addr": None}, {"len": None}, {"index": None},
    {"status": None}, {"ws": None},
    {"stride": 0},
    {"n": (1 << 40) + 1, "ws_bytes": 1 << 62},
    {"ws_bytes": 0}, {"ws_bytes": "short"},
    {"ws": "misaligned"},
])
def test_einval_before_any_hip_call(over):
    lib, keep, args = _args(**over)
    assert lib.aipstack_chksum_tx_fill_hsplit(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_n_zero_is_a_noop():
    lib, keep, args = _args(n=0)
    assert lib.aipstack_chksum_tx_fill_hsplit(*args) == A.AIPSTACK_CHKSUM_OK
    lib, keep, args = _args(n=0, ws=None, ws_bytes=0)
    assert lib.aipstack_chksum_tx_fill_hsplit(*args) == A.AIPSTACK_CHKSUM_OK


def test_workspace_bound_and_monotonic():
    lib = _lib.load()
    f = lib.aipstack_chksum_tx_fill_hsplit_workspace_bytes
    assert f(0) == 0
    prev = 0
    for n in list(range(0, 70)) + [255, 256, 257, 4095, 4096, 1 << 20, (1 << 20) + 1, 1 << 40]:
        b = int(f(n))
        assert b % 8 == 0
        assert 10 * n <= b <= 16 * n + 256, n   # seeds 4n + records 4n + sums 2n fit
        assert b >= prev, n
        prev = b


def test_constants():
    assert A.AIPSTACK_TX_SPLIT_LAYOUT == 9
    assert A.AIPSTACK_CHKSUM_MAX_SPLIT_HEADER == 256


@pytest.mark.parametrize("stride", [128, 256])
@pytest.mark.parametrize("cls", H.SPLIT_CLASSES)
def test_split_frames_round_trip(cls, stride):
    frs = H.golden_frames()[:600]
    buf, off = H.pack(frs)
    at = H.split_points(frs, cls, stride)
    pieces = [(1, 3)] * len(frs) if cls == "l4_plus3" else None
    sp = A.split_frames(buf, off, at, hdr_stride=stride, payload_pieces=pieces,
                        payload_gap=1 if cls == "l4_plus1" else 0, reverse=cls == "tcp_opts")
    assert sp.headers.size == len(frs) * stride and sp.hdr_lens.dtype == np.uint32
    for i, fr in enumerate(frs):
        assert sp.hdr_lens[i] == max(0, min(at[i], len(fr), stride))
        assert sp.hdr_lens[i] + sum(l for _, l in sp.chunks[i]) == len(fr)
    back, boff = sp.linearise()
    assert np.array_equal(boff, off) and np.array_equal(back, buf[:int(off[-1])])
    addr, lens, index = sp.chunk_table(1000)
    assert index[-1] == addr.size == lens.size and index.size == len(frs) + 1
    assert all(a >= 1000 for a in addr)
    headers, hdr_lens, payload, chunks = sp
    assert headers is sp.headers and chunks is sp.chunks


def test_split_frames_pieces_gap_and_reverse():
    fr = np.arange(100, dtype=np.uint8)
    off = np.array([0, 40, 100], dtype=np.uint64)
    sp = A.split_frames(fr, off, [10, 20], hdr_stride=32, payload_pieces=[(1, 3), (7,)],
                        payload_gap=3, reverse=True)
    assert [l for _, l in sp.chunks[0]] == [1, 3, 26]
    assert [l for _, l in sp.chunks[1]] == [7, 33]
    # reverse memory order: later chunks lie at lower addresses
    flat = [o for seg in sp.chunks for o, _ in seg]
    assert flat == sorted(flat, reverse=True)
    back, boff = sp.linearise()
    assert np.array_equal(back, fr) and list(boff) == [0, 40, 100]


def test_wrapper_rejects_host_tensors():
    import torch
    hdr = torch.zeros(128, dtype=torch.uint8)
    ln = torch.zeros(2, dtype=torch.int32)
    addr = torch.zeros(2, dtype=torch.int64)
    cl = torch.zeros(2, dtype=torch.int32)
    idx = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError):
        A.tx_fill_header_split(hdr, 64, ln, addr, cl, idx)
