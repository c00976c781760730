"""TCP Rx parse, the parts that need no GPU: the model of tcprx_cases.py pinned against answers
recorded from the reference's own ParseTcpOptions and CompareKeys
(tests/golden/tcp_rx_ref_cases.json), the fixture's coverage, aipstack_tcp_pcb_table_sort against
the model's order, the structs and constants, the argument validation of the two batch calls
(rejected before any HIP call), and the host code under ASan/UBSan as a stand-alone program
(tests/cpp/tcprx_table_test.cpp)."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib
from conftest import ROOT

import tcp_rx_ref as R
import tcprx_cases as T

REFERENCE = "/root/reference"


# ---- the model against the reference's recorded answers ----------------------------------------

def test_model_options_equal_the_reference():
    opts, _ = R.load()
    assert len(opts) >= 2000 + 40
    for b, fl, mss, ws in opts:
        assert T.parse_options(b) == (fl, mss, ws), b.hex()


def test_model_key_order_equals_the_reference():
    _, keys = R.load()
    assert len(keys) >= 500
    for a, b, r in keys:
        assert T.compare_keys(a, b)[0] == r, (a, b)
        assert (T.sort_order(a) < T.sort_order(b), T.sort_order(a) == T.sort_order(b)) == (r < 0, r == 0)


def test_fixture_covers_the_branches():
    """Each of the four flag combinations at least 20 times, each stop or skip branch at least 5
    times; each CompareKeys outcome decided by each of the four fields (0: by none differing)."""
    opts, keys = R.load()
    combos = collections.Counter(fl for _, fl, _, _ in opts)
    assert all(combos[c] >= 20 for c in (0, 1, 2, 3)), combos
    branches = collections.Counter()
    for b, _, _, _ in opts:
        tr = []
        T.parse_options(b, tr)
        branches.update(set(tr))
    assert all(branches[k] >= 5 for k in T.STOP_SKIP_BRANCHES), branches
    assert max(len(b) for b, _, _, _ in opts) == 40
    decided = collections.Counter(T.compare_keys(a, b) for a, b, _ in keys)
    for name in ("remote_port", "remote_addr", "local_port", "local_addr"):
        assert decided[(-1, name)] >= 1 and decided[(1, name)] >= 1, decided
    assert decided[(0, None)] >= 1
    one_field = sum(1 for a, b, _ in keys if sum(x != y for x, y in zip(a, b)) == 1)
    assert one_field >= 32


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "src", "aipstack")),
                    reason="reference tree not present")
def test_generator_reproduces_the_fixture():
    with open(R.FIXTURE) as f:
        assert R.generate(REFERENCE) == f.read()


def test_fixture_is_small():
    assert os.path.getsize(R.FIXTURE) < 256 * 1024


# ---- the table sort ----------------------------------------------------------------------------

def _random_keys(n, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=A.TCP_PCB_KEY_DTYPE)
    t["local_addr"] = rng.integers(0, 3, n) + T.LOCAL_IP
    t["remote_addr"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    t["local_port"] = rng.integers(0, 4, n) * 0x4000
    t["remote_port"] = rng.integers(0, 50, n) * 1300
    t["cookie"] = np.arange(n)
    return t


@pytest.mark.parametrize("n", [0, 1, 2, 3, 100, 5000])
def test_sort_agrees_with_the_model(n):
    t = _random_keys(n, n)
    got = A.tcp_pcb_table_sort(t)
    assert got.tobytes() == T.model_sort(t).tobytes()
    assert np.array_equal(t["cookie"], np.arange(n))           # the input is not touched
    assert A.tcp_pcb_table_sort(got[::-1]).tobytes() == got.tobytes()


def test_sort_orders_by_each_field():
    _, keys = R.load()
    for a, b, r in keys:
        if r == 0:
            continue
        t = T.table([a + (1,), b + (2,)], A.TCP_PCB_KEY_DTYPE)
        assert list(A.tcp_pcb_table_sort(t)["cookie"]) == ([1, 2] if r < 0 else [2, 1]), (a, b)


def test_sort_rejects_duplicates_and_the_reserved_cookie():
    t = _random_keys(50, 3)
    t[17] = t[40]
    t["cookie"][17] = 999                                      # the same key, another cookie
    with pytest.raises(A.ChksumError) as e:
        A.tcp_pcb_table_sort(t)
    assert e.value.status == A.AIPSTACK_CHKSUM_EINVAL
    t = _random_keys(50, 3)
    t["cookie"][49] = A.AIPSTACK_TCP_NO_PCB
    with pytest.raises(A.ChksumError):
        A.tcp_pcb_table_sort(t)
    # through the C-ABI: the array is left as a permutation of its input
    t = _random_keys(50, 3)
    t[17] = t[40]
    before = sorted(x.tobytes() for x in t)
    lib = _lib.load()
    assert lib.aipstack_tcp_pcb_table_sort(t.ctypes.data, t.size) == A.AIPSTACK_CHKSUM_EINVAL
    assert sorted(x.tobytes() for x in t) == before
    assert lib.aipstack_tcp_pcb_table_sort(None, 1) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_tcp_pcb_table_sort(None, 0) == A.AIPSTACK_CHKSUM_OK


# ---- structs and constants ---------------------------------------------------------------------

class _CSeg(ctypes.Structure):
    _fields_ = [("remote_addr", ctypes.c_uint32), ("local_addr", ctypes.c_uint32),
                ("remote_port", ctypes.c_uint16), ("local_port", ctypes.c_uint16),
                ("seq_num", ctypes.c_uint32), ("ack_num", ctypes.c_uint32),
                ("flags", ctypes.c_uint16), ("window_size", ctypes.c_uint16),
                ("data_off", ctypes.c_uint16), ("data_len", ctypes.c_uint16),
                ("mss", ctypes.c_uint16), ("wnd_scale", ctypes.c_uint8), ("opts", ctypes.c_uint8)]


class _CKey(ctypes.Structure):
    _fields_ = [("local_addr", ctypes.c_uint32), ("remote_addr", ctypes.c_uint32),
                ("local_port", ctypes.c_uint16), ("remote_port", ctypes.c_uint16),
                ("cookie", ctypes.c_uint32)]


@pytest.mark.parametrize("dtype,cstruct,size", [(A.TCP_RX_SEG_DTYPE, _CSeg, 32),
                                                (A.TCP_PCB_KEY_DTYPE, _CKey, 16)])
def test_dtypes_match_the_c_structs(dtype, cstruct, size):
    assert dtype.itemsize == size == ctypes.sizeof(cstruct)
    assert list(dtype.names) == [n for n, _ in cstruct._fields_]
    for name, ct in cstruct._fields_:
        assert dtype.fields[name][1] == getattr(cstruct, name).offset, name
        assert dtype.fields[name][0].itemsize == ctypes.sizeof(ct), name


def test_constants():
    assert A.AIPSTACK_RX_DROP_TCP_OFFSET == 11 and A.AIPSTACK_TCP_NO_PCB == 0xFFFFFFFF
    assert (A.AIPSTACK_TCP_OPT_MSS, A.AIPSTACK_TCP_OPT_WND_SCALE, A.AIPSTACK_TCP_SEG_VALID) == (1, 2, 0x80)
    assert A.RX_VERDICTS[11] == "DROP_TCP_OFFSET"
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for line in ("#define AIPSTACK_RX_DROP_TCP_OFFSET 11 ", "#define AIPSTACK_TCP_NO_PCB 0xFFFFFFFFu",
                 "#define AIPSTACK_TCP_OPT_MSS 1u", "#define AIPSTACK_TCP_OPT_WND_SCALE 2u",
                 "#define AIPSTACK_TCP_SEG_VALID 0x80u", "#define AIPSTACK_CHKSUM_ABI_VERSION 1"):
        assert line in text, line


# ---- argument validation of the batch calls ----------------------------------------------------

_CSR = ("base", "offsets", "n", "pcbs", "n_pcbs", "verdict", "segs", "pcb", "stream")
_SLOT = ("base", "stride", "lens", "n", "pcbs", "n_pcbs", "verdict", "segs", "pcb", "stream")


def _args(names, **over):
    """A well-formed argument list for 4 frames (host buffers standing in for device ones: a
    rejected call must return before touching them)."""
    bufs = {k: ctypes.create_string_buffer(512 + 16) for k in
            ("base", "offsets", "lens", "pcbs", "verdict", "segs", "pcb")}
    a = {k: (ctypes.addressof(v) + 15) & ~15 for k, v in bufs.items()}
    a.update(n=4, n_pcbs=2, stride=128, stream=None)
    for k, v in over.items():
        a[k] = a[k] + int(v[1:]) if isinstance(v, str) else v
    return bufs, [a[k] for k in names]


_BAD = [{"base": None}, {"verdict": None}, {"segs": None}, {"pcb": None}, {"pcbs": None},
        {"n": (1 << 40) + 1}, {"n_pcbs": (1 << 40) + 1},
        {"segs": "+4"}, {"segs": "+1"}, {"pcb": "+2"}, {"pcb": "+1"}, {"pcbs": "+4"}]


@pytest.mark.parametrize("over", _BAD + [{"offsets": None}])
def test_csr_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_CSR, **over)
    assert lib.aipstack_tcp_rx_parse(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


@pytest.mark.parametrize("over", _BAD + [{"lens": None}, {"stride": 0}, {"stride": 65537}])
def test_slotted_einval_before_any_hip_call(over):
    lib = _lib.load()
    keep, args = _args(_SLOT, **over)
    assert lib.aipstack_tcp_rx_parse_slotted(*args) == A.AIPSTACK_CHKSUM_EINVAL
    assert lib.aipstack_chksum_last_hip_error() == 0


def test_no_frames_is_a_noop():
    lib = _lib.load()
    keep, args = _args(_CSR, n=0)
    assert lib.aipstack_tcp_rx_parse(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_CSR, n=0, segs=None, pcbs=None, base=None)
    assert lib.aipstack_tcp_rx_parse(*args) == A.AIPSTACK_CHKSUM_OK
    keep, args = _args(_SLOT, n=0, stride=0)
    assert lib.aipstack_tcp_rx_parse_slotted(*args) == A.AIPSTACK_CHKSUM_OK


def test_wrappers_reject_host_tensors():
    torch = pytest.importorskip("torch")
    fr, off = torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError):
        A.tcp_rx_parse(fr, off)
    with pytest.raises(ValueError):
        A.tcp_rx_parse_slotted(fr, 64, torch.zeros(1, dtype=torch.int32))


# ---- the frame sets of the GPU tests are not vacuous (from the model and the oracle alone) -----

def test_frame_sets_contain_their_classes(oracle):
    frames, v = T.fill(oracle, [f for f, _ in T.bad_offset_frames()])
    assert (v == T.ACCEPT).all()
    e = T.expected(frames, v, None, A.TCP_RX_SEG_DTYPE)
    valid = np.array([ok for _, ok in T.bad_offset_frames()])
    assert (e.verdict[~valid] == T.DROP_TCP_OFFSET).all() and (e.verdict[valid] == T.ACCEPT).all()
    assert (e.segs["data_len"][valid] == 0).all() and (e.segs["opts"][valid] == T.SEG_VALID).all()
    frames, v = T.fill(oracle, T.geometry_frames())
    e = T.expected(frames, v, None, A.TCP_RX_SEG_DTYPE)
    assert (v == T.ACCEPT).all() and e.segs["data_off"].max() == 134
    opts = R.load()[0]
    frames, v = T.fill(oracle, T.option_frames(opts))
    e = T.expected(frames, v, None, A.TCP_RX_SEG_DTYPE)
    assert (v == T.ACCEPT).all()
    for i, (b, fl, mss, ws) in enumerate(opts):
        assert (e.segs["opts"][i], e.segs["mss"][i], e.segs["wnd_scale"][i]) == (fl | T.SEG_VALID, mss, ws)


# ---- the host code under ASan + UBSan, as a stand-alone program -------------------------------

def test_host_code_under_asan_ubsan():
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "tcprx.mk"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "tcprx_table_test")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
