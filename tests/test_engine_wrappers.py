"""The rules of the host-memory engine wrappers (ChksumEngine, ChksumEngineGroup), pinned
without a device: a recording stand-in takes the place of the ``aipstack_chksum_engine_*``
functions of the library, everything else (strerror, ...) is the real library's.

Pinned per class, batch kind and form (synchronous / submit): the C function called and its
arguments; which calls hand the caller's offsets / lengths to C as they are and which hand a
private copy; what stays referenced while a ticket is in flight; what a failing submit does;
the group's ``last_status``; every ValueError; empty batches."""
import ctypes
import functools

import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

ENGINE = "aipstack_chksum_engine_"
HANDLE = 0x5EED0000
FIRST_TICKET = 41

# kind -> (layout, result dtype, takes flags, fills the frames in place)
KINDS = {
    "strided": ("strided", np.uint16, True, False),
    "csr": ("csr", np.uint16, True, False),
    "rx_verify": ("csr", np.uint8, False, False),
    "tx_fill": ("csr", np.uint8, False, True),
    "slotted": ("slots", np.uint16, True, False),
    "rx_verify_slotted": ("slots", np.uint8, False, False),
    "tx_fill_slotted": ("slots", np.uint8, False, True),
}
INDEXED = [k for k in KINDS if KINDS[k][0] != "strided"]
TX = [k for k in KINDS if KINDS[k][3]]
INDEX_AT = {"csr": 2, "slots": 3}  # position of the offsets / lengths among the C arguments
CLASSES = ["engine", "group"]
FORMS = [False, True]  # submit?
GROUP_SIZE = 3


def _target(ref):
    """The ctypes object behind a byref() / pointer() argument."""
    return ref._obj if hasattr(ref, "_obj") else ref.contents


class RecordingLib:
    """Forwards every attribute to the real library except the engine functions, which are
    recorded as (name, args) and return 0 (or what the test asked for)."""

    def __init__(self, real):
        self._real = real
        self.calls = []
        self.ticket = FIRST_TICKET   # the next submit's ticket
        self.submit_failure = None   # (status, ticket) for the next submits
        self.host_failure = 0        # status of the synchronous calls
        self.poll_result = 0
        self.dev_status = [0] * GROUP_SIZE

    def __getattr__(self, name):
        if not name.startswith(ENGINE):
            return getattr(self._real, name)
        return functools.partial(self._engine_call, name)

    def _engine_call(self, name, *args):
        self.calls.append((name, args))
        if name.endswith("_destroy"):
            return None
        if name.endswith("_create"):
            _target(args[-1]).value = HANDLE
            return 0
        if "_submit_" in name:
            if self.submit_failure is not None:
                status, ticket = self.submit_failure
                _target(args[-1]).value = ticket
                return status
            _target(args[-1]).value = self.ticket
            self.ticket += 1
            return 0
        if name.endswith("_poll") and self.poll_result == 1:
            return 1
        if isinstance(args[-1], ctypes.Array):  # the group's dev_status
            for k, s in enumerate(self.dev_status):
                args[-1][k] = s
        if "_host_" in name:
            return self.host_failure
        if name.endswith("_region_mapped"):
            return 1
        return 0

    def named(self, suffix):
        return [(n, a) for n, a in self.calls if n.endswith(suffix)]


@pytest.fixture
def lib(monkeypatch):
    rec = RecordingLib(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    return rec


def make(cls, lib):
    obj = A.ChksumEngine(0) if cls == "engine" else A.ChksumEngineGroup([0] * GROUP_SIZE)
    assert lib.calls[-1][0] == prefix(cls) + "create"
    return obj


def prefix(cls):
    return ENGINE if cls == "engine" else ENGINE + "group_"


def batch(kind, n=4, index_dtype=None):
    """(buf, where): a buffer and the layout arguments of an n-entry batch of `kind`."""
    layout = KINDS[kind][0]
    buf = np.zeros(n * 256 + 64, dtype=np.uint8)
    if layout == "strided":
        return buf, (256, 200, n)
    if layout == "csr":
        return buf, (np.arange(n + 1, dtype=index_dtype or np.int64) * 200,)
    return buf, (256, np.full(n, 60, dtype=index_dtype or np.int32))


def call(obj, kind, submit, buf, where, res=None, final=None):
    """Run one wrapper; returns (ticket or None, result array)."""
    kw = {}
    if res is not None:
        kw["status" if KINDS[kind][3] else "out"] = res
    if final is not None:
        kw["final"] = final
    r = getattr(obj, ("submit_" if submit else "") + kind)(buf, *where, **kw)
    if submit:
        assert isinstance(r, tuple) and len(r) == 2
        return r
    return None, r


def c_name(cls, kind, submit):
    return prefix(cls) + ("submit_" if submit else "host_") + kind


def check_args(cls, kind, submit, args, buf, where, n, out, final):
    """The recorded C arguments but the offsets / lengths address (checked by the caller)."""
    layout, dtype, has_flags, _ = KINDS[kind]
    assert args[0].value == HANDLE
    assert out.dtype == dtype and out.size >= n
    want = [buf.ctypes.data]
    if layout == "strided":
        want += list(where)
    elif layout == "csr":
        want += [None, n]
    else:
        want += [where[0], None, n]
    want.append(out.ctypes.data)
    if has_flags:
        want.append(A.AIPSTACK_CHKSUM_FINAL if final else 0)
    got = list(args[1:1 + len(want)])
    if layout != "strided":
        got[INDEX_AT[layout] - 1] = None
    assert got == want
    tail = args[1 + len(want):]
    assert len(tail) == (1 if submit or cls == "group" else 0)
    if submit:
        assert isinstance(_target(tail[0]), ctypes.c_uint64)
    elif cls == "group":
        assert isinstance(tail[0], ctypes.Array) and len(tail[0]) == GROUP_SIZE


def copies_index(cls, kind, submit):
    """The rule: a group submit reads the index on a worker thread after the call returns, the
    engine's Tx fill on its applier thread at completion; nothing else outlives the call."""
    return submit and (cls == "group" or kind == "tx_fill")


@pytest.mark.parametrize("submit", FORMS)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cls", CLASSES)
def test_c_function_and_arguments(lib, cls, kind, submit):
    layout, dtype, has_flags, in_place = KINDS[kind]
    obj = make(cls, lib)
    buf, where = batch(kind)
    # a fresh result array and the caller's own; FINAL only when asked for; the default is not
    cases = [(None, None), (np.zeros(6, dtype=dtype), None)]
    if has_flags:
        cases += [(None, True), (np.zeros(4, dtype=dtype), False)]
    for given, final in cases:
        lib.calls.clear()
        ticket, out = call(obj, kind, submit, buf, where, res=given, final=final)
        assert given is None or out is given
        assert [n for n, _ in lib.calls] == [c_name(cls, kind, submit)]
        args = lib.calls[0][1]
        check_args(cls, kind, submit, args, buf, where, 4, out, final)
        if submit:
            assert ticket == lib.ticket - 1 and ticket >= FIRST_TICKET
        if layout != "strided":
            index = where[-1]
            addr = args[INDEX_AT[layout]]
            if copies_index(cls, kind, submit):
                assert addr != index.ctypes.data
            else:
                assert addr == index.ctypes.data  # a view of the caller's array: no copy
    obj.close()
    assert lib.calls[-1][0] == prefix(cls) + "destroy"


@pytest.mark.parametrize("kind", INDEXED)
@pytest.mark.parametrize("cls", CLASSES)
def test_index_of_another_dtype_is_converted(lib, cls, kind):
    """uint64 offsets / uint32 lengths go as they are too; anything else is converted."""
    layout = KINDS[kind][0]
    obj = make(cls, lib)
    same = np.uint64 if layout == "csr" else np.uint32
    buf, where = batch(kind, index_dtype=same)
    call(obj, kind, False, buf, where)
    assert lib.calls[-1][1][INDEX_AT[layout]] == where[-1].ctypes.data
    buf, where = batch(kind, index_dtype=np.int16)
    call(obj, kind, False, buf, where)
    assert lib.calls[-1][1][INDEX_AT[layout]] != where[-1].ctypes.data


@pytest.mark.parametrize("kind", INDEXED)
@pytest.mark.parametrize("cls", CLASSES)
def test_submit_keeps_arrays_until_completion(lib, cls, kind):
    layout = KINDS[kind][0]
    obj = make(cls, lib)
    buf, where = batch(kind)
    index = where[-1]
    before = index.copy()
    ticket, out = call(obj, kind, True, buf, where)
    held = obj._inflight[ticket]
    assert any(a is buf for a in held) and any(a is out for a in held)
    # the index array handed to C is the one kept alive
    addr = lib.calls[-1][1][INDEX_AT[layout]]
    kept = [a for a in held if a is not buf and a is not out]
    assert len(kept) == 1 and kept[0].ctypes.data == addr
    assert kept[0].itemsize == index.itemsize and np.array_equal(kept[0].view(index.dtype), before)
    if copies_index(cls, kind, True):
        assert not np.shares_memory(kept[0], index)
        index[:] = 7  # the caller refills its array at once: the private copy does not move
        assert np.array_equal(kept[0].view(index.dtype), before)
    else:
        assert np.shares_memory(kept[0], index)
    # still there while poll says "running", gone once it completes
    lib.poll_result = 1
    assert obj.poll(ticket) is False and ticket in obj._inflight
    lib.poll_result = 0
    assert obj.poll(ticket) is True and ticket not in obj._inflight
    assert lib.calls[-1][0] == prefix(cls) + "poll" and lib.calls[-1][1][1] == ticket
    # and gone after wait
    ticket, out = call(obj, kind, True, buf, where)
    assert ticket in obj._inflight
    assert obj.wait(ticket) is None and ticket not in obj._inflight
    assert lib.calls[-1][0] == prefix(cls) + "wait" and lib.calls[-1][1][1] == ticket
    obj.close()
    assert obj._inflight == {}


@pytest.mark.parametrize("cls", CLASSES)
def test_submit_strided_keeps_buffer_and_result(lib, cls):
    obj = make(cls, lib)
    buf, where = batch("strided")
    ticket, out = call(obj, "strided", True, buf, where)
    held = obj._inflight[ticket]
    assert len(held) == 2 and held[0] is buf and held[1] is out
    obj.wait(ticket)
    assert ticket not in obj._inflight


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cls", CLASSES)
def test_failing_submit_waits_for_its_ticket_then_raises(lib, cls, kind):
    obj = make(cls, lib)
    buf, where = batch(kind)
    # failed part-way: the pieces it did enqueue are completed before the error is raised
    lib.submit_failure = (A.AIPSTACK_CHKSUM_EHIP, 77)
    lib.calls.clear()
    with pytest.raises(A.ChksumError) as e:
        call(obj, kind, True, buf, where)
    assert e.value.status == A.AIPSTACK_CHKSUM_EHIP
    assert [n for n, _ in lib.calls] == [c_name(cls, kind, True), prefix(cls) + "wait"]
    assert lib.calls[1][1][1] == 77
    assert 77 not in obj._inflight
    # failed before anything was enqueued: no ticket, no wait
    lib.submit_failure = (A.AIPSTACK_CHKSUM_EINVAL, 0)
    lib.calls.clear()
    with pytest.raises(A.ChksumError) as e:
        call(obj, kind, True, buf, where)
    assert e.value.status == A.AIPSTACK_CHKSUM_EINVAL
    assert [n for n, _ in lib.calls] == [c_name(cls, kind, True)]
    assert obj._inflight == {}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cls", CLASSES)
def test_failing_synchronous_call_raises_its_status(lib, cls, kind):
    obj = make(cls, lib)
    buf, where = batch(kind)
    lib.host_failure = A.AIPSTACK_CHKSUM_ENODEV
    with pytest.raises(A.ChksumError) as e:
        call(obj, kind, False, buf, where)
    assert e.value.status == A.AIPSTACK_CHKSUM_ENODEV


@pytest.mark.parametrize("kind", list(KINDS))
def test_group_last_status(lib, kind):
    grp = make("group", lib)
    assert grp.size == GROUP_SIZE and grp.last_status == [0] * GROUP_SIZE
    buf, where = batch(kind)

    def is_status(want):
        got = grp.last_status
        return isinstance(got, list) and all(type(s) is int for s in got) and got == want

    lib.dev_status = [0, -2, 0]
    lib.host_failure = A.AIPSTACK_CHKSUM_EHIP
    with pytest.raises(A.ChksumError):
        call(grp, kind, False, buf, where)
    assert is_status([0, -2, 0])  # filled before the status is raised
    lib.host_failure = 0
    lib.dev_status = [0, 0, 0]
    call(grp, kind, False, buf, where)
    assert is_status([0, 0, 0])
    ticket, _ = call(grp, kind, True, buf, where)
    lib.dev_status = [-3, 0, -1]
    lib.poll_result = 1
    assert grp.poll(ticket) is False and is_status([0, 0, 0])  # nothing completed
    lib.poll_result = 0
    assert grp.poll(ticket) is True and is_status([-3, 0, -1])
    ticket, _ = call(grp, kind, True, buf, where)
    lib.dev_status = [0, 0, -2]
    grp.wait(ticket)
    assert is_status([0, 0, -2])


@pytest.mark.parametrize("submit", FORMS)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cls", CLASSES)
def test_value_errors(lib, cls, kind, submit):
    layout, dtype, _, in_place = KINDS[kind]
    obj = make(cls, lib)
    lib.calls.clear()

    def rejected(buf, where, res=None):
        with pytest.raises(ValueError):
            call(obj, kind, submit, buf, where, res=res)

    buf, where = batch(kind)
    if layout == "strided":
        rejected(buf, (256, 200, buf.size // 256 + 1))   # the batch exceeds the buffer
        rejected(buf[:3 * 256 + 199], where)
    elif layout == "csr":
        rejected(buf[:799], where)                       # the offsets exceed the buffer
    else:
        rejected(buf[:4 * 256 - 1], where)               # fewer than n whole slots
        rejected(buf, (0, where[1]))                     # slot_stride <= 0
        rejected(buf, (-256, where[1]))
    wide = np.zeros((buf.size, 2), dtype=np.uint8)
    rejected(wide[:, 0], where)                          # buf not C-contiguous
    other = np.uint8 if dtype == np.uint16 else np.uint16
    rejected(buf, where, res=np.zeros(4, dtype=other))   # out: wrong dtype
    rejected(buf, where, res=np.zeros(3, dtype=dtype))   # too small
    rejected(buf, where, res=np.zeros(8, dtype=dtype)[::2])  # not contiguous
    read_only = np.zeros(4, dtype=dtype)
    read_only.flags.writeable = False
    rejected(buf, where, res=read_only)
    frozen = buf.copy()
    frozen.flags.writeable = False
    if in_place:
        rejected(frozen, where)                          # Tx fills write the frames
    assert lib.calls == [] and obj._inflight == {}       # nothing reached C
    if not in_place:
        call(obj, kind, submit, frozen, where)           # the others only read them
        assert len(lib.calls) == 1


@pytest.mark.parametrize("submit", FORMS)
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cls", CLASSES)
def test_empty_batches_pass_n_zero(lib, cls, kind, submit):
    layout, dtype, _, _ = KINDS[kind]
    obj = make(cls, lib)
    buf = np.zeros(64, dtype=np.uint8)
    if layout == "strided":
        empties = [(256, 200, 0)]
    elif layout == "csr":
        empties = [(np.zeros(0, dtype=np.int64),), (np.zeros(1, dtype=np.int64),)]
    else:
        empties = [(256, np.zeros(0, dtype=np.int32))]
    n_at = {"strided": 4, "csr": 3, "slots": 4}[layout]
    for where in empties:
        _, out = call(obj, kind, submit, buf, where)
        name, args = lib.calls[-1]
        assert name == c_name(cls, kind, submit)
        assert args[n_at] == 0, (name, where)
        assert out.dtype == dtype and out.size == 0


@pytest.mark.parametrize("cls", CLASSES)
def test_lifecycle_and_registration(lib, cls):
    arr = np.zeros(4096, dtype=np.uint8)
    with make(cls, lib) as obj:
        obj.register(arr)
        assert lib.calls[-1] == (prefix(cls) + "register", (obj._h, arr.ctypes.data, arr.nbytes))
        assert any(a is arr for a in obj._registered)
        obj.unregister(arr)
        assert lib.calls[-1] == (prefix(cls) + "unregister", (obj._h, arr.ctypes.data))
        assert obj._registered == []
    assert len(lib.named("destroy")) == 1
    obj.close()  # closing twice destroys once
    assert len(lib.named("destroy")) == 1


def test_group_locality_and_region_mapped(lib):
    grp = make("group", lib)
    lib.calls.clear()
    assert grp.locality() == [(-1, 0)] * GROUP_SIZE  # the stand-in writes nothing
    assert [n for n, _ in lib.calls] == [ENGINE + "group_engine", ENGINE + "locality"] * GROUP_SIZE
    arr = np.zeros(64, dtype=np.uint8)
    assert grp.region_mapped(arr) is True
    assert lib.calls[-1] == (ENGINE + "group_region_mapped", (grp._h, arr.ctypes.data))
    eng = make("engine", lib)
    assert eng.locality() == (-1, 0)
    assert lib.calls[-1][0] == ENGINE + "locality" and lib.calls[-1][1][0] is eng._h
