"""The host-memory engines: :class:`ChksumEngine` (C-ABI ``aipstack_chksum_engine_*``, one
device) and :class:`ChksumEngineGroup` (``aipstack_chksum_engine_group_*``, several devices
behind one batch). Both checksum, verify or fill batches held in HOST memory (numpy arrays) and
return the results in host memory; ``include/aipstack_amd/chksum.h`` has the contracts.

Every batch kind (``_KINDS``) exists in a synchronous form, ``kind(...)``, which returns the
result array, and as ``submit_kind(...)``, which returns ``(ticket, result array)`` at once;
``poll`` / ``wait`` complete a ticket. A kind is described once and each argument rule is
written once, in the function of its layout; the two classes differ only where the C-ABI does.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib
# (chksum imports this module in turn, below the names taken here; the package imports
# chksum first, so this order holds whichever module a caller names)
from .chksum import AIPSTACK_CHKSUM_FINAL, AIPSTACK_CHKSUM_OK, ChksumError, _check


def _host_u64(a):
    """Host offsets as the C-ABI's uint64: a contiguous int64 array is passed as it is (a
    view; the engine rejects the huge values a negative entry becomes, as non-decreasing
    offsets within the frames), anything else is converted (a copy)."""
    if isinstance(a, np.ndarray) and a.dtype == np.int64 and a.flags.c_contiguous:
        return a.view(np.uint64)
    return np.ascontiguousarray(a, dtype=np.uint64)


def _host_u32(a):
    """Host lengths as the C-ABI's uint32 (int32 viewed, as _host_u64; the engine rejects
    lengths above the slot stride)."""
    if isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous:
        return a.view(np.uint32)
    return np.ascontiguousarray(a, dtype=np.uint32)


class _Kind(NamedTuple):
    layout: str           # where packet i lies: a key of _LAYOUTS
    result: type          # uint16 checksums, or uint8 verdicts / statuses of a frame call
    flags: bool = False   # takes AIPSTACK_CHKSUM_* flags (`final`)
    in_place: bool = False  # writes the checksum fields into the frames


# The batch kinds; the name is the suffix of the C functions (..._host_<kind>, ..._submit_<kind>).
_KINDS = {
    "strided": _Kind("strided", np.uint16, flags=True),
    "csr": _Kind("csr", np.uint16, flags=True),
    "rx_verify": _Kind("csr", np.uint8),
    "tx_fill": _Kind("csr", np.uint8, in_place=True),
    "slotted": _Kind("slots", np.uint16, flags=True),
    "rx_verify_slotted": _Kind("slots", np.uint8),
    "tx_fill_slotted": _Kind("slots", np.uint8, in_place=True),
}


# One function per layout: (index array or None, n, C arguments between the buffer and the
# results) of a checked batch in `buf` (called `name` in messages). `private`: the index array
# handed to C is a copy of the caller's, taken before it is checked.

def _strided(buf, name, private, stride, length, n):
    """Packet i = the `length` bytes at buf[i * stride:]."""
    if n and (n - 1) * stride + length > buf.nbytes:
        raise ValueError("batch exceeds buf")
    return None, n, (stride, length, n)


def _csr(buf, name, private, offsets):
    """Packet i = buf[offsets[i]:offsets[i+1]]; n + 1 offsets (none at all: an empty batch)."""
    o = _host_u64(offsets).copy() if private else _host_u64(offsets)
    n = max(o.size - 1, 0)
    if n and int(o[-1]) > buf.nbytes:
        raise ValueError(f"offsets exceed {name}")
    return o, n, (o.ctypes.data, n)


def _slots(buf, name, private, slot_stride, lens):
    """Ring slots: packet i = the lens[i] bytes at buf[i * slot_stride:]."""
    ln = _host_u32(lens).copy() if private else _host_u32(lens)
    n = ln.size
    if slot_stride <= 0 or n * slot_stride > buf.nbytes:
        raise ValueError("the buffer must hold n whole slots of slot_stride bytes")
    return ln, n, (slot_stride, ln.ctypes.data, n)


_LAYOUTS = {"strided": _strided, "csr": _csr, "slots": _slots}


def _result(buf, out, n, dtype):
    """The result array of an n-entry batch in `buf`: the caller's `out`, checked, or a new one."""
    if not isinstance(buf, np.ndarray) or not buf.flags.c_contiguous:
        raise ValueError("buf must be a C-contiguous numpy array")
    if out is None:
        return np.empty(n, dtype=dtype)
    if (not isinstance(out, np.ndarray) or out.dtype != dtype
            or not out.flags.c_contiguous or not out.flags.writeable or out.size < n):
        raise ValueError(f"out must be a writable C-contiguous {np.dtype(dtype).name} array "
                         "of >= n elements")
    return out


def _batch(kind, buf, where, out, final, private):
    """One batch of `kind` in `buf`, laid out by `where` (the arguments of its layout), checked:
    (C arguments after the handle, the arrays C uses until the batch completes, result array)."""
    k = _KINDS[kind]
    if k.in_place and not (isinstance(buf, np.ndarray) and buf.flags.writeable):
        raise ValueError("frames must be writable (filled in place)")
    name = "frames" if k.result is np.uint8 else "buf"
    index, n, between = _LAYOUTS[k.layout](buf, name, private, *where)
    out = _result(buf, out, n, k.result)
    args = (buf.ctypes.data, *between, out.ctypes.data)
    if k.flags:
        args += (AIPSTACK_CHKSUM_FINAL if final else 0,)
    return args, (buf, out) if index is None else (buf, index, out), out


class _HostEngine:
    """What the two engines share: life cycle, registration, the 14 batch methods, tickets.
    A subclass gives the C symbol prefix, creates the handle and says which submits take a
    private copy of the index array."""

    _PREFIX = ""
    # Kinds whose submit hands C a private copy of the caller's offsets / lengths, because C
    # reads them after the call has returned and the caller may refill its array at once:
    #   engine: tx_fill alone -- the applier thread reads the offsets again at completion, to
    #           find the frames whose fields it writes (ring slots are found by their stride);
    #   group:  every kind -- a range may be submitted later, on its device's worker thread,
    #           and must see the values that were checked here.
    # Every other call, the synchronous ones included, passes a contiguous int64 / int32 array
    # as a view: no per-call copy of what may be a 1 M-entry array.
    _PRIVATE_INDEX = frozenset()
    _WAIT_NO_STATUS = ()  # trailing arguments of a ..._wait whose status nobody reads

    def _create(self, *args):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        _check(self._c("create")(*args, ctypes.byref(h)), self._PREFIX + "create")
        self._h = h
        self._registered = []
        self._inflight = {}

    def _c(self, name):
        return getattr(self._lib, self._PREFIX + name)

    def _completing(self, name, *args):
        """Status of a C call that completes batches (host_<kind>, poll, wait)."""
        return self._c(name)(self._h, *args)

    def close(self) -> None:
        if self._h:
            self._c("destroy")(self._h)  # completes every batch in flight
            self._h = None
            self._registered = []
            self._inflight = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def register(self, arr: np.ndarray) -> None:
        """Page-lock `arr` (kept alive by the engine) so that the kernels read batches in it
        where they lie (zero copy; or DMA'd directly with tune("engine_zero_copy", 0))."""
        _check(self._c("register")(self._h, arr.ctypes.data, arr.nbytes),
               self._PREFIX + "register")
        self._registered.append(arr)

    def unregister(self, arr: np.ndarray) -> None:
        """Unpin `arr`; batches still in flight are completed first (C engine)."""
        _check(self._c("unregister")(self._h, arr.ctypes.data), self._PREFIX + "unregister")
        self._registered = [a for a in self._registered if a is not arr]

    def _sync(self, kind, buf, where, out, final=False):
        args, _, out = _batch(kind, buf, where, out, final, False)
        _check(self._completing("host_" + kind, *args), f"{self._PREFIX}host_{kind}")
        return out

    def _submit(self, kind, buf, where, out, final=False):
        """(ticket, result array). The arrays C still uses stay referenced until the ticket
        completes; if the submit failed part-way, the pieces it did enqueue (they read the
        arrays and, for Tx, write into the frames) are completed before raising."""
        args, keep, out = _batch(kind, buf, where, out, final, kind in self._PRIVATE_INDEX)
        t = ctypes.c_uint64(0)
        st = self._c("submit_" + kind)(self._h, *args, ctypes.byref(t))
        if st != AIPSTACK_CHKSUM_OK:
            if t.value:
                self._c("wait")(self._h, t.value, *self._WAIT_NO_STATUS)
            raise ChksumError(st, f"{self._PREFIX}submit_{kind}")
        if t.value:
            self._inflight[t.value] = keep
        return t.value, out

    def poll(self, ticket: int) -> bool:
        """True once batch `ticket` is complete (its results in place); False while running."""
        st = self._completing("poll", ticket)
        if st == 1:
            return False
        self._inflight.pop(ticket, None)
        _check(st, self._PREFIX + "poll")
        return True

    def wait(self, ticket: int) -> None:
        """Block until batch `ticket` is complete."""
        st = self._completing("wait", ticket)
        self._inflight.pop(ticket, None)
        _check(st, self._PREFIX + "wait")

    # ---- packets `stride` apart, `length` bytes each ------------------------------------

    def strided(self, buf: np.ndarray, stride: int, length: int, n: int, *, out=None,
                final: bool = False) -> np.ndarray:
        """``out[i] = IpChksumInverted(buf[i*stride:][:length])`` (``IpChksum`` with `final`)."""
        return self._sync("strided", buf, (stride, length, n), out, final)

    def submit_strided(self, buf: np.ndarray, stride: int, length: int, n: int, *, out=None,
                       final: bool = False):
        """Enqueue a strided batch; returns (ticket, out). `out` is filled when the batch
        completes (wait / poll); a registered `buf` must not change until then."""
        return self._submit("strided", buf, (stride, length, n), out, final)

    # ---- CSR: packet / frame i = buf[offsets[i]:offsets[i+1]] ---------------------------

    def csr(self, buf: np.ndarray, offsets: np.ndarray, *, out=None,
            final: bool = False) -> np.ndarray:
        return self._sync("csr", buf, (offsets,), out, final)

    def submit_csr(self, buf: np.ndarray, offsets: np.ndarray, *, out=None,
                   final: bool = False):
        """Enqueue a CSR batch; returns (ticket, out) (see submit_strided)."""
        return self._submit("csr", buf, (offsets,), out, final)

    def rx_verify(self, frames: np.ndarray, offsets: np.ndarray, *, out=None) -> np.ndarray:
        """Rx verify of raw Ethernet frames in HOST memory: one AIPSTACK_RX_* verdict per
        frame (uint8), as :func:`rx_verify` on the device."""
        return self._sync("rx_verify", frames, (offsets,), out)

    def submit_rx_verify(self, frames: np.ndarray, offsets: np.ndarray, *, out=None):
        """Enqueue an Rx verify batch; returns (ticket, out) (see submit_strided)."""
        return self._submit("rx_verify", frames, (offsets,), out)

    def tx_fill(self, frames: np.ndarray, offsets: np.ndarray, *, status=None) -> np.ndarray:
        """Tx fill of raw Ethernet frames in HOST memory, IN PLACE: the IPv4 header and L4
        checksum fields are written as :func:`tx_fill` does on the device; returns the
        per-frame AIPSTACK_TX_* statuses (uint8)."""
        return self._sync("tx_fill", frames, (offsets,), status)

    def submit_tx_fill(self, frames: np.ndarray, offsets: np.ndarray, *, status=None):
        """Enqueue a Tx fill batch; returns (ticket, status). The frames are filled and
        `status` written when the batch completes (wait / poll); `frames` must not be
        touched until then."""
        return self._submit("tx_fill", frames, (offsets,), status)

    # ---- ring slots: packet / frame i = the lens[i] bytes at buf[i * slot_stride:] ------

    def slotted(self, buf: np.ndarray, slot_stride: int, lens, *, out=None,
                final: bool = False) -> np.ndarray:
        """Checksums of the packets of a ring of slots in HOST memory."""
        return self._sync("slotted", buf, (slot_stride, lens), out, final)

    def submit_slotted(self, buf: np.ndarray, slot_stride: int, lens, *, out=None,
                       final: bool = False):
        return self._submit("slotted", buf, (slot_stride, lens), out, final)

    def rx_verify_slotted(self, frames: np.ndarray, slot_stride: int, lens, *,
                          out=None) -> np.ndarray:
        """Rx verify of a ring of frame slots in HOST memory."""
        return self._sync("rx_verify_slotted", frames, (slot_stride, lens), out)

    def submit_rx_verify_slotted(self, frames: np.ndarray, slot_stride: int, lens, *,
                                 out=None):
        """Enqueue an Rx verify batch of frame slots; returns (ticket, out). The slots must
        not be refilled until the ticket completes (the receive loop of a TAP ring:
        tap/linux/TapDeviceLinux.cpp:156-178)."""
        return self._submit("rx_verify_slotted", frames, (slot_stride, lens), out)

    def tx_fill_slotted(self, frames: np.ndarray, slot_stride: int, lens, *,
                        status=None) -> np.ndarray:
        """Tx fill, in place, of a ring of frame slots in HOST memory."""
        return self._sync("tx_fill_slotted", frames, (slot_stride, lens), status)

    def submit_tx_fill_slotted(self, frames: np.ndarray, slot_stride: int, lens, *,
                               status=None):
        """Enqueue a Tx fill of frame slots, in place; returns (ticket, status). The frames
        are filled when the ticket completes and must not be touched until then."""
        return self._submit("tx_fill_slotted", frames, (slot_stride, lens), status)


class ChksumEngine(_HostEngine):
    """Host-memory streaming engine (C-ABI ``aipstack_chksum_engine_*``): checksums
    batches held in HOST memory (numpy arrays) and returns results in host memory,
    pipelining H2D / kernel / D2H over ``nstreams`` HIP streams. ``strided`` / ``csr`` / ...
    are synchronous; ``submit_strided`` / ``submit_csr`` / ... return a ticket at once and
    ``poll`` / ``wait`` complete it, so the caller can prepare its next batch meanwhile."""

    _PREFIX = "aipstack_chksum_engine_"
    _PRIVATE_INDEX = frozenset({"tx_fill"})

    def __init__(self, device: int = 0, chunk_bytes: int = 0, nstreams: int = 2):
        self._create(device, chunk_bytes, nstreams)

    def locality(self):
        """(NUMA node of the device or -1, CPUs the engine's host threads are pinned to)."""
        return _locality(self._lib, self._h)


class ChksumEngineGroup(_HostEngine):
    """Several devices behind one host-memory batch in ONE process (C-ABI
    ``aipstack_chksum_engine_group_*``): one engine per entry of ``devices`` (repeats
    allowed), each batch split into contiguous ranges of about equal bytes run concurrently
    (small batches go whole to one device, round robin). The synchronous calls return the
    results; ``submit_*`` return ``(ticket, out)`` at once, ``poll`` / ``wait`` complete a
    ticket. ``last_status`` holds each engine's status of the last completed call."""

    _PREFIX = "aipstack_chksum_engine_group_"
    _PRIVATE_INDEX = frozenset(_KINDS)
    _WAIT_NO_STATUS = (None,)

    def __init__(self, devices, chunk_bytes: int = 0, nstreams: int = 4):
        devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        self._create(devs, len(devices), chunk_bytes, nstreams)
        self.size = len(devices)
        self.last_status = [0] * self.size

    def _completing(self, name, *args):
        # the completing calls of the group end in a dev_status array: one status per engine
        ds = (ctypes.c_int * self.size)()
        st = super()._completing(name, *args, ds)
        if st != 1:  # (poll: still running, nothing completed)
            self.last_status = list(ds)
        return st

    def locality(self):
        """Per engine: (NUMA node of its device or -1, CPUs its host threads are pinned to)."""
        return [_locality(self._lib, self._c("engine")(self._h, k)) for k in range(self.size)]

    def region_mapped(self, arr: np.ndarray) -> bool:
        """Whether every device's kernels read the registered `arr` in place (zero copy)."""
        st = self._c("region_mapped")(self._h, arr.ctypes.data)
        _check(min(st, 0), self._PREFIX + "region_mapped")
        return st == 1


def _locality(lib, engine):
    node, cpus = ctypes.c_int(-1), ctypes.c_int(0)
    _check(lib.aipstack_chksum_engine_locality(engine, ctypes.byref(node), ctypes.byref(cpus)),
           "aipstack_chksum_engine_locality")
    return node.value, cpus.value
