"""Host-side mirror of aipstack's checksum interface + the batched GPU entry points.

Reference interface mirrored (ambrop72/aipstack, ``src/aipstack/infra``):

=========================================  ================================================
reference (file:line)                      here
=========================================  ================================================
``IpChksumInverted`` Chksum.h:77-99        :func:`IpChksumInverted` (host C hook in the .so)
``IpChksum(ptr,len)`` Chksum.h:122-125     :func:`IpChksum` (bytes-like argument)
``IpChksum(IpBufRef)`` Chksum.h:332-336    :func:`IpChksum` (``IpBufRef`` argument)
``IpChksumAccumulator`` Chksum.h:148-316   :class:`IpChksumAccumulator`
``IpBufNode`` Buf.h:68-83                  :class:`IpBufNode`
``IpBufRef`` Buf.h:118-251                 :class:`IpBufRef`
``ipBufProcessBytes`` BufUtils.h:129-178   :func:`ipBufProcessBytes`
=========================================  ================================================

The per-packet functions run on the host (one packet is ~0.35 us of scalar work; a GPU
launch costs more). Batches go to the GPU through :func:`chksum_batch_strided`,
:func:`chksum_batch_csr` and :func:`chksum_batch_seeded_csr`, which call the C-ABI
(``include/aipstack_amd/chksum.h``) on device-resident torch tensors. torch is only the
device-memory / stream plumbing here; there is no CPU fallback for the batch calls.
"""
from __future__ import annotations

import collections
import ctypes
from typing import Callable, Optional

import numpy as np

from . import _lib

AIPSTACK_CHKSUM_OK = 0
AIPSTACK_CHKSUM_EINVAL = -1
AIPSTACK_CHKSUM_EHIP = -2
AIPSTACK_CHKSUM_ENODEV = -3
AIPSTACK_CHKSUM_FINAL = 1
AIPSTACK_CHKSUM_ZERO_AS_FFFF = 2
AIPSTACK_CHKSUM_JUST_WRITTEN = 4  # hint: written by device stores since last read (chksum.h)
AIPSTACK_CHKSUM_MAX_LEN = 65535


class ChksumError(RuntimeError):
    """A batch entry point returned a negative status."""

    def __init__(self, status: int, where: str):
        lib = _lib.load()
        msg = lib.aipstack_chksum_strerror(status).decode()
        hip = lib.aipstack_chksum_last_hip_error()
        super().__init__(f"{where}: {msg} (status {status}, hip error {hip})")
        self.status = status
        self.hip_error = hip


def _check(status: int, where: str) -> None:
    if status != AIPSTACK_CHKSUM_OK:
        raise ChksumError(status, where)


# --------------------------------------------------------------------------------------
# Per-packet host functions
# --------------------------------------------------------------------------------------

def _as_pointer(data, length: Optional[int]):
    """(keepalive, address, length) of a bytes-like object's first `length` bytes."""
    arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) \
        else data.reshape(-1).view(np.uint8)
    n = arr.nbytes if length is None else int(length)
    if n < 0 or n > arr.nbytes:
        raise ValueError("length exceeds the buffer")
    if n == 0:  # the hook requires a non-null pointer even for len 0
        arr = np.zeros(1, dtype=np.uint8)
    return arr, arr.ctypes.data, n


def IpChksumInverted(data, length: Optional[int] = None) -> int:
    """Inverted IP checksum (ones'-complement sum of big-endian 16-bit words) of the first
    `length` bytes of `data` (default: all). Reference Chksum.h:77-99; len <= 65535."""
    keep, addr, n = _as_pointer(data, length)
    if n > AIPSTACK_CHKSUM_MAX_LEN:
        raise ValueError("IpChksumInverted: len must not exceed 65535 (Chksum.h:73-74)")
    r = _lib.load().IpChksumInverted(addr, n)
    del keep
    return int(r)


def IpChksum(data, length: Optional[int] = None) -> int:
    """IP checksum. With a bytes-like `data`: ``~IpChksumInverted`` (Chksum.h:122-125).
    With an :class:`IpBufRef`: the checksum of the referenced chain (Chksum.h:332-336)."""
    if isinstance(data, IpBufRef):
        return IpChksumAccumulator().getChksum(data)
    return (~IpChksumInverted(data, length)) & 0xFFFF


# --------------------------------------------------------------------------------------
# Buffer chains (Buf.h / BufUtils.h)
# --------------------------------------------------------------------------------------

class IpBufNode:
    """Node of a buffer chain: ``ptr`` (a bytes-like object; its first ``len`` bytes are
    the node's data), ``len`` and ``next`` (reference Buf.h:68-83)."""

    __slots__ = ("ptr", "len", "next")

    def __init__(self, ptr=b"", len: int = 0, next: "Optional[IpBufNode]" = None):
        self.ptr = memoryview(ptr).cast("B") if ptr is not None else memoryview(b"")
        self.len = int(len)
        self.next = next
        if self.len > self.ptr.nbytes:
            raise ValueError("IpBufNode: len exceeds the buffer")


class IpBufRef:
    """Reference to ``tot_len`` bytes of a chain starting at ``offset`` in ``node``
    (reference Buf.h:118-251)."""

    __slots__ = ("node", "offset", "tot_len")

    def __init__(self, node: Optional[IpBufNode] = None, offset: int = 0, tot_len: int = 0):
        self.node = node
        self.offset = int(offset)
        self.tot_len = int(tot_len)

    def _assert_sanity(self) -> None:  # Buf.h:242-246
        assert self.node is not None and self.offset <= self.node.len

    def getChunkPtr(self) -> memoryview:  # Buf.h:137-142
        self._assert_sanity()
        return self.node.ptr[self.offset:]

    def getChunkLength(self) -> int:  # Buf.h:149-154
        self._assert_sanity()
        return min(self.tot_len, self.node.len - self.offset)

    def revealHeader(self, amount: int) -> "IpBufRef":  # Buf.h:166-175
        assert amount <= self.offset
        return IpBufRef(self.node, self.offset - amount, self.tot_len + amount)

    def hasHeader(self, amount: int) -> bool:  # Buf.h:184-189
        self._assert_sanity()
        return amount <= self.tot_len and amount <= self.node.len - self.offset

    def hideHeader(self, amount: int) -> "IpBufRef":  # Buf.h:201-212
        self._assert_sanity()
        assert amount <= self.tot_len and amount <= self.node.len - self.offset
        return IpBufRef(self.node, self.offset + amount, self.tot_len - amount)

    def subTo(self, new_tot_len: int) -> "IpBufRef":  # Buf.h:226-235
        assert new_tot_len <= self.tot_len
        return IpBufRef(self.node, self.offset, new_tot_len)


def ipBufProcessBytes(buf: IpBufRef, processLen: int,
                      processChunk: Callable[[memoryview, int], int]) -> IpBufRef:
    """BufUtils.h:129-178 (same contract): hands ``processChunk(piece, piece_len)`` the
    non-empty pieces of the first `processLen` bytes of `buf`, node by node; it returns how
    many bytes of its piece it took, and taking fewer ends the walk inside that node. The
    returned reference starts after the bytes taken and keeps everything not taken. A used-up
    node is left behind whenever it has a successor, even when nothing more is wanted (the
    reference's eager advance, which also steps over empty nodes)."""
    assert buf.node is not None and processLen <= buf.tot_len
    untouched = buf.tot_len - processLen
    at, pos, want = buf.node, buf.offset, processLen
    while True:
        assert pos <= at.len
        avail = at.len - pos
        uses_up_node = want >= avail
        piece = avail if uses_up_node else want
        if piece:
            took = processChunk(at.ptr[pos:pos + piece], piece)
            assert 0 <= took <= piece
            pos += took
            want -= took
            if took != piece:  # the visitor stopped early
                break
        if not uses_up_node or at.next is None:
            break
        at, pos = at.next, 0
    return IpBufRef(at, pos, want + untouched)


# --------------------------------------------------------------------------------------
# Incremental accumulator (Chksum.h:148-316)
# --------------------------------------------------------------------------------------

class IpChksumAccumulator:
    """Incremental IP checksum of header words followed by data.

    ``State`` is the exported 32-bit running sum (Chksum.h:156, getState :181,
    resume :171). Header words are added without carry handling, as the reference does
    (addWord :191-217); chunk sums are added with end-around carry and the odd-chunk
    byte-swap rule (addIpBuf :283-315); getChksum folds twice and inverts (:245-250)."""

    __slots__ = ("_sum",)

    def __init__(self, state: Optional[int] = None):
        self._sum = 0 if state is None else int(state) & 0xFFFFFFFF

    def getState(self) -> int:
        return self._sum

    def addWord16(self, word: int) -> None:  # addWord(WrapType<uint16_t>) :191-194
        self._sum = (self._sum + (int(word) & 0xFFFF)) & 0xFFFFFFFF

    def addWordOctets(self, high_octet: int, low_octet: int) -> None:  # :202-206
        self.addWord16(((int(high_octet) & 0xFF) << 8) | (int(low_octet) & 0xFF))

    def addWord32(self, word: int) -> None:  # addWord(WrapType<uint32_t>) :213-217
        self.addWord16((int(word) >> 16) & 0xFFFF)
        self.addWord16(int(word) & 0xFFFF)

    def addEvenBytes(self, data, num_bytes: Optional[int] = None) -> None:  # :225-235
        mv = memoryview(data).cast("B")
        n = mv.nbytes if num_bytes is None else int(num_bytes)
        assert n % 2 == 0, "addEvenBytes: odd byte count"
        for i in range(0, n, 2):
            self.addWord16((mv[i] << 8) | mv[i + 1])

    @staticmethod
    def _swap(x: int) -> int:  # swapBytes :277-281
        return ((x >> 8) & 0x00FF00FF) | ((x << 8) & 0xFF00FF00)

    def _addIpBuf(self, buf: IpBufRef) -> None:  # :283-315
        swapped = [False]

        def chunk(mv: memoryview, n: int) -> int:
            b = IpChksumInverted(mv, n)
            s = self._sum + b
            if s > 0xFFFFFFFF:  # end-around carry
                s = (s & 0xFFFFFFFF) + 1
            if n % 2:
                s = self._swap(s)
                swapped[0] = not swapped[0]
            self._sum = s
            return n

        ipBufProcessBytes(buf, buf.tot_len, chunk)
        if swapped[0]:
            self._sum = self._swap(self._sum)

    def getChksum(self, buf: Optional[IpBufRef] = None) -> int:  # :245-250, :263-269
        if buf is not None and buf.tot_len > 0:
            self._addIpBuf(buf)
        s = self._sum
        s = (s & 0xFFFF) + (s >> 16)
        s = (s & 0xFFFF) + (s >> 16)
        return (~s) & 0xFFFF


# --------------------------------------------------------------------------------------
# Batched GPU entry points (device-resident torch tensors)
# --------------------------------------------------------------------------------------

def _torch():
    import torch  # plumbing only: device memory and streams
    return torch


def _stream_handle(stream, like=None) -> int:
    """The raw hipStream_t of `stream`; for None, torch's current stream of `like`'s device
    (a tensor), so every wrapper launches on the stream of the device its data lives on."""
    torch = _torch()
    if stream is None:  # torch's current stream, as a raw handle
        dev = like.device.index if like is not None and like.device.index is not None \
            else torch.cuda.current_device()
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        if raw is not None:  # skips building a Stream object per call (small batches)
            return int(raw(dev))
        stream = torch.cuda.current_stream(dev)
    return int(stream.cuda_stream) if hasattr(stream, "cuda_stream") else int(stream)


def _require_device(t, name: str) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device (HIP) tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _require_offsets(offsets, name: str = "offsets") -> None:
    """CSR offsets: a contiguous device tensor of 64-bit integers (the C-ABI reads uint64)."""
    torch = _torch()
    _require_device(offsets, name)
    if offsets.dtype not in (torch.int64, torch.uint64):
        raise ValueError(f"{name} must be an int64/uint64 device tensor")


def _same_device(a, b, names: str) -> None:
    if a.device != b.device:
        raise ValueError(f"{names} must be on the same device")


def _out_tensor(out, n: int, like):
    torch = _torch()
    if out is None:
        return torch.empty(n, dtype=torch.uint16, device=like.device)
    _require_device(out, "out")
    if out.dtype not in (torch.uint16, torch.int16) or out.numel() < n:
        raise ValueError("out must be a uint16/int16 device tensor with >= n elements")
    _same_device(out, like, "out and the input")
    return out


def _records_out(out, n: int, frames):
    """The 64-bit device tensor the Tx records go to: the caller's, checked, or a new one."""
    if out is None:
        torch = _torch()
        return torch.empty(n, dtype=torch.int64, device=frames.device)
    _require_device(out, "out")
    if out.element_size() != 8 or out.numel() < n:
        raise ValueError("out must be a 64-bit device tensor with >= n elements")
    _same_device(out, frames, "out and frames")
    return out


def chksum_batch_strided(buf, stride: int, length: int, n: int, *, out=None,
                         final: bool = False, byte_offset: int = 0, stream=None,
                         just_written: bool = False):
    """``out[i] = IpChksumInverted(buf[byte_offset + i*stride :][:length])`` for i < n
    (``IpChksum`` with ``final=True``), on the GPU. ``buf`` is a device uint8 tensor.
    ``just_written``: the AIPSTACK_CHKSUM_JUST_WRITTEN hint (the bytes were written by device
    kernels with ordinary stores since they were last read); the results do not change."""
    _require_device(buf, "buf")
    if n and byte_offset + (n - 1) * stride + length > buf.numel() * buf.element_size():
        raise ValueError("batch exceeds buf")
    out = _out_tensor(out, n, buf)
    flags = (AIPSTACK_CHKSUM_FINAL if final else 0) | (
        AIPSTACK_CHKSUM_JUST_WRITTEN if just_written else 0)
    st = _lib.load().aipstack_chksum_batch_strided(
        buf.data_ptr() + byte_offset, stride, length, n, out.data_ptr(), flags,
        _stream_handle(stream, buf))
    _check(st, "aipstack_chksum_batch_strided")
    return out


def chksum_batch_csr(buf, offsets, *, out=None, final: bool = False, stream=None):
    """``out[i] = IpChksumInverted(buf[offsets[i]:offsets[i+1]])`` on the GPU. ``offsets``
    is a device int64/uint64 tensor of n+1 non-decreasing byte offsets."""
    _require_device(buf, "buf")
    _require_offsets(offsets)
    _same_device(buf, offsets, "buf and offsets")
    n = offsets.numel() - 1
    if n < 0:
        raise ValueError("offsets must hold n+1 entries")
    out = _out_tensor(out, n, buf)
    st = _lib.load().aipstack_chksum_batch_csr(
        buf.data_ptr(), offsets.data_ptr(), n, out.data_ptr(),
        AIPSTACK_CHKSUM_FINAL if final else 0, _stream_handle(stream, buf))
    _check(st, "aipstack_chksum_batch_csr")
    return out


def _require_lens(lens, n_slots_bytes, slot_stride, buf):
    torch = _torch()
    _require_device(lens, "lens")
    if lens.dtype not in (torch.int32, torch.uint32):
        raise ValueError("lens must be an int32/uint32 device tensor")
    _same_device(buf, lens, "buf and lens")
    if slot_stride <= 0 or lens.numel() * slot_stride > n_slots_bytes:
        raise ValueError("buf must hold n whole slots of slot_stride bytes")
    return lens.numel()


def chksum_batch_slotted(buf, slot_stride: int, lens, *, out=None, final: bool = False,
                         stream=None, just_written: bool = False):
    """Ring slots on the GPU: ``out[i] = IpChksumInverted(buf[i*slot_stride:][:lens[i]])``
    (``IpChksum`` with ``final=True``). ``lens``: int32/uint32 device tensor of n lengths,
    each <= min(slot_stride, 65535); ``buf`` holds n whole slots."""
    _require_device(buf, "buf")
    n = _require_lens(lens, buf.numel() * buf.element_size(), slot_stride, buf)
    out = _out_tensor(out, n, buf)
    _check(_lib.load().aipstack_chksum_batch_slotted(
        buf.data_ptr(), slot_stride, lens.data_ptr(), n, out.data_ptr(),
        (AIPSTACK_CHKSUM_FINAL if final else 0) | (AIPSTACK_CHKSUM_JUST_WRITTEN if just_written else 0),
        _stream_handle(stream, buf)),
        "aipstack_chksum_batch_slotted")
    return out


def rx_verify_slotted(frames, slot_stride: int, lens, *, out=None, stream=None):
    """Rx verify of a ring of frame slots on the GPU (frame i = the lens[i] bytes at
    frames[i*slot_stride:]); one AIPSTACK_RX_* verdict per frame."""
    _require_device(frames, "frames")
    n = _require_lens(lens, frames.numel() * frames.element_size(), slot_stride, frames)
    out = _u8_out(out, n, frames)
    _check(_lib.load().aipstack_chksum_rx_verify_slotted(
        frames.data_ptr(), slot_stride, lens.data_ptr(), n, out.data_ptr(),
        _stream_handle(stream, frames)), "aipstack_chksum_rx_verify_slotted")
    return out


def tx_fill_slotted(frames, slot_stride: int, lens, *, out=None, stream=None, split=False,
                    workspace=None):
    """Tx fill, in place, of a ring of frame slots on the GPU; one status per frame.
    ``split=True`` runs ``aipstack_chksum_tx_fill_slotted_split`` (records pass + scatter pass
    through a workspace of 8 bytes per frame, as :func:`tx_fill`); both write the same bytes."""
    _require_device(frames, "frames")
    n = _require_lens(lens, frames.numel() * frames.element_size(), slot_stride, frames)
    out = _u8_out(out, n, frames)
    lib = _lib.load()
    if not split:
        _check(lib.aipstack_chksum_tx_fill_slotted(
            frames.data_ptr(), slot_stride, lens.data_ptr(), n, out.data_ptr(),
            _stream_handle(stream, frames)), "aipstack_chksum_tx_fill_slotted")
        return out
    _split_call(lib, "aipstack_chksum_tx_fill_slotted_split", frames, n, stream, workspace,
                lambda ws, ws_bytes, h: (frames.data_ptr(), slot_stride, lens.data_ptr(), n,
                                         out.data_ptr(), ws, ws_bytes, h))
    return out


def tx_fill_records_slotted(frames, slot_stride: int, lens, *, out=None, stream=None):
    """The Tx records (see :func:`tx_fill_records`) of a ring of frame slots."""
    _require_device(frames, "frames")
    n = _require_lens(lens, frames.numel() * frames.element_size(), slot_stride, frames)
    out = _records_out(out, n, frames)
    _check(_lib.load().aipstack_chksum_tx_fill_records_slotted(
        frames.data_ptr(), slot_stride, lens.data_ptr(), n, out.data_ptr(),
        _stream_handle(stream, frames)), "aipstack_chksum_tx_fill_records_slotted")
    return out


def chksum_batch_seeded_csr(buf, offsets, states, *, out=None, stream=None):
    """``out[i] = IpChksumAccumulator(State(states[i])).getChksum(IpBufRef(packet i))`` on
    the GPU (final checksum). ``states`` is a device int32/uint32 tensor of n states."""
    _require_device(buf, "buf")
    _require_offsets(offsets)
    _require_device(states, "states")
    _same_device(buf, offsets, "buf and offsets")
    _same_device(buf, states, "buf and states")
    n = offsets.numel() - 1
    if n < 0:
        raise ValueError("offsets must hold n+1 entries")
    if states.numel() < n or states.element_size() != 4:
        raise ValueError("states must hold n 32-bit entries")
    out = _out_tensor(out, n, buf)
    st = _lib.load().aipstack_chksum_batch_seeded_csr(
        buf.data_ptr(), offsets.data_ptr(), states.data_ptr(), n, out.data_ptr(),
        _stream_handle(stream, buf))
    _check(st, "aipstack_chksum_batch_seeded_csr")
    return out


# The host-memory engines (numpy arrays in, numpy arrays out) live in engine.py, which takes
# ChksumError and the status constants from the top of this module.
from .engine import ChksumEngine, ChksumEngineGroup, _host_u32, _host_u64  # noqa: E402,F401


def _chunk_table_count(chunk_addr, chunk_len, chunk_index, fields=None) -> int:
    """Checks a chunk table's element sizes (and those of ``fields``, where the call has them);
    returns n, the chains its index of n + 1 entries holds."""
    if chunk_addr.element_size() != 8 or chunk_len.element_size() != 4 \
            or chunk_index.element_size() != 8 or (fields is not None and fields.element_size() != 8):
        wide = "chunk_addr/chunk_index" + ("" if fields is None else "/fields")
        raise ValueError(f"{wide} must be 64-bit, chunk_len 32-bit")
    n = chunk_index.numel() - 1
    if n < 0:
        raise ValueError("chunk_index must hold n+1 entries")
    return n


def _states_ptr(states, n: int):
    """The pointer to a chained batch's n states (None for no states)."""
    if states is None:
        return None
    _require_device(states, "states")
    if states.numel() < n or states.element_size() != 4:
        raise ValueError("states must hold n 32-bit entries")
    return states.data_ptr() or None


def _non_null_chunk_table(chunk_addr, chunk_len, empty: bool):
    """The chunk table as the C-ABI wants it, non-null: with no chunk at all (`empty`: pure ACKs,
    FIN-only bursts, empty datagrams) and a null table, a stand-in of one entry, which the caller
    gives to ``record_stream`` after the launch (the allocator must not reuse it before)."""
    if empty and (chunk_addr.data_ptr() == 0 or chunk_len.data_ptr() == 0):
        torch = _torch()
        chunk_addr = torch.zeros(1, dtype=torch.int64, device=chunk_addr.device)
        chunk_len = torch.zeros(1, dtype=torch.int32, device=chunk_addr.device)
    return chunk_addr, chunk_len


def chksum_batch_chain(chunk_addr, chunk_len, chunk_index, states=None, *, out=None,
                       final: bool = False, stream=None, just_written: bool = False):
    """Chained (scatter-gather) batch on the GPU: chain i = chunks
    ``[chunk_index[i], chunk_index[i+1])``, chunk k = ``chunk_len[k]`` bytes at DEVICE
    address ``chunk_addr[k]``. ``final=True`` gives
    ``IpChksumAccumulator(State(states[i])).getChksum(chain i)``; ``final=False`` its NOT.
    Tensors: int64 addresses, int32 lengths, int64 index (n+1), int32 states (or None)."""
    for t, name in ((chunk_addr, "chunk_addr"), (chunk_len, "chunk_len"),
                    (chunk_index, "chunk_index")):
        _require_device(t, name)
    n = _chunk_table_count(chunk_addr, chunk_len, chunk_index)
    sp = _states_ptr(states, n)
    out = _out_tensor(out, n, chunk_index)
    st = _lib.load().aipstack_chksum_batch_chain(
        chunk_addr.data_ptr(), chunk_len.data_ptr(), chunk_index.data_ptr(), sp, n,
        out.data_ptr(),
        (AIPSTACK_CHKSUM_FINAL if final else 0) | (AIPSTACK_CHKSUM_JUST_WRITTEN if just_written else 0),
        _stream_handle(stream, chunk_index))
    _check(st, "aipstack_chksum_batch_chain")
    return out


def chksum_chain_fill(chunk_addr, chunk_len, chunk_index, states, fields, *, out=None,
                      zero_as_ffff: bool = False, stream=None, just_written: bool = False):
    """The Tx form of :func:`chksum_batch_chain`: chain i's final checksum
    (``IpChksumAccumulator(State(states[i])).getChksum(chain i)``) is stored big-endian at
    DEVICE address ``fields[i]`` (int64 tensor; 0 = no store) -- the checksum field of the
    header the chain starts with, which must read 0 when the batch runs, as the reference
    sets it before summing (tcp/IpTcpProto_output.h:1251-1277, udp/IpUdpProto.h:164-179).
    ``zero_as_ffff`` sends a computed 0 as 0xFFFF (UDP). ``just_written``: the
    AIPSTACK_CHKSUM_JUST_WRITTEN hint (results unchanged). Returns the checksums (``out``)."""
    for t, name in ((chunk_addr, "chunk_addr"), (chunk_len, "chunk_len"),
                    (chunk_index, "chunk_index"), (fields, "fields")):
        _require_device(t, name)
    n = _chunk_table_count(chunk_addr, chunk_len, chunk_index, fields)
    if fields.numel() < n:
        raise ValueError("fields must hold n entries")
    sp = _states_ptr(states, n)
    out = _out_tensor(out, n, chunk_index)
    st = _lib.load().aipstack_chksum_batch_chain_fill(
        chunk_addr.data_ptr(), chunk_len.data_ptr(), chunk_index.data_ptr(), sp,
        fields.data_ptr(), n, out.data_ptr(),
        (AIPSTACK_CHKSUM_ZERO_AS_FFFF if zero_as_ffff else 0) |
        (AIPSTACK_CHKSUM_JUST_WRITTEN if just_written else 0),
        _stream_handle(stream, chunk_index))
    _check(st, "aipstack_chksum_batch_chain_fill")
    return out


def _u8_out(out, n, like):
    torch = _torch()
    if out is None:
        return torch.empty(n, dtype=torch.uint8, device=like.device)
    _require_device(out, "out")
    if out.element_size() != 1 or out.numel() < n:
        raise ValueError("out must be a uint8 device tensor with >= n elements")
    _same_device(out, like, "out and frames")
    return out


def rx_verify(frames, offsets, *, out=None, stream=None):
    """Rx verify on the GPU: frame i = ``frames[offsets[i]:offsets[i+1]]`` (raw Ethernet);
    returns one AIPSTACK_RX_* verdict per frame (uint8 device tensor). Read-only."""
    _require_device(frames, "frames")
    _require_offsets(offsets)
    _same_device(frames, offsets, "frames and offsets")
    n = offsets.numel() - 1
    out = _u8_out(out, max(n, 0), frames)
    _check(_lib.load().aipstack_chksum_rx_verify(frames.data_ptr(), offsets.data_ptr(), n,
                                                 out.data_ptr(), _stream_handle(stream, frames)),
           "aipstack_chksum_rx_verify")
    return out


def tx_fill(frames, offsets, *, out=None, stream=None, split=None, workspace=None):
    """Tx fill on the GPU, IN PLACE: writes the IPv4 header checksum and the TCP / UDP /
    ICMP checksum of every frame; returns one status per frame (AIPSTACK_RX_* codes).

    ``split=True`` runs the two-pass ``aipstack_chksum_tx_fill_split`` with a workspace of
    8 bytes per frame (``workspace``: a device tensor of at least that many bytes, else one
    is taken from torch's allocator); ``split=False`` the one-pass
    ``aipstack_chksum_tx_fill``; ``None`` (default) the one pass, the faster at every batch
    size measured (round 5, driver protocol, 1 M frames: 193.4 against 194.5 us on rotated
    batches, 159.8 against 161.6 on one buffer, profiles/r05/txrot, txsplit; round 2: 57
    against 61 us at 256 K). Both write the same bytes."""
    _require_device(frames, "frames")
    _require_offsets(offsets)
    _same_device(frames, offsets, "frames and offsets")
    n = offsets.numel() - 1
    out = _u8_out(out, max(n, 0), frames)
    lib = _lib.load()
    if split is None:
        split = False
    if not split:
        _check(lib.aipstack_chksum_tx_fill(frames.data_ptr(), offsets.data_ptr(), n,
                                           out.data_ptr(), _stream_handle(stream, frames)),
               "aipstack_chksum_tx_fill")
        return out
    _split_call(lib, "aipstack_chksum_tx_fill_split", frames, n, stream, workspace,
                lambda ws, ws_bytes, h: (frames.data_ptr(), offsets.data_ptr(), n,
                                         out.data_ptr(), ws, ws_bytes, h))
    return out


def _launch_stream(stream, dev):
    """`stream` as a torch stream of device `dev` (record_stream wants one): torch's current
    stream for None, an ExternalStream for a raw hipStream_t handle."""
    torch = _torch()
    launch_stream = torch.cuda.current_stream(dev) if stream is None else stream
    if not hasattr(launch_stream, "cuda_stream"):  # a raw hipStream_t handle
        launch_stream = torch.cuda.ExternalStream(int(launch_stream), device=dev)
    return launch_stream


def _workspace(workspace, need: int, like, like_name: str):
    """(workspace, its size in bytes): the caller's tensor, which must be on `like`'s device (the
    library checks its size and alignment), or `need` bytes from torch's allocator."""
    if workspace is None:
        torch = _torch()
        workspace = torch.empty(need, dtype=torch.uint8, device=like.device)
    else:
        _require_device(workspace, "workspace")
        _same_device(like, workspace, f"{like_name} and workspace")
    return workspace, workspace.numel() * workspace.element_size()


def _split_call(lib, name, frames, n, stream, workspace, args):
    """A split Tx fill (read pass + scatter pass through a workspace of 8 bytes per frame):
    ``args(workspace_ptr, workspace_bytes, stream_handle)`` gives the entry point's arguments."""
    need = int(lib.aipstack_chksum_tx_fill_workspace_bytes(max(n, 0)))
    workspace, ws_bytes = _workspace(workspace, max(need, 8), frames, "frames")
    launch_stream = _launch_stream(stream, frames.device)
    _check(getattr(lib, name)(*args(workspace.data_ptr(), ws_bytes,
                                    _stream_handle(launch_stream))), name)
    # The caching allocator must not hand the workspace out again before both passes on
    # the launch stream are done with it (it may not be torch's current stream).
    workspace.record_stream(launch_stream)


AIPSTACK_TX_SPLIT_LAYOUT = 9   # tx_fill_header_split: the split is out of layout, untouched
AIPSTACK_CHKSUM_MAX_SPLIT_HEADER = 256


def tx_fill_header_split(headers, hdr_stride: int, hdr_lens, chunk_addr, chunk_len, chunk_index,
                         *, out=None, workspace=None, just_written: bool = False, stream=None):
    """Tx fill of header-split segments on the GPU (``aipstack_chksum_tx_fill_hsplit``):
    segment i = the first ``hdr_lens[i]`` bytes of slot i of ``headers`` (a device uint8 tensor
    of n slots of ``hdr_stride`` bytes) followed by the chunks
    ``[chunk_index[i], chunk_index[i+1])`` of the chunk table (as :func:`chksum_batch_chain`:
    int64 device addresses, int32 lengths, int64 index of n+1 entries). Writes the IPv4 header
    checksum and the TCP / UDP / ICMP checksum into the header slots, as :func:`tx_fill` does
    to the linearised frames; the payload is only read. Returns one status per segment
    (AIPSTACK_RX_* codes, or AIPSTACK_TX_SPLIT_LAYOUT for a segment whose split is out of
    layout and was left untouched; chksum.h has the rule). ``workspace``: a device tensor of at
    least ``aipstack_chksum_tx_fill_hsplit_workspace_bytes(n)`` bytes (else one is taken from
    torch's allocator). ``just_written``: the AIPSTACK_CHKSUM_JUST_WRITTEN hint for the
    payload read (results unchanged)."""
    torch = _torch()
    for t, name in ((headers, "headers"), (hdr_lens, "hdr_lens"), (chunk_addr, "chunk_addr"),
                    (chunk_len, "chunk_len"), (chunk_index, "chunk_index")):
        _require_device(t, name)
        _same_device(headers, t, f"headers and {name}")
    n = _chunk_table_count(chunk_addr, chunk_len, chunk_index)
    if hdr_lens.dtype not in (torch.int32, torch.uint32):
        raise ValueError("hdr_lens must be an int32/uint32 device tensor")
    if hdr_lens.numel() < n:
        raise ValueError("hdr_lens must hold n entries")
    if hdr_stride <= 0 or n * hdr_stride > headers.numel() * headers.element_size():
        raise ValueError("headers must hold n whole slots of hdr_stride bytes")
    if chunk_addr.numel() != chunk_len.numel():
        raise ValueError("chunk_addr and chunk_len must hold one entry per chunk")
    out = _u8_out(out, n, headers)
    if n == 0:
        return out
    lib = _lib.load()
    need = int(lib.aipstack_chksum_tx_fill_hsplit_workspace_bytes(n))
    workspace, ws_bytes = _workspace(workspace, need, headers, "headers")
    launch_stream = _launch_stream(stream, headers.device)
    chunk_addr, chunk_len = _non_null_chunk_table(chunk_addr, chunk_len, chunk_addr.numel() == 0)
    _check(lib.aipstack_chksum_tx_fill_hsplit(
        headers.data_ptr(), hdr_stride, hdr_lens.data_ptr(), chunk_addr.data_ptr(),
        chunk_len.data_ptr(), chunk_index.data_ptr(), n, out.data_ptr(), workspace.data_ptr(),
        ws_bytes, AIPSTACK_CHKSUM_JUST_WRITTEN if just_written else 0,
        _stream_handle(launch_stream)), "aipstack_chksum_tx_fill_hsplit")
    # as _split_call: the allocator must not reuse the workspace (or a stand-in chunk table)
    # before the launch stream has passed the call
    for t in (workspace, chunk_addr, chunk_len):
        t.record_stream(launch_stream)
    return out


# What differs between the two Tx producers for _tx_produce. min_hdr: the longest header, the
# least hdr_stride. descs, index, count, owners: the caller's names, for the messages.
# workspace_bytes(lib, n_owners, n). outs: the tensors of an `out=` result (attribute, its name,
# element size, which of (n, n_chunks, n + 1, n_owners) it holds at least). owner_status: the
# result's per-owner status, for a producer that writes one and hdr_lens (UDP).
_TxProducer = collections.namedtuple(
    "_TxProducer", "entry dtype min_hdr result descs index count owners workspace_bytes outs "
    "owner_status", defaults=(None,))
_TX_OUTS = (("chunk_addr", "out.chunk_addr", 8, 1), ("chunk_len", "out.chunk_len", 4, 1),
            ("chunk_index", "out.chunk_index", 8, 2), ("status", "out.status", 1, 0))


def _tx_produce(p, descs, index, chunk_base, n, n_chunks, *, hdr_stride, headers, just_written,
                stream, workspace, out, device):
    """What :func:`tcp_tx_segment` and :func:`udp_tx_fragment` share: the entry point of the
    :class:`_TxProducer` `p` on the owners `descs` (host arrays, uploaded on the launch stream, or
    device tensors) with their running sums `index` and `chunk_base`, into `out` or a fresh
    result of ``p.result``."""
    torch = _torch()
    size = p.dtype.itemsize
    if hasattr(index, "data_ptr"):
        if n is None or n_chunks is None:
            raise ValueError(f"device {p.index}/chunk_base need {p.count} and n_chunks")
        _require_device(descs, p.descs)
        _require_device(index, p.index)
        _require_device(chunk_base, "chunk_base")
        if index.element_size() != 8 or chunk_base.element_size() != 8:
            raise ValueError(f"{p.index}/chunk_base must be 64-bit")
        if index.numel() != chunk_base.numel() or index.numel() < 1:
            raise ValueError(f"{p.index} and chunk_base must hold {p.owners} + 1 entries each")
        n_owners = index.numel() - 1
        if descs.numel() * descs.element_size() < size * n_owners:
            raise ValueError(f"{p.descs} must hold {p.owners} descriptors of {size} bytes")
        d_descs, d_index, d_base = descs, index, chunk_base
        dev = descs.device
    else:
        g = np.ascontiguousarray(descs, dtype=p.dtype).reshape(-1)
        ix = np.array(index, dtype=np.uint64).reshape(-1)   # (copies: torch wants them writable)
        cb = np.array(chunk_base, dtype=np.uint64).reshape(-1)
        if ix.size != g.size + 1 or cb.size != g.size + 1:
            raise ValueError(f"{p.index} and chunk_base must hold len({p.descs}) + 1 entries each")
        n_owners = g.size
        n = int(ix[-1]) if n is None else n
        n_chunks = int(cb[-1]) if n_chunks is None else n_chunks
        if out is not None:
            dev = out.headers.device
        elif headers is not None:
            dev = headers.device
        else:
            dev = torch.device("cuda" if device is None else device)
        raw = np.zeros(max(g.size, 1) * size, dtype=np.uint8)
        raw[:g.size * size] = g.view(np.uint8)
        with torch.cuda.stream(_launch_stream(stream, dev)):  # uploads ordered before the call
            d_descs = torch.from_numpy(raw).to(dev)
            d_index = torch.from_numpy(ix.view(np.int64)).to(dev)
            d_base = torch.from_numpy(cb.view(np.int64)).to(dev)
    n, nc = int(n), int(n_chunks)
    if n < 0 or nc < 0:
        raise ValueError(f"{p.count} and n_chunks must not be negative")
    udp = p.owner_status is not None  # the producer writes hdr_lens and a per-owner status
    if out is not None:
        headers, hdr_stride = out.headers, out.hdr_stride
        least = (n, nc, n + 1, n_owners)
        for attr, name, esize, which in p.outs:
            t = getattr(out, attr)
            _require_device(t, name)
            if t.element_size() != esize or t.numel() < least[which]:
                raise ValueError(f"{name} is too small or of the wrong element size")
        if out.chunk_index.numel() != n + 1 or out.status.numel() != n \
                or (udp and out.hdr_lens.numel() != n):
            raise ValueError("out.chunk_index must hold n + 1 entries, out.status"
                             + (" and out.hdr_lens" if udp else "") + " n")
    if hdr_stride < p.min_hdr:
        raise ValueError(f"hdr_stride must be at least {p.min_hdr}")
    if headers is None:
        headers = torch.zeros(max(n * hdr_stride, 1), dtype=torch.uint8, device=dev)
    else:
        _require_device(headers, "headers")
        if headers.element_size() != 1 or headers.numel() < n * hdr_stride:
            raise ValueError("headers must be a uint8 tensor of n whole slots of hdr_stride bytes")
    if headers.device != d_descs.device:
        raise ValueError(f"headers and {p.descs} must be on the same device")
    res = out
    if out is None:
        def zeros(cnt, dt):  # (storage of 1 entry at least: the C-ABI wants non-null arrays)
            return torch.zeros(max(cnt, 1), dtype=dt, device=dev)[:cnt]
        tables = (zeros(nc, torch.int64), zeros(nc, torch.int32),
                  torch.zeros(n + 1, dtype=torch.int64, device=dev),
                  torch.empty(n, dtype=torch.uint8, device=dev))
        if udp:
            res = p.result(headers, hdr_stride, zeros(n, torch.int32), *tables,
                           zeros(n_owners, torch.uint8))
        else:
            res = p.result(headers, hdr_stride, *tables)
    if n == 0:
        return res
    lib = _lib.load()
    workspace, ws_bytes = _workspace(workspace, int(p.workspace_bytes(lib, n_owners, n)), headers,
                                     "headers")
    launch_stream = _launch_stream(stream, dev)
    ca, cl = _non_null_chunk_table(res.chunk_addr, res.chunk_len, nc == 0)
    flags = AIPSTACK_CHKSUM_JUST_WRITTEN if just_written else 0
    fn = getattr(lib, p.entry)
    if udp:
        os_ = getattr(res, p.owner_status)
        if n_owners == 0 and os_.data_ptr() == 0:  # no owner: a non-null array all the same
            os_ = torch.zeros(1, dtype=torch.uint8, device=dev)
        st = fn(d_descs.data_ptr(), d_index.data_ptr(), d_base.data_ptr(), n_owners, n, nc,
                headers.data_ptr(), hdr_stride, res.hdr_lens.data_ptr(), ca.data_ptr(),
                cl.data_ptr(), res.chunk_index.data_ptr(), res.status.data_ptr(), os_.data_ptr(),
                workspace.data_ptr(), ws_bytes, flags, _stream_handle(launch_stream))
    else:
        st = fn(d_descs.data_ptr(), d_index.data_ptr(), d_base.data_ptr(), n_owners, n, nc,
                headers.data_ptr(), hdr_stride, ca.data_ptr(), cl.data_ptr(),
                res.chunk_index.data_ptr(), res.status.data_ptr(), workspace.data_ptr(), ws_bytes,
                flags, _stream_handle(launch_stream))
    _check(st, p.entry)
    # the allocator must not reuse the workspace, the uploaded descriptors or a stand-in array
    # before the launch stream has passed the call
    for t in (workspace, d_descs, d_index, d_base, ca, cl):
        t.record_stream(launch_stream)
    if udp:
        os_.record_stream(launch_stream)
    return res


AIPSTACK_TCP_SEGMENT_HEADER = 54   # Ethernet 14 + IPv4 20 + TCP 20
AIPSTACK_TCP_BURST_FIN = 1         # burst flag: the last segment carries FIN|PSH
AIPSTACK_TX_BURST_INVALID = 10     # tcp_tx_segment: the segment's burst breaks the contract

# ``aipstack_tcp_burst`` (chksum.h): one TCP data burst of one connection, host-made.
TCP_BURST_DTYPE = np.dtype({
    "names": ["data_addr", "data_len", "seq", "psh_offset", "mss", "ip_id", "flags", "reserved",
              "hdr"],
    "formats": [("<u8", (2,)), ("<u4", (2,)), "<u4", "<u4", "<u2", "<u2", "u1", ("u1", (3,)),
                ("u1", (56,))],
    "offsets": [0, 16, 24, 28, 32, 34, 36, 37, 40],
    "itemsize": 96,
})
assert TCP_BURST_DTYPE.itemsize == 96


def tcp_burst_layout(bursts):
    """Host side of :func:`tcp_tx_segment` (``aipstack_tcp_burst_layout``, no GPU): the segment
    and chunk counts of each burst of ``bursts`` (a ``TCP_BURST_DTYPE`` array) as running sums,
    ``(seg_index, chunk_base)``, uint64 arrays of ``len(bursts) + 1`` entries. Raises
    :class:`ChksumError` (``AIPSTACK_CHKSUM_EINVAL``) if a burst breaks the contract."""
    b = np.ascontiguousarray(bursts, dtype=TCP_BURST_DTYPE).reshape(-1)
    seg_index = np.zeros(b.size + 1, dtype=np.uint64)
    chunk_base = np.zeros(b.size + 1, dtype=np.uint64)
    _check(_lib.load().aipstack_tcp_burst_layout(b.ctypes.data if b.size else None, b.size,
                                                 seg_index.ctypes.data, chunk_base.ctypes.data),
           "aipstack_tcp_burst_layout")
    return seg_index, chunk_base


class TcpSegments:
    """What :func:`tcp_tx_segment` leaves (device tensors): ``headers`` (uint8, n slots of
    ``hdr_stride`` bytes), the chunk table ``chunk_addr`` (int64) / ``chunk_len`` (int32) /
    ``chunk_index`` (int64, n + 1 entries) and ``status`` (uint8, n). ``hdr_lens`` (int32, all
    54, made on first use) completes the arguments of :func:`tx_fill_header_split`; the chunk
    table is what :func:`chksum_batch_chain` takes."""

    def __init__(self, headers, hdr_stride, chunk_addr, chunk_len, chunk_index, status):
        self.headers, self.hdr_stride = headers, hdr_stride
        self.chunk_addr, self.chunk_len, self.chunk_index = chunk_addr, chunk_len, chunk_index
        self.status = status
        self._hdr_lens = None

    @property
    def n_segments(self) -> int:
        return self.chunk_index.numel() - 1

    @property
    def hdr_lens(self):
        if self._hdr_lens is None:
            torch = _torch()
            self._hdr_lens = torch.full((self.n_segments,), AIPSTACK_TCP_SEGMENT_HEADER,
                                        dtype=torch.int32, device=self.headers.device)
        return self._hdr_lens


def tcp_tx_segment(bursts, seg_index, chunk_base, *, hdr_stride: int = 64, headers=None,
                   just_written: bool = False, stream=None, workspace=None, out=None,
                   n_segments: Optional[int] = None, n_chunks: Optional[int] = None,
                   device=None) -> TcpSegments:
    """TCP burst segmentation on the GPU (``aipstack_tcp_tx_segment``): for every burst of
    ``bursts`` (``TCP_BURST_DTYPE``), every segment's complete 54-byte frame header in slot i of
    a header ring, the chunk table of its data bytes and both checksums -- what the reference's
    ``pcb_output_segment`` / ``sendSegment`` / ``sendIp4DgramFast`` loop produces.

    ``bursts``, ``seg_index``, ``chunk_base``: host numpy arrays (the latter two from
    :func:`tcp_burst_layout`; uploaded here), or device tensors already resident (uint8 /
    int64 / int64), in which case ``n_segments`` and ``n_chunks`` (the last index entries) must
    be given. ``headers``: the ring to write (device uint8 tensor of at least n slots of
    ``hdr_stride`` bytes; else a fresh one). ``out``: a :class:`TcpSegments` whose tensors are
    reused (``headers`` / ``hdr_stride`` then come from it). ``workspace``: a device tensor of
    at least ``aipstack_tcp_tx_segment_workspace_bytes(n)`` bytes, 8-byte aligned.
    ``just_written``: the AIPSTACK_CHKSUM_JUST_WRITTEN hint for the data read. Status per
    segment: ``AIPSTACK_RX_ACCEPT``, or ``AIPSTACK_TX_BURST_INVALID`` (slot untouched)."""
    return _tx_produce(_TCP_SEGMENTS, bursts, seg_index, chunk_base, n_segments, n_chunks,
                       hdr_stride=hdr_stride, headers=headers, just_written=just_written,
                       stream=stream, workspace=workspace, out=out, device=device)


_TCP_SEGMENTS = _TxProducer(
    entry="aipstack_tcp_tx_segment", dtype=TCP_BURST_DTYPE, min_hdr=AIPSTACK_TCP_SEGMENT_HEADER,
    result=TcpSegments, descs="bursts", index="seg_index", count="n_segments", owners="n_bursts",
    outs=_TX_OUTS,
    workspace_bytes=lambda lib, n_bursts, n: lib.aipstack_tcp_tx_segment_workspace_bytes(n))


AIPSTACK_UDP_FIRST_FRAGMENT_HEADER = 42   # Ethernet 14 + IPv4 20 + UDP 8
AIPSTACK_UDP_NEXT_FRAGMENT_HEADER = 34    # Ethernet 14 + IPv4 20: fragments after the first
AIPSTACK_UDP_MIN_MTU = 256
AIPSTACK_TX_FRAG_NEEDED = 12       # udp_tx_fragment: above the MTU with DF set, nothing emitted
AIPSTACK_TX_DGRAM_INVALID = 13     # udp_tx_fragment: the datagram breaks the contract

# ``aipstack_udp_dgram`` (chksum.h): one UDP datagram to send, host-made.
UDP_DGRAM_DTYPE = np.dtype({
    "names": ["data_addr", "data_len", "mtu", "ip_id", "reserved", "hdr"],
    "formats": [("<u8", (2,)), ("<u4", (2,)), "<u2", "<u2", "<u4", ("u1", (48,))],
    "offsets": [0, 16, 24, 26, 28, 32],
    "itemsize": 80,
})
assert UDP_DGRAM_DTYPE.itemsize == 80


def udp_dgram_layout(dgrams):
    """Host side of :func:`udp_tx_fragment` (``aipstack_udp_dgram_layout``, no GPU): the fragment
    and chunk counts of each datagram of ``dgrams`` (a ``UDP_DGRAM_DTYPE`` array) as running
    sums and each datagram's status, ``(frag_index, chunk_base, status)``: uint64 arrays of
    ``len(dgrams) + 1`` entries and a uint8 array (``AIPSTACK_RX_ACCEPT``, or
    ``AIPSTACK_TX_FRAG_NEEDED`` for a datagram above its MTU with DF set: no fragment, no
    chunk). Raises :class:`ChksumError` (``AIPSTACK_CHKSUM_EINVAL``) if a datagram breaks the
    contract."""
    g = np.ascontiguousarray(dgrams, dtype=UDP_DGRAM_DTYPE).reshape(-1)
    frag_index = np.zeros(g.size + 1, dtype=np.uint64)
    chunk_base = np.zeros(g.size + 1, dtype=np.uint64)
    status = np.zeros(max(g.size, 1), dtype=np.uint8)
    _check(_lib.load().aipstack_udp_dgram_layout(g.ctypes.data if g.size else None, g.size,
                                                 frag_index.ctypes.data, chunk_base.ctypes.data,
                                                 status.ctypes.data),
           "aipstack_udp_dgram_layout")
    return frag_index, chunk_base, status[:g.size]


class UdpFragments:
    """What :func:`udp_tx_fragment` leaves (device tensors): ``headers`` (uint8, n slots of
    ``hdr_stride`` bytes), ``hdr_lens`` (int32, n: 42 for a datagram's first fragment, 34 for
    the others, 0 where nothing was emitted), the chunk table ``chunk_addr`` (int64) /
    ``chunk_len`` (int32) / ``chunk_index`` (int64, n + 1 entries), ``status`` (uint8, n) and
    ``dgram_status`` (uint8, one per datagram). Headers, lengths and the chunk table are the
    arguments of :func:`tx_fill_header_split`; the chunk table is what
    :func:`chksum_batch_chain` takes."""

    def __init__(self, headers, hdr_stride, hdr_lens, chunk_addr, chunk_len, chunk_index, status,
                 dgram_status):
        self.headers, self.hdr_stride, self.hdr_lens = headers, hdr_stride, hdr_lens
        self.chunk_addr, self.chunk_len, self.chunk_index = chunk_addr, chunk_len, chunk_index
        self.status, self.dgram_status = status, dgram_status

    @property
    def n_frags(self) -> int:
        return self.chunk_index.numel() - 1


def udp_tx_fragment(dgrams, frag_index, chunk_base, *, hdr_stride: int = 64, headers=None,
                    just_written: bool = False, stream=None, workspace=None, out=None,
                    n_frags: Optional[int] = None, n_chunks: Optional[int] = None,
                    device=None) -> UdpFragments:
    """UDP send with IPv4 fragmentation on the GPU (``aipstack_udp_tx_fragment``): for every
    datagram of ``dgrams`` (``UDP_DGRAM_DTYPE``), every fragment's complete frame header in slot
    i of a header ring (one fragment for a datagram that fits its MTU), the chunk table of its
    data bytes, the IPv4 header checksums and the UDP checksum -- what the reference's
    ``sendUdpIp4Packet`` / ``sendIp4Dgram`` / ``send_fragmented`` produce.

    ``dgrams``, ``frag_index``, ``chunk_base``: host numpy arrays (the latter two from
    :func:`udp_dgram_layout`; uploaded here), or device tensors already resident (uint8 /
    int64 / int64), in which case ``n_frags`` and ``n_chunks`` (the last index entries) must be
    given. ``headers``: the ring to write (device uint8 tensor of at least n slots of
    ``hdr_stride`` bytes; else a fresh one). ``out``: a :class:`UdpFragments` whose tensors are
    reused (``headers`` / ``hdr_stride`` then come from it). ``workspace``: a device tensor of
    at least ``aipstack_udp_tx_fragment_workspace_bytes(n_dgrams, n)`` bytes, 8-byte aligned.
    ``just_written``: the AIPSTACK_CHKSUM_JUST_WRITTEN hint for the data read. Status per
    fragment: ``AIPSTACK_RX_ACCEPT``, or ``AIPSTACK_TX_DGRAM_INVALID`` (slot untouched); per
    datagram also ``AIPSTACK_TX_FRAG_NEEDED``. With no fragment at all nothing runs and
    ``dgram_status`` is not written (:func:`udp_dgram_layout` has it)."""
    return _tx_produce(_UDP_FRAGMENTS, dgrams, frag_index, chunk_base, n_frags, n_chunks,
                       hdr_stride=hdr_stride, headers=headers, just_written=just_written,
                       stream=stream, workspace=workspace, out=out, device=device)


_UDP_FRAGMENTS = _TxProducer(
    entry="aipstack_udp_tx_fragment", dtype=UDP_DGRAM_DTYPE,
    min_hdr=AIPSTACK_UDP_FIRST_FRAGMENT_HEADER, result=UdpFragments, descs="dgrams",
    index="frag_index", count="n_frags", owners="n_dgrams", owner_status="dgram_status",
    outs=_TX_OUTS + (("hdr_lens", "out.hdr_lens", 4, 0), ("dgram_status", "out.dgram_status", 1, 3)),
    workspace_bytes=lambda lib, n_dgrams, n: lib.aipstack_udp_tx_fragment_workspace_bytes(n_dgrams, n))


AIPSTACK_RX_DROP_TCP_OFFSET = 11    # tcp_rx_parse: TCP checksum good, data offset out of range
AIPSTACK_TCP_NO_PCB = 0xFFFFFFFF
AIPSTACK_TCP_OPT_MSS = 1            # = TcpOptionFlags::Mss
AIPSTACK_TCP_OPT_WND_SCALE = 2      # = TcpOptionFlags::WndScale
AIPSTACK_TCP_SEG_VALID = 0x80

# ``aipstack_tcp_rx_seg`` (chksum.h): one parsed TCP segment, host byte order.
TCP_RX_SEG_DTYPE = np.dtype({
    "names": ["remote_addr", "local_addr", "remote_port", "local_port", "seq_num", "ack_num",
              "flags", "window_size", "data_off", "data_len", "mss", "wnd_scale", "opts"],
    "formats": ["<u4", "<u4", "<u2", "<u2", "<u4", "<u4", "<u2", "<u2", "<u2", "<u2", "<u2", "u1",
                "u1"],
    "offsets": [0, 4, 8, 10, 12, 16, 20, 22, 24, 26, 28, 30, 31],
    "itemsize": 32,
})
# ``aipstack_tcp_pcb_key`` (chksum.h): one entry of the PCB table.
TCP_PCB_KEY_DTYPE = np.dtype({
    "names": ["local_addr", "remote_addr", "local_port", "remote_port", "cookie"],
    "formats": ["<u4", "<u4", "<u2", "<u2", "<u4"],
    "offsets": [0, 4, 8, 10, 12],
    "itemsize": 16,
})
assert TCP_RX_SEG_DTYPE.itemsize == 32 and TCP_PCB_KEY_DTYPE.itemsize == 16


def tcp_pcb_table_sort(keys):
    """Host side of :func:`tcp_rx_parse` (``aipstack_tcp_pcb_table_sort``, no GPU): a copy of
    ``keys`` (a ``TCP_PCB_KEY_DTYPE`` array) sorted into the order of the reference's
    ``CompareKeys`` (remote_port, remote_addr, local_port, local_addr), the order the lookup
    searches. Raises :class:`ChksumError` (``AIPSTACK_CHKSUM_EINVAL``) for a duplicate key or a
    cookie equal to ``AIPSTACK_TCP_NO_PCB``."""
    k = np.array(keys, dtype=TCP_PCB_KEY_DTYPE).reshape(-1)
    _check(_lib.load().aipstack_tcp_pcb_table_sort(k.ctypes.data if k.size else None, k.size),
           "aipstack_tcp_pcb_table_sort")
    return k


class TcpRxParsed:
    """What :func:`tcp_rx_parse` leaves (device tensors): ``verdict`` (uint8, n), ``segs`` (uint8,
    n * 32 bytes: n ``aipstack_tcp_rx_seg`` records) and ``pcb`` (int32, n: the cookies, bit
    pattern of ``AIPSTACK_TCP_NO_PCB`` = -1 where no PCB matches)."""

    def __init__(self, verdict, segs, pcb):
        self.verdict, self.segs, self.pcb = verdict, segs, pcb

    @property
    def n(self) -> int:
        return self.verdict.numel()

    def segs_numpy(self) -> np.ndarray:
        """The records on the host as a ``TCP_RX_SEG_DTYPE`` array (synchronises)."""
        return self.segs[:self.n * 32].cpu().numpy().view(TCP_RX_SEG_DTYPE)

    def pcb_numpy(self) -> np.ndarray:
        """The cookies on the host as uint32 (synchronises)."""
        return self.pcb[:self.n].cpu().numpy().view(np.uint32)


def _rx_parse_outputs(n, frames, verdict, segs, pcb):
    torch = _torch()
    verdict = _u8_out(verdict, n, frames)
    if segs is None:
        segs = torch.empty(n * 32, dtype=torch.uint8, device=frames.device)
    else:
        _require_device(segs, "segs")
        if segs.element_size() != 1 or segs.numel() < n * 32:
            raise ValueError("segs must be a uint8 device tensor of at least n * 32 bytes")
        _same_device(segs, frames, "segs and frames")
    if pcb is None:
        pcb = torch.empty(n, dtype=torch.int32, device=frames.device)
    else:
        _require_device(pcb, "pcb")
        if pcb.element_size() != 4 or pcb.numel() < n:
            raise ValueError("pcb must be an int32/uint32 device tensor with >= n elements")
        _same_device(pcb, frames, "pcb and frames")
    return verdict, segs, pcb


def _rx_parse_table(pcbs, frames):
    """(pointer, entries, tensor to keep alive) of the PCB table: None, a device uint8 tensor of
    whole 16-byte entries, or a host ``TCP_PCB_KEY_DTYPE`` array (uploaded here)."""
    torch = _torch()
    if pcbs is None:
        return 0, 0, None
    if not hasattr(pcbs, "data_ptr"):
        k = np.ascontiguousarray(pcbs, dtype=TCP_PCB_KEY_DTYPE).reshape(-1)
        if k.size == 0:
            return 0, 0, None
        pcbs = torch.from_numpy(k.view(np.uint8).copy()).to(frames.device)
    _require_device(pcbs, "pcbs")
    _same_device(pcbs, frames, "pcbs and frames")
    nbytes = pcbs.numel() * pcbs.element_size()
    if nbytes % 16:
        raise ValueError("pcbs must hold whole 16-byte entries")
    return (pcbs.data_ptr() if nbytes else 0), nbytes // 16, pcbs


def _rx_parse_call(name, frames, where, n, pcbs, verdict, segs, pcb, stream):
    """What the two parse entry points share: the outputs, the PCB table (uploaded on the
    launch stream), the call `name` on n frames laid out by `where`, the table kept alive."""
    verdict, segs, pcb = _rx_parse_outputs(n, frames, verdict, segs, pcb)
    launch_stream = _launch_stream(stream, frames.device)
    with _torch().cuda.stream(launch_stream):  # an upload is ordered before the call
        tp, tn, keep = _rx_parse_table(pcbs, frames)
    _check(getattr(_lib.load(), name)(
        frames.data_ptr(), *where, n, tp, tn, verdict.data_ptr(), segs.data_ptr(),
        pcb.data_ptr(), _stream_handle(launch_stream)), name)
    if keep is not None and keep is not pcbs:
        keep.record_stream(launch_stream)
    return TcpRxParsed(verdict, segs, pcb)


def tcp_rx_parse(frames, offsets, pcbs=None, *, verdict=None, segs=None, pcb=None, stream=None):
    """Rx verify plus the TCP parse on the GPU (``aipstack_tcp_rx_parse``): frame i =
    ``frames[offsets[i]:offsets[i+1]]``. Per frame the verdict of :func:`rx_verify` (an accepted
    TCP frame whose data offset is out of range becomes ``AIPSTACK_RX_DROP_TCP_OFFSET``), for an
    accepted TCP frame the ``aipstack_tcp_rx_seg`` record (segment fields, where the data lies,
    the MSS / window-scale options as the reference's ``ParseTcpOptions`` reads them), and the
    cookie of its PCB in ``pcbs``: a table sorted by :func:`tcp_pcb_table_sort`, a host
    ``TCP_PCB_KEY_DTYPE`` array (uploaded on the launch stream) or a device uint8 tensor already
    resident; ``None`` = no table. Returns a :class:`TcpRxParsed`."""
    _require_device(frames, "frames")
    _require_offsets(offsets)
    _same_device(frames, offsets, "frames and offsets")
    n = max(offsets.numel() - 1, 0)
    return _rx_parse_call("aipstack_tcp_rx_parse", frames, (offsets.data_ptr(),), n, pcbs,
                          verdict, segs, pcb, stream)


def tcp_rx_parse_slotted(frames, slot_stride: int, lens, pcbs=None, *, verdict=None, segs=None,
                         pcb=None, stream=None):
    """:func:`tcp_rx_parse` on a ring of frame slots (frame i = the lens[i] bytes at
    ``frames[i*slot_stride:]``, as :func:`rx_verify_slotted`)."""
    _require_device(frames, "frames")
    n = _require_lens(lens, frames.numel() * frames.element_size(), slot_stride, frames)
    return _rx_parse_call("aipstack_tcp_rx_parse_slotted", frames,
                          (slot_stride, lens.data_ptr()), n, pcbs, verdict, segs, pcb, stream)


AIPSTACK_RX_FRAG_MEMBER = 14       # ip4_rx_reassemble: fragment of a datagram reassembled in this batch
AIPSTACK_RX_DROP_FRAG = 15         # ip4_rx_reassemble: fragment reassembleIp4 ignores or rejects by itself
AIPSTACK_RX_REASS_TRUNCATED = 16   # per datagram: UDP length below the reassembled length
AIPSTACK_REASS_NONE = 0xFFFFFFFF
AIPSTACK_IP4_MAX_REASS_SIZE = 65531

# ``aipstack_ip4_dgram`` (chksum.h): one reassembled datagram, at its head frame's index.
IP4_DGRAM_DTYPE = np.dtype({
    "names": ["n_frags", "last_frame", "data_len", "proto", "verdict", "reserved"],
    "formats": ["<u4", "<u4", "<u2", "u1", "u1", "<u4"],
    "offsets": [0, 4, 8, 10, 11, 12],
    "itemsize": 16,
})
assert IP4_DGRAM_DTYPE.itemsize == 16


def ip4_reass_workspace_bytes(n: int) -> int:
    """``aipstack_ip4_reass_workspace_bytes``: the workspace :func:`ip4_rx_reassemble` needs for
    n frames."""
    return int(_lib.load().aipstack_ip4_reass_workspace_bytes(max(n, 0)))


class Ip4Reassembled:
    """What :func:`ip4_rx_reassemble` leaves (device tensors, n frames): ``verdict`` (uint8),
    ``chunk_addr`` (int64: device addresses), ``chunk_len``, ``next``, ``head`` (int32; the bit
    pattern of ``AIPSTACK_REASS_NONE`` = -1 for no link) and ``dgram`` (uint8, n * 16 bytes: n
    ``aipstack_ip4_dgram`` records, zero except at head frames)."""

    def __init__(self, verdict, chunk_addr, chunk_len, next, head, dgram):  # noqa: A002
        self.verdict, self.chunk_addr, self.chunk_len = verdict, chunk_addr, chunk_len
        self.next, self.head, self.dgram = next, head, dgram

    @property
    def n(self) -> int:
        return self.verdict.numel()

    def dgram_numpy(self) -> np.ndarray:
        """The datagram records on the host as an ``IP4_DGRAM_DTYPE`` array (synchronises)."""
        return self.dgram[:self.n * 16].cpu().numpy().view(IP4_DGRAM_DTYPE)

    def next_numpy(self) -> np.ndarray:
        return self.next[:self.n].cpu().numpy().view(np.uint32)

    def head_numpy(self) -> np.ndarray:
        return self.head[:self.n].cpu().numpy().view(np.uint32)


def _reass_out(t, n, itemsize, dtype, frames, name):
    torch = _torch()
    if t is None:
        return torch.empty(n, dtype=dtype, device=frames.device)
    _require_device(t, name)
    if t.element_size() != itemsize or t.numel() < n:
        raise ValueError(f"{name} must be a device tensor of >= n {itemsize}-byte elements")
    _same_device(t, frames, f"{name} and frames")
    return t


def _reass_call(name, frames, where, n, max_reass_size, verdict, chunk_addr, chunk_len, next,  # noqa: A002
                head, dgram, workspace, stream):
    """What the two reassembly entry points share: the outputs, the workspace, the call `name`
    on n frames laid out by `where`."""
    torch = _torch()
    lib = _lib.load()
    verdict = _u8_out(verdict, n, frames)
    chunk_addr = _reass_out(chunk_addr, n, 8, torch.int64, frames, "chunk_addr")
    chunk_len = _reass_out(chunk_len, n, 4, torch.int32, frames, "chunk_len")
    next = _reass_out(next, n, 4, torch.int32, frames, "next")  # noqa: A001
    head = _reass_out(head, n, 4, torch.int32, frames, "head")
    dgram = _reass_out(dgram, n * 16, 1, torch.uint8, frames, "dgram")
    need = int(lib.aipstack_ip4_reass_workspace_bytes(n))
    workspace, ws_bytes = _workspace(workspace, need, frames, "frames")
    launch_stream = _launch_stream(stream, frames.device)
    _check(getattr(lib, name)(
        frames.data_ptr(), *where, n, max_reass_size, verdict.data_ptr(), chunk_addr.data_ptr(),
        chunk_len.data_ptr(), next.data_ptr(), head.data_ptr(), dgram.data_ptr(),
        workspace.data_ptr(), ws_bytes, _stream_handle(launch_stream)), name)
    workspace.record_stream(launch_stream)
    return Ip4Reassembled(verdict, chunk_addr, chunk_len, next, head, dgram)


def ip4_rx_reassemble(frames, offsets, *, max_reass_size: int = AIPSTACK_IP4_MAX_REASS_SIZE,
                      verdict=None, chunk_addr=None, chunk_len=None, next=None, head=None,  # noqa: A002
                      dgram=None, workspace=None, stream=None):
    """Rx verify plus IPv4 reassembly on the GPU (``aipstack_ip4_rx_reassemble``): frame i =
    ``frames[offsets[i]:offsets[i+1]]``. The fragments of the batch are grouped by (source,
    destination, ident, protocol); a group that is one complete datagram (``max_reass_size`` = the
    reference's ``MaxReassSize``) gets verdict ``AIPSTACK_RX_FRAG_MEMBER`` on every member, its
    members linked in offset order (``head``, ``next``) and, at its head frame, an
    ``aipstack_ip4_dgram`` record with the verdict of the TCP / UDP / ICMP checksum over the
    linked payload; every other group is left whole for the host's reassembly (verdict 3), but
    for empty and oversize fragments (``AIPSTACK_RX_DROP_FRAG``). ``chunk_addr`` / ``chunk_len``
    give every fragment's payload where it lies: nothing is copied. ``workspace``: a device tensor
    of at least :func:`ip4_reass_workspace_bytes` bytes, else one is taken from torch's allocator.
    Returns an :class:`Ip4Reassembled`."""
    _require_device(frames, "frames")
    _require_offsets(offsets)
    _same_device(frames, offsets, "frames and offsets")
    n = max(offsets.numel() - 1, 0)
    return _reass_call("aipstack_ip4_rx_reassemble", frames, (offsets.data_ptr(),), n,
                       max_reass_size, verdict, chunk_addr, chunk_len, next, head, dgram, workspace,
                       stream)


def ip4_rx_reassemble_slotted(frames, slot_stride: int, lens, *,
                              max_reass_size: int = AIPSTACK_IP4_MAX_REASS_SIZE, verdict=None,
                              chunk_addr=None, chunk_len=None, next=None, head=None, dgram=None,  # noqa: A002
                              workspace=None, stream=None):
    """:func:`ip4_rx_reassemble` on a ring of frame slots (frame i = the lens[i] bytes at
    ``frames[i*slot_stride:]``, as :func:`rx_verify_slotted`)."""
    _require_device(frames, "frames")
    n = _require_lens(lens, frames.numel() * frames.element_size(), slot_stride, frames)
    return _reass_call("aipstack_ip4_rx_reassemble_slotted", frames, (slot_stride, lens.data_ptr()),
                       n, max_reass_size, verdict, chunk_addr, chunk_len, next, head, dgram,
                       workspace, stream)


AIPSTACK_TX_LIN_WRITTEN = 17     # tx_linearise: the frame's L bytes are in place
AIPSTACK_TX_LIN_SKIPPED = 18     # the producer emitted nothing for this segment
AIPSTACK_TX_LIN_INVALID = 19     # header length, a chunk length or the index breaks the contract
AIPSTACK_TX_LIN_TOO_SHORT = 20   # L < 14 (sendFrame's HardwareError)
AIPSTACK_TX_LIN_TOO_LARGE = 21   # L > frame_max (sendFrame's PacketTooLarge)
AIPSTACK_TX_LIN_WRONG_ROOM = 22  # offsets form: L is not offsets[i+1] - offsets[i]
AIPSTACK_CHKSUM_MAX_SLOT_STRIDE = 65536


class LinearFrames:
    """What :func:`tx_linearise` / :func:`tx_linearise_slotted` leave: ``frames`` (the caller's
    uint8 ring, frame i at ``offsets[i]`` or at ``i * slot_stride``; the one that does not apply
    is None), ``lens`` (int32, n: the frame's length where it was written, else 0) and
    ``status`` (uint8, n: AIPSTACK_TX_LIN_*). ``frames``, ``slot_stride`` and ``lens`` are the
    arguments of the ring-slot calls (:func:`rx_verify_slotted`, :func:`tcp_rx_parse_slotted`,
    :func:`ip4_rx_reassemble_slotted`, :func:`tx_fill_slotted`)."""

    def __init__(self, frames, slot_stride, offsets, lens, status):
        self.frames, self.slot_stride, self.offsets = frames, slot_stride, offsets
        self.lens, self.status = lens, status

    @property
    def n(self) -> int:
        return self.status.numel()


def _linearise_call(name, where, segments, headers, hdr_stride, hdr_lens, chunk_addr, chunk_len,
                    chunk_index, seg_status, frames, frame_max, lens, status, just_written, stream):
    torch = _torch()
    if segments is not None:  # a TcpSegments / UdpFragments object: its tensors and statuses
        headers, hdr_stride, hdr_lens = segments.headers, segments.hdr_stride, segments.hdr_lens
        chunk_addr, chunk_len, chunk_index = (segments.chunk_addr, segments.chunk_len,
                                              segments.chunk_index)
        seg_status = segments.status if seg_status is None else seg_status
    tables = [(headers, "headers"), (hdr_lens, "hdr_lens"), (chunk_addr, "chunk_addr"),
              (chunk_len, "chunk_len"), (chunk_index, "chunk_index")]
    missing = [tname for t, tname in tables if t is None] + (["hdr_stride"] if hdr_stride is None else [])
    if missing:
        raise ValueError("pass `segments` (a TcpSegments / UdpFragments object) or every one of "
                         "headers, hdr_stride, hdr_lens, chunk_addr, chunk_len, chunk_index; "
                         f"missing: {', '.join(missing)}")
    if seg_status is not None:
        tables.append((seg_status, "seg_status"))
    for t, tname in tables:
        _require_device(t, tname)
        _same_device(headers, t, f"headers and {tname}")
    if not (frames.is_cuda or frames.is_pinned()) or not frames.is_contiguous() \
            or frames.element_size() != 1:
        raise ValueError("frames must be a contiguous uint8 tensor in device or pinned host memory")
    n = _chunk_table_count(chunk_addr, chunk_len, chunk_index)
    if hdr_lens.dtype not in (torch.int32, torch.uint32):
        raise ValueError("hdr_lens must be an int32/uint32 device tensor")
    if hdr_lens.numel() < n or (seg_status is not None and
                                (seg_status.numel() < n or seg_status.element_size() != 1)):
        raise ValueError("hdr_lens and seg_status (uint8) must hold n entries")
    if hdr_stride <= 0 or n * hdr_stride > headers.numel() * headers.element_size():
        raise ValueError("headers must hold n whole slots of hdr_stride bytes")
    if chunk_addr.numel() != chunk_len.numel():
        raise ValueError("chunk_addr and chunk_len must hold one entry per chunk")
    kind, arg = where
    if kind == "slots":
        if arg <= 0 or n * arg > frames.numel():
            raise ValueError("frames must hold n whole slots of slot_stride bytes")
        place = (int(arg),)
    else:
        _require_offsets(arg)
        _same_device(headers, arg, "headers and offsets")
        if arg.numel() != n + 1:
            raise ValueError("offsets must hold n+1 entries")
        place = (arg.data_ptr(),)
    if lens is None:
        lens = torch.empty(n, dtype=torch.int32, device=headers.device)
    else:
        _require_device(lens, "lens")
        if lens.dtype not in (torch.int32, torch.uint32) or lens.numel() < n:
            raise ValueError("lens must be an int32/uint32 device tensor with >= n elements")
    status = _u8_out(status, n, headers)
    if n:
        launch_stream = _launch_stream(stream, headers.device)
        ca, cl = _non_null_chunk_table(chunk_addr, chunk_len, chunk_addr.numel() == 0)
        _check(getattr(_lib.load(), name)(
            headers.data_ptr(), hdr_stride, hdr_lens.data_ptr(), ca.data_ptr(), cl.data_ptr(),
            chunk_index.data_ptr(), n,
            seg_status.data_ptr() if seg_status is not None else None, frames.data_ptr(), *place,
            int(frame_max), lens.data_ptr(), status.data_ptr(),
            AIPSTACK_CHKSUM_JUST_WRITTEN if just_written else 0, _stream_handle(launch_stream)),
            name)
        if ca is not chunk_addr:  # the allocator must not reuse a stand-in before the launch is done
            ca.record_stream(launch_stream)
            cl.record_stream(launch_stream)
    return LinearFrames(frames, arg if kind == "slots" else None,
                        arg if kind != "slots" else None, lens, status)


def tx_linearise_slotted(frames, slot_stride: int, segments=None, *, headers=None, hdr_stride=None,
                         hdr_lens=None, chunk_addr=None, chunk_len=None, chunk_index=None,
                         seg_status=None, frame_max: int = 1514, lens=None, status=None,
                         just_written: bool = False, stream=None) -> LinearFrames:
    """Linearise header-split Tx segments into the slots of a send ring on the GPU
    (``aipstack_tx_linearise_slotted``): the batched form of the copy in the reference's
    ``TapDeviceLinux::sendFrame``. Segment i (the first ``hdr_lens[i]`` bytes of header slot i,
    then its chunks, as :func:`tx_fill_header_split` takes them) becomes the linear frame at
    ``frames[i * slot_stride:]``; ``frames`` is a uint8 tensor of n slots in device memory or in
    pinned host memory. Pass either ``segments`` (a :class:`TcpSegments` or
    :class:`UdpFragments`: its tensors, its ``hdr_lens``, and its ``status`` as ``seg_status``, so
    that segments of an invalid burst or datagram are skipped) or the tensors by keyword.
    ``frame_max``: the frame MTU (at most ``min(slot_stride, 65535)``). Returns
    :class:`LinearFrames`; nothing outside a written frame's bytes is stored (chksum.h has the
    outcomes and the byte rules). ``just_written``: the AIPSTACK_CHKSUM_JUST_WRITTEN hint for
    the payload read (results unchanged)."""
    return _linearise_call("aipstack_tx_linearise_slotted", ("slots", slot_stride), segments,
                           headers, hdr_stride, hdr_lens, chunk_addr, chunk_len, chunk_index,
                           seg_status, frames, frame_max, lens, status, just_written, stream)


def tx_linearise(frames, offsets, segments=None, *, headers=None, hdr_stride=None, hdr_lens=None,
                 chunk_addr=None, chunk_len=None, chunk_index=None, seg_status=None,
                 frame_max: int = 1514, lens=None, status=None, just_written: bool = False,
                 stream=None) -> LinearFrames:
    """As :func:`tx_linearise_slotted` with frame i at ``frames[offsets[i]:offsets[i+1]]``
    (``aipstack_tx_linearise``; ``offsets``: int64 device tensor of n+1 entries): a segment whose
    length is not exactly its room is AIPSTACK_TX_LIN_WRONG_ROOM and not written. The result is
    what :func:`rx_verify`, :func:`tx_fill`, :func:`tcp_rx_parse` and :func:`ip4_rx_reassemble`
    take when every segment was written."""
    return _linearise_call("aipstack_tx_linearise", ("csr", offsets), segments, headers, hdr_stride,
                           hdr_lens, chunk_addr, chunk_len, chunk_index, seg_status, frames,
                           frame_max, lens, status, just_written, stream)


AIPSTACK_ICMP_RESPONSE_HEADER = 42   # Ethernet 14 + IPv4 20 + ICMP 8
AIPSTACK_ICMP_NONE = 23              # icmp_rx_respond: no response for this frame
AIPSTACK_ICMP_ECHO_REPLY = 24
AIPSTACK_ICMP_UNREACH = 25
AIPSTACK_ICMP_TOO_LARGE = 26         # a response is due but 28 + data > mtu: left to the host
AIPSTACK_ICMP_NO_UNREACH = 0xFF      # unreach_code[i]: no request
AIPSTACK_ICMP_ALLOW_BROADCAST_PING = 1

# ``aipstack_icmp_iface`` (chksum.h): the receiving interface, host-made.
ICMP_IFACE_DTYPE = np.dtype({
    "names": ["local_addr", "bcast_addr", "mtu", "ip_id", "ttl", "flags", "mac", "reserved"],
    "formats": ["<u4", "<u4", "<u2", "<u2", "u1", "u1", ("u1", (6,)), ("u1", (12,))],
    "offsets": [0, 4, 8, 10, 12, 13, 14, 20],
    "itemsize": 32,
})
assert ICMP_IFACE_DTYPE.itemsize == 32


def icmp_iface(local_addr: int, bcast_addr: int, mac, *, mtu: int = 1500, ip_id: int = 0,
               ttl: int = 64, allow_broadcast_ping: bool = False) -> np.ndarray:
    """One ``ICMP_IFACE_DTYPE`` record (addresses in host byte order, ``mac``: 6 bytes)."""
    f = np.zeros(1, dtype=ICMP_IFACE_DTYPE)
    f["local_addr"], f["bcast_addr"], f["mtu"], f["ip_id"], f["ttl"] = (
        local_addr, bcast_addr, mtu, ip_id & 0xFFFF, ttl)
    f["flags"] = AIPSTACK_ICMP_ALLOW_BROADCAST_PING if allow_broadcast_ping else 0
    f["mac"][0] = np.frombuffer(bytes(mac), dtype=np.uint8)
    return f


def icmp_rx_respond_workspace_bytes(n: int) -> int:
    """``aipstack_icmp_rx_respond_workspace_bytes``: the workspace :func:`icmp_rx_respond` needs
    for n frames."""
    return int(_lib.load().aipstack_icmp_rx_respond_workspace_bytes(max(n, 0)))


class IcmpResponses:
    """What :func:`icmp_rx_respond` leaves (device tensors, n frames): ``headers`` (uint8, n slots
    of ``hdr_stride`` bytes; slot i holds frame i's response), ``hdr_lens`` (int32: 42 or 0), the
    compact chunk table ``chunk_addr`` (int64, n) / ``chunk_len`` (int32, n) / ``chunk_index``
    (int64, n + 1), ``status`` (uint8: AIPSTACK_ICMP_*), ``verdict`` (uint8: Rx verify's),
    ``response_frame`` (int64, n: the frame index of response j, -1 beyond the count) and
    ``counts`` (int64, 2: responses, chunks). Headers, lengths and the chunk table are the
    arguments of :func:`tx_fill_header_split`; the object is a ``segments`` argument of
    :func:`tx_linearise` / :func:`tx_linearise_slotted` (a frame without a response is skipped)."""

    def __init__(self, headers, hdr_stride, hdr_lens, chunk_addr, chunk_len, chunk_index, status,
                 verdict, response_frame, counts):
        self.headers, self.hdr_stride, self.hdr_lens = headers, hdr_stride, hdr_lens
        self.chunk_addr, self.chunk_len, self.chunk_index = chunk_addr, chunk_len, chunk_index
        self.status, self.verdict = status, verdict
        self.response_frame, self.counts = response_frame, counts

    @property
    def n(self) -> int:
        return self.chunk_index.numel() - 1


_ICMP_OUTS = (("hdr_lens", 4, 0), ("chunk_addr", 8, 0), ("chunk_len", 4, 0), ("chunk_index", 8, 1),
              ("status", 1, 0), ("verdict", 1, 0), ("response_frame", 8, 0))


def _icmp_call(name, frames, where, n, iface, unreach_code, hdr_stride, headers, workspace, out,
               stream):
    """What the two responder entry points share: the outputs (fresh, or those of ``out``), the
    workspace, the call `name` on n frames laid out by `where`."""
    torch = _torch()
    lib = _lib.load()
    f = np.ascontiguousarray(iface, dtype=ICMP_IFACE_DTYPE).reshape(-1)
    if f.size != 1:
        raise ValueError("iface must be one ICMP_IFACE_DTYPE record")
    dev = frames.device
    if out is not None:
        headers, hdr_stride = out.headers, out.hdr_stride
    if headers is None:
        headers = torch.zeros(max(n, 1) * hdr_stride, dtype=torch.uint8, device=dev)
    _require_device(headers, "headers")
    _same_device(frames, headers, "frames and headers")
    if headers.element_size() != 1 or hdr_stride <= 0 or headers.numel() < n * hdr_stride:
        raise ValueError("headers must be a uint8 device tensor of n whole slots of hdr_stride bytes")
    if out is None:
        dt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
        outs = {k: torch.empty(n + extra, dtype=dt[size], device=dev) for k, size, extra in _ICMP_OUTS}
        outs["counts"] = torch.empty(2, dtype=torch.int64, device=dev)
    else:
        outs = {k: getattr(out, k) for k, _, _ in _ICMP_OUTS}
        outs["counts"] = out.counts
        for k, size, count in [(k, size, n + extra) for k, size, extra in _ICMP_OUTS] + [("counts", 8, 2)]:
            t = outs[k]
            _require_device(t, f"out.{k}")
            _same_device(frames, t, f"frames and out.{k}")
            if t.element_size() != size or t.numel() != count:
                raise ValueError(f"out.{k} must hold {count} {size}-byte elements")
    if unreach_code is not None:
        _require_device(unreach_code, "unreach_code")
        _same_device(frames, unreach_code, "frames and unreach_code")
        if unreach_code.element_size() != 1 or unreach_code.numel() < n:
            raise ValueError("unreach_code must be a uint8 device tensor with >= n elements")
    res = IcmpResponses(headers, hdr_stride, outs["hdr_lens"], outs["chunk_addr"], outs["chunk_len"],
                        outs["chunk_index"], outs["status"], outs["verdict"], outs["response_frame"],
                        outs["counts"])
    if n == 0:  # nothing to launch: the index's one entry and the counts are 0, every other output is empty
        res.chunk_index.zero_()
        res.counts.zero_()
        return res
    workspace, ws_bytes = _workspace(workspace, icmp_rx_respond_workspace_bytes(n), frames, "frames")
    launch_stream = _launch_stream(stream, dev)
    _check(getattr(lib, name)(
        frames.data_ptr(), *where, n, f.ctypes.data,
        unreach_code.data_ptr() if unreach_code is not None else None, res.verdict.data_ptr(),
        res.status.data_ptr(), headers.data_ptr(), hdr_stride, res.hdr_lens.data_ptr(),
        res.chunk_addr.data_ptr(), res.chunk_len.data_ptr(), res.chunk_index.data_ptr(),
        res.response_frame.data_ptr(), res.counts.data_ptr(), workspace.data_ptr(), ws_bytes,
        _stream_handle(launch_stream)), name)
    workspace.record_stream(launch_stream)
    return res


def icmp_rx_respond(frames, offsets, iface, unreach_code=None, *, hdr_stride: int = 64,
                    headers=None, workspace=None, out=None, stream=None) -> IcmpResponses:
    """Rx verify plus the ICMP responder on the GPU (``aipstack_icmp_rx_respond``): frame i =
    ``frames[offsets[i]:offsets[i+1]]``. For every echo request the reference would answer, and for
    every frame the host asks a Destination Unreachable for (``unreach_code``: a uint8 device
    tensor, the ICMP code per frame or ``AIPSTACK_ICMP_NO_UNREACH``; ``None`` = no requests) and
    the reference would send one, the response's 42 header bytes go to slot i of the header ring
    and its data becomes one chunk that points into ``frames``: nothing is copied. ``iface``: an
    ``ICMP_IFACE_DTYPE`` record (:func:`icmp_iface`); response j in frame order carries the Ident
    ``ip_id + j``. ``headers``: the ring to write (device uint8 tensor of at least n slots of
    ``hdr_stride`` bytes; else a fresh, zeroed one); ``out``: an :class:`IcmpResponses` whose
    tensors are reused; ``workspace``: a device tensor of at least
    :func:`icmp_rx_respond_workspace_bytes` bytes, 8-byte aligned. Returns an
    :class:`IcmpResponses` (chksum.h has the rules and the byte layout). With no frame at all
    nothing runs: ``chunk_index`` (one entry) and ``counts`` are set to 0 and the header ring is
    left as it is."""
    _require_device(frames, "frames")
    _require_offsets(offsets)
    _same_device(frames, offsets, "frames and offsets")
    n = max(offsets.numel() - 1, 0)
    return _icmp_call("aipstack_icmp_rx_respond", frames, (offsets.data_ptr(),), n, iface,
                      unreach_code, hdr_stride, headers, workspace, out, stream)


def icmp_rx_respond_slotted(frames, slot_stride: int, lens, iface, unreach_code=None, *,
                            hdr_stride: int = 64, headers=None, workspace=None, out=None,
                            stream=None) -> IcmpResponses:
    """:func:`icmp_rx_respond` on a ring of frame slots (frame i = the lens[i] bytes at
    ``frames[i*slot_stride:]``, as :func:`rx_verify_slotted`)."""
    _require_device(frames, "frames")
    n = _require_lens(lens, frames.numel() * frames.element_size(), slot_stride, frames)
    return _icmp_call("aipstack_icmp_rx_respond_slotted", frames, (slot_stride, lens.data_ptr()),
                      n, iface, unreach_code, hdr_stride, headers, workspace, out, stream)


AIPSTACK_UDP_NO_ASSOC = 0xFFFFFFFF
AIPSTACK_UDP_ASSOC_NONLOCAL = 0x80000000   # association cookie bit 31: accept_nonlocal_dst
AIPSTACK_UDP_MAX_LISTENERS = 64
AIPSTACK_UDP_LIS_BROADCAST = 1             # UdpListenParams::accept_broadcast
AIPSTACK_UDP_LIS_NONLOCAL = 2              # UdpListenParams::accept_nonlocal_dst
AIPSTACK_UDP_DGRAM_VALID = 0x80
AIPSTACK_UDP_DGRAM_HAS_CHKSUM = 1          # UdpRxInfo::has_checksum
AIPSTACK_UDP_DGRAM_DST_LOCAL = 2           # the destination is the interface's address
AIPSTACK_UDP_DGRAM_DST_BCAST = 4           # all-ones or the subnet broadcast

# ``aipstack_udp_listener`` (chksum.h): one entry of the listener table, in list order.
UDP_LISTENER_DTYPE = np.dtype({
    "names": ["iface_addr", "port", "flags", "reserved0", "cookie", "reserved1"],
    "formats": ["<u4", "<u2", "u1", "u1", "<u4", "<u4"],
    "offsets": [0, 4, 6, 7, 8, 12],
    "itemsize": 16,
})
# ``aipstack_udp_rx_dgram`` (chksum.h): one demultiplexed UDP datagram, host byte order.
UDP_RX_DGRAM_DTYPE = np.dtype({
    "names": ["remote_addr", "local_addr", "remote_port", "local_port", "data_off", "data_len",
              "listeners", "assoc", "flags", "ttl", "reserved"],
    "formats": ["<u4", "<u4", "<u2", "<u2", "<u2", "<u2", "<u8", "<u4", "u1", "u1", "<u2"],
    "offsets": [0, 4, 8, 10, 12, 14, 16, 24, 28, 29, 30],
    "itemsize": 32,
})
assert UDP_LISTENER_DTYPE.itemsize == 16 and UDP_RX_DGRAM_DTYPE.itemsize == 32


def udp_rx_demux_workspace_bytes(n: int) -> int:
    """``aipstack_udp_rx_demux_workspace_bytes``: the workspace :func:`udp_rx_demux` needs for n
    frames."""
    return int(_lib.load().aipstack_udp_rx_demux_workspace_bytes(max(n, 0)))


class UdpRxDemuxed:
    """What :func:`udp_rx_demux` leaves (device tensors, n frames): ``verdict`` (uint8: Rx
    verify's), ``dgrams`` (uint8, n * 32 bytes: n ``aipstack_udp_rx_dgram`` records),
    ``unreach_code`` (uint8: 3 or ``AIPSTACK_ICMP_NO_UNREACH``; the ``unreach_code`` argument of
    :func:`icmp_rx_respond` as it is), ``deliver_frame`` (int64, n: the frame index of delivery
    j, -1 beyond the count) and ``counts`` (int64, 2: deliveries, unreach requests)."""

    def __init__(self, verdict, dgrams, unreach_code, deliver_frame, counts):
        self.verdict, self.dgrams, self.unreach_code = verdict, dgrams, unreach_code
        self.deliver_frame, self.counts = deliver_frame, counts

    @property
    def n(self) -> int:
        return self.verdict.numel()

    def dgrams_numpy(self) -> np.ndarray:
        """The records on the host as a ``UDP_RX_DGRAM_DTYPE`` array (synchronises)."""
        return self.dgrams[:self.n * 32].cpu().numpy().view(UDP_RX_DGRAM_DTYPE)


def _udp_table(table, dtype, name, frames):
    """(pointer, entries, tensor to keep alive) of a 16-byte-entry table: None, a device uint8
    tensor of whole entries, or a host array of `dtype` (uploaded here)."""
    torch = _torch()
    if table is None:
        return 0, 0, None
    if not hasattr(table, "data_ptr"):
        k = np.ascontiguousarray(table, dtype=dtype).reshape(-1)
        if k.size == 0:
            return 0, 0, None
        table = torch.from_numpy(k.view(np.uint8).copy()).to(frames.device)
    _require_device(table, name)
    _same_device(table, frames, f"{name} and frames")
    nbytes = table.numel() * table.element_size()
    if nbytes % 16:
        raise ValueError(f"{name} must hold whole 16-byte entries")
    return (table.data_ptr() if nbytes else 0), nbytes // 16, table


def _udp_out(t, count, size, name, frames):
    torch = _torch()
    if t is None:
        return torch.empty(count, dtype={1: torch.uint8, 8: torch.int64}[size], device=frames.device)
    _require_device(t, name)
    _same_device(t, frames, f"{name} and frames")
    if t.element_size() != size or t.numel() < count:
        raise ValueError(f"{name} must be a device tensor of at least {count} {size}-byte elements")
    return t


def _udp_demux_call(name, frames, where, n, iface, assocs, listeners, verdict, dgrams,
                    unreach_code, deliver_frame, counts, workspace, stream):
    """What the two demux entry points share: the outputs, the tables (uploaded on the launch
    stream), the workspace, the call `name` on n frames laid out by `where`."""
    f = np.ascontiguousarray(iface, dtype=ICMP_IFACE_DTYPE).reshape(-1)
    if f.size != 1:
        raise ValueError("iface must be one ICMP_IFACE_DTYPE record")
    res = UdpRxDemuxed(_u8_out(verdict, n, frames), _udp_out(dgrams, n * 32, 1, "dgrams", frames),
                       _udp_out(unreach_code, n, 1, "unreach_code", frames),
                       _udp_out(deliver_frame, n, 8, "deliver_frame", frames),
                       _udp_out(counts, 2, 8, "counts", frames))
    launch_stream = _launch_stream(stream, frames.device)
    with _torch().cuda.stream(launch_stream):  # an upload is ordered before the call
        ap, an, akeep = _udp_table(assocs, TCP_PCB_KEY_DTYPE, "assocs", frames)
        lp, ln, lkeep = _udp_table(listeners, UDP_LISTENER_DTYPE, "listeners", frames)
        if n == 0:  # nothing to launch: the counts are 0, every other output is empty
            res.counts.zero_()
            return res
    workspace, ws_bytes = _workspace(workspace, udp_rx_demux_workspace_bytes(n), frames, "frames")
    _check(getattr(_lib.load(), name)(
        frames.data_ptr(), *where, n, f.ctypes.data, ap, an, lp, ln, res.verdict.data_ptr(),
        res.dgrams.data_ptr(), res.unreach_code.data_ptr(), res.deliver_frame.data_ptr(),
        res.counts.data_ptr(), workspace.data_ptr(), ws_bytes, _stream_handle(launch_stream)), name)
    workspace.record_stream(launch_stream)
    for keep, given in ((akeep, assocs), (lkeep, listeners)):
        if keep is not None and keep is not given:
            keep.record_stream(launch_stream)
    return res


def udp_rx_demux(frames, offsets, iface, assocs=None, listeners=None, *, verdict=None, dgrams=None,
                 unreach_code=None, deliver_frame=None, counts=None, workspace=None,
                 stream=None) -> UdpRxDemuxed:
    """Rx verify plus the UDP demux on the GPU (``aipstack_udp_rx_demux``): frame i =
    ``frames[offsets[i]:offsets[i+1]]``, all received on the interface ``iface`` (an
    ``ICMP_IFACE_DTYPE`` record, :func:`icmp_iface`). For every frame accepted as UDP the
    ``aipstack_udp_rx_dgram`` record: ports, where the data lies (cut to the UDP length), the
    eligible association of ``assocs`` (a table of ``TCP_PCB_KEY_DTYPE`` entries sorted by
    :func:`tcp_pcb_table_sort`; cookie bit 31 = accept_nonlocal_dst) and the mask of the matching
    ``listeners`` (at most 64 ``UDP_LISTENER_DTYPE`` entries, newest first as the reference walks
    them). Each table: a host array (uploaded on the launch stream), a device uint8 tensor
    already resident, or ``None``. ``unreach_code`` is 3 where the reference would send a port
    unreachable with no handler called. Returns a :class:`UdpRxDemuxed` (chksum.h has the rules)."""
    _require_device(frames, "frames")
    _require_offsets(offsets)
    _same_device(frames, offsets, "frames and offsets")
    n = max(offsets.numel() - 1, 0)
    return _udp_demux_call("aipstack_udp_rx_demux", frames, (offsets.data_ptr(),), n, iface, assocs,
                           listeners, verdict, dgrams, unreach_code, deliver_frame, counts, workspace,
                           stream)


def udp_rx_demux_slotted(frames, slot_stride: int, lens, iface, assocs=None, listeners=None, *,
                         verdict=None, dgrams=None, unreach_code=None, deliver_frame=None,
                         counts=None, workspace=None, stream=None) -> UdpRxDemuxed:
    """:func:`udp_rx_demux` on a ring of frame slots (frame i = the lens[i] bytes at
    ``frames[i*slot_stride:]``, as :func:`rx_verify_slotted`)."""
    _require_device(frames, "frames")
    n = _require_lens(lens, frames.numel() * frames.element_size(), slot_stride, frames)
    return _udp_demux_call("aipstack_udp_rx_demux_slotted", frames, (slot_stride, lens.data_ptr()),
                           n, iface, assocs, listeners, verdict, dgrams, unreach_code,
                           deliver_frame, counts, workspace, stream)


AIPSTACK_ARP_REPLY_HEADER = 42       # Ethernet 14 + ARP 28
AIPSTACK_ARP_NONE = 27               # arp_rx_respond: shorter than 14 bytes, or EtherType != 0x0806
AIPSTACK_ARP_MALFORMED = 28          # ARP, but short or with a wrong HwType / ProtoType / length
AIPSTACK_ARP_SEEN = 29               # a valid ARP packet, no reply due
AIPSTACK_ARP_REPLY = 30              # a valid ARP packet, reply emitted
AIPSTACK_ARP_HAVE_ADDR = 1           # iface flag: the interface has an address
AIPSTACK_ARP_REC_LEARN = 1           # record flags: the sender MAC is not broadcast
AIPSTACK_ARP_REC_NEW_OK = 2          # an entry for the sender address may be created
AIPSTACK_ARP_REC_NOTIFY = 4          # the observers are notified
AIPSTACK_ARP_REC_REPLY = 8           # a reply was emitted

# ``aipstack_arp_iface`` (chksum.h): the receiving interface, host-made.
ARP_IFACE_DTYPE = np.dtype({
    "names": ["local_addr", "netmask", "mac", "flags", "reserved"],
    "formats": ["<u4", "<u4", ("u1", (6,)), "u1", ("u1", (17,))],
    "offsets": [0, 4, 8, 14, 15],
    "itemsize": 32,
})
# ``aipstack_arp_record`` (chksum.h): what the host's ARP table does with one frame's sender.
ARP_RECORD_DTYPE = np.dtype({
    "names": ["sender_addr", "sender_mac", "op", "flags", "status", "reserved"],
    "formats": ["<u4", ("u1", (6,)), "<u2", "u1", "u1", "<u2"],
    "offsets": [0, 4, 10, 12, 13, 14],
    "itemsize": 16,
})
assert ARP_IFACE_DTYPE.itemsize == 32 and ARP_RECORD_DTYPE.itemsize == 16


def arp_iface(local_addr: int, netmask: int, mac, *, have_addr: bool = True) -> np.ndarray:
    """One ``ARP_IFACE_DTYPE`` record (address and mask in host byte order, ``mac``: 6 bytes;
    ``have_addr=False``: an interface without an address, as before DHCP has one)."""
    f = np.zeros(1, dtype=ARP_IFACE_DTYPE)
    f["local_addr"], f["netmask"] = local_addr, netmask
    f["flags"] = AIPSTACK_ARP_HAVE_ADDR if have_addr else 0
    f["mac"][0] = np.frombuffer(bytes(mac), dtype=np.uint8)
    return f


def arp_rx_respond_workspace_bytes(n: int) -> int:
    """``aipstack_arp_rx_respond_workspace_bytes``: the workspace :func:`arp_rx_respond` needs for
    n frames."""
    return int(_lib.load().aipstack_arp_rx_respond_workspace_bytes(max(n, 0)))


class ArpResponses:
    """What :func:`arp_rx_respond` leaves (device tensors, n frames): ``status`` (uint8:
    AIPSTACK_ARP_*), ``records`` (uint8, n * 16 bytes: n ``aipstack_arp_record`` records),
    ``headers`` (uint8, n slots of ``hdr_stride`` bytes; slot i holds frame i's reply),
    ``hdr_lens`` (int32: 42 or 0), ``chunk_index`` (int64, n + 1, all zero: a reply has no chunk),
    ``reply_frame`` / ``seen_frame`` (int64, n: the frame indices of the replies and of the valid
    ARP packets in frame order, -1 beyond the count) and ``counts`` (int64, 2: replies, seen).
    ``chunk_addr`` / ``chunk_len`` are empty, which makes the object a ``segments`` argument of
    :func:`tx_linearise` / :func:`tx_linearise_slotted` (a frame without a reply is skipped)."""

    def __init__(self, headers, hdr_stride, hdr_lens, chunk_index, status, records, reply_frame,
                 seen_frame, counts):
        torch = _torch()
        self.headers, self.hdr_stride, self.hdr_lens = headers, hdr_stride, hdr_lens
        self.chunk_index, self.status, self.records = chunk_index, status, records
        self.reply_frame, self.seen_frame, self.counts = reply_frame, seen_frame, counts
        self.chunk_addr = torch.empty(0, dtype=torch.int64, device=headers.device)
        self.chunk_len = torch.empty(0, dtype=torch.int32, device=headers.device)

    @property
    def n(self) -> int:
        return self.chunk_index.numel() - 1

    def records_numpy(self) -> np.ndarray:
        """The records on the host as an ``ARP_RECORD_DTYPE`` array (synchronises)."""
        return self.records[:self.n * 16].cpu().numpy().view(ARP_RECORD_DTYPE)


_ARP_OUTS = (("hdr_lens", 4, 1, 0), ("chunk_index", 8, 1, 1), ("status", 1, 1, 0), ("records", 1, 16, 0),
             ("reply_frame", 8, 1, 0), ("seen_frame", 8, 1, 0))


def _arp_call(name, frames, where, n, iface, hdr_stride, headers, workspace, out, stream):
    """What the two ARP entry points share: the outputs (fresh, or those of ``out``), the
    workspace, the call `name` on n frames laid out by `where`."""
    torch = _torch()
    lib = _lib.load()
    f = np.ascontiguousarray(iface, dtype=ARP_IFACE_DTYPE).reshape(-1)
    if f.size != 1:
        raise ValueError("iface must be one ARP_IFACE_DTYPE record")
    dev = frames.device
    if out is not None:
        headers, hdr_stride = out.headers, out.hdr_stride
    if headers is None:
        headers = torch.zeros(max(n, 1) * hdr_stride, dtype=torch.uint8, device=dev)
    _require_device(headers, "headers")
    _same_device(frames, headers, "frames and headers")
    if headers.element_size() != 1 or hdr_stride <= 0 or headers.numel() < n * hdr_stride:
        raise ValueError("headers must be a uint8 device tensor of n whole slots of hdr_stride bytes")
    sizes = [(k, size, n * per + extra) for k, size, per, extra in _ARP_OUTS] + [("counts", 8, 2)]
    if out is None:
        dt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
        outs = {k: torch.empty(count, dtype=dt[size], device=dev) for k, size, count in sizes}
    else:
        outs = {k: getattr(out, k) for k, _, _ in sizes}
        for k, size, count in sizes:
            t = outs[k]
            _require_device(t, f"out.{k}")
            _same_device(frames, t, f"frames and out.{k}")
            if t.element_size() != size or t.numel() != count:
                raise ValueError(f"out.{k} must hold {count} {size}-byte elements")
    res = ArpResponses(headers, hdr_stride, outs["hdr_lens"], outs["chunk_index"], outs["status"],
                       outs["records"], outs["reply_frame"], outs["seen_frame"], outs["counts"])
    if n == 0:  # nothing to launch: the index's one entry and the counts are 0, every other output is empty
        res.chunk_index.zero_()
        res.counts.zero_()
        return res
    workspace, ws_bytes = _workspace(workspace, arp_rx_respond_workspace_bytes(n), frames, "frames")
    launch_stream = _launch_stream(stream, dev)
    _check(getattr(lib, name)(
        frames.data_ptr(), *where, n, f.ctypes.data, res.status.data_ptr(), res.records.data_ptr(),
        headers.data_ptr(), hdr_stride, res.hdr_lens.data_ptr(), res.chunk_index.data_ptr(),
        res.reply_frame.data_ptr(), res.seen_frame.data_ptr(), res.counts.data_ptr(),
        workspace.data_ptr(), ws_bytes, _stream_handle(launch_stream)), name)
    workspace.record_stream(launch_stream)
    return res


def arp_rx_respond(frames, offsets, iface, *, hdr_stride: int = 64, headers=None, workspace=None,
                   out=None, stream=None) -> ArpResponses:
    """ARP on receive on the GPU (``aipstack_arp_rx_respond``): frame i =
    ``frames[offsets[i]:offsets[i+1]]``, all received on the interface ``iface`` (an
    ``ARP_IFACE_DTYPE`` record, :func:`arp_iface`). Every frame gets its status and its
    ``aipstack_arp_record`` (the sender's address and MAC, and what the host's ARP table and the
    observers do with them); a request for the interface's address gets its 42-byte reply in slot
    i of the header ring, addressed to the ARP sender hardware address. No Rx verify runs (ARP
    carries no checksum) and at most the first 42 bytes of a frame are read. ``headers``: the ring
    to write (device uint8 tensor of at least n slots of ``hdr_stride`` bytes; else a fresh,
    zeroed one); ``out``: an :class:`ArpResponses` whose tensors are reused; ``workspace``: a
    device tensor of at least :func:`arp_rx_respond_workspace_bytes` bytes, 8-byte aligned.
    Returns an :class:`ArpResponses` (chksum.h has the rules and the byte layout). With no frame
    at all nothing runs: ``chunk_index`` (one entry) and ``counts`` are set to 0 and the header
    ring is left as it is."""
    _require_device(frames, "frames")
    _require_offsets(offsets)
    _same_device(frames, offsets, "frames and offsets")
    n = max(offsets.numel() - 1, 0)
    return _arp_call("aipstack_arp_rx_respond", frames, (offsets.data_ptr(),), n, iface, hdr_stride,
                     headers, workspace, out, stream)


def arp_rx_respond_slotted(frames, slot_stride: int, lens, iface, *, hdr_stride: int = 64,
                           headers=None, workspace=None, out=None, stream=None) -> ArpResponses:
    """:func:`arp_rx_respond` on a ring of frame slots (frame i = the lens[i] bytes at
    ``frames[i*slot_stride:]``, as :func:`rx_verify_slotted`)."""
    _require_device(frames, "frames")
    n = _require_lens(lens, frames.numel() * frames.element_size(), slot_stride, frames)
    return _arp_call("aipstack_arp_rx_respond_slotted", frames, (slot_stride, lens.data_ptr()), n,
                     iface, hdr_stride, headers, workspace, out, stream)


AIPSTACK_TCP_RSP_HEADER = 54         # = AIPSTACK_TCP_SEGMENT_HEADER: an RST is a segment without data
AIPSTACK_TCP_RSP_NONE = 31           # tcp_rx_respond: no valid segment record
AIPSTACK_TCP_RSP_NOT_LOCAL = 32      # the destination is not the interface's address
AIPSTACK_TCP_RSP_PCB = 33            # a PCB was found: the host calls pcb_input
AIPSTACK_TCP_RSP_DROP = 34           # no PCB (or an RST requested), nothing sent
AIPSTACK_TCP_RSP_SYN = 35            # a listener matched a pure SYN with an acceptable MSS
AIPSTACK_TCP_RSP_RST = 36            # an RST was emitted
AIPSTACK_TCP_NO_LISTENER = 0xFFFFFFFF
AIPSTACK_TCP_MAX_LISTENERS = 256

# ``aipstack_tcp_listener`` (chksum.h): one entry of the listener table, in list order.
TCP_LISTENER_DTYPE = np.dtype({
    "names": ["addr", "port", "reserved0", "cookie", "reserved1"],
    "formats": ["<u4", "<u2", "<u2", "<u4", "<u4"],
    "offsets": [0, 4, 6, 8, 12],
    "itemsize": 16,
})
assert TCP_LISTENER_DTYPE.itemsize == 16


def tcp_listeners(entries) -> np.ndarray:
    """A ``TCP_LISTENER_DTYPE`` table from ``(addr, port, cookie)`` triples (addr in host byte
    order, 0 = any), in the order given: the order the reference walks its listener list, newest
    first."""
    entries = list(entries)
    t = np.zeros(len(entries), dtype=TCP_LISTENER_DTYPE)
    for k, (addr, port, cookie) in enumerate(entries):
        t[k]["addr"], t[k]["port"], t[k]["cookie"] = addr, port, cookie
    return t


def tcp_rx_respond_workspace_bytes(n: int) -> int:
    """``aipstack_tcp_rx_respond_workspace_bytes``: the workspace :func:`tcp_rx_respond` needs for
    n frames."""
    return int(_lib.load().aipstack_tcp_rx_respond_workspace_bytes(max(n, 0)))


class TcpResponses:
    """What :func:`tcp_rx_respond` leaves (device tensors, n frames): ``verdict`` (uint8), ``segs``
    (uint8, n * 32 bytes) and ``pcb`` (int32) as :func:`tcp_rx_parse` writes them; ``status``
    (uint8: AIPSTACK_TCP_RSP_*); ``listener`` (int32: the matched listener's cookie, bit pattern of
    ``AIPSTACK_TCP_NO_LISTENER`` = -1 where none was consulted and matched); ``headers`` (uint8, n
    slots of ``hdr_stride`` bytes; slot i holds frame i's RST), ``hdr_lens`` (int32: 54 or 0),
    ``chunk_index`` (int64, n + 1, all zero: an RST has no chunk); ``response_frame`` /
    ``syn_frame`` (int64, n: the frame indices of the RSTs and of the ``_RSP_SYN`` frames in frame
    order, -1 beyond the count) and ``counts`` (int64, 2: RSTs, SYNs). ``chunk_addr`` /
    ``chunk_len`` are empty, which makes the object a ``segments`` argument of
    :func:`tx_linearise` / :func:`tx_linearise_slotted` (a frame without an RST is skipped)."""

    def __init__(self, headers, hdr_stride, outs):
        torch = _torch()
        self.headers, self.hdr_stride = headers, hdr_stride
        for k, t in outs.items():
            setattr(self, k, t)
        self.chunk_addr = torch.empty(0, dtype=torch.int64, device=headers.device)
        self.chunk_len = torch.empty(0, dtype=torch.int32, device=headers.device)

    @property
    def n(self) -> int:
        return self.chunk_index.numel() - 1

    def segs_numpy(self) -> np.ndarray:
        """The records on the host as a ``TCP_RX_SEG_DTYPE`` array (synchronises)."""
        return self.segs[:self.n * 32].cpu().numpy().view(TCP_RX_SEG_DTYPE)

    def pcb_numpy(self) -> np.ndarray:
        """The PCB cookies on the host as uint32 (synchronises)."""
        return self.pcb[:self.n].cpu().numpy().view(np.uint32)

    def listener_numpy(self) -> np.ndarray:
        """The listener cookies on the host as uint32 (synchronises)."""
        return self.listener[:self.n].cpu().numpy().view(np.uint32)


# name, element size, elements per frame, extra elements
_TCP_RSP_OUTS = (("verdict", 1, 1, 0), ("segs", 1, 32, 0), ("pcb", 4, 1, 0), ("status", 1, 1, 0),
                 ("listener", 4, 1, 0), ("hdr_lens", 4, 1, 0), ("chunk_index", 8, 1, 1),
                 ("response_frame", 8, 1, 0), ("syn_frame", 8, 1, 0))


def _tcp_rsp_call(name, frames, where, n, iface, tcp_ttl, pcbs, listeners, rst_request, hdr_stride,
                  headers, workspace, out, stream):
    """What the two entry points share: the outputs (fresh, or those of ``out``), the tables
    (uploaded on the launch stream), the workspace, the call `name` on n frames laid out by
    `where`."""
    torch = _torch()
    lib = _lib.load()
    f = np.ascontiguousarray(iface, dtype=ICMP_IFACE_DTYPE).reshape(-1)
    if f.size != 1:
        raise ValueError("iface must be one ICMP_IFACE_DTYPE record")
    dev = frames.device
    if out is not None:
        headers, hdr_stride = out.headers, out.hdr_stride
    if headers is None:
        headers = torch.zeros(max(n, 1) * hdr_stride, dtype=torch.uint8, device=dev)
    _require_device(headers, "headers")
    _same_device(frames, headers, "frames and headers")
    if headers.element_size() != 1 or hdr_stride <= 0 or headers.numel() < n * hdr_stride:
        raise ValueError("headers must be a uint8 device tensor of n whole slots of hdr_stride bytes")
    sizes = [(k, size, n * per + extra) for k, size, per, extra in _TCP_RSP_OUTS] + [("counts", 8, 2)]
    if out is None:
        dt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
        outs = {k: torch.empty(count, dtype=dt[size], device=dev) for k, size, count in sizes}
    else:
        outs = {k: getattr(out, k) for k, _, _ in sizes}
        for k, size, count in sizes:
            t = outs[k]
            _require_device(t, f"out.{k}")
            _same_device(frames, t, f"frames and out.{k}")
            if t.element_size() != size or t.numel() != count:
                raise ValueError(f"out.{k} must hold {count} {size}-byte elements")
    if rst_request is not None:
        _require_device(rst_request, "rst_request")
        _same_device(frames, rst_request, "frames and rst_request")
        if rst_request.element_size() != 1 or rst_request.numel() < n:
            raise ValueError("rst_request must be a uint8 device tensor with >= n elements")
    res = TcpResponses(headers, hdr_stride, outs)
    launch_stream = _launch_stream(stream, dev)
    with torch.cuda.stream(launch_stream):  # an upload is ordered before the call
        pp, pn, pkeep = _udp_table(pcbs, TCP_PCB_KEY_DTYPE, "pcbs", frames)
        lp, ln, lkeep = _udp_table(listeners, TCP_LISTENER_DTYPE, "listeners", frames)
        if n == 0:  # nothing to launch: the index's one entry and the counts are 0, the rest is empty
            res.chunk_index.zero_()
            res.counts.zero_()
            return res
    workspace, ws_bytes = _workspace(workspace, tcp_rx_respond_workspace_bytes(n), frames, "frames")
    _check(getattr(lib, name)(
        frames.data_ptr(), *where, n, f.ctypes.data, tcp_ttl, pp, pn, lp, ln,
        rst_request.data_ptr() if rst_request is not None else None, res.verdict.data_ptr(),
        res.segs.data_ptr(), res.pcb.data_ptr(), res.status.data_ptr(), res.listener.data_ptr(),
        headers.data_ptr(), hdr_stride, res.hdr_lens.data_ptr(), res.chunk_index.data_ptr(),
        res.response_frame.data_ptr(), res.syn_frame.data_ptr(), res.counts.data_ptr(),
        workspace.data_ptr(), ws_bytes, _stream_handle(launch_stream)), name)
    workspace.record_stream(launch_stream)
    for keep, given in ((pkeep, pcbs), (lkeep, listeners)):
        if keep is not None and keep is not given:
            keep.record_stream(launch_stream)
    return res


def tcp_rx_respond(frames, offsets, iface, pcbs=None, listeners=None, rst_request=None, *,
                   tcp_ttl: int = 64, hdr_stride: int = 64, headers=None, workspace=None, out=None,
                   stream=None) -> TcpResponses:
    """Rx verify, the TCP parse and the answer to segments without a connection on the GPU
    (``aipstack_tcp_rx_respond``): frame i = ``frames[offsets[i]:offsets[i+1]]``, all received on
    the interface ``iface`` (an ``ICMP_IFACE_DTYPE`` record, :func:`icmp_iface`; its ``ttl`` is
    the ICMP one and is not used: ``tcp_ttl`` is the RSTs'). ``verdict``, ``segs`` and ``pcb`` are
    what :func:`tcp_rx_parse` gives with the same ``pcbs``; ``status`` says what is left for the
    host: ``pcb_input`` (``_RSP_PCB``), the rest of ``listen_input`` for the listener whose cookie
    is in ``listener`` (``_RSP_SYN``), or nothing. ``listeners``: at most 256
    ``TCP_LISTENER_DTYPE`` entries (:func:`tcp_listeners`), newest first as the reference walks
    them; the first match wins. Each table: a host array (uploaded on the launch stream), a device
    uint8 tensor already resident, or ``None``. ``rst_request``: a uint8 device tensor, nonzero
    where the host wants an RST whatever the tables say; ``None`` = no requests. RST j in frame
    order carries the Ident ``ip_id + j`` and lies in slot i of the header ring. ``headers``,
    ``out`` (a :class:`TcpResponses` whose tensors are reused) and ``workspace``
    (:func:`tcp_rx_respond_workspace_bytes` bytes) as for :func:`arp_rx_respond`. Returns a
    :class:`TcpResponses` (chksum.h has the rules and the byte layout). With no frame at all
    nothing runs: ``chunk_index`` (one entry) and ``counts`` are set to 0 and the header ring is
    left as it is."""
    _require_device(frames, "frames")
    _require_offsets(offsets)
    _same_device(frames, offsets, "frames and offsets")
    n = max(offsets.numel() - 1, 0)
    return _tcp_rsp_call("aipstack_tcp_rx_respond", frames, (offsets.data_ptr(),), n, iface, tcp_ttl,
                         pcbs, listeners, rst_request, hdr_stride, headers, workspace, out, stream)


def tcp_rx_respond_slotted(frames, slot_stride: int, lens, iface, pcbs=None, listeners=None,
                           rst_request=None, *, tcp_ttl: int = 64, hdr_stride: int = 64,
                           headers=None, workspace=None, out=None, stream=None) -> TcpResponses:
    """:func:`tcp_rx_respond` on a ring of frame slots (frame i = the lens[i] bytes at
    ``frames[i*slot_stride:]``, as :func:`rx_verify_slotted`)."""
    _require_device(frames, "frames")
    n = _require_lens(lens, frames.numel() * frames.element_size(), slot_stride, frames)
    return _tcp_rsp_call("aipstack_tcp_rx_respond_slotted", frames, (slot_stride, lens.data_ptr()),
                         n, iface, tcp_ttl, pcbs, listeners, rst_request, hdr_stride, headers,
                         workspace, out, stream)


AIPSTACK_ICMP_DU_NONE = 37           # icmp_rx_unreach: no Destination Unreachable a handler would see
AIPSTACK_ICMP_DU_PARSED = 38         # a valid record; the quoted protocol's handler returns at once
AIPSTACK_ICMP_DU_TCP_NO_PCB = 39     # quoted TCP, code 4, >= 8 quoted bytes: no PCB
AIPSTACK_ICMP_DU_TCP_PCB = 40        # the same, and the PCB table holds the connection

# ``aipstack_icmp_du_record`` (chksum.h): one parsed Destination Unreachable, host byte order.
ICMP_DU_RECORD_DTYPE = np.dtype({
    "names": ["local_addr", "remote_addr", "local_port", "remote_port", "seq", "rest", "pcb", "ip_off",
              "l4_len", "code", "proto", "ttl", "hl"],
    "formats": ["<u4", "<u4", "<u2", "<u2", "<u4", "<u4", "<u4", "<u2", "<u2", "u1", "u1", "u1", "u1"],
    "offsets": [0, 4, 8, 10, 12, 16, 20, 24, 26, 28, 29, 30, 31],
    "itemsize": 32,
})
assert ICMP_DU_RECORD_DTYPE.itemsize == 32


def icmp_rx_unreach_workspace_bytes(n: int) -> int:
    """``aipstack_icmp_rx_unreach_workspace_bytes``: the workspace :func:`icmp_rx_unreach` needs for
    n frames."""
    return int(_lib.load().aipstack_icmp_rx_unreach_workspace_bytes(max(n, 0)))


class IcmpUnreachParsed:
    """What :func:`icmp_rx_unreach` leaves (device tensors, n frames): ``verdict`` (uint8: Rx
    verify's), ``status`` (uint8: AIPSTACK_ICMP_DU_*), ``records`` (uint8, n * 32 bytes: n
    ``aipstack_icmp_du_record`` records, zero where the status is ``_DU_NONE``), ``pcb_frame``
    (int64, n: the frame index of the j-th ``_DU_TCP_PCB`` frame, -1 beyond the count) and
    ``counts`` (int64, 2: ``_DU_TCP_PCB`` frames, valid records)."""

    def __init__(self, verdict, status, records, pcb_frame, counts):
        self.verdict, self.status, self.records = verdict, status, records
        self.pcb_frame, self.counts = pcb_frame, counts

    @property
    def n(self) -> int:
        return self.verdict.numel()

    def records_numpy(self) -> np.ndarray:
        """The records on the host as an ``ICMP_DU_RECORD_DTYPE`` array (synchronises)."""
        return self.records[:self.n * 32].cpu().numpy().view(ICMP_DU_RECORD_DTYPE)


def _icmp_unreach_call(name, frames, where, n, iface, pcbs, verdict, status, records, pcb_frame,
                       counts, workspace, stream):
    """What the two entry points share: the outputs, the PCB table (uploaded on the launch
    stream), the workspace, the call `name` on n frames laid out by `where`."""
    f = np.ascontiguousarray(iface, dtype=ICMP_IFACE_DTYPE).reshape(-1)
    if f.size != 1:
        raise ValueError("iface must be one ICMP_IFACE_DTYPE record")
    res = IcmpUnreachParsed(_u8_out(verdict, n, frames), _udp_out(status, n, 1, "status", frames),
                            _udp_out(records, n * 32, 1, "records", frames),
                            _udp_out(pcb_frame, n, 8, "pcb_frame", frames),
                            _udp_out(counts, 2, 8, "counts", frames))
    for what in ("records", "pcb_frame", "counts"):
        t = getattr(res, what)
        if t.numel() and t.data_ptr() % 8:
            raise ValueError(f"{what} must be 8-byte aligned")
    launch_stream = _launch_stream(stream, frames.device)
    with _torch().cuda.stream(launch_stream):  # an upload is ordered before the call
        pp, pn, pkeep = _udp_table(pcbs, TCP_PCB_KEY_DTYPE, "pcbs", frames)
        if pn and pp % 8:
            raise ValueError("pcbs must be 8-byte aligned")
        if n == 0:  # nothing to launch: the counts are 0, every other output is empty
            res.counts.zero_()
            return res
    workspace, ws_bytes = _workspace(workspace, icmp_rx_unreach_workspace_bytes(n), frames, "frames")
    _check(getattr(_lib.load(), name)(
        frames.data_ptr(), *where, n, f.ctypes.data, pp, pn, res.verdict.data_ptr(),
        res.status.data_ptr(), res.records.data_ptr(), res.pcb_frame.data_ptr(),
        res.counts.data_ptr(), workspace.data_ptr(), ws_bytes, _stream_handle(launch_stream)), name)
    workspace.record_stream(launch_stream)
    if pkeep is not None and pkeep is not pcbs:
        pkeep.record_stream(launch_stream)
    return res


def icmp_rx_unreach(frames, offsets, iface, pcbs=None, *, verdict=None, status=None, records=None,
                    pcb_frame=None, counts=None, workspace=None, stream=None) -> IcmpUnreachParsed:
    """Rx verify plus the parse of received ICMP Destination Unreachable messages on the GPU
    (``aipstack_icmp_rx_unreach``): frame i = ``frames[offsets[i]:offsets[i+1]]``, all received on
    the interface ``iface`` (an ``ICMP_IFACE_DTYPE`` record, :func:`icmp_iface`). For every message
    the reference would hand to a protocol handler the ``aipstack_icmp_du_record``: the quoted
    addresses, ports and sequence number, the ICMP code and ``rest`` (the next-hop MTU is ``rest &
    0xFFFF``), and for a quoted TCP segment of a frag-needed message (code 4) the cookie of its
    PCB in ``pcbs`` (a table of ``TCP_PCB_KEY_DTYPE`` entries sorted by
    :func:`tcp_pcb_table_sort`: a host array, uploaded on the launch stream, a device uint8 tensor
    already resident, or ``None``). ``pcb_frame`` lists the frames with a PCB in frame order: the
    host applies the ``snd_una <= seq <= snd_nxt`` test and calls ``handleIcmpPacketTooBig`` for
    those alone. Returns an :class:`IcmpUnreachParsed` (chksum.h has the rules)."""
    _require_device(frames, "frames")
    _require_offsets(offsets)
    _same_device(frames, offsets, "frames and offsets")
    n = max(offsets.numel() - 1, 0)
    return _icmp_unreach_call("aipstack_icmp_rx_unreach", frames, (offsets.data_ptr(),), n, iface,
                              pcbs, verdict, status, records, pcb_frame, counts, workspace, stream)


def icmp_rx_unreach_slotted(frames, slot_stride: int, lens, iface, pcbs=None, *, verdict=None,
                            status=None, records=None, pcb_frame=None, counts=None, workspace=None,
                            stream=None) -> IcmpUnreachParsed:
    """:func:`icmp_rx_unreach` on a ring of frame slots (frame i = the lens[i] bytes at
    ``frames[i*slot_stride:]``, as :func:`rx_verify_slotted`)."""
    _require_device(frames, "frames")
    n = _require_lens(lens, frames.numel() * frames.element_size(), slot_stride, frames)
    return _icmp_unreach_call("aipstack_icmp_rx_unreach_slotted", frames,
                              (slot_stride, lens.data_ptr()), n, iface, pcbs, verdict, status,
                              records, pcb_frame, counts, workspace, stream)


AIPSTACK_TX_RES_NONE = 41            # tx_resolve: nothing to resolve for this segment
AIPSTACK_TX_RES_SENT = 42            # bytes 0..13 of the slot are the Ethernet header
AIPSTACK_TX_RES_NO_ROUTE = 43        # IpErr::NoIpRoute
AIPSTACK_TX_RES_BCAST_REJECTED = 44  # IpErr::BroadcastRejected
AIPSTACK_TX_RES_NONLOCAL_SRC = 45    # IpErr::NonLocalSrc
AIPSTACK_TX_RES_NO_HW_ROUTE = 46     # IpErr::NoHardwareRoute
AIPSTACK_TX_RES_ARP_QUERY = 47       # IpErr::ArpQueryInProgress
AIPSTACK_TX_MAX_IFACES = 16
AIPSTACK_TX_HAVE_ADDR = 1            # iface flags
AIPSTACK_TX_HAVE_GATEWAY = 2
AIPSTACK_TX_ALLOW_BROADCAST = 1      # send flags: IpSendFlags::AllowBroadcastFlag
AIPSTACK_TX_ALLOW_NONLOCAL_SRC = 2   # IpSendFlags::AllowNonLocalSrc
AIPSTACK_TX_ROUTE_ANY = 0xFFFF       # force_iface[i]: no interface named
AIPSTACK_TX_NO_ARP_ENTRY = 0xFFFFFFFF
AIPSTACK_ARP_STATE_QUERY = 1         # ArpEntryState
AIPSTACK_ARP_STATE_VALID = 2
AIPSTACK_ARP_STATE_REFRESHING = 3
AIPSTACK_TX_ROUTE_GATEWAY = 1        # route flags: next_hop is the gateway
AIPSTACK_TX_ROUTE_BROADCAST = 2      # the MAC is ff:ff:ff:ff:ff:ff
AIPSTACK_TX_ROUTE_NEW_ENTRY = 4      # _ARP_QUERY without an entry: the host makes one
AIPSTACK_TX_ROUTE_FORCED = 8         # the segment named its interface

# ``aipstack_tx_iface`` (chksum.h): one interface of the device table, host byte order.
TX_IFACE_DTYPE = np.dtype({
    "names": ["addr", "netmask", "gateway", "prefix", "flags", "mac", "reserved"],
    "formats": ["<u4", "<u4", "<u4", "u1", "u1", ("u1", (6,)), ("u1", (12,))],
    "offsets": [0, 4, 8, 12, 13, 14, 20],
    "itemsize": 32,
})
# ``aipstack_arp_entry``: one entry of the ARP table snapshot.
ARP_ENTRY_DTYPE = np.dtype({
    "names": ["addr", "iface", "state", "mac", "reserved"],
    "formats": ["<u4", "<u2", "u1", ("u1", (6,)), ("u1", (3,))],
    "offsets": [0, 4, 6, 7, 13],
    "itemsize": 16,
})
# ``aipstack_tx_route``: the record of one segment.
TX_ROUTE_DTYPE = np.dtype({
    "names": ["next_hop", "arp_index", "iface", "status", "flags", "reserved"],
    "formats": ["<u4", "<u4", "<u2", "u1", "u1", "<u4"],
    "offsets": [0, 4, 8, 10, 11, 12],
    "itemsize": 16,
})
assert (TX_IFACE_DTYPE.itemsize, ARP_ENTRY_DTYPE.itemsize, TX_ROUTE_DTYPE.itemsize) == (32, 16, 16)


def tx_ifaces(entries) -> np.ndarray:
    """The interface table of :func:`tx_resolve` as a ``TX_IFACE_DTYPE`` array, from
    ``(addr or None, prefix, gateway or None, mac)`` per interface **in the order the stack's
    interface list iterates** (the reference prepends: last constructed first)."""
    entries = list(entries)
    t = np.zeros(len(entries), dtype=TX_IFACE_DTYPE)
    for k, (addr, prefix, gateway, mac) in enumerate(entries):
        if not 0 <= int(prefix) <= 32 or len(bytes(mac)) != 6:
            raise ValueError("prefix must be 0..32 and mac 6 bytes")
        if addr is not None:
            t[k]["addr"], t[k]["prefix"] = addr, prefix
            t[k]["netmask"] = (0xFFFFFFFF << (32 - int(prefix))) & 0xFFFFFFFF if prefix else 0
        if gateway is not None:
            t[k]["gateway"] = gateway
        t[k]["flags"] = (AIPSTACK_TX_HAVE_ADDR if addr is not None else 0) | \
            (AIPSTACK_TX_HAVE_GATEWAY if gateway is not None else 0)
        t[k]["mac"] = np.frombuffer(bytes(mac), dtype=np.uint8)
    return t


def arp_table_sort(entries):
    """Host side of :func:`tx_resolve` (``aipstack_arp_table_sort``, no GPU): a copy of ``entries``
    (an ``ARP_ENTRY_DTYPE`` array) sorted by (iface, addr), the order the lookup searches. Raises
    :class:`ChksumError` (``AIPSTACK_CHKSUM_EINVAL``) for a duplicate key, a state outside 1..3,
    an interface index of 16 or more or a nonzero reserved byte."""
    e = np.array(entries, dtype=ARP_ENTRY_DTYPE).reshape(-1)
    _check(_lib.load().aipstack_arp_table_sort(e.ctypes.data if e.size else None, e.size),
           "aipstack_arp_table_sort")
    return e


def tx_resolve_workspace_bytes(n: int) -> int:
    """``aipstack_tx_resolve_workspace``: the workspace :func:`tx_resolve` needs for n segments."""
    return int(_lib.load().aipstack_tx_resolve_workspace(max(n, 0)))


class TxResolved:
    """What :func:`tx_resolve` leaves (device tensors, n segments): ``status`` (uint8:
    AIPSTACK_TX_RES_*), ``routes`` (uint8, n * 16 bytes: n ``aipstack_tx_route`` records),
    ``send_lens`` (int32, n: the header length for ``_SENT`` and ``_RES_NONE``, else 0: the
    ``hdr_lens`` to linearise with), ``arp_used`` (uint8, one per ARP entry), ``held_seg`` /
    ``failed_seg`` (int64, n: the ``_ARP_QUERY`` / the rejected segments in order, -1 beyond the
    count) and ``counts`` (int64, 2: held, failed)."""

    def __init__(self, status, routes, send_lens, arp_used, held_seg, failed_seg, counts):
        self.status, self.routes, self.send_lens, self.arp_used = status, routes, send_lens, arp_used
        self.held_seg, self.failed_seg, self.counts = held_seg, failed_seg, counts

    @property
    def n(self) -> int:
        return self.status.numel()

    def routes_numpy(self) -> np.ndarray:
        """The records on the host as a ``TX_ROUTE_DTYPE`` array (synchronises)."""
        return self.routes[:self.n * 16].cpu().numpy().view(TX_ROUTE_DTYPE)


def _tx_table(table, dtype, name, like):
    """(pointer, entries, tensor to keep alive) of a device table: None, a device uint8 tensor of
    whole entries, or a host array of `dtype` (uploaded here)."""
    torch = _torch()
    if table is None:
        return 0, 0, None
    if not hasattr(table, "data_ptr"):
        k = np.ascontiguousarray(table, dtype=dtype).reshape(-1)
        if k.size == 0:
            return 0, 0, None
        table = torch.from_numpy(k.view(np.uint8).copy()).to(like.device)
    _require_device(table, name)
    _same_device(table, like, f"{name} and headers")
    nbytes = table.numel() * table.element_size()
    if nbytes % dtype.itemsize:
        raise ValueError(f"{name} must hold whole {dtype.itemsize}-byte entries")
    return (table.data_ptr() if nbytes else 0), nbytes // dtype.itemsize, table


def tx_resolve(headers, hdr_stride: int, hdr_lens, ifaces, arp=None, *, seg_status=None,
               send_flags=None, force_iface=None, status=None, routes=None, send_lens=None,
               arp_used=None, held_seg=None, failed_seg=None, counts=None, workspace=None,
               stream=None) -> TxResolved:
    """Route, permission tests, next-hop MAC and Ethernet header of a batch of Tx header slots on
    the GPU (``aipstack_tx_resolve``): the batched form of the reference's ``routeIp4`` /
    ``routeIp4ForceIface``, ``checkSendIp4Allowed`` and ``EthIpIface::driverSendIp4Packet``.
    Segment i is the ``hdr_lens[i]`` bytes at ``headers[i * hdr_stride:]`` (what the Tx producers
    and the responders emit); its IPv4 addresses are read and, where it resolves
    (``AIPSTACK_TX_RES_SENT``), its bytes 0..13 are stored in place. ``ifaces``: the interface
    table (:func:`tx_ifaces`; a host array, uploaded on the launch stream, or a device uint8
    tensor); ``arp``: the ARP table snapshot sorted by :func:`arp_table_sort` (the same, or None).
    ``seg_status`` (uint8), ``send_flags`` (uint8: AIPSTACK_TX_ALLOW_*) and ``force_iface``
    (int16/uint16: an interface index or AIPSTACK_TX_ROUTE_ANY) are optional device tensors of n
    entries. Returns a :class:`TxResolved`; pass its ``send_lens`` to :func:`tx_linearise_slotted`
    as ``hdr_lens`` (chksum.h has the rules)."""
    torch = _torch()
    _require_device(headers, "headers")
    _require_device(hdr_lens, "hdr_lens")
    _same_device(headers, hdr_lens, "headers and hdr_lens")
    if hdr_lens.dtype not in (torch.int32, torch.uint32):
        raise ValueError("hdr_lens must be an int32/uint32 device tensor")
    n = hdr_lens.numel()
    if hdr_stride <= 0 or n * hdr_stride > headers.numel() * headers.element_size():
        raise ValueError("headers must hold n whole slots of hdr_stride bytes")
    opt = []
    for t, name, sizes in ((seg_status, "seg_status", (1,)), (send_flags, "send_flags", (1,)),
                           (force_iface, "force_iface", (2,))):
        if t is not None:
            _require_device(t, name)
            _same_device(headers, t, f"headers and {name}")
            if t.element_size() not in sizes or t.numel() < n:
                raise ValueError(f"{name} must hold n {sizes[0]}-byte entries")
        opt.append(t.data_ptr() if t is not None and n else None)
    launch_stream = _launch_stream(stream, headers.device)
    with torch.cuda.stream(launch_stream):  # an upload is ordered before the call
        ip, n_ifaces, ikeep = _tx_table(ifaces, TX_IFACE_DTYPE, "ifaces", headers)
        ap, n_arp, akeep = _tx_table(arp, ARP_ENTRY_DTYPE, "arp", headers)
    if ikeep is None:
        raise ValueError("ifaces must hold at least one interface")
    if send_lens is None:
        send_lens = torch.empty(n, dtype=torch.int32, device=headers.device)
    else:
        _require_device(send_lens, "send_lens")
        if send_lens.dtype not in (torch.int32, torch.uint32) or send_lens.numel() < n:
            raise ValueError("send_lens must be an int32/uint32 device tensor with >= n elements")
    res = TxResolved(_udp_out(status, n, 1, "status", headers), _udp_out(routes, n * 16, 1, "routes", headers),
                     send_lens, _udp_out(arp_used, n_arp, 1, "arp_used", headers),
                     _udp_out(held_seg, n, 8, "held_seg", headers),
                     _udp_out(failed_seg, n, 8, "failed_seg", headers),
                     _udp_out(counts, 2, 8, "counts", headers))
    if n == 0:  # nothing to launch: no entry was used, the counts are 0
        res.arp_used.zero_()
        res.counts.zero_()
        return res
    workspace, ws_bytes = _workspace(workspace, tx_resolve_workspace_bytes(n), headers, "headers")
    _check(_lib.load().aipstack_tx_resolve(
        headers.data_ptr(), hdr_stride, hdr_lens.data_ptr(), n, *opt, ip, n_ifaces, ap, n_arp,
        res.status.data_ptr(), res.routes.data_ptr(), res.send_lens.data_ptr(),
        res.arp_used.data_ptr() if n_arp else None, res.held_seg.data_ptr(),
        res.failed_seg.data_ptr(), res.counts.data_ptr(), workspace.data_ptr(), ws_bytes, 0,
        _stream_handle(launch_stream)), "aipstack_tx_resolve")
    workspace.record_stream(launch_stream)
    for keep, given in ((ikeep, ifaces), (akeep, arp)):
        if keep is not None and keep is not given:
            keep.record_stream(launch_stream)
    return res


AIPSTACK_TCP_CTL_MAX_HEADER = 62     # 54 + MSS 4 + window scale 4
AIPSTACK_TCP_CTL_EMITTED = 48        # tcp_tx_control: the slot holds the descriptor's segment
AIPSTACK_TCP_CTL_INVALID = 49        # a reserved field or an unknown option bit is set

# ``aipstack_tcp_ctl`` (chksum.h): one TCP segment without data, host byte order.
TCP_CTL_DTYPE = np.dtype({
    "names": ["local_addr", "remote_addr", "local_port", "remote_port", "seq", "ack", "window", "mss",
              "flags", "options", "wnd_scale", "reserved0", "reserved1"],
    "formats": ["<u4", "<u4", "<u2", "<u2", "<u4", "<u4", "<u2", "<u2", "u1", "u1", "u1", "u1", "<u4"],
    "offsets": [0, 4, 8, 10, 12, 16, 20, 22, 24, 25, 26, 27, 28],
    "itemsize": 32,
})
assert TCP_CTL_DTYPE.itemsize == 32


def tcp_ctl(entries) -> np.ndarray:
    """A ``TCP_CTL_DTYPE`` array from one mapping per segment: ``local_addr``, ``remote_addr``,
    ``local_port``, ``remote_port``, ``seq``, ``ack``, ``window``, ``flags`` (the low byte of
    OffsetFlags) and, where the segment carries them, ``mss`` and ``wnd_scale`` with their bits in
    ``options`` (``AIPSTACK_TCP_OPT_MSS`` / ``AIPSTACK_TCP_OPT_WND_SCALE``). A field left out is 0."""
    entries = list(entries)
    t = np.zeros(len(entries), dtype=TCP_CTL_DTYPE)
    for k, e in enumerate(entries):
        for name, v in e.items():
            if name not in TCP_CTL_DTYPE.names:
                raise ValueError(f"aipstack_tcp_ctl has no field {name!r}")
            t[k][name] = v
    return t


def tcp_tx_control_workspace_bytes(n: int) -> int:
    """``aipstack_tcp_tx_control_workspace_bytes``: the workspace :func:`tcp_tx_control` needs for
    n descriptors."""
    return int(_lib.load().aipstack_tcp_tx_control_workspace_bytes(max(n, 0)))


class TcpControlSegments:
    """What :func:`tcp_tx_control` leaves (device tensors, n descriptors): ``headers`` (uint8, n
    slots of ``hdr_stride`` bytes; slot i holds descriptor i's segment), ``hdr_lens`` (int32: 54,
    58, 62 or 0), ``chunk_index`` (int64, n + 1, all zero: no chunks), ``status`` (uint8:
    AIPSTACK_TCP_CTL_*) and ``counts`` (int64, 2: emitted, invalid). ``chunk_addr`` /
    ``chunk_len`` are empty, which makes the object a ``segments`` argument of
    :func:`tx_linearise` / :func:`tx_linearise_slotted` (an invalid descriptor is skipped);
    ``headers``, ``hdr_stride`` and ``hdr_lens`` are what :func:`tx_resolve` takes."""

    def __init__(self, headers, hdr_stride, hdr_lens, chunk_index, status, counts):
        torch = _torch()
        self.headers, self.hdr_stride, self.hdr_lens = headers, hdr_stride, hdr_lens
        self.chunk_index, self.status, self.counts = chunk_index, status, counts
        self.chunk_addr = torch.empty(0, dtype=torch.int64, device=headers.device)
        self.chunk_len = torch.empty(0, dtype=torch.int32, device=headers.device)

    @property
    def n(self) -> int:
        return self.chunk_index.numel() - 1


def tcp_tx_control(ctl, iface, *, tcp_ttl: int = 64, hdr_stride: int = 64, headers=None,
                   workspace=None, stream=None) -> TcpControlSegments:
    """TCP segments without data on the GPU (``aipstack_tcp_tx_control``): the batched form of the
    reference's ``send_tcp_nodata`` for SYN, SYN-ACK, empty ACK, FIN and RST. ``ctl``: the
    descriptors, a ``TCP_CTL_DTYPE`` host array (:func:`tcp_ctl`; uploaded on the launch stream)
    or a device uint8 tensor of whole 32-byte descriptors already resident. ``iface``: an
    ``ICMP_IFACE_DTYPE`` record (:func:`icmp_iface`; its ``mac`` is the Ethernet source, its
    ``ip_id`` the Ident of the first valid descriptor; ``tcp_ttl`` is the TTL). The j-th valid
    descriptor carries the Ident ``ip_id + j`` and lies in slot i of the header ring ``headers``
    (a uint8 device tensor of n slots of ``hdr_stride`` >= 62 bytes; fresh and zeroed when None);
    bytes 0..5 of a slot are 0 until :func:`tx_resolve` writes the next hop's MAC. Returns a
    :class:`TcpControlSegments`; the host advances its Ident counter by ``counts[0]`` (chksum.h
    has the rules and the byte layout). With no descriptor at all nothing runs: ``chunk_index``
    (one entry) and ``counts`` are set to 0."""
    torch = _torch()
    f = np.ascontiguousarray(iface, dtype=ICMP_IFACE_DTYPE).reshape(-1)
    if f.size != 1:
        raise ValueError("iface must be one ICMP_IFACE_DTYPE record")
    if hasattr(ctl, "data_ptr"):
        dev = ctl.device
    elif headers is not None:
        dev = headers.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    launch_stream = _launch_stream(stream, dev)
    with torch.cuda.stream(launch_stream):  # an upload is ordered before the call
        if not hasattr(ctl, "data_ptr"):
            k = np.ascontiguousarray(ctl, dtype=TCP_CTL_DTYPE).reshape(-1)
            given, ctl = None, torch.from_numpy(k.view(np.uint8).copy()).to(dev)
        else:
            given = ctl
        _require_device(ctl, "ctl")
        nbytes = ctl.numel() * ctl.element_size()
        if nbytes % 32:
            raise ValueError("ctl must hold whole 32-byte descriptors")
        n = nbytes // 32
        if headers is None:
            headers = torch.zeros(max(n, 1) * hdr_stride, dtype=torch.uint8, device=dev)
        _require_device(headers, "headers")
        _same_device(ctl, headers, "ctl and headers")
        if headers.element_size() != 1 or hdr_stride <= 0 or headers.numel() < n * hdr_stride:
            raise ValueError("headers must be a uint8 device tensor of n whole slots of hdr_stride bytes")
        res = TcpControlSegments(headers, hdr_stride,
                                 torch.empty(n, dtype=torch.int32, device=dev),
                                 torch.empty(n + 1, dtype=torch.int64, device=dev),
                                 torch.empty(n, dtype=torch.uint8, device=dev),
                                 torch.empty(2, dtype=torch.int64, device=dev))
        if n == 0:  # nothing to launch
            res.chunk_index.zero_()
            res.counts.zero_()
            return res
    workspace, ws_bytes = _workspace(workspace, tcp_tx_control_workspace_bytes(n), headers, "headers")
    _check(_lib.load().aipstack_tcp_tx_control(
        ctl.data_ptr(), n, f.ctypes.data, tcp_ttl, headers.data_ptr(), hdr_stride,
        res.hdr_lens.data_ptr(), res.chunk_index.data_ptr(), res.status.data_ptr(),
        res.counts.data_ptr(), workspace.data_ptr(), ws_bytes, _stream_handle(launch_stream)),
        "aipstack_tcp_tx_control")
    workspace.record_stream(launch_stream)
    if ctl is not given:
        ctl.record_stream(launch_stream)
    return res


class SplitFrames:
    """What :func:`split_frames` returns (host arrays): ``headers`` (n slots of ``hdr_stride``
    bytes), ``hdr_lens`` (uint32), ``payload`` (uint8, every chunk's bytes) and ``chunks``
    (per segment, its ``(offset into payload, length)`` chunks in order)."""

    def __init__(self, headers, hdr_stride, hdr_lens, payload, chunks):
        self.headers, self.hdr_stride, self.hdr_lens = headers, hdr_stride, hdr_lens
        self.payload, self.chunks = payload, chunks

    def __iter__(self):  # headers, hdr_lens, payload, chunks = split_frames(...)
        return iter((self.headers, self.hdr_lens, self.payload, self.chunks))

    def chunk_table(self, payload_base: int = 0):
        """(addr uint64, len uint32, index uint64) of the chunk table with the payload buffer
        at address ``payload_base`` (a device copy's ``data_ptr()``)."""
        addr = [payload_base + o for seg in self.chunks for o, _ in seg]
        lens = [l for seg in self.chunks for _, l in seg]
        index = np.zeros(len(self.chunks) + 1, dtype=np.uint64)
        index[1:] = np.cumsum([len(seg) for seg in self.chunks])
        return np.array(addr, dtype=np.uint64), np.array(lens, dtype=np.uint32), index

    def linearise(self, headers=None, payload=None):
        """The segments back to back again: (uint8 buffer, uint64 offsets of n+1 entries), from
        this layout's arrays or from ``headers`` / ``payload`` given in their place."""
        h = self.headers if headers is None else np.asarray(headers).reshape(-1).view(np.uint8)
        p = self.payload if payload is None else np.asarray(payload).reshape(-1).view(np.uint8)
        parts, offs = [], [0]
        for i, seg in enumerate(self.chunks):
            s = i * self.hdr_stride
            parts.append(h[s:s + int(self.hdr_lens[i])])
            parts += [p[o:o + l] for o, l in seg]
            offs.append(offs[-1] + int(self.hdr_lens[i]) + sum(l for _, l in seg))
        buf = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        return buf.astype(np.uint8, copy=False), np.array(offs, dtype=np.uint64)


def split_frames(frames, offsets, split_at, *, hdr_stride: int, payload_pieces=None,
                 payload_gap: int = 0, reverse: bool = False) -> SplitFrames:
    """Host helper: lay linear frames out as header-split segments. Frame i =
    ``frames[offsets[i]:offsets[i+1]]``; its first ``split_at[i]`` bytes (clipped to the frame
    and to ``hdr_stride``) go into header slot i, the rest into a payload buffer, cut into the
    chunk lengths ``payload_pieces[i]`` (a sequence; the last chunk takes what remains, empty
    chunks are dropped; None = one chunk). ``payload_gap`` bytes separate consecutive chunks in
    the payload buffer (so chunks land at odd addresses); ``reverse`` places them in reverse
    memory order. Slot bytes past a header are 0xEE, gaps 0xDD."""
    fr = np.asarray(frames).reshape(-1).view(np.uint8)
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    n = off.size - 1
    if hdr_stride <= 0:
        raise ValueError("hdr_stride must be positive")
    headers = np.full(max(n, 0) * hdr_stride, 0xEE, dtype=np.uint8)
    hdr_lens = np.zeros(max(n, 0), dtype=np.uint32)
    pieces = []  # (segment, bytes)
    per_seg = []
    for i in range(n):
        f = fr[off[i]:off[i + 1]]
        h = max(0, min(int(split_at[i]), f.size, hdr_stride))
        hdr_lens[i] = h
        headers[i * hdr_stride:i * hdr_stride + h] = f[:h]
        rest = f[h:]
        cuts = list(payload_pieces[i]) if payload_pieces is not None else []
        segs, at = [], 0
        for c in cuts:
            c = min(int(c), rest.size - at)
            if c > 0:
                segs.append(rest[at:at + c])
                at += c
        if at < rest.size:
            segs.append(rest[at:])
        per_seg.append(len(segs))
        pieces += segs
    # place the chunks: in order or reversed, payload_gap bytes apart
    order = range(len(pieces) - 1, -1, -1) if reverse else range(len(pieces))
    where = [0] * len(pieces)
    at = payload_gap
    for k in order:
        where[k] = at
        at += pieces[k].size + payload_gap
    payload = np.full(max(at, 1), 0xDD, dtype=np.uint8)
    for k, pc in enumerate(pieces):
        payload[where[k]:where[k] + pc.size] = pc
    chunks, k = [], 0
    for cnt in per_seg:
        chunks.append([(where[k + j], int(pieces[k + j].size)) for j in range(cnt)])
        k += cnt
    return SplitFrames(headers, hdr_stride, hdr_lens, payload, chunks)


def tx_fill_records(frames, offsets, *, out=None, stream=None):
    """The split Tx fill's read pass alone (``aipstack_chksum_tx_fill_records``): one 8-byte
    record per frame, nothing written into the frames. Record i = ``w0 | w1 << 32`` with
    ``w0`` = IPv4 header checksum | L4 checksum << 16 and ``w1`` = L4 field offset (bits
    0-7) | write the IPv4 field (8) | write the L4 field (9) | status (16-23); the host
    applies them (:func:`apply_tx_records`). Returns the records (int64 device tensor)."""
    _require_device(frames, "frames")
    _require_offsets(offsets)
    _same_device(frames, offsets, "frames and offsets")
    n = max(offsets.numel() - 1, 0)
    out = _records_out(out, n, frames)
    _check(_lib.load().aipstack_chksum_tx_fill_records(frames.data_ptr(), offsets.data_ptr(), n,
                                                       out.data_ptr(), _stream_handle(stream, frames)),
           "aipstack_chksum_tx_fill_records")
    return out


def slots_to_offsets(n: int, slot_stride: int) -> np.ndarray:
    """Frame start offsets of n ring slots (for :func:`apply_tx_records`): i * slot_stride."""
    return np.arange(n + 1, dtype=np.uint64) * np.uint64(slot_stride)


def apply_tx_records(frames: np.ndarray, offsets: np.ndarray, records: np.ndarray,
                     status: Optional[np.ndarray] = None) -> np.ndarray:
    """Apply Tx fill records (:func:`tx_fill_records`) to frames in HOST memory (numpy, in
    place), as the engine's completion does: the IPv4 header checksum big-endian at frame
    byte 24, the L4 checksum at the record's field offset, each when its flag is set.
    Returns the per-frame statuses (uint8)."""
    rec = np.ascontiguousarray(records).view(np.uint64)
    o = np.ascontiguousarray(offsets, dtype=np.uint64)[:rec.size]
    w0 = (rec & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    w1 = (rec >> np.uint64(32)).astype(np.uint32)
    if status is None:
        status = np.empty(rec.size, dtype=np.uint8)
    status[:rec.size] = (w1 >> 16) & 0xFF
    flat = frames.reshape(-1).view(np.uint8)
    for flag, at, val in ((0x100, o + np.uint64(24), w0 & 0xFFFF),
                          (0x200, o + (w1 & 0xFF).astype(np.uint64), w0 >> 16)):
        sel = (w1 & flag) != 0
        a = at[sel].astype(np.int64)
        v = val[sel]
        flat[a] = (v >> 8).astype(np.uint8)
        flat[a + 1] = (v & 0xFF).astype(np.uint8)
    return status


RX_VERDICTS = {0: "NOT_IP4", 1: "DROP_IP_MALFORMED", 2: "DROP_IP_CHKSUM", 3: "FRAGMENT",
               4: "DROP_L4_MALFORMED", 5: "DROP_L4_CHKSUM", 6: "ACCEPT",
               7: "ACCEPT_NO_CHKSUM", 8: "ACCEPT_OTHER", 11: "DROP_TCP_OFFSET",
               14: "FRAG_MEMBER", 15: "DROP_FRAG", 16: "REASS_TRUNCATED"}


def flatten_chains(refs, host_base: np.ndarray, device_base: int):
    """Flatten IpBufRef chains whose nodes point into `host_base` (a numpy byte array
    mirrored on the device at `device_base`) into the chunk table of
    :func:`chksum_batch_chain`: the non-empty chunks ipBufProcessBytes visits
    (BufUtils.h:129-178), translated to device addresses. Returns numpy
    (addr uint64, len uint32, index uint64)."""
    base_ptr = host_base.ctypes.data
    addrs, lens, index = [], [], [0]
    for ref in refs:
        if ref.tot_len > 0:
            def visit(mv, n):
                ptr = np.frombuffer(mv, dtype=np.uint8).ctypes.data
                if not base_ptr <= ptr < base_ptr + host_base.nbytes:
                    raise ValueError("chain node outside host_base")
                addrs.append(device_base + (ptr - base_ptr))
                lens.append(n)
                return n
            ipBufProcessBytes(ref, ref.tot_len, visit)
        index.append(len(addrs))
    return (np.array(addrs, dtype=np.uint64), np.array(lens, dtype=np.uint32),
            np.array(index, dtype=np.uint64))


VIOLATION_PACKET_LEN = 1
VIOLATION_CHUNK_LEN = 2
VIOLATION_SPAN = 4


def contract_violations(device: int = 0, clear: bool = True) -> int:
    """Sticky contract-violation bits (VIOLATION_*) the kernels met on `device` since the
    last clear (``aipstack_chksum_contract_violations``; waits for the device to go idle)."""
    m = ctypes.c_uint32(0)
    _check(_lib.load().aipstack_chksum_contract_violations(device, ctypes.byref(m), int(clear)),
           "aipstack_chksum_contract_violations")
    return int(m.value)


def device_check(device: int = 0) -> int:
    """AIPSTACK_CHKSUM_OK if `device` is a gfx950 device the library can launch on."""
    return int(_lib.load().aipstack_chksum_device_check(device))
