"""TEST INFRASTRUCTURE -- where the bytes of the large-span linearise cases lie
(test_gpu_large_span_linearise.py), on the arena and windows of large_span_cases.py. Pure
functions of the arena's device address P; test_large_span_linearise_cases.py runs them for fake
pointers and checks what they cover.

Three layouts:
  ring_case     the destination is a ring of N_RING slots of 65536 bytes from P + shift: slots
                32768 and 65536 start 2^31 and 2^32 bytes from d_frames. Sources are small and lie
                outside the arena (headers and a 64 KiB payload pool the test uploads).
  csr_case      the destination is the arena from P + shift with CSR offsets: runs of small frames
                round offset 0, across 2^31, across 2^32 and at the end, skipped filler segments
                (header length 0) with rooms of gigabytes between them. Sources as above.
  source_case   the sources lie in the arena round A = a multiple of 2^32 as a device address:
                the payload chunks (below, above and across A at every distance of DISTANCES) or
                the header ring (slot n/2 starts at A). The destination is a small ring elsewhere.
The frames are small (at most 54 + MAX_PAY bytes); the model is linearise_cases.outcome plus
plain concatenation."""
import numpy as np

import large_span_cases as L
import linearise_cases as LC

STRIDE = 65536
N_RING = 65538
MAX_PAY = 200
ROW = 54 + MAX_PAY + 2           # bytes of a slot the test reads back (every frame ends before)
POOL = 64 * L.KiB
DISTANCES = (1, 15, 16, 17, "len-1")
HDR_STRIDE = 64


class Case:
    """hdr (the header ring, n * 64 bytes), hdr_lens, chunk table (chunk k: chunk_len[k] bytes at
    device address chunk_addr[k]; its bytes are chunk_bytes(k)), index, and one of slot_stride /
    offsets. windows: what the test copies into the arena before the call. dest_off: arena offset
    of d_frames, None when the destination is a tensor of its own; hdr_off / pool_off likewise."""

    frame_max = 54 + MAX_PAY

    @property
    def n(self):
        return self.hdr_lens.size

    def chunk_bytes(self, k):
        o = int(self.chunk_src[k])
        return self.pool[o:o + int(self.chunk_len[k])]

    def plan(self):
        """(lens, status) of every segment by the model's rule."""
        lens, status = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.uint8)
        for i in range(self.n):
            st, ln = LC.outcome(int(self.hdr_lens[i]), HDR_STRIDE, None, int(self.index[i]),
                                int(self.index[i + 1]), self.chunk_len, self.frame_max)
            if st == LC.WRITTEN and self.offsets is not None and \
                    ln != int(self.offsets[i + 1]) - int(self.offsets[i]):
                st, ln = LC.WRONG_ROOM, 0
            lens[i], status[i] = ln, st
        return lens, status

    def frame(self, i):
        parts = [self.hdr[i * HDR_STRIDE:i * HDR_STRIDE + int(self.hdr_lens[i])]]
        parts += [self.chunk_bytes(k) for k in range(int(self.index[i]), int(self.index[i + 1]))]
        return np.concatenate(parts)

    def frame_start(self, i):
        return i * self.slot_stride if self.offsets is None else int(self.offsets[i])


def _segments(rng, n, pool_addr, pool_bytes, skip=()):
    """n small TCP-shaped segments (54-byte headers; 0, 1 or 2 chunks from the pool); those in
    `skip` have header length 0."""
    c = Case()
    c.hdr = rng.integers(0, 256, n * HDR_STRIDE, dtype=np.uint8)
    c.hdr_lens = np.full(n, 54, dtype=np.uint32)
    c.hdr_lens[list(skip)] = 0
    addr, ln, src, index = [], [], [], [0]
    for i in range(n):
        for _ in range(int(rng.integers(0, 3)) if i not in skip else 0):
            l = int(rng.integers(0, MAX_PAY // 2 + 1))
            o = int(rng.integers(0, pool_bytes - l))
            addr.append(pool_addr + o); ln.append(l); src.append(o)
        index.append(len(ln))
    addr.append(pool_addr); ln.append(0); src.append(0)     # never an empty table
    c.chunk_addr = np.array(addr, dtype=np.uint64)
    c.chunk_len = np.array(ln, dtype=np.uint32)
    c.chunk_src = np.array(src, dtype=np.int64)
    c.index = np.array(index, dtype=np.uint64)
    c.offsets, c.slot_stride = None, None
    c.windows, c.dest_off, c.hdr_off, c.pool_off = [], None, None, None
    return c


def ring_rows(n=N_RING):
    """The rows compared byte for byte: near both edges and the ends, and every 61st."""
    near = [0, 1, 2, 32766, 32767, 32768, 32769, 32770, 65534, 65535, 65536, n - 1]
    return sorted(set(near) | set(range(0, n, 61)))


def ring_case(pool_addr, shift, seed=0):
    rng = np.random.default_rng(500 + seed + shift)
    c = _segments(rng, N_RING, pool_addr, POOL)
    c.pool = rng.integers(0, 256, POOL, dtype=np.uint8)
    c.slot_stride, c.dest_off = STRIDE, shift
    assert shift + N_RING * STRIDE <= L.ARENA_BYTES
    return c


def csr_case(pool_addr, shift, distance, seed=0):
    """Runs of RUN small frames at offset 0, across each edge (the frame across it starts
    `distance` bytes before the edge) and after a last filler; c.across = those two frames,
    c.runs = (first segment, count) of every run, c.fillers = the skipped segments."""
    RUN = 40
    rng = np.random.default_rng(600 + seed + shift)
    n = 4 * RUN + 3
    fillers = [RUN, 2 * RUN + 1, 3 * RUN + 2]
    c = _segments(rng, n, pool_addr, POOL, skip=fillers)
    c.pool = rng.integers(0, 256, POOL, dtype=np.uint8)
    lens = c.hdr_lens.astype(np.int64) + np.array(
        [int(c.chunk_len[int(c.index[i]):int(c.index[i + 1])].sum()) for i in range(n)])
    off = np.zeros(n + 1, dtype=np.uint64)
    c.runs, c.across = [], []
    at, i = 0, 0
    for r, edge in enumerate((None,) + L.EDGES + (None,)):
        if r:                                              # segment i: the filler before this run
            first = i + 1
            j = first + RUN // 2                           # the frame across the edge
            d = int(lens[j]) - 1 if distance == "len-1" else distance
            if edge is not None:
                start = edge - d - int(lens[first:j].sum())
                c.across.append(j)
            else:
                start = at + (1 << 29)
            off[first] = start                             # the filler's room: gigabytes
            i = first
        c.runs.append((i, RUN))
        for k in range(i, i + RUN):
            off[k + 1] = off[k] + np.uint64(lens[k])
        at, i = int(off[i + RUN]), i + RUN
    c.fillers = fillers
    c.offsets, c.dest_off = off, shift
    assert shift + int(off[-1]) <= L.ARENA_BYTES
    return c


def address_edge(P):
    """Arena offset of a device address that is a multiple of 2^32, at least 1 MiB inside."""
    e = L.a4_of(P) - P
    if e < L.MiB:
        e += L.E32
    assert L.MiB <= e <= L.ARENA_BYTES - L.MiB
    return e


def source_case(P, what, seed=0):
    """what = "payload": the pool lies in the arena, POOL / 2 bytes on either side of A; chunks
    below, above and across it (one per distance). what = "headers": the header ring lies in the
    arena with slot n / 2 starting at A; the pool is a tensor of its own at `pool_addr` 0 (the
    test adds its address)."""
    rng = np.random.default_rng(700 + seed)
    e = address_edge(P)
    n = 600
    if what == "payload":
        pool_off = e - POOL // 2
        c = _segments(rng, n, P + pool_off, POOL)
        c.pool = rng.integers(0, 256, POOL, dtype=np.uint8)
        c.pool_off = pool_off
        # the first chunk of segments 8, 16, ... across A at each distance
        c.across = []
        ones = [i for i in range(8, n, 8) if c.index[i + 1] > c.index[i]]
        for i, dist in zip(ones, DISTANCES * 4):
            k = int(c.index[i])
            l = max(int(c.chunk_len[k]), 20)
            d = l - 1 if dist == "len-1" else dist
            c.chunk_len[k], c.chunk_src[k] = l, POOL // 2 - d
            c.chunk_addr[k] = P + pool_off + POOL // 2 - d
            c.across.append(k)
        c.windows = [L.Window(pool_off, c.pool)]
    else:
        c = _segments(rng, n, 0, POOL)
        c.pool = rng.integers(0, 256, POOL, dtype=np.uint8)
        c.hdr_off = e - (n // 2) * HDR_STRIDE
        c.windows = [L.Window(c.hdr_off, c.hdr)]
    c.slot_stride = 512
    c.edge = e
    return c
