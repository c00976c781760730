"""Model and generator for the linearise tests (aipstack_tx_linearise / _slotted).

The model is plain concatenation per segment (SplitFrames.linearise's idea) plus the status rule
of chksum.h written out here, independently of aipstack_amd/csrc/linearise_common.h. A Scenario
is host arrays only; tests/test_gpu_linearise.py puts it on the device."""
import numpy as np

WRITTEN, SKIPPED, INVALID, TOO_SHORT, TOO_LARGE, WRONG_ROOM = 17, 18, 19, 20, 21, 22
OUTCOMES = (WRITTEN, SKIPPED, INVALID, TOO_SHORT, TOO_LARGE, WRONG_ROOM)
BURST_INVALID, DGRAM_INVALID, SPLIT_LAYOUT, ACCEPT = 10, 13, 9, 6
MAX_SPLIT_HEADER = 256
SENTINEL = 0xA5      # destination bytes nobody may touch
HDR_SLACK = 0xEE     # header slot bytes past hdr_len


def outcome(H, cap, seg_status, kbeg, kend, chunk_len, frame_max):
    """(status, L) of one segment by the rule of chksum.h, the room not yet looked at."""
    if H == 0 or seg_status in (BURST_INVALID, DGRAM_INVALID):
        return SKIPPED, 0
    if H > cap or kend < kbeg:
        return INVALID, 0
    total = H
    for k in range(kbeg, kend):
        if total > frame_max:       # the sum stopped here: what follows is not looked at
            break
        if chunk_len[k] > 65535:
            return INVALID, 0
        total += int(chunk_len[k])
    if total < 14:
        return TOO_SHORT, 0
    if total > frame_max:
        return TOO_LARGE, 0
    return WRITTEN, total


class Seg:
    """One segment as the generator describes it: header length, chunk lengths, the producer's
    status, and where its pieces should lie (src_align: address of the first chunk mod 16)."""

    def __init__(self, H, chunks=(), status=ACCEPT, src_align=None, room=None, tag=""):
        self.H, self.chunks, self.status = H, list(chunks), status
        self.src_align, self.room, self.tag = src_align, room, tag


class Scenario:
    """Host arrays of one call. bufs: the source allocations; chunk k is chunk_len[k] bytes at
    offset chunk_off[k] of bufs[chunk_buf[k]]. form "slots": frame i at i * slot_stride of a
    destination of n * slot_stride bytes; "csr": at offsets[i] of one of offsets[n] bytes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n(self):
        return self.hdr_lens.size

    def dest_bytes(self):
        return self.n * self.slot_stride if self.form == "slots" else int(self.offsets[-1])

    def frame_start(self, i):
        return i * self.slot_stride if self.form == "slots" else int(self.offsets[i])

    def gather(self, i, L):
        """The first L bytes of segment i, byte by byte what sendFrame's copy gives."""
        s = i * self.hdr_stride
        parts = [self.headers[s:s + int(self.hdr_lens[i])]]
        for k in range(int(self.index[i]), int(self.index[i + 1])):
            b, o, l = self.chunk_buf[k], int(self.chunk_off[k]), int(self.chunk_len[k])
            parts.append(self.bufs[b][o:o + l])
        out = np.concatenate(parts)
        assert out.size == L
        return out

    def expected(self):
        """(destination bytes, lens int32, status uint8) the call must leave, the destination
        prefilled with SENTINEL."""
        n = self.n
        cap = min(self.hdr_stride, MAX_SPLIT_HEADER)
        dest = np.full(self.dest_bytes(), SENTINEL, dtype=np.uint8)
        lens = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.uint8)
        for i in range(n):
            ss = int(self.seg_status[i]) if self.seg_status is not None else None
            st, L = outcome(int(self.hdr_lens[i]), cap, ss, int(self.index[i]),
                            int(self.index[i + 1]), self.chunk_len, self.frame_max)
            if st == WRITTEN and self.form == "csr" and \
                    L != (int(self.offsets[i + 1]) - int(self.offsets[i])) % (1 << 64):
                st, L = WRONG_ROOM, 0
            status[i], lens[i] = st, L
            if st == WRITTEN:
                at = self.frame_start(i)
                dest[at:at + L] = self.gather(i, L)
        return dest, lens, status

    def pieces(self, i):
        """Header + non-empty chunks of segment i (what a frame's piece prefix holds)."""
        return 1 + max(0, int(self.index[i + 1]) - int(self.index[i]))


def build(segs, rng, *, form, frame_max=1514, slot_stride=2048, hdr_stride=64, n_bufs=3,
          decreasing=(), with_status=True, max_gap=17):
    """Lay the described segments out. Chunks go to n_bufs source buffers at random gaps (0 =
    back to back), each buffer sized so that its last chunk ends at its last byte (three spare
    chunks lie in one more buffer). `decreasing`:
    segment numbers (of zero-chunk segments) whose index entry is pushed 3 above the next one.
    CSR rooms: a written frame gets exactly L (or seg.room), anything else seg.room or a few
    bytes that must stay untouched."""
    n = len(segs)
    headers = np.full(max(n, 1) * hdr_stride, HDR_SLACK, dtype=np.uint8)
    hdr_lens = np.array([s.H for s in segs], dtype=np.uint32)
    seg_status = np.array([s.status for s in segs], dtype=np.uint8) if with_status else None
    index = np.zeros(n + 1, dtype=np.uint64)
    chunk_buf, chunk_off, chunk_len = [], [], []
    fill = [0] * n_bufs
    for i, s in enumerate(segs):
        h = min(s.H, hdr_stride)
        headers[i * hdr_stride:i * hdr_stride + h] = rng.integers(0, 256, h, dtype=np.uint8)
        for c, l in enumerate(s.chunks):
            b = int(rng.integers(0, n_bufs))
            at = fill[b] + int(rng.integers(0, max_gap + 1))
            if c == 0 and s.src_align is not None:
                at += (s.src_align - at) % 16
            real = l if l <= 65535 else 0     # an oversized chunk's bytes are never read
            chunk_buf.append(b); chunk_off.append(at); chunk_len.append(l)
            fill[b] = at + real
        index[i + 1] = len(chunk_len)
    fill.append(0)                            # spare chunks a pushed-up index entry may reach, in
    for _ in range(3):                        # a buffer of their own: the others end with a chunk
        chunk_buf.append(n_bufs); chunk_off.append(fill[n_bufs]); chunk_len.append(2)
        fill[n_bufs] += 2
    for i in decreasing:
        assert not segs[i].chunks
        index[i] += 3
    bufs = [rng.integers(0, 256, max(f, 1), dtype=np.uint8) for f in fill]
    sc = Scenario(form=form, frame_max=frame_max, slot_stride=slot_stride, hdr_stride=hdr_stride,
                  headers=headers, hdr_lens=hdr_lens, seg_status=seg_status, index=index,
                  chunk_buf=np.array(chunk_buf, dtype=np.int64),
                  chunk_off=np.array(chunk_off, dtype=np.int64),
                  chunk_len=np.array(chunk_len, dtype=np.uint32), bufs=bufs, offsets=None,
                  tags=[s.tag for s in segs])
    if form == "csr":
        cap = min(hdr_stride, MAX_SPLIT_HEADER)
        off = np.zeros(n + 1, dtype=np.uint64)
        for i, s in enumerate(segs):
            st, L = outcome(s.H, cap, s.status if with_status else None, int(index[i]),
                            int(index[i + 1]), sc.chunk_len, frame_max)
            room = s.room if s.room is not None else (L if st == WRITTEN else int(rng.integers(0, 40)))
            off[i + 1] = off[i] + room
        sc.offsets = off
    return sc


# ---- seeded scenarios -------------------------------------------------------------------

def _tcp_segs(rng, n, frame_max):
    mss = frame_max - 54
    segs = []
    for _ in range(n):
        r = rng.random()
        p = mss if r < 0.6 else int(rng.integers(0, mss + 1))
        if p and rng.random() < 0.2:          # the burst's range wraps: two pieces
            a = int(rng.integers(1, p + 1))
            ch = [a, p - a] if p - a else [a]
        else:
            ch = [p] if p else []
        st = BURST_INVALID if rng.random() < 0.03 else ACCEPT
        segs.append(Seg(54, ch, st, tag="tcp"))
    return segs


def _udp_segs(rng, n, frame_max):
    segs = []
    for _ in range(n):
        first = rng.random() < 0.3
        H = 42 if first else 34
        if rng.random() < 0.05:               # an invalid datagram: nothing emitted
            segs.append(Seg(0, [], DGRAM_INVALID, tag="udp-none"))
            continue
        p = int(rng.integers(0, frame_max - H + 1)) & (~7 if rng.random() < 0.7 else ~0)
        if p and rng.random() < 0.15:
            a = int(rng.integers(1, p + 1))
            ch = [a, p - a] if p - a else [a]
        else:
            ch = [p] if p else []
        segs.append(Seg(H, ch, ACCEPT, tag="udp"))
    return segs


def _adversarial_segs(rng, n, frame_max, form, hdr_stride):
    segs, decreasing = [], []
    cap = min(hdr_stride, MAX_SPLIT_HEADER)
    kinds = ["many", "nochunk", "l14", "lmax", "lmax1", "short", "hbig", "chunkbig", "decr",
             "skip0", "skip10", "skip13", "st9", "plain"] + (["room"] if form == "csr" else [])
    for _ in range(n):
        k = kinds[int(rng.integers(0, len(kinds)))]
        H = int(rng.integers(14, cap + 1))
        if k == "many":
            cnt = int(rng.integers(65, 301))
            segs.append(Seg(H, [int(x) for x in rng.integers(0, 4, cnt)], tag=k))
        elif k == "nochunk":
            segs.append(Seg(H, [], tag=k))
        elif k == "l14":
            h = int(rng.integers(1, 15))
            segs.append(Seg(h, [14 - h] if h < 14 else [], tag=k))
        elif k in ("lmax", "lmax1"):
            L = frame_max + (k == "lmax1")
            a = int(rng.integers(0, L - H + 1))
            segs.append(Seg(H, [a, L - H - a], tag=k))
        elif k == "short":
            h = int(rng.integers(1, 13))
            segs.append(Seg(h, [int(rng.integers(0, 13 - h + 1))], tag=k))
        elif k == "hbig":
            segs.append(Seg(cap + int(rng.integers(1, 5)), [20], tag=k))
        elif k == "chunkbig":
            segs.append(Seg(H, [3, 65536 + int(rng.integers(0, 9))], tag=k))
        elif k == "decr":
            decreasing.append(len(segs))
            segs.append(Seg(H, [], tag=k))
        elif k == "skip0":
            segs.append(Seg(0, [30], tag=k))
        elif k in ("skip10", "skip13"):
            segs.append(Seg(H, [40], BURST_INVALID if k == "skip10" else DGRAM_INVALID, tag=k))
        elif k == "st9":
            segs.append(Seg(H, [int(rng.integers(0, 200))], SPLIT_LAYOUT, tag=k))
        elif k == "room":
            p = int(rng.integers(1, 300))
            d = int(rng.integers(1, 20))
            segs.append(Seg(H, [p], room=H + p + (d if rng.random() < 0.5 else -d), tag=k))
        else:
            segs.append(Seg(H, [int(rng.integers(0, frame_max - H + 1))], tag=k))
    return segs, decreasing


N_SCENARIOS = 40


def scenario(seed):
    """Seeded scenario `seed` of N_SCENARIOS: TCP-shaped, UDP-fragment-shaped and adversarial in
    turn, slotted and offsets forms alternating."""
    rng = np.random.default_rng(9000 + seed)
    form = "slots" if seed % 2 == 0 else "csr"
    kind = ("tcp", "udp", "adversarial")[seed % 3]
    frame_max = (1514, 576, 300, 1514)[seed % 4]
    hdr_stride = (64, 64, 256, 300)[(seed // 2) % 4] if kind == "adversarial" else 64
    slot_stride = (2048, 1536, frame_max)[seed % 3] if frame_max <= 1536 else 2048
    n = int(rng.integers(150, 400))
    decreasing = ()
    if kind == "tcp":
        segs = _tcp_segs(rng, n, frame_max)
    elif kind == "udp":
        segs = _udp_segs(rng, n, frame_max)
    else:
        segs, decreasing = _adversarial_segs(rng, n, frame_max, form, hdr_stride)
    return build(segs, rng, form=form, frame_max=frame_max, slot_stride=slot_stride,
                 hdr_stride=hdr_stride, decreasing=decreasing)
