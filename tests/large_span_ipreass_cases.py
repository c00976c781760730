"""TEST INFRASTRUCTURE -- the case generator of test_gpu_large_span_ipreass.py, on the arena,
windows and filler of large_span_cases.py: fragments of one datagram on both sides of a 2^31 and a
2^32 byte offset from the base handed to aipstack_ip4_rx_reassemble, and of a device address that
is a multiple of 2^32. It needs no GPU: test_large_span_ipreass_cases.py runs it for fake base
pointers.

A case is a pure function of (P, shift, distance): CSR offsets from the base P + shift; filler
frames of 65535 zero bytes (64 of them span less than 4 MiB, the frame batches' contract); one
window round each edge with the frames back to back: a `pre` side, the frame that holds the edge
byte -- it starts `distance` bytes before it -- and a `post` side. Every datagram has a fragment
in every side of every window, and datagram 0 owns the straddling frames, so every link of its
list goes from one side of an edge to the other. The expectation is the model of
ipreass_cases.py on the windows' frames alone, its frame indices mapped to the batch's."""
import numpy as np

import ipreass_cases as R
import large_span_cases as L

DISTANCES = (1, 17, 40, "len-1")      # the Ethernet header, the IPv4 header, the payload straddle
N_DGRAMS = 24
PIECE = 1400                          # >= 32 KiB of fragments on either side of an edge


def edges_of(P, shift):
    """Offsets from the base P + shift: 2^31, 2^32 and the first one at an address that is a
    multiple of 2^32 with room for its window (none only if such an address lies within 128 KiB
    of one of the two offsets: for shift 0 and an aligned P the 2^32 offset is that address)."""
    es = [L.E31, L.E32]
    room = 128 * L.KiB
    for a4 in (L.a4_of(P) - (P + shift), L.a4_of(P) + L.E32 - (P + shift)):
        if all(abs(a4 - e) > room for e in es) and room < a4 < L.ARENA_BYTES - shift - room:
            es.append(a4)
            break
    return sorted(es)


class Case:
    """offsets (uint64, n + 1), windows, runs [(first frame, count, window)], across [frame that
    holds each edge byte], frames {frame index: bytes} of the windows' frames, edges."""


def case(P, shift, distance, seed=0):
    rng = np.random.default_rng(900 + seed + shift)
    edges = edges_of(P, shift)
    W = len(edges)
    sides = 2 * W + W                                   # pre, straddler (datagram 0 only), post
    # datagram d: UDP, cut into 2 * W pieces of PIECE bytes (datagram 0: 3 * W); some are made
    # incomplete or corrupt so that not everything round an edge is one verdict
    per = [[[] for _ in range(3)] for _ in range(W)]    # per window: pre, mid, post frames
    for d in range(N_DGRAMS):
        k = sides if d == 0 else 2 * W
        src, dst = 0x0A640000 + d, 0x0A650001
        data = rng.integers(0, 256, k * PIECE - 8 - int(rng.integers(0, 9)), dtype=np.uint8).tobytes()
        body = R.udp_body(src, dst, 1000 + d, 53, data) if d % 5 != 4 else R.tcp_body(src, dst, 80, d, data)
        if d % 6 == 3:
            body = body[:4000] + bytes([body[4000] ^ 2]) + body[4001:]       # a bad checksum
        pieces = R.cut(body, range(PIECE, k * PIECE, PIECE))
        frames = R.frag_frames(src, dst, 40000 + d, 6 if d % 5 == 4 else 17, pieces,
                               ihl=5 + d % 3)
        if d % 6 == 5:
            frames[2 * W - 1] = R.ETH[:9]                                    # a piece missing
        order = list(rng.permutation(k)) if d else list(range(k))
        slots = [(w, s) for w in range(W) for s in ((0, 1, 2) if d == 0 else (0, 2))]
        for (w, s), j in zip(slots, order):
            per[w][s].append(frames[int(j)])
    whole = R.whole_frames(rng, 4 * W)
    for w in range(W):
        per[w][0] += whole[4 * w:4 * w + 2]
        per[w][2] += whole[4 * w + 2:4 * w + 4]
        for s in (0, 2):
            per[w][s] = [per[w][s][int(j)] for j in rng.permutation(len(per[w][s]))]
    c = Case()
    lens, c.runs, c.windows, c.across, c.frames = [], [], [], [], {}
    at = 0
    for w, e in enumerate(edges):
        pre, (mid,), post = per[w]
        d = len(mid) - 1 if distance == "len-1" else distance
        assert 0 < d < len(mid)
        items = pre + [mid] + post
        ws = e - d - sum(len(f) for f in pre)
        assert ws >= at
        q, r = divmod(ws - at, L.FILL)
        lens += [L.FILL] * q + ([r] if r else [])
        c.runs.append((len(lens), len(items), w))
        c.across.append(len(lens) + len(pre))
        for j, f in enumerate(items):
            c.frames[len(lens) + j] = f
        data = np.frombuffer(b"".join(items), dtype=np.uint8).copy()
        c.windows.append(L.Window(shift + ws, data))
        lens += [len(f) for f in items]
        at = ws + data.size
    lens += [L.FILL] * 3
    c.offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(np.array(lens, dtype=np.uint64), out=c.offsets[1:])
    c.n, c.edges, c.shift = len(lens), edges, shift
    assert shift + int(c.offsets[-1]) <= L.ARENA_BYTES
    return c


def expected(oracle, c, filler_verdict):
    """The model's Expected for the whole batch: ipreass_cases.model on the windows' frames, its
    indices mapped to the batch's; the filler frames get `filler_verdict`, no chunk, no link."""
    idx = sorted(c.frames)
    local = R.model(oracle, R.Batch([c.frames[i] for i in idx]))
    g = np.array(idx, dtype=np.uint32)
    e = R.Expected()
    e.verdict = np.full(c.n, filler_verdict, dtype=np.uint8)
    e.chunk_off = np.full(c.n, -1, dtype=np.int64)
    e.chunk_len = np.zeros(c.n, dtype=np.uint32)
    e.next = np.full(c.n, R.NONE, dtype=np.uint32)
    e.head = np.full(c.n, R.NONE, dtype=np.uint32)
    e.dgram = np.zeros(c.n, dtype=R.DGRAM_DTYPE)
    to_global = lambda a: np.where(a == R.NONE, R.NONE, g[np.minimum(a, len(idx) - 1)]).astype(np.uint32)  # noqa: E731
    e.verdict[g], e.chunk_off[g], e.chunk_len[g] = local.verdict, local.chunk_off, local.chunk_len
    e.next[g], e.head[g] = to_global(local.next), to_global(local.head)
    dg = local.dgram.copy()
    heads = dg["n_frags"] != 0
    dg["last_frame"][heads] = g[dg["last_frame"][heads]]
    e.dgram[g] = dg
    e.complete = {k: [idx[i] for i in o] for k, o in local.complete.items()}
    e.local = local
    return e
