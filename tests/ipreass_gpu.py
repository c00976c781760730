"""TEST INFRASTRUCTURE -- the GPU harness test_gpu_ipreass.py, test_gpu_random_ipreass.py and
test_gpu_large_span_ipreass.py share: guarded outputs and workspace, the call, the byte-for-byte
comparison with the model of ipreass_cases.py."""
import numpy as np
import torch

import aipstack_amd as A

import ipreass_cases as R

DEV = "cuda"
GUARD = 256
GUARD_BYTE, POISON = 0xA7, 0xC3


class Guarded:
    """`nbytes` device bytes preset to POISON with guard bytes on both sides."""

    def __init__(self, nbytes):
        self.lo, self.hi = GUARD, GUARD + nbytes
        self.buf = torch.full((self.hi + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.view = self.buf[self.lo:self.hi]
        self.view.fill_(POISON)

    def intact(self):
        h = self.buf.cpu().numpy()
        return bool((h[:self.lo] == GUARD_BYTE).all() and (h[self.hi:] == GUARD_BYTE).all())


class Outputs:
    SIZES = (("verdict", 1), ("chunk_addr", 8), ("chunk_len", 4), ("next", 4), ("head", 4), ("dgram", 16))

    def __init__(self, n):
        self.n = n
        self.g = {k: Guarded(n * sz) for k, sz in self.SIZES}
        self.ws = Guarded(A.ip4_reass_workspace_bytes(n))

    def kw(self):
        v = {k: g.view for k, g in self.g.items()}
        return dict(verdict=v["verdict"], chunk_addr=v["chunk_addr"].view(torch.int64),
                    chunk_len=v["chunk_len"].view(torch.int32), next=v["next"].view(torch.int32),
                    head=v["head"].view(torch.int32), dgram=v["dgram"], workspace=self.ws.view)

    def poison(self):
        for g in list(self.g.values()) + [self.ws]:
            g.view.fill_(POISON)

    def bytes(self):
        return tuple(self.g[k].view.cpu().numpy().tobytes() for k, _ in self.SIZES)

    def intact(self):
        return all(g.intact() for g in self.g.values()) and self.ws.intact()


def expected_bytes(e, frame_addr):
    """The six outputs the model expects, as bytes; frame_addr[i] = device address of frame i."""
    addr = np.where(e.chunk_off >= 0, np.asarray(frame_addr, dtype=np.uint64) +
                    np.maximum(e.chunk_off, 0).astype(np.uint64), np.uint64(0)).astype(np.uint64)
    return (e.verdict.astype(np.uint8).tobytes(), addr.tobytes(), e.chunk_len.astype(np.uint32).tobytes(),
            e.next.astype(np.uint32).tobytes(), e.head.astype(np.uint32).tobytes(), e.dgram.tobytes())


def compare(e, out, frame_addr):
    want, got = expected_bytes(e, frame_addr), out.bytes()
    for (name, sz), w, g in zip(Outputs.SIZES, want, got):
        if w != g:
            wa = np.frombuffer(w, dtype=np.uint8).reshape(-1, sz)
            ga = np.frombuffer(g, dtype=np.uint8).reshape(-1, sz)
            bad = np.nonzero((wa != ga).any(axis=1))[0]
            raise AssertionError((name, bad[:8].tolist(), [ga[i].tobytes().hex() for i in bad[:4]],
                                  [wa[i].tobytes().hex() for i in bad[:4]]))
    assert out.intact()


def upload(batch):
    """(frames tensor of exactly the batch's bytes, offsets tensor, the frames' device addresses)."""
    dbuf = torch.from_numpy(batch.buf if batch.buf.size else np.zeros(1, dtype=np.uint8)).to(DEV)
    doff = torch.from_numpy(batch.offsets.view(np.int64)).to(DEV)
    return dbuf, doff, np.uint64(dbuf.data_ptr()) + batch.offsets[:-1]


def run(oracle, batch, max_reass=R.MAX_REASS, e=None):
    """The CSR call on the batch, compared with the model; (model, outputs, device tensors)."""
    e = R.model(oracle, batch, max_reass) if e is None else e
    dbuf, doff, addr = upload(batch)
    out = Outputs(batch.n)
    res = A.ip4_rx_reassemble(dbuf, doff, max_reass_size=max_reass, **out.kw())
    compare(e, out, addr)
    assert res.n == batch.n and np.array_equal(res.dgram_numpy(), e.dgram.view(A.IP4_DGRAM_DTYPE))
    return e, out, (dbuf, doff, addr)


def ring_of(batch, stride=2048):
    ring = np.full(batch.n * stride, 0x3C, dtype=np.uint8)
    lens = np.array([len(f) for f in batch.frames], dtype=np.uint32)
    assert int(lens.max()) <= stride
    for i, f in enumerate(batch.frames):
        ring[i * stride:i * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
    dring, dlens = torch.from_numpy(ring).to(DEV), torch.from_numpy(lens.view(np.int32)).to(DEV)
    addr = np.uint64(dring.data_ptr()) + np.arange(batch.n, dtype=np.uint64) * np.uint64(stride)
    return dring, dlens, addr
