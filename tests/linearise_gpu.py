"""A linearise_cases.Scenario on the device, and the comparison every GPU linearise test makes:
every destination byte (the whole allocation, prefilled with the sentinel), every length, every
status, and every source buffer afterwards."""
import numpy as np
import torch

import aipstack_amd as A

import linearise_cases as LC

DEV = "cuda"


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pinned(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).pin_memory()


class Dev:
    def __init__(self, sc, pinned_bufs=(), pinned_dest=False):
        self.sc = sc
        self.headers = d(sc.headers)
        self.hdr_lens = d(sc.hdr_lens.view(np.int32))
        self.bufs = [pinned(b) if k in pinned_bufs else d(b) for k, b in enumerate(sc.bufs)]
        base = np.array([b.data_ptr() for b in self.bufs], dtype=np.uint64)
        self.addr = d((base[sc.chunk_buf] + sc.chunk_off.astype(np.uint64)).view(np.int64))
        self.len = d(sc.chunk_len.view(np.int32))
        self.index = d(sc.index.view(np.int64))
        self.seg_status = d(sc.seg_status) if sc.seg_status is not None else None
        self.offsets = d(sc.offsets.view(np.int64)) if sc.form == "csr" else None
        poison = np.full(max(sc.dest_bytes(), 1), LC.SENTINEL, dtype=np.uint8)
        self.dest = pinned(poison) if pinned_dest else d(poison)
        self.lens = torch.full((sc.n,), -1, dtype=torch.int32, device=DEV)
        self.status = torch.full((sc.n,), 0xFF, dtype=torch.uint8, device=DEV)

    def poison(self):
        self.dest.fill_(LC.SENTINEL)
        self.lens.fill_(-1)
        self.status.fill_(0xFF)

    def run(self, **kw):
        sc = self.sc
        args = dict(headers=self.headers, hdr_stride=sc.hdr_stride, hdr_lens=self.hdr_lens,
                    chunk_addr=self.addr, chunk_len=self.len, chunk_index=self.index,
                    seg_status=self.seg_status, frame_max=sc.frame_max, lens=self.lens,
                    status=self.status, **kw)
        if sc.form == "slots":
            return A.tx_linearise_slotted(self.dest, sc.slot_stride, **args)
        return A.tx_linearise(self.dest, self.offsets, **args)

    def compare(self, want=None):
        sc = self.sc
        torch.cuda.synchronize()
        dest, lens, status = want if want is not None else sc.expected()
        got_st = self.status.cpu().numpy()
        bad = np.nonzero(got_st != status)[0]
        assert bad.size == 0, (bad[:8], got_st[bad[:8]], status[bad[:8]],
                               [sc.tags[i] for i in bad[:8]])
        got_len = self.lens.cpu().numpy()
        bad = np.nonzero(got_len != lens)[0]
        assert bad.size == 0, (bad[:8], got_len[bad[:8]], lens[bad[:8]])
        got = self.dest.cpu().numpy()[:dest.size]
        bad = np.nonzero(got != dest)[0]
        if bad.size:
            at = int(bad[0])
            starts = np.array([sc.frame_start(i) for i in range(sc.n)])
            i = int(np.searchsorted(starts, at, side="right") - 1)
            raise AssertionError((f"{bad.size} bytes differ, first at {at}: frame {i} "
                                  f"(+{at - starts[i]}, L {lens[i]}, tag {sc.tags[i]})",
                                  got[at:at + 16], dest[at:at + 16]))
        assert np.array_equal(self.headers.cpu().numpy(), sc.headers)
        for b, h in zip(self.bufs, sc.bufs):
            assert np.array_equal(b.cpu().numpy(), h)
        return dest, lens, status


def check(sc, **kw):
    dev = Dev(sc, **{k: kw.pop(k) for k in ("pinned_bufs", "pinned_dest") if k in kw})
    dev.run(**kw)
    return dev, dev.compare()
