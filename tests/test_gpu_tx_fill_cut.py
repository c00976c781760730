"""The Tx fills on linear frames (tx_fill in one pass and split, tx_fill_records with
apply_tx_records, and their three ring-slot forms) on the inputs of tx_fill_cut_cases.py: the
receive sweep's frames at every length with both tails, and its 513-frame mixed batch in its plain
and inverted-surroundings layouts; each as built, with the checksum fields zeroed (before the
fill), and already filled. tx_store 1 and 2 rewrite whole 32-byte sectors and 128-byte lines from
the header bytes the kernel holds, so a wrong length or offset there corrupts a neighbour's bytes:
the whole buffer is compared byte for byte, guards, tails, slot rests and the shift in front
included, and the inverted layout must come back inverted outside the frames (it is part of the
expected buffer). Statuses, the records and the split workspace lie in guarded buffers; the records
are checked by applying them on the host, which must give the expected buffer and statuses.

Expectations: oracle.tx_fill_batch / tx_fill_slotted on a copy; none comes from a GPU call.
test_tx_fill_cut_cases.py shows on the CPU that every Tx status occurs and that both checksum
fields meet every position within a 32-byte sector."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import rx_cut_cases as X
import tx_fill_cut_cases as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON, GUARD = 0xC3, 64


def _tune(key, value):
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == A.AIPSTACK_CHKSUM_OK


@pytest.fixture
def tunables():
    """Yields the setter; restores the defaults of the three tunables used here afterwards."""
    yield _tune
    torch.cuda.synchronize()
    for k, v in (("tx_gather", -1), ("tx_store", -1), ("stream", 0)):
        _tune(k, v)


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


class Guarded:
    def __init__(self, nbytes, dtype=None):
        self.raw = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
        self.view = self.raw[GUARD:GUARD + nbytes]
        if dtype is not None:
            self.view = self.view.view(dtype)
        self.n = nbytes

    def intact(self):
        r = self.raw.cpu().numpy()
        return (r[:GUARD] == POISON).all() and (r[GUARD + self.n:] == POISON).all()


def _one(lay, host, want, want_st, shift, kind):
    """One call of `kind` on the layout's bytes `shift` bytes into a device buffer; everything the
    call leaves is compared."""
    n = len(lay.frames)
    full = torch.from_numpy(np.concatenate([np.full(shift, 0x3C, np.uint8), host])).to(DEV)
    first = shift + (X.GUARD if lay.slotted else 0)
    view = full[first:]
    status = Guarded(n)
    if lay.slotted:
        lens = torch.from_numpy(lay.lens.astype(np.int32)).to(DEV)
        view = view[:n * lay.stride]
        where, offs = (view, lay.stride, lens), X.GUARD + A.slots_to_offsets(n, lay.stride)
        fill, records = A.tx_fill_slotted, A.tx_fill_records_slotted
    else:
        where, offs = (view, torch.from_numpy(lay.offsets.astype(np.int64)).to(DEV)), lay.offsets
        fill, records = A.tx_fill, A.tx_fill_records
    if kind == "records":
        rec = Guarded(8 * n, torch.int64)
        records(*where, out=rec.view)
        after = full.cpu().numpy()[shift:]
        assert np.array_equal(after, host) and rec.intact()          # the read pass writes nothing
        got = host.copy()
        got_st = A.apply_tx_records(got, offs, rec.view.cpu().numpy())
    else:
        ws = Guarded(max(8 * n, 8))
        kw = dict(split=True, workspace=ws.view) if kind == "split" else dict(split=False)
        fill(*where, out=status.view, **kw)
        torch.cuda.synchronize()
        whole = full.cpu().numpy()
        assert (whole[:shift] == 0x3C).all() and ws.intact() and status.intact()
        got, got_st = whole[shift:], status.view.cpu().numpy()
    bad = np.flatnonzero(got_st != want_st)
    assert bad.size == 0, (kind, shift, bad[:8], got_st[bad[:8]], want_st[bad[:8]], lay.lens[bad[:8]])
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(np.searchsorted(lay.start, bad[0], side="right")) - 1
        raise AssertionError((kind, shift, bad.size, "byte", int(bad[0]), "frame", i, "at", int(bad[0] - lay.start[i]),
                              "len", int(lay.lens[i]), hex(int(got[bad[0]])), hex(int(want[bad[0]]))))


@pytest.mark.parametrize("store", [0, 1, 2])
@pytest.mark.parametrize("gather", [0, 1, 2])
@pytest.mark.parametrize("layout", list(T.LAYOUTS))
@pytest.mark.parametrize("name", T.STAGES)
def test_tx_fill_every_length(oracle, tunables, name, layout, gather, store):
    """Family A in all three variants at every shift of the layout; family C in all three variants
    and both layouts at two shifts; the one-pass fill at each shift, and the one-pass fill, the split
    fill and the records with the default stream mode and with stream -1."""
    tunables("tx_gather", gather)
    tunables("tx_store", store)
    runs = [("A", False, v) for v in T.VARIANTS] + [("C", alt, v) for alt in (False, True) for v in T.VARIANTS]
    for family, alt, variant in runs:
        lay, host, want, want_st = T.cached(oracle, name, family, layout, alt, variant)
        for shift in (T.SHIFTS[layout] if family == "A" else T.SHIFTS[layout][:2]):
            _one(lay, host, want, want_st, shift, "fill")
        for su in (0, -1):
            tunables("stream", su)
            for kind in ("fill", "split", "records"):
                _one(lay, host, want, want_st, T.SHIFTS[layout][1], kind)
        tunables("stream", 0)
