"""IPv4 reassembly on receive (aipstack_ip4_rx_reassemble / _slotted) on the GPU against the
declarative model of ipreass_cases.py (Rx verify by the frame oracle; group, sort, test; the
checksum over the linearised payload in plain Python).

Every test compares all six outputs byte for byte, with guard bytes around each of them and around
the workspace; the frames lie in an allocation of exactly their bytes."""
import numpy as np
import pytest

import aipstack_amd as A
from aipstack_amd import _lib

import ipreass_cases as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ipreass_gpu as H  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield
    assert A.contract_violations(clear=True) == 0


_cache = {}


def _once(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


# ---- round trips: what the project sends is what it receives --------------------------------

def test_round_trip_of_the_senders_trains(oracle):
    frames, cases = _once("round_trip", lambda: R.round_trip_batch(oracle))
    batch = R.Batch(frames)
    assert 300 <= batch.n <= 900 and max(len(f) for f in frames) == 1514
    e, _, _ = H.run(oracle, batch)
    multi = [c for c in cases if len(R.F.ip_packets_of(c)) > 1]
    assert len(e.complete) == len(multi) >= 40                   # every train is reassembled
    assert all(e.dgram[o[0]]["verdict"] == R.ACCEPT for o in e.complete.values())
    assert {6, 7, 8, 14}.issubset(set(e.verdict.tolist())) and (e.verdict <= 2).any()


def test_largest_datagrams(oracle):
    """65,515 bytes in 45 fragments (mtu 1500); 1,000 eight-byte fragments; P = 65,535, whose last
    fragment is past max_reass_size: left to the host, that fragment dropped."""
    big, over, tiny = _once("big", lambda: R.big_datagrams(oracle))
    rng = np.random.default_rng(2)
    frames = big + over + tiny
    batch = R.Batch([frames[int(p)] for p in rng.permutation(len(frames))])
    e, _, _ = H.run(oracle, batch)
    got = sorted((int(e.dgram[o[0]]["n_frags"]), int(e.dgram[o[0]]["data_len"]),
                  int(e.dgram[o[0]]["verdict"])) for o in e.complete.values())
    assert got == [(45, 65515, R.ACCEPT), (1000, 7998, R.ACCEPT)]
    assert (e.verdict == R.DROP_FRAG).sum() == 1 and (e.verdict == R.FRAGMENT).sum() == len(over) - 1


# ---- every branch, one crafted group each ---------------------------------------------------

def test_every_branch_in_one_batch(oracle):
    groups = _once("crafted", R.crafted)
    rng = np.random.default_rng(4)
    frames = [f for _, fr, _ in groups for f in fr]
    batch = R.Batch([frames[int(p)] for p in rng.permutation(len(frames))])
    e, _, _ = H.run(oracle, batch)
    verdicts = {int(e.dgram[o[0]]["verdict"]) for o in e.complete.values()}
    assert verdicts == {R.ACCEPT, R.NO_CHKSUM, R.OTHER, R.L4_MALFORMED, R.L4_CHKSUM, R.TRUNCATED}
    assert len(e.complete) == sum(w is not None for *_, w in groups)


@pytest.mark.parametrize("name", [g[0] for g in R.crafted()])
def test_each_branch_alone(oracle, name):
    frames, what = next((fr, w) for nm, fr, w in _once("crafted", R.crafted) if nm == name)
    batch = R.Batch(frames)
    e, _, _ = H.run(oracle, batch)
    heads = np.nonzero(e.dgram["n_frags"])[0]
    assert (int(e.dgram[heads[0]]["verdict"]) if heads.size else None) == what


@pytest.mark.parametrize("name", [g[0] for g in R.crafted_small_max()])
def test_offset_and_length_on_both_sides_of_max_reass_size(oracle, name):
    frames, what = next((fr, w) for nm, fr, w in R.crafted_small_max() if nm == name)
    e, _, _ = H.run(oracle, R.Batch(frames), R.SMALL_MAX)
    assert bool(e.complete) == (what is not None)
    if what is None:
        assert (e.verdict == R.DROP_FRAG).sum() == 1
    # the same frames under the largest size are one datagram (but for a hole)
    e2, _, _ = H.run(oracle, R.Batch(frames))
    assert bool(e2.complete) == (name != "off_past_max")


def test_fragments_at_every_byte_alignment(oracle):
    batch = R.Batch(R.alignment_batch())
    e, _, (dbuf, _, addr) = H.run(oracle, batch)
    assert len(e.complete) == 16
    starts = {int(addr[i] + np.uint64(e.chunk_off[i])) % 16 for i in e.frags}
    assert starts == set(range(16))


# ---- collisions -------------------------------------------------------------------------------

def test_keys_that_share_a_home_slot(oracle):
    frames, keys, want = _once("collide", R.colliding_batch)
    assert len(keys) >= 64
    batch = R.Batch(frames)
    e, _, _ = H.run(oracle, batch)
    assert len(e.complete) == len(keys) + 1
    rng = np.random.default_rng(9)
    H.run(oracle, batch.permuted(rng.permutation(batch.n)))


# ---- grid-stride ---------------------------------------------------------------------------------

def _tune(key, value):
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == A.AIPSTACK_CHKSUM_OK


def _multipass(oracle, n):
    def make():
        rng = np.random.default_rng(n)
        frames = [f for _, fr, _ in R.crafted() if len(fr) < 8 for f in fr]
        frames += [f for f in R.round_trip_batch(oracle, seed=n)[0]]
        frames = frames[:n - 40] if len(frames) > n - 40 else frames
        j = 0
        while len(frames) < n:
            body = R.udp_body(R.A_ + 9, R.B_, 1, 2, bytes([j & 0xFF]) * (17 + j % 50))
            frames += R.frag_frames(R.A_ + 9, R.B_, 30000 + j, 17, R.cut(body, [8, 16]))[:n - len(frames)]
            j += 1
        batch = R.Batch([frames[int(p)] for p in rng.permutation(n)])
        return batch, R.model(oracle, batch)
    return _once(f"multipass{n}", make)


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("n", [257, 1000, 1537])
def test_later_iterations_of_the_passes(oracle, n, cap):
    """At most `cap` blocks ("aux_blocks"): every lane pass loops; CSR frames and ring slots."""
    batch, e = _multipass(oracle, n)
    assert batch.n == n and len(e.complete) >= 20 and (e.verdict == R.FRAGMENT).any()
    late = [o for o in e.complete.values() if min(o) >= 256 * cap]
    assert late or n == 257
    dring, dlens, raddr = H.ring_of(batch)
    got = {}
    for c in (cap, -1):
        _tune("aux_blocks", c)
        try:
            _, out, _ = H.run(oracle, batch, e=e)
            slot = H.Outputs(n)
            A.ip4_rx_reassemble_slotted(dring, 2048, dlens, **slot.kw())
            H.compare(e, slot, raddr)
        finally:
            _tune("aux_blocks", -1)
        got[c] = (out.bytes(), slot.bytes())
    # the ring: the same bytes under either grid; the packed frames were uploaded anew, so all but
    # their addresses (output 1) are the same, and the same as the ring's
    assert got[cap][1] == got[-1][1]
    for x in (got[cap][0], got[-1][0]):
        assert x[0] == got[cap][1][0] and x[2:] == got[cap][1][2:]


# ---- determinism -----------------------------------------------------------------------------------

def test_twice_the_same_and_permuted_the_same_datagrams(oracle):
    batch, e = _multipass(oracle, 1000)
    _, out, (dbuf, doff, addr) = H.run(oracle, batch, e=e)
    first = out.bytes()
    out.poison()
    A.ip4_rx_reassemble(dbuf, doff, **out.kw())
    assert out.bytes() == first
    H.compare(e, out, addr)
    perm = np.random.default_rng(11).permutation(batch.n)
    pb = batch.permuted(perm)
    pe, _, _ = H.run(oracle, pb)
    assert set(pe.complete) == set(e.complete)
    for key, order in e.complete.items():
        assert [int(perm[i]) for i in pe.complete[key]] == order
        a, b = e.dgram[order[0]], pe.dgram[pe.complete[key][0]]
        assert (a["n_frags"], a["data_len"], a["verdict"]) == (b["n_frags"], b["data_len"], b["verdict"])
        assert int(perm[int(b["last_frame"])]) == int(a["last_frame"])


def test_captured_into_a_graph_and_replayed_on_changed_frames(oracle):
    batch, e = _multipass(oracle, 1000)
    dbuf, doff, addr = H.upload(batch)
    out = H.Outputs(batch.n)
    A.ip4_rx_reassemble(dbuf, doff, **out.kw())   # warm-up outside the capture (the CU count is cached)
    torch.cuda.synchronize()
    H.compare(e, out, addr)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        A.ip4_rx_reassemble(dbuf, doff, **out.kw())
    out.poison()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    H.compare(e, out, addr)
    # the same layout, other bytes: a payload byte of a complete datagram's middle fragment and a
    # header byte (the ident) of another one's change under the graph
    orders = [o for o in e.complete.values() if len(o) >= 3 and e.frags[o[0]]["proto"] in (1, 6, 17)
              and e.dgram[o[0]]["verdict"] == R.ACCEPT]
    frames = list(batch.frames)
    i = orders[0][1]
    f = bytearray(frames[i]); f[e.frags[i]["poff"]] ^= 0x20; frames[i] = bytes(f)
    i = orders[1][1]
    f = bytearray(frames[i]); f[19] ^= 0x01; f[24:26] = b"\0\0"
    f[24:26] = (~R.wsum(bytes(f[14:14 + 4 * (f[14] & 15)])) & 0xFFFF).to_bytes(2, "big"); frames[i] = bytes(f)
    changed = R.Batch(frames)
    assert np.array_equal(changed.offsets, batch.offsets)
    ce = R.model(oracle, changed)
    assert len(ce.complete) < len(e.complete) and e.frags[i]["key"] not in ce.complete
    assert ce.dgram[orders[0][0]]["verdict"] == R.L4_CHKSUM
    dbuf.copy_(torch.from_numpy(changed.buf))
    out.poison()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    H.compare(ce, out, addr)


# ---- ring slots ---------------------------------------------------------------------------------------

def test_slotted_form_on_a_2k_ring(oracle):
    groups = [g for g in _once("crafted", R.crafted) if all(len(f) <= 2048 for f in g[1])]
    frames = [f for _, fr, _ in groups for f in fr] + R.alignment_batch()
    rng = np.random.default_rng(12)
    batch = R.Batch([frames[int(p)] for p in rng.permutation(len(frames))])
    e = R.model(oracle, batch)
    assert len(e.complete) >= 30 and (e.verdict == R.FRAGMENT).any() and (e.verdict == R.DROP_FRAG).any()
    dring, dlens, raddr = H.ring_of(batch)
    slot = H.Outputs(batch.n)
    res = A.ip4_rx_reassemble_slotted(dring, 2048, dlens, **slot.kw())
    H.compare(e, slot, raddr)
    assert res.n == batch.n
