"""aipstack_tx_linearise / aipstack_tx_linearise_slotted on the GPU against the model of
linearise_cases: every output byte of the whole destination allocation (prefilled with a
sentinel), every length, every status, and every source buffer afterwards."""
import numpy as np
import pytest

import aipstack_amd as A

import linearise_cases as LC
from linearise_cases import Seg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import linearise_gpu as G  # noqa: E402


def _tune(key, value):
    from aipstack_amd import _lib
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == A.AIPSTACK_CHKSUM_OK


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield


def test_every_source_and_destination_alignment():
    """One-chunk segments at source alignment 0-15 x destination alignment 0-15 x payload 0-80;
    a skipped filler segment before each one sets the destination alignment (its room must stay
    untouched)."""
    rng = np.random.default_rng(1)
    segs, at = [], 0
    for sa in range(16):
        for da in range(16):
            for p in range(81):
                r = (da - at) % 16
                segs.append(Seg(0, [], room=r, tag="fill"))
                segs.append(Seg(54, [p] if p else [], src_align=sa, tag=f"sa{sa} da{da} p{p}"))
                at += r + 54 + p
    sc = LC.build(segs, rng, form="csr", frame_max=1514, max_gap=3)
    assert sc.n == 2 * 16 * 16 * 81
    _, (_, _, status) = G.check(sc)
    assert (status == LC.WRITTEN).sum() == 16 * 16 * 81


SEAM_H = [14, 15, 16, 17, 34, 42, 54, 63, 64, 255, 256]
SEAM_L = [0, 1, 2, 15, 16, 17, 31, 33, 63, 64, 65]


def _seam_segs(rng):
    segs = []
    for H in SEAM_H:
        for a in SEAM_L:
            segs.append(Seg(H, [a], tag=f"H{H} [{a}]"))
            for b in SEAM_L:
                segs.append(Seg(H, [a, b], tag=f"H{H} [{a},{b}]"))
                c = SEAM_L[int(rng.integers(0, len(SEAM_L)))]
                segs.append(Seg(H, [a, b, c], tag=f"H{H} [{a},{b},{c}]"))
        segs.append(Seg(H, [1] * 300, tag=f"H{H} 300x1"))
        segs.append(Seg(H, [int(x) for x in rng.integers(0, 4, 70)], tag=f"H{H} 70 mixed"))
        segs.append(Seg(H, [int(x) for x in rng.integers(1, 34, 70)], tag=f"H{H} 70 longer"))
    return segs


@pytest.mark.parametrize("form", ["slots", "csr"])
def test_seams(form):
    rng = np.random.default_rng(2)
    sc = LC.build(_seam_segs(rng), rng, form=form, frame_max=4096, slot_stride=4100,
                  hdr_stride=256)
    _, (_, _, status) = G.check(sc)
    assert (status == LC.WRITTEN).all()


@pytest.mark.parametrize("frame_max,slot_stride", [(1514, 1514), (1514, 2048), (65535, 65535),
                                                   (65535, 65536)])
def test_limits_slotted(frame_max, slot_stride):
    rng = np.random.default_rng(3)
    segs = [Seg(13, [], tag="L13"), Seg(14, [], tag="L14"), Seg(10, [3], tag="L13"),
            Seg(10, [4], tag="L14"),
            Seg(54, [frame_max - 54], tag="Lmax"), Seg(54, [frame_max - 53], tag="Lmax+1"),
            Seg(54, [100, frame_max - 154], tag="Lmax"), Seg(54, [100, frame_max - 153], tag="Lmax+1"),
            Seg(54, [frame_max - 54], tag="Lmax")]   # the last frame ends where the ring does
    sc = LC.build(segs, rng, form="slots", frame_max=frame_max, slot_stride=slot_stride)
    _, (_, lens, status) = G.check(sc)
    assert list(status) == [LC.TOO_SHORT, LC.WRITTEN, LC.TOO_SHORT, LC.WRITTEN, LC.WRITTEN,
                            LC.TOO_LARGE, LC.WRITTEN, LC.TOO_LARGE, LC.WRITTEN]
    assert lens[4] == frame_max and lens[-1] == frame_max


@pytest.mark.parametrize("frame_max", [1514, 65535])
def test_limits_offsets_and_wrong_room(frame_max):
    rng = np.random.default_rng(4)
    segs = [Seg(54, [frame_max - 54], tag="Lmax"), Seg(54, [500], tag="ok"),
            Seg(54, [300], room=353, tag="room-1"), Seg(54, [500], tag="ok"),
            Seg(54, [300], room=355, tag="room+1"), Seg(54, [frame_max - 53], room=7, tag="Lmax+1"),
            Seg(14, [], tag="L14"), Seg(13, [], room=13, tag="L13"), Seg(54, [300], room=0, tag="room0"),
            Seg(54, [frame_max - 54], tag="Lmax")]   # ends at the allocation's last byte
    sc = LC.build(segs, rng, form="csr", frame_max=frame_max)
    _, (_, _, status) = G.check(sc)
    assert list(status) == [LC.WRITTEN, LC.WRITTEN, LC.WRONG_ROOM, LC.WRITTEN, LC.WRONG_ROOM,
                            LC.TOO_LARGE, LC.WRITTEN, LC.TOO_SHORT, LC.WRONG_ROOM, LC.WRITTEN]


@pytest.mark.parametrize("form", ["slots", "csr"])
def test_skips_between_written_frames(form):
    rng = np.random.default_rng(5)
    segs = []
    for k in range(120):
        segs.append(Seg(54, [int(rng.integers(0, 1461))], tag="ok"))
        segs.append([Seg(0, [50], tag="hdr0"), Seg(54, [50], LC.BURST_INVALID, tag="st10"),
                     Seg(42, [50], LC.DGRAM_INVALID, tag="st13"),
                     Seg(54, [50], LC.SPLIT_LAYOUT, tag="st9")][k % 4])
    sc = LC.build(segs, rng, form=form)
    _, (_, _, status) = G.check(sc)
    for first, want in ((1, LC.SKIPPED), (3, LC.SKIPPED), (5, LC.SKIPPED), (7, LC.WRITTEN)):
        assert (status[first::8] == want).all()
    assert (status[0::2] == LC.WRITTEN).all()
    # without d_seg_status only the empty headers are skipped
    sc2 = LC.build(segs, np.random.default_rng(5), form=form, with_status=False)
    _, (_, _, status2) = G.check(sc2)
    assert (status2 == LC.SKIPPED).sum() == 30


def test_invalid_segments_and_the_sticky_chunk_len_bit():
    rng = np.random.default_rng(6)
    segs = [Seg(54, [100], tag="ok"), Seg(65, [100], tag="H>stride"), Seg(54, [], tag="decr"),
            Seg(54, [100], tag="ok"), Seg(54, [3, 70000], tag="chunk>65535"), Seg(54, [7], tag="ok")]
    sc = LC.build(segs, rng, form="slots", decreasing=[2])
    A.contract_violations(clear=True)
    _, (_, _, status) = G.check(sc)
    assert status[1] == status[2] == status[4] == LC.INVALID
    assert A.contract_violations(clear=True) & A.VIOLATION_CHUNK_LEN


@pytest.mark.parametrize("aux", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000, 1537])
def test_counts(n, aux):
    rng = np.random.default_rng(100 + n)
    frame_max = 1514 if n != 257 else 200      # 8 and 61 segments per wave
    segs = LC._tcp_segs(rng, n, frame_max)
    sc = LC.build(segs, rng, form="csr" if n % 2 else "slots", frame_max=frame_max)
    _tune("aux_blocks", aux)
    try:
        G.check(sc)
    finally:
        _tune("aux_blocks", -1)


def test_just_written_reads_the_same():
    sc = LC.scenario(2)
    dev = G.Dev(sc)
    dev.run(just_written=True)
    dev.compare()


def test_pinned_host_source_and_destination():
    """A source buffer, and separately the destination ring, in pinned host memory; sources
    spread over separate allocations, each ending at its last chunk's last byte."""
    rng = np.random.default_rng(7)
    segs = LC._tcp_segs(rng, 200, 1514) + [Seg(54, [16], tag="tail")]
    sc = LC.build(segs, rng, form="slots", n_bufs=4, max_gap=0)
    G.check(sc, pinned_bufs=(1,))
    G.check(sc, pinned_dest=True)
    sc = LC.build(segs, np.random.default_rng(8), form="csr", n_bufs=4)
    G.check(sc, pinned_dest=True, pinned_bufs=(0, 3))


def test_graph_replay_on_changed_bytes():
    sc = LC.scenario(0)
    dev = G.Dev(sc)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev.run(stream=s)              # warm up outside the capture
    s.synchronize()
    dev.poison()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        dev.run(stream=torch.cuda.current_stream())
    rng = np.random.default_rng(9)
    for _ in range(2):
        sc.headers = rng.integers(0, 256, sc.headers.size, dtype=np.uint8)
        sc.bufs = [rng.integers(0, 256, b.size, dtype=np.uint8) for b in sc.bufs]
        dev.headers.copy_(G.d(sc.headers))
        for t, b in zip(dev.bufs, sc.bufs):
            t.copy_(G.d(b))
        dev.poison()
        torch.cuda.synchronize()
        g.replay()
        dev.compare()
