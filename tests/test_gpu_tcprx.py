"""TCP Rx parse (aipstack_tcp_rx_parse / _slotted) on the GPU against the model of tcprx_cases.py
(the reference's recvIp4Dgram steps restated in Python; the option parser and the key order
pinned by answers recorded from the reference's own code; verdicts from the frame oracle).

Every test compares, byte for byte, the verdicts, the 32-byte records and the cookies, with guard
bytes before and after each of the three outputs."""
import struct

import numpy as np
import pytest

import aipstack_amd as A

import frame_cases as F
import tcp_rx_ref as R
import tcprx_cases as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256
GUARD_BYTE, POISON = 0xA7, 0xC3


@pytest.fixture(scope="module", autouse=True)
def _violations_cleared_first():
    A.contract_violations(clear=True)
    yield


_cache = {}


def _set(oracle, name):
    """(frames, Rx verify verdicts by the oracle): computed once, shared."""
    if name not in _cache:
        if name == "geometry":
            v = T.fill(oracle, T.geometry_frames())
        elif name == "padding":
            v = T.fill(oracle, T.padding_frames())
        elif name == "bad_offsets":
            v = T.fill(oracle, [f for f, _ in T.bad_offset_frames()])
        elif name == "options":
            v = T.fill(oracle, T.option_frames(R.load()[0]))
        elif name == "mixed":
            fr = T.mixed_frames()
            buf, off = F.pack(fr)
            v = (fr, oracle.rx_verify_batch(buf, off))
        _cache[name] = v
    return _cache[name]


def _table_for(frames, verdicts, every=3, extra=()):
    """A sorted table holding every `every`-th accepted TCP frame's tuple (cookie = 7 + rank)."""
    ks = [T.key_of(f) for f, v in zip(frames, verdicts) if v == T.ACCEPT and f[23] == 6][::every]
    ks = list(dict.fromkeys(ks + list(extra)))
    return A.tcp_pcb_table_sort(T.table([k + (7 + i,) for i, k in enumerate(ks)], A.TCP_PCB_KEY_DTYPE))


class Guarded:
    """`nbytes` device bytes preset to POISON with guard bytes on both sides; `shift` moves the
    start off its 256-byte boundary."""

    def __init__(self, nbytes, shift=0):
        self.lo, self.hi = GUARD + shift, GUARD + shift + nbytes
        self.buf = torch.full((self.hi + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.view = self.buf[self.lo:self.hi]
        self.view.fill_(POISON)

    def intact(self):
        h = self.buf.cpu().numpy()
        return (h[:self.lo] == GUARD_BYTE).all() and (h[self.hi:] == GUARD_BYTE).all()


class Outputs:
    def __init__(self, n, seg_shift=0):
        self.verdict, self.segs, self.pcb = Guarded(n), Guarded(n * 32, seg_shift), Guarded(n * 4)

    def kw(self):
        return dict(verdict=self.verdict.view, segs=self.segs.view, pcb=self.pcb.view.view(torch.int32))

    def poison(self):
        for g in (self.verdict, self.segs, self.pcb):
            g.view.fill_(POISON)

    def bytes(self):
        return tuple(g.view.cpu().numpy().tobytes() for g in (self.verdict, self.segs, self.pcb))


def _compare(e, out):
    v, s, p = out.bytes()
    v = np.frombuffer(v, dtype=np.uint8)
    bad = np.nonzero(v != e.verdict)[0]
    assert bad.size == 0, (bad[:8], v[bad[:8]], e.verdict[bad[:8]])
    got = np.frombuffer(s, dtype=A.TCP_RX_SEG_DTYPE)
    rows = [i for i in range(len(got)) if got[i].tobytes() != e.segs[i].tobytes()]
    assert not rows, (rows[:8], got[rows[0]], e.segs[rows[0]])
    pc = np.frombuffer(p, dtype=np.uint32)
    bad = np.nonzero(pc != e.pcb)[0]
    assert bad.size == 0, (bad[:8], pc[bad[:8]], e.pcb[bad[:8]])
    for g in (out.verdict, out.segs, out.pcb):
        assert g.intact()


def _run_csr(frames, verdicts, tbl, *, lead=0, seg_shift=0):
    """The CSR call on `frames` packed back to back after `lead` bytes; compared with the model."""
    e = T.expected(frames, verdicts, tbl, A.TCP_RX_SEG_DTYPE)
    buf, off = F.pack(frames)
    dbuf = torch.from_numpy(np.concatenate([np.full(lead, 0x99, dtype=np.uint8), buf])).to(DEV)
    doff = torch.from_numpy((off + np.uint64(lead)).view(np.int64)).to(DEV)
    out = Outputs(len(frames), seg_shift)
    res = A.tcp_rx_parse(dbuf, doff, tbl, **out.kw())
    _compare(e, out)
    assert res.n == len(frames) and np.array_equal(res.segs_numpy(), e.segs)
    return e, out, (dbuf, doff)


# ---- wave edges, alignment ---------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_wave_edges(oracle, n):
    frames, v = _set(oracle, "mixed")
    frames, v = frames[:n], v[:n]
    tbl = _table_for(frames, v, every=2)
    e, _, _ = _run_csr(frames, v, tbl)
    if n >= 63:
        assert (e.pcb != T.NO_PCB).any() and (e.segs["opts"] == 0).any() and (e.segs["opts"] != 0).any()


@pytest.mark.parametrize("lead", range(16))
def test_frame_start_alignment(oracle, lead):
    """Frames starting at every byte offset (the lengths vary, so every alignment mod 16 occurs
    within each run as well); the records at an address that is 8 but not 16 bytes aligned for
    odd `lead`."""
    g, gv = _set(oracle, "geometry")
    o, ov = _set(oracle, "options")
    frames = g[lead::16] + o[lead:200:16] + [g[-1]]
    v = np.concatenate([gv[lead::16], ov[lead:200:16], gv[-1:]])
    starts = np.cumsum([lead] + [len(f) for f in frames[:-1]]) % 16
    assert starts[0] == lead and len(set(starts.tolist())) >= 6
    _run_csr(frames, v, _table_for(frames, v), lead=lead, seg_shift=8 * (lead & 1))


# ---- header geometry, padding, bad offsets, options --------------------------------------------

def test_header_geometry(oracle):
    frames, v = _set(oracle, "geometry")
    assert (v == T.ACCEPT).all() and len(frames) == 11 * 11 * 3
    e, _, _ = _run_csr(frames, v, _table_for(frames, v))
    s = e.segs
    assert int(s["data_off"].max()) == 134 and int(s["data_off"].min()) == 54
    assert set(s["data_len"].tolist()) == {0, 1, 1460}
    last = frames[-1]                       # IHL 15, offset 15: the MSS option ends at byte 133
    assert last[14] & 0xF == 15 and last[130:134] == struct.pack(">BBH", 2, 4, 500 + 15 * 16 + 15)
    assert s["mss"][-1] == 500 + 15 * 16 + 15
    assert (s["opts"] == (T.SEG_VALID | T.OPT_MSS)).sum() == 11 * 10 * 3


def test_padding_is_not_data(oracle):
    frames, v = _set(oracle, "padding")
    assert (v == T.ACCEPT).all()
    e, _, _ = _run_csr(frames, v, _table_for(frames, v))
    assert len(frames[0]) == 60 and e.segs["data_len"][0] == 0 and e.segs["data_off"][0] == 54
    for f, r in zip(frames, e.segs):
        total, = struct.unpack_from(">H", f, 16)
        assert r["data_off"] + r["data_len"] == 14 + total <= len(f)
    assert sum(1 for f, r in zip(frames, e.segs) if r["data_off"] + r["data_len"] < len(f)) >= 30


def test_bad_data_offsets(oracle):
    frames, v = _set(oracle, "bad_offsets")
    valid = np.array([ok for _, ok in T.bad_offset_frames()])
    assert (v == T.ACCEPT).all()             # the TCP checksum is good in every one of them
    e, _, _ = _run_csr(frames, v, _table_for(frames, v, every=1))
    assert (e.verdict[~valid] == A.AIPSTACK_RX_DROP_TCP_OFFSET).all() and (~valid).sum() == 30
    assert not e.segs[~valid].tobytes().strip(b"\0") and (e.pcb[~valid] == A.AIPSTACK_TCP_NO_PCB).all()
    assert (e.verdict[valid] == T.ACCEPT).all() and (e.segs["data_len"][valid] == 0).all()
    assert (e.pcb[valid] != A.AIPSTACK_TCP_NO_PCB).all() and valid.sum() == 20


def test_every_option_buffer_of_the_fixture(oracle):
    frames, v = _set(oracle, "options")
    cases = R.load()[0]
    assert (v == T.ACCEPT).all() and len(frames) == len(cases) > 2000
    e, _, _ = _run_csr(frames, v, _table_for(frames, v, every=5))
    # the model's answers for the frames are the reference's recorded ones for the buffers
    want = np.array([(fl | T.SEG_VALID, mss, ws) for _, fl, mss, ws in cases])
    assert np.array_equal(e.segs["opts"], want[:, 0]) and np.array_equal(e.segs["mss"], want[:, 1])
    assert np.array_equal(e.segs["wnd_scale"], want[:, 2])


# ---- every other verdict class -----------------------------------------------------------------

def test_other_verdict_classes(oracle):
    frames, v = _set(oracle, "mixed")
    assert set(v.tolist()) == set(range(9))
    tbl = _table_for(frames, v, every=2)
    e, out, (dbuf, doff) = _run_csr(frames, v, tbl)
    assert np.array_equal(A.rx_verify(dbuf, doff).cpu().numpy(), e.verdict)   # no bad offset here
    tcp_ok = np.array([x == T.ACCEPT and f[23] == 6 for f, x in zip(frames, v)])
    assert tcp_ok.sum() >= 100 and (~tcp_ok).sum() >= 300
    assert (e.segs["opts"][tcp_ok] & T.SEG_VALID).all()
    assert not e.segs[~tcp_ok].tobytes().strip(b"\0") and (e.pcb[~tcp_ok] == T.NO_PCB).all()
    assert ((v == T.ACCEPT) & ~tcp_ok).sum() >= 50          # accepted UDP / ICMP frames: no record


# ---- PCB tables --------------------------------------------------------------------------------

def _lookup_frames(oracle, keys):
    fr = [T.tcp_frame(dst=la, src=ra, dport=lp, sport=rp, seq=i) for i, (la, ra, lp, rp) in enumerate(keys)]
    return T.fill(oracle, fr)


def _spread_keys(n):
    """n distinct keys whose order is decided by every field somewhere."""
    return [(T.LOCAL_IP + (i * 7) % 3, T.PEER_IP + (i * 5) % 11, 80 + (i * 3) % 5, 1024 + i // 4)
            for i in range(n)]


@pytest.mark.parametrize("size", [0, 1, 2, 3, 1000, 4097])
def test_tables(oracle, size):
    keys = _spread_keys(size)
    assert len(set(keys)) == size
    tbl = A.tcp_pcb_table_sort(T.table([k + (1000 + i,) for i, k in enumerate(keys)],
                                       A.TCP_PCB_KEY_DTYPE)) if size else None
    probes = []
    if size:
        st = [tuple(int(tbl[f][j]) for f in ("local_addr", "remote_addr", "local_port", "remote_port"))
              for j in range(size)]
        first, last = st[0], st[-1]
        probes += [first, last, st[size // 2]]                        # hits: first, last, middle
        probes += [(first[0], first[1], first[2], first[3] - 1),      # misses: below, above
                   (last[0], last[1], last[2], last[3] + 1)]
        for k in (first, last, st[size // 2]):                        # one field off, each field
            for f in range(4):
                for d in (1, -1):
                    q = list(k)
                    q[f] += d
                    probes.append(tuple(q))
            probes.append((k[1], k[0], k[3], k[2]))                   # local and remote swapped
        if size > 3:
            probes += st[1:size:max(1, size // 40)]
            a, b = st[size // 3], st[size // 3 + 1]                   # a miss between two entries
            mid = (a[0], a[1], a[2] + 1000, a[3])
            probes.append(mid)
    else:
        probes = _spread_keys(5)
    frames, v = _lookup_frames(oracle, probes)
    assert (v == T.ACCEPT).all()
    e, _, _ = _run_csr(frames, v, tbl)
    hits = e.pcb != T.NO_PCB
    if size:
        in_tbl = np.array([p in set(st) for p in probes])
        assert np.array_equal(hits, in_tbl) and hits[:3].all() and not hits[3:5].any()
        assert e.pcb[0] == tbl["cookie"][0] and e.pcb[1] == tbl["cookie"][-1]
        swapped = [i for i, p in enumerate(probes) if (p[1], p[0], p[3], p[2]) in set(st) and p not in set(st)]
        assert swapped and not hits[swapped].any()
        assert (~hits).sum() >= 10
    else:
        assert not hits.any()


def test_device_table_and_empty_device_table(oracle):
    frames, v = _set(oracle, "padding")
    tbl = _table_for(frames, v, every=2)
    e = T.expected(frames, v, tbl, A.TCP_RX_SEG_DTYPE)
    buf, off = F.pack(frames)
    dbuf, doff = torch.from_numpy(buf).to(DEV), torch.from_numpy(off.view(np.int64)).to(DEV)
    dt = torch.from_numpy(tbl.view(np.uint8).copy()).to(DEV)
    out = Outputs(len(frames))
    A.tcp_rx_parse(dbuf, doff, dt, **out.kw())
    _compare(e, out)
    out.poison()
    A.tcp_rx_parse(dbuf, doff, dt[:0], **out.kw())
    _compare(T.expected(frames, v, None, A.TCP_RX_SEG_DTYPE), out)


# ---- the slotted form --------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [192, 2048])
def test_slotted_equals_csr(oracle, stride):
    g, gv = _set(oracle, "geometry")
    m, mv = _set(oracle, "mixed")
    b, bv = _set(oracle, "bad_offsets")
    frames = [f for f in g[::5] + m[:200] + b if len(f) <= stride]
    assert len(frames) > 100
    ring = np.full(len(frames) * stride, 0x3C, dtype=np.uint8)
    lens = np.zeros(len(frames), dtype=np.uint32)
    for i, f in enumerate(frames):
        ring[i * stride:i * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
        lens[i] = len(f)
    # a length above the stride is clamped to it, as verify clamps it: the frame is the slot
    # (a long frame with trailing bytes up to the slot's end, here the filler bytes)
    big = [i for i, f in enumerate(frames) if len(f) >= 54 and f[23] == 6][:3]
    for i in big:
        lens[i] = stride + 1 + i
    seen = [ring[i * stride:i * stride + min(int(lens[i]), stride)].tobytes() for i in range(len(frames))]
    v = oracle.rx_verify_slotted(ring, stride, lens)
    tbl = _table_for(seen, v, every=2)
    e = T.expected(seen, v, tbl, A.TCP_RX_SEG_DTYPE)
    assert (e.verdict == A.AIPSTACK_RX_DROP_TCP_OFFSET).sum() >= 10 and (e.pcb != T.NO_PCB).sum() >= 20
    dring = torch.from_numpy(ring).to(DEV)
    dlens = torch.from_numpy(lens.view(np.int32)).to(DEV)
    out = Outputs(len(frames))
    A.tcp_rx_parse_slotted(dring, stride, dlens, tbl, **out.kw())
    _compare(e, out)
    # and the CSR form on the same frames gives the same bytes
    buf, off = F.pack(seen)
    out2 = Outputs(len(frames))
    A.tcp_rx_parse(torch.from_numpy(buf).to(DEV), torch.from_numpy(off.view(np.int64)).to(DEV), tbl,
                   **out2.kw())
    assert out.bytes() == out2.bytes()
    A.contract_violations(clear=True)        # the lengths above the stride were reported


# ---- later iterations of the grid-stride loop --------------------------------------------------

def _tune(key, value):
    from aipstack_amd import _lib
    assert _lib.load().aipstack_chksum_tune(key.encode(), value) == A.AIPSTACK_CHKSUM_OK


def _multipass_set(oracle, n):
    """n frames: mixed_frames (every verdict class) with the bad_offsets set from frame 800 on
    (or at the end of a short batch); their verdicts, a table, the expectation. Computed once."""
    name = f"multipass{n}"
    if name not in _cache:
        b, bv = _set(oracle, "bad_offsets")
        m = T.mixed_frames(n - len(b))
        buf, off = F.pack(m)
        mv = oracle.rx_verify_batch(buf, off)
        at = 800 if len(m) > 800 else len(m)
        frames, v = m[:at] + b + m[at:], np.concatenate([mv[:at], bv, mv[at:]])
        tbl = _table_for(frames, v, every=2)
        _cache[name] = (frames, v, tbl, T.expected(frames, v, tbl, A.TCP_RX_SEG_DTYPE))
    return _cache[name]


@pytest.mark.parametrize("seg_shift", [0, 8])
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("n", [257, 1000, 1537])
def test_later_iterations_of_the_parse(oracle, n, cap, seg_shift):
    """At most `cap` blocks ("aux_blocks"): the parse loops, in both store forms (seg_shift 0:
    records through LDS; 8: per-lane stores), over CSR frames and over ring slots; every record
    from 256 * cap on is produced by a later iteration alone, on poisoned memory."""
    frames, v, tbl, e = _multipass_set(oracle, n)
    assert len(frames) == n
    late = slice(256 * cap, None)
    if n >= 1000:
        assert (e.verdict[late] == T.DROP_TCP_OFFSET).sum() == 30
        assert (e.pcb[late] != T.NO_PCB).any() and (e.segs["opts"][late] == 0).any()
    buf, off = F.pack(frames)
    dbuf, doff = torch.from_numpy(buf).to(DEV), torch.from_numpy(off.view(np.int64)).to(DEV)
    stride = 2048
    ring = np.full(n * stride, 0x3C, dtype=np.uint8)
    lens = np.array([len(f) for f in frames], dtype=np.uint32)
    assert int(lens.max()) <= stride
    for i, f in enumerate(frames):
        ring[i * stride:i * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
    dring, dlens = torch.from_numpy(ring).to(DEV), torch.from_numpy(lens.view(np.int32)).to(DEV)
    got = {}
    for c in (cap, -1):
        _tune("aux_blocks", c)
        try:
            out = Outputs(n, seg_shift)
            A.tcp_rx_parse(dbuf, doff, tbl, **out.kw())
            _compare(e, out)
            slot = Outputs(n, seg_shift)
            A.tcp_rx_parse_slotted(dring, stride, dlens, tbl, **slot.kw())
            _compare(e, slot)
        finally:
            _tune("aux_blocks", -1)
        got[c] = (out.bytes(), slot.bytes())
    assert got[cap] == got[-1] and got[cap][0] == got[cap][1]
    assert A.contract_violations(clear=True) == 0


# ---- closing the loop with the send side -------------------------------------------------------

def test_segments_of_tcp_tx_segment_parse_back(oracle):
    import tcpseg_cases as S
    pay = S.payload_bytes()
    hdrs = [S.template(src=0x0A000001 + j, dst=0x0A000002, sport=40000 + j, dport=80 + j,
                       window=0x1000 + j) for j in range(3)]
    cases = [S.burst((100 * j + 1, 3000 + j), mss=1460, seq=0xFFFFF000 + j, hdr=hdrs[j],
                     flags=S.FIN if j == 1 else 0, psh_offset=1460) for j in range(3)]
    batch = S.Batch(cases, pay)
    dpay = torch.from_numpy(pay.copy()).to(DEV)
    desc = S.descriptors(batch, dpay.data_ptr(), A.TCP_BURST_DTYPE)
    si, cb = A.tcp_burst_layout(desc)
    seg = A.tcp_tx_segment(desc, si, cb)
    n = seg.n_segments
    assert n == 9 and (seg.status.cpu().numpy() == T.ACCEPT).all()
    hd = seg.headers.cpu().numpy().reshape(n, 64)
    ci = seg.chunk_index.cpu().numpy()
    ca, cl = seg.chunk_addr.cpu().numpy(), seg.chunk_len.cpu().numpy()
    frames = []
    for i in range(n):
        data = b"".join(pay[int(ca[c]) - dpay.data_ptr():][:int(cl[c])].tobytes()
                        for c in range(int(ci[i]), int(ci[i + 1])))
        frames.append(hd[i, :54].tobytes() + data)
    buf, off = F.pack(frames)
    # the sender's peer looks the connections up: its local side is the segments' destination
    tbl = A.tcp_pcb_table_sort(T.table([(0x0A000002, 0x0A000001 + j, 80 + j, 40000 + j, 500 + j)
                                        for j in range(3)], A.TCP_PCB_KEY_DTYPE))
    res = A.tcp_rx_parse(torch.from_numpy(buf).to(DEV), torch.from_numpy(off.view(np.int64)).to(DEV), tbl)
    assert (res.verdict.cpu().numpy() == T.ACCEPT).all()
    s, pc = res.segs_numpy(), res.pcb_numpy()
    e = S.expected(oracle, batch)
    for i in range(n):
        j, k = int(e.seg_case[i]), int(e.seg_k[i])
        ln = min(1460, 3000 + j - 1460 * k)
        assert s["seq_num"][i] == (0xFFFFF000 + j + 1460 * k) & 0xFFFFFFFF
        assert s["flags"][i] == e.seg_flags[i] and s["window_size"][i] == 0x1000 + j
        assert (s["remote_port"][i], s["local_port"][i]) == (40000 + j, 80 + j)
        assert (s["remote_addr"][i], s["local_addr"][i]) == (0x0A000001 + j, 0x0A000002)
        assert s["data_len"][i] == ln and s["data_off"][i] == 54 and s["ack_num"][i] == 0x0A0B0C0D
        assert s["opts"][i] == T.SEG_VALID and pc[i] == 500 + j
    assert {0x5010, 0x5018, 0x5019} <= set(s["flags"].tolist())


# ---- repeatability -----------------------------------------------------------------------------

def test_second_call_over_poisoned_outputs(oracle):
    frames, v = _set(oracle, "mixed")
    b, bv = _set(oracle, "bad_offsets")
    frames, v = frames[:150] + b, np.concatenate([v[:150], bv])
    tbl = _table_for(frames, v, every=2)
    e, out, (dbuf, doff) = _run_csr(frames, v, tbl)
    first = out.bytes()
    out.poison()
    A.tcp_rx_parse(dbuf, doff, tbl, **out.kw())
    assert out.bytes() == first
    _compare(e, out)
    assert A.contract_violations(clear=True) == 0
