"""TEST INFRASTRUCTURE -- the inputs of test_gpu_rx_cut.py and what the eight receive entry points
must make of them. The property: a frame's result depends only on the bytes inside its length, and
it is right at every length. The kernels read a frame through an unbounded dword load, kept inside
the frame by the length tests of the *_common.h functions alone; behind a frame's end lies, in a
ring slot, the slot's previous occupant, and in the CSR form the next frame: bytes that look like
headers. A length test that is off by a few bytes gives a wrong record, not a fault.

Per stage (STAGES) three families of cases, each one batch:
  A  every seed at every length k = 0..len(seed), the bytes unchanged, twice: behind the cut lies
     the seed's own continuation (the uncut frame is there, only the length says otherwise), or
     the bytes of another seed of the stage at the same place.
  B  the seeds at full length with one inner length swept and the checksums repaired by the frame
     oracle's Tx fill: the IPv4 total length 0..len-12, the UDP length 0..payload+2, the TCP data
     offset 0..15 against three total lengths, the quoted IHL 0..15 and the quoted total length
     0..dlen+2 of a Destination Unreachable; for ARP (no inner length) the four fixed-value fields.
     Each twice, with the two tails of A.
  C  513 frames of the stage's existing mixed batch, laid out twice: the second time every byte
     outside every frame (tails, slot rests, gaps, lead, guard areas) is inverted.
A case is (frame, tail). In ring slots the tail lies in the slot behind lens[i]. In the CSR form,
whose n + 1 offsets leave no room between frames, the tail is the next frame: the batch is the
interleaved list frame 0, tail 0, frame 1, tail 1, ... and the models answer for every entry.

The seeds (``Stage.seeds``) take, uncut, the stage's interesting path; the companions
(``Stage.companions``: a fragment, bad checksums, another protocol, UDP without a checksum, a TCP
datagram below 20 bytes) are swept like seeds so that every Rx verdict occurs in every stage, and
serve as the other seed of a tail. Reassembly is different in one respect: a case is a whole train
of three fragments under an Ident of its own, one member cut or swept.

Expectations come from the models of the case modules, which see ``frame`` alone, and from the
frame oracle; nothing here needs a GPU or torch."""
import struct

import numpy as np

import arp_cases as AC
import frame_cases as F
import icmp_cases as IC
import icmp_du_cases as DU
import icmp_du_ref as DR
import icmp_ref as IR
import ipreass_cases as RC
import tcp_rsp_cases as TR
import tcp_rsp_ref as TRR
import tcprx_cases as TC
import udp_rx_cases as UC

GUARD = 256                  # bytes the buffer keeps in front of the first and behind the last frame
EXTRA = 8                    # bytes of tail behind an uncut seed
FAMILIES = ("A", "B", "C")
C_FRAMES = 513               # two tiles of 256 frames and one frame
LOCAL, PEER, BCAST = IR.LOCAL, IR.PEER, IR.BCAST

SEG = np.dtype({"names": ["remote_addr", "local_addr", "remote_port", "local_port", "seq_num", "ack_num",
                          "flags", "window_size", "data_off", "data_len", "mss", "wnd_scale", "opts"],
                "formats": ["<u4", "<u4", "<u2", "<u2", "<u4", "<u4", "<u2", "<u2", "<u2", "<u2", "<u2", "u1",
                            "u1"],
                "offsets": [0, 4, 8, 10, 12, 16, 20, 22, 24, 26, 28, 30, 31], "itemsize": 32})
KEY = TR.KEY
LIS = np.dtype({"names": ["iface_addr", "port", "flags", "reserved0", "cookie", "reserved1"],
                "formats": ["<u4", "<u2", "u1", "u1", "<u4", "<u4"], "offsets": [0, 4, 6, 7, 8, 12],
                "itemsize": 16})
DGRAM = np.dtype({"names": ["remote_addr", "local_addr", "remote_port", "local_port", "data_off", "data_len",
                            "listeners", "assoc", "flags", "ttl", "reserved"],
                  "formats": ["<u4", "<u4", "<u2", "<u2", "<u2", "<u2", "<u8", "<u4", "u1", "u1", "<u2"],
                  "offsets": [0, 4, 8, 10, 12, 14, 16, 24, 28, 29, 30], "itemsize": 32})


def verdicts_of(oracle, frames):
    buf, off = F.pack(frames)
    return oracle.rx_verify_batch(buf, off)


def filled(oracle, frames):
    """The frames with the checksums the frame oracle's Tx fill writes (wherever it finds a sane
    IPv4 header; elsewhere the frame stays as it is)."""
    return TC.fill(oracle, list(frames))[0]


# ---- the companions: the verdicts the seeds of a stage do not reach -------------------------------

def companions():
    """Frames that are swept like seeds without taking a stage's interesting path of their own
    accord (the echo request does in the ICMP responder)."""
    bad_ip = bytearray(IC.eth(IR.echo(IR.pattern(9, 3))))
    bad_ip[24] ^= 0x40
    return [IC.eth(IR.ip_packet(17, IR.udp(IR.pattern(16, 2)), flags_off=0x2000)),           # 3 fragment
            bytes(bad_ip),                                                                     # 2
            IC.eth(IR.ip_packet(1, IR.icmp(8, 0, IR.REST, IR.pattern(20, 6), bad=True))),     # 5
            IC.eth(IR.ip_packet(47, IR.pattern(30, 1))),                                      # 8
            UC.dgram(5000, n=3, pad60=True, chk="zero"),                                      # 7
            IC.eth(IR.ip_packet(6, IR.pattern(10, 2)), pad60=True),                           # 4
            IC.eth(IR.echo(IR.pattern(9, 4)))]                                                # 6, no TCP / UDP


# ---- the stages ------------------------------------------------------------------------------------

class Stage:
    """name; seeds(oracle) (uncut: the interesting path); expect(oracle, frames) (the model's
    Expected for a list of frames); outcome(e) (one code per frame, what the conditions of
    test_rx_cut_cases.py count); interesting (the codes of the interesting path); codes (every
    code a single frame can get) and exempt ({code: why the sweeps cannot reach it}); verdict(e)
    (the verdict array, or None); sweeps (the inner lengths of family B); mixed(oracle, n)."""
    stride = 256
    has_verdict = True
    sweeps = ("total",)
    exempt = {}

    def companions(self, oracle):
        return companions()

    def verdict(self, e):
        return e.verdict


class Verify(Stage):
    name = "rx_verify"
    interesting, codes = (6, 7, 8), tuple(range(9))
    sweeps = ("total", "udp_len", "doff")

    def seeds(self, oracle):
        opts = bytes([1]) * 8 + struct.pack(">BBH", 2, 4, 1400)
        return filled(oracle, [
            TC.tcp_frame(ihl=6, doff=8, opts=opts, sport=40001),          # options end on the last byte
            TC.tcp_frame(payload=IR.pattern(31, 4), sport=40002),
            TC.tcp_frame(pad60=True, sport=40003)]) + [
            UC.dgram(5000, n=3, pad60=True), IC.eth(IR.echo(IR.pattern(40, 5), ihl=7)),
            UC.dgram(5001, n=30, chk="zero"), IC.eth(IR.ip_packet(47, IR.pattern(50, 9), ihl=6))]

    def companions(self, oracle):
        return companions()[:3] + companions()[5:6]

    def expect(self, oracle, frames):
        e = type("Expected", (), {})()
        e.verdict = verdicts_of(oracle, frames)
        return e

    def outcome(self, e):
        return np.asarray(e.verdict)

    def mixed(self, oracle, n):
        return F.frames(seed=20261101, n=n)


def _tcp_seeds(oracle):
    """Segments of the connections of _TCP_KEYS."""
    ws_mss = struct.pack(">BBBBBBH", 3, 3, 7, 1, 2, 4, 1400)
    return filled(oracle, [
        TC.tcp_frame(sport=40000, dport=80, payload=IR.pattern(24, 1)),
        TC.tcp_frame(sport=40001, dport=80, ihl=6, doff=7, opts=ws_mss),  # options end on the last byte
        TC.tcp_frame(sport=40002, dport=80, pad60=True, flags=0x011),
        TC.tcp_frame(sport=40003, dport=81, doff=15, opts=bytes([1]) * 36 + struct.pack(">BBH", 2, 4, 536)),
        TC.tcp_frame(sport=40004, dport=81, ihl=15, doff=6, payload=IR.pattern(7, 2))])


_TCP_KEYS = [(LOCAL, PEER, 80, 40000), (LOCAL, PEER, 80, 40001), (LOCAL, PEER, 80, 40002),
             (LOCAL, PEER, 81, 40003), (LOCAL, PEER, 81, 40004)]


class TcpRx(Stage):
    name = "tcp_rx_parse"
    interesting, codes = ("pcb",), tuple(range(9)) + (11, "pcb", "no_pcb")
    sweeps = ("total", "doff")
    pcbs = TC.model_sort(TC.table([k + (700 + j,) for j, k in enumerate(_TCP_KEYS)], KEY))

    def seeds(self, oracle):
        return _tcp_seeds(oracle)

    def companions(self, oracle):
        return companions() + filled(oracle, [TC.tcp_frame(sport=45000, dport=80, payload=b"no pcb")])

    def expect(self, oracle, frames):
        return TC.expected(frames, verdicts_of(oracle, frames), self.pcbs, SEG)

    def outcome(self, e):
        valid = (e.segs["opts"] & TC.SEG_VALID) != 0
        return [("pcb" if e.pcb[i] != TC.NO_PCB else "no_pcb") if valid[i] else int(e.verdict[i])
                for i in range(len(valid))]

    def mixed(self, oracle, n):
        fr = TC.mixed_frames(n)
        for i, f in zip(range(0, n, 37), _tcp_seeds(oracle) * 3):
            fr[i] = f
        return fr


class Reass(Stage):
    name = "ip4_rx_reassemble"
    stride = 2048
    interesting, codes = (RC.MEMBER,), tuple(range(9)) + (RC.MEMBER, RC.DROP_FRAG)
    SRC, DST = 0x0A141E65, LOCAL

    def train(self, ident):
        """Three fragments (IHL 6, padded to 60 bytes and beyond) of one UDP datagram."""
        body = RC.udp_body(self.SRC, self.DST, 7, 5000, IR.pattern(45, ident & 0xFF), ulen=None, chk=None)
        return RC.frag_frames(self.SRC, self.DST, ident, 17, RC.cut(body, [16, 32]), ihl=6, ttl=64, pad=6,
                              total=None)

    def seeds(self, oracle):
        return self.train(1)

    def expect(self, oracle, frames):
        return RC.model(oracle, RC.Batch(frames), RC.MAX_REASS)

    def outcome(self, e):
        return np.asarray(e.verdict)

    def mixed(self, oracle, n):
        fr = []
        for s in range(1, 20):
            fr += RC.scenario(oracle, s).batch.frames
            if len(fr) >= n:
                break
        fr = [f for f in fr if len(f) <= 1600][:n]
        assert len(fr) == n
        return fr


class Icmp(Stage):
    name = "icmp_rx_respond"
    interesting, codes = (IC.ECHO_REPLY, IC.UNREACH), (IC.NONE, IC.ECHO_REPLY, IC.UNREACH, IC.TOO_LARGE)
    exempt = {IC.TOO_LARGE: "needs a response above the interface's MTU, which is at least 256: a frame of "
                            "more than 256 bytes, and the sweeps' slots are 256 bytes"}
    sweeps = ("total", "udp_len")
    ifc = IC.iface(local=LOCAL, bcast=BCAST, mtu=1500, ip_id=0xFFF0, ttl=64, allow=False)
    has_headers, header = True, 42

    def seeds(self, oracle):
        return [IC.eth(IR.echo(b""), pad60=True), IC.eth(IR.echo(IR.pattern(5, 1), ihl=6)),
                IC.eth(IR.echo(IR.pattern(33, 2))), UC.dgram(9000, n=3, pad60=True),
                UC.dgram(9001, n=20, ihl=7), UC.dgram(9002, n=0)]

    def codes_of(self, frames):
        return IC.host_codes(frames)

    def expect(self, oracle, frames):
        return IC.respond(frames, verdicts_of(oracle, frames), self.codes_of(frames), self.ifc)

    def outcome(self, e):
        return np.asarray(e.status)

    def mixed(self, oracle, n):
        return IC.mixed_batch(n, set(range(0, n, 7)) | {255, 256, n - 1})


class UdpRx(Stage):
    name = "udp_rx_demux"
    interesting = ("deliver", "unreach")
    codes = (0, 1, 2, 3, 4, 5, 6, 8, "deliver", "unreach", "valid")     # 7 is always a valid record
    sweeps = ("total", "udp_len")
    ifc = Icmp.ifc
    listeners = UC.listeners([(0, 5000, 0, 0, 11), (LOCAL, 5001, 1, 0, 12)], LIS)
    assocs = UC.assocs([(LOCAL, PEER, 6000, UC.R.SPORT, False, 5)], KEY)

    def seeds(self, oracle):
        return [UC.dgram(5000, n=3, pad60=True), UC.dgram(6000, n=17, ihl=6), UC.dgram(9000, n=20),
                UC.dgram(5001, n=0, chk="zero", pad60=True), UC.dgram(9001, n=1, ihl=15)]

    def companions(self, oracle):
        return companions() + [UC.dgram(9000, n=4, dst=LOCAL + 1)]      # valid, nobody's: no unreach

    def expect(self, oracle, frames):
        return UC.expected(frames, verdicts_of(oracle, frames), self.ifc, self.assocs, self.listeners, DGRAM)

    def outcome(self, e):
        n = len(e.verdict)
        delivered = set(e.deliver_frame[:int(e.counts[0])].tolist())
        return ["deliver" if i in delivered else "unreach" if e.unreach[i] == UC.PORT_UNREACH else
                "valid" if e.dgrams["flags"][i] & UC.VALID else int(e.verdict[i]) for i in range(n)]

    def mixed(self, oracle, n):
        return UC.mixed(n)


class Arp(Stage):
    name = "arp_rx_respond"
    has_verdict = False
    interesting, codes = (AC.REPLY,), (AC.NONE, AC.MALFORMED, AC.SEEN, AC.REPLY)
    sweeps = ("arp",)
    ifc = AC.iface()
    has_headers, header = True, 42

    def seeds(self, oracle):
        return [AC.request(1, self.ifc, pad=18), AC.request(2, self.ifc, pad=0), AC.request(3, self.ifc, pad=7)]

    def companions(self, oracle):
        return [AC.other(1, self.ifc), AC.other(2, self.ifc), IC.eth(IR.echo(IR.pattern(4, 1)))]

    def verdict(self, e):
        return None

    def expect(self, oracle, frames):
        return AC.respond(frames, self.ifc)

    def outcome(self, e):
        return np.asarray(e.status)

    def mixed(self, oracle, n):
        return AC.sized_batch(n, "mixed")


class TcpRsp(Stage):
    name = "tcp_rx_respond"
    interesting = (TR.PCB, TR.SYN, TR.RST)
    codes = (TR.NONE, TR.NOT_LOCAL, TR.PCB, TR.DROP, TR.SYN, TR.RST)
    sweeps = ("total", "doff")
    ifc = TR.iface(ip_id=0xFFF0)
    lis = TR.LISTENERS
    pcbs = TR.pcb_table(8)
    has_headers, header = True, 54

    def seeds(self, oracle):
        R = TRR
        return [R.frame(R.ACK, src=PEER, dst=LOCAL, dport=R.CLOSED, data=IR.pattern(5, 1), pad60=True),   # RST
                R.frame(R.SYN, src=PEER, dst=LOCAL, dport=R.SPECIFIC, opts=R.mss_opt(1460), ihl=6),       # SYN
                TR.pcb_frame(self.pcbs, 3, data=IR.pattern(11, 2)),                                       # PCB
                R.frame(R.SYN, src=PEER, dst=LOCAL, dport=R.CLOSED, opts=bytes([1]) * 12 + R.mss_opt(300)),
                R.frame(R.FIN | R.ACK, src=PEER, dst=LOCAL, dport=R.WILDCARD, ihl=15, data=IR.pattern(30, 3))]

    def companions(self, oracle):
        R = TRR
        return companions() + [R.frame(R.RST, src=PEER, dst=LOCAL),                        # DROP
                               R.frame(R.SYN, src=PEER, dst=LOCAL ^ 0x80, pad60=True)]     # NOT_LOCAL

    def expect(self, oracle, frames):
        return TR.respond(frames, verdicts_of(oracle, frames), self.ifc, self.pcbs, self.lis, None)

    def outcome(self, e):
        return np.asarray(e.status)

    def mixed(self, oracle, n):
        return TR.random_batch(20261102, n, self.pcbs)[0]


class IcmpDu(Stage):
    name = "icmp_rx_unreach"
    interesting = (DU.TCP_PCB,)
    codes = (DU.NONE, DU.PARSED, DU.TCP_NO_PCB, DU.TCP_PCB)
    sweeps = ("total", "qihl", "qtotal")
    ifc = DU.iface()
    pcbs = DU.pcb_table(8)

    def _msg(self, i, *, l4=8, qihl=5, qtotal=1500, **kw):
        la, ra, lp, rp = DU.key_of(self.pcbs, i)
        q = DR.quoted(6, DR.tcp_head(l4, sport=lp, dport=rp, seq=0x01020304 + i), src=la, dst=ra, ihl=qihl,
                      total=qtotal)
        return DR.frame(q, src=PEER, dst=LOCAL, code=4, rest=1400, **kw)

    def seeds(self, oracle):
        """A frame of this kind has at least 62 bytes, so there is none that padding brings to 60:
        the padded seeds carry 5 and 9 bytes behind the IPv4 total length."""
        return [self._msg(0),                                   # quoted total above dlen
                self._msg(1, l4=20, qihl=6, pad=5),             # quoted IHL 6
                self._msg(2, l4=20, qtotal=20 + 8),             # quoted total below dlen: 12 bytes not L4
                self._msg(3, l4=8, qtotal=20 + 8, ihl=6),       # quoted total equal to dlen; IHL 6
                self._msg(4, l4=28, qihl=15, qtotal=60 + 8, pad=9)]

    def companions(self, oracle):
        la, ra, lp, rp = DU.near_miss(self.pcbs, 0, 0)
        q = DR.quoted(6, DR.tcp_head(8, sport=lp, dport=rp), src=la, dst=ra)
        return companions() + [DR.frame(q, src=PEER, dst=LOCAL, code=4),                     # TCP_NO_PCB
                               DR.frame(DR.quoted(17, DR.udp_head(8), src=LOCAL), src=PEER, dst=LOCAL, code=3)]

    def expect(self, oracle, frames):
        return DU.expected(frames, verdicts_of(oracle, frames), self.ifc, self.pcbs)

    def outcome(self, e):
        return np.asarray(e.status)

    def mixed(self, oracle, n):
        return DU.random_batch(20261103, n, self.pcbs)


STAGES = {s.name: s for s in (Verify(), TcpRx(), Reass(), Icmp(), UdpRx(), Arp(), TcpRsp(), IcmpDu())}


# ---- tails ---------------------------------------------------------------------------------------

def tails(seed, other, k, room):
    """The two tails of a frame cut at k in `room` bytes: the seed's own continuation (behind its
    end: the seed once more, as the next frame of a ring would be), and the bytes another seed has
    at the same place."""
    own = (seed * 3)[k:room]
    alt = (other * (2 + room // max(len(other), 1)))[k:room]
    if alt == own and own:
        alt = bytes([own[0] ^ 0x55]) + own[1:]
    return own, alt


# ---- family B: one inner length swept -------------------------------------------------------------

def _hl(f):
    return (f[14] & 0xF) * 4


def _is_ip(f, proto=None):
    return len(f) >= 34 and f[12:14] == b"\x08\x00" and (proto is None or f[23] == proto)


def _put(f, at, fmt, v):
    f = bytearray(f)
    struct.pack_into(fmt, f, at, v)
    return bytes(f)


def swept(f, sweeps):
    """[(name of the sweep, value, the frame with that value)] for the seed f, checksums not yet
    repaired."""
    out = []
    if "total" in sweeps and _is_ip(f):
        out += [("total", t, _put(f, 16, ">H", t)) for t in range(0, len(f) - 14 + 3)]
    if "udp_len" in sweeps and _is_ip(f, 17):
        T = 14 + _hl(f)
        payload = struct.unpack_from(">H", f, 16)[0] - _hl(f)
        out += [("udp_len", u, _put(f, T + 4, ">H", u)) for u in range(0, payload + 3)]
    if "doff" in sweeps and _is_ip(f, 6):
        T = 14 + _hl(f)
        full = struct.unpack_from(">H", f, 16)[0]
        for total in sorted({_hl(f) + 20, (_hl(f) + 20 + full) // 2, full}):
            g = _put(f, 16, ">H", total)
            out += [("doff", (total, d), _put(g, T + 12, "B", d << 4 | g[T + 12] & 0xF)) for d in range(16)]
    if ("qihl" in sweeps or "qtotal" in sweeps) and _is_ip(f, 1):
        Q = 14 + _hl(f) + 8
        dlen = struct.unpack_from(">H", f, 16)[0] - _hl(f) - 8
        if "qihl" in sweeps:
            out += [("qihl", q, _put(f, Q, "B", 0x40 | q)) for q in range(16)]
        if "qtotal" in sweeps:
            out += [("qtotal", t, _put(f, Q + 2, ">H", t)) for t in range(0, dlen + 3)]
    if "arp" in sweeps:
        for at, fmt, values in ((14, ">H", (0, 1, 2, 6, 256)), (16, ">H", (0, 0x0800, 0x0806, 0x86DD, 8)),
                                (18, "B", range(16)), (19, "B", range(16)), (20, ">H", (0, 1, 2, 3, 256))):
            out += [("arp", (at, v), _put(f, at, fmt, v)) for v in values]
    return out


# ---- the batches -----------------------------------------------------------------------------------

class Batch:
    """stage, family, lead (CSR: bytes in front of the first frame), stride; cases: [(frame,
    tail)]; per case seed (index into stage seeds + companions, -1: an uncut member of a train), k
    (A: the length; B: the frame's running number), variant (0, 1: which tail), partner (the case
    with the other tail), room (bytes the case may be read in without leaving its own place:
    len(frame) + len(tail)), what (B: the sweep's name)."""

    def tail(self, i, room, alt):
        """The bytes behind frame i in `room` bytes of space; alt: every one inverted."""
        if self.family == "C":
            src = self.cases[(i + 1) % len(self.cases)][0] or b"\x45"
            t = (src * (1 + room // len(src)))[:room]
        else:
            t = self.cases[i][1]
        return bytes(b ^ 0xFF for b in t) if alt else t


def _add(b, frame, tail, seed, k, variant, what=""):
    b.cases.append((frame, tail))
    b.seed.append(seed)
    b.k.append(k)
    b.variant.append(variant)
    b.what.append(what)


def _add_pair(b, frame, seed, other, j, k, what=""):
    """The frame (a seed cut at k, or a seed-long frame) with both tails."""
    i = len(b.cases)
    for variant, t in enumerate(tails(seed, other, len(frame), len(seed) + EXTRA)):
        _add(b, frame, t, j, k, variant, what)
    b.partner += [i + 1, i]


def _finish(b):
    for name in ("seed", "k", "variant"):
        setattr(b, name, np.array(getattr(b, name), dtype=np.int64))
    b.room = np.array([len(f) + len(t) for f, t in b.cases], dtype=np.int64)
    assert len(b.partner) == len(b.cases)
    assert all(b.variant[p] == 1 - b.variant[i] and len(b.cases[p][0]) == len(b.cases[i][0])
               for i, p in enumerate(b.partner))
    return b


def _new(stage, family, lead):
    b = Batch()
    b.stage, b.family, b.lead, b.stride = stage, family, lead, stage.stride
    b.cases, b.seed, b.k, b.variant, b.what, b.partner = [], [], [], [], [], []
    return b


def _sweep_into(b, oracle, every, n_seeds, sweeps):
    """Families A and B over frames that stand alone."""
    for j, s in enumerate(every):
        other = every[(j + 1) % len(every)]
        if b.family == "A":
            for k in range(len(s) + 1):
                _add_pair(b, s[:k], s, other, b.first_seed + j, k)
        elif j < n_seeds:
            sw = swept(s, sweeps)
            for (what, _, _), f in zip(sw, filled(oracle, [f for _, _, f in sw])):
                _add_pair(b, f, s, other, b.first_seed + j, len(b.cases), what)


def _reass_batch(oracle, stage, family, lead):
    """Every case a train of three fragments under an Ident of its own: member j cut at k (A) or
    with its total length swept (B), the other two whole, all three with tails (the other tail:
    the next member of a train that stays incomplete); the two tail variants are two trains. Then
    the companions, alone."""
    b = _new(stage, family, lead)
    ident = 0x100
    base = stage.train(0)[:2]
    for j in range(3):
        whole = stage.train(1)[j]
        if family == "A":
            edits = [(k, None) for k in range(len(whole) + 1)]
        else:
            edits = [(len(whole), t) for t in range(0, len(whole) - 14 + 3)]
        for k, total in edits:
            i = len(b.cases)
            for variant in (0, 1):
                ident += 1
                train = stage.train(ident)
                if total is not None:
                    train[j] = filled(oracle, [_put(train[j], 16, ">H", total)])[0]
                for m, f in enumerate(train):
                    cut = k if m == j else len(f)
                    t = tails(f, base[m % 2], cut, len(f) + EXTRA)[variant]
                    _add(b, f[:cut], t, j if m == j else -1, k if family == "A" else len(b.cases), variant,
                         "total" if total is not None else "")
            b.partner += [i + 3, i + 4, i + 5, i, i + 1, i + 2]
    b.seeds = stage.train(1)
    b.n_seeds, b.first_seed = 3, 3
    comp = stage.companions(oracle)
    b.seeds = b.seeds + comp
    _sweep_into(b, oracle, comp, 0, ())
    return _finish(b)


def batch(oracle, name, family):
    """The batch of family A, B or C of the stage `name`."""
    stage = STAGES[name]
    lead = (list(STAGES).index(name) + FAMILIES.index(family)) % 4
    if family == "C":
        b = _new(stage, "C", lead)
        frames = stage.mixed(oracle, C_FRAMES)
        assert len(frames) == C_FRAMES
        b.stride = 256 if max(len(f) for f in frames) <= 256 - EXTRA else 2048
        for i, f in enumerate(frames):
            _add(b, f, b"", -1, len(f), 0)
        b.partner = list(range(C_FRAMES))
        b.seeds = []
        b.room = np.array([len(f) for f in frames], dtype=np.int64)
        return b
    if name == "ip4_rx_reassemble":
        return _reass_batch(oracle, stage, family, lead)
    b = _new(stage, family, lead)
    seeds = list(stage.seeds(oracle))
    b.seeds = seeds + list(stage.companions(oracle))
    b.n_seeds, b.first_seed = len(seeds), 0
    assert max(len(s) for s in b.seeds) + EXTRA <= stage.stride
    _sweep_into(b, oracle, b.seeds, len(seeds), stage.sweeps)
    return _finish(b)


_cache = {}


def cached(oracle, name, family):
    """batch(), computed once per process and left unchanged."""
    if (name, family) not in _cache:
        _cache[(name, family)] = batch(oracle, name, family)
    return _cache[(name, family)]


# ---- the layouts -----------------------------------------------------------------------------------

class Lay:
    """host (the whole buffer, GUARD bytes of fill in front of the first frame and behind the last
    place); slotted; frames (the batch as the entry point sees it: the cases, or in the CSR form
    the cases and their tails in turn); index (case -> its entry in frames); start (per entry, in
    host); lens (per entry); offsets (CSR: n + 1, in host); stride; first (where the buffer handed
    to a slotted call starts in host)."""


def lay_out(b, slotted, alt=False):
    """The batch in ring slots or in the CSR form. alt: every byte outside every frame of the
    batch's cases inverted (tails, slot rests, lead and guard areas)."""
    lay = Lay()
    lay.slotted, lay.stride, lay.first = slotted, b.stride, GUARD
    fill = 0x5C ^ (0xFF if alt else 0)
    n = len(b.cases)
    if slotted:
        lay.frames = [f for f, _ in b.cases]
        lay.index = np.arange(n)
        lay.start = GUARD + np.arange(n, dtype=np.int64) * b.stride
        host = np.full(GUARD + n * b.stride + GUARD, fill, dtype=np.uint8)
        for i, (f, _) in enumerate(b.cases):
            room = b.stride - len(f) if b.family == "C" else len(b.cases[i][1])
            body = f + b.tail(i, room, alt)
            assert len(body) <= b.stride
            host[lay.start[i]:lay.start[i] + len(body)] = np.frombuffer(body, dtype=np.uint8)
        lay.offsets = None
    else:
        lay.frames = []
        for i, (f, _) in enumerate(b.cases):
            lay.frames += [f, b.tail(i, (5 * i + 3) % 8 if b.family == "C" else len(b.cases[i][1]), alt)]
        lay.index = 2 * np.arange(n)
        ln = np.array([len(f) for f in lay.frames], dtype=np.int64)
        lay.offsets = GUARD + b.lead + np.concatenate([[0], np.cumsum(ln)])
        lay.start = lay.offsets[:-1]
        host = np.full(int(lay.offsets[-1]) + GUARD, fill, dtype=np.uint8)
        body = np.frombuffer(b"".join(lay.frames), dtype=np.uint8)
        host[GUARD + b.lead:GUARD + b.lead + body.size] = body
    lay.lens = np.array([len(f) for f in lay.frames], dtype=np.int64)
    lay.host = host
    return lay


def outside(b, lay):
    """A mask over lay.host: the bytes that belong to no frame of the batch's cases."""
    m = np.ones(lay.host.size, dtype=bool)
    for i in range(len(b.cases)):
        s = int(lay.start[lay.index[i]])
        m[s:s + len(b.cases[i][0])] = False
    return m
