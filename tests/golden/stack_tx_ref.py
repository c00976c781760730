"""TEST INFRASTRUCTURE -- what the reference stack puts on the wire for the two Tx builders: the
reference's own IpStack with IpTcpProto and IpUdpProto, instantiated by oracle/stack_ref_gen.cpp
(which includes reference headers only) on a stub platform and a capture driver of this project's,
run on the scenarios below. Every captured IP packet is recorded in stack_tx_ref_cases.json as its
header bytes in hex, its data length and the FNV-1a 64 of its data; the payloads themselves follow
from a salt, so the fixture holds none:

  {"udp": ["<mtu> <sport> <dport> <dst> <len0> <len1> <salt> <fix>|<fragment>;<fragment>...", ...],
        fragment = "<20 IP header bytes> <8 UDP header bytes, - beyond the first> <data length> <FNV>"
   "tcp": [{"conn": "<dst> <dport> <peer mss> <peer window> <peer shift> <ring> <salt> <clock> <peer isn>",
            "handshake": ["<kind> <IP header> <TCP header and options> <length> <FNV>", ...],
            "snd_mss": n,
            "bursts": ["<tokens>|<off0> <len0> <off1> <len1> <snd_mss> <push> <fin> <seq> <stream index>|<segment>;...", ...]}, ...]
        segment = "<kind> <20 IP header bytes> <20 TCP header bytes> <data length> <FNV>"
   "min_mss": [[<peer mss>, <connection established>], ...]}

UDP payload byte k is (salt + 3k) & 0xFF; with fix >= 0 bytes 0 and 1 are fix, big-endian (the
leading two bytes that make the datagram's sum 0xFFFF, as call_sites.py makes its zero-sum
datagrams). TCP stream byte k is (salt + 3k) & 0xFF and lies at ring position k % ring. A burst is
what the stack emits when its output timer fires after the tokens (<n> = n bytes written and
extendSendBuf, P = sendPush, F = closeSending); the scripted peer then ACKs every segment on its
own, so the congestion window grows by one mss per segment. The per-burst values are the
connection's public state (getSendBuf, getSndBufOverhead) and what the script did; none is read
from a captured header. Segment kinds: D = data or FIN, sent first; S / A / R = SYN, pure ACK and
retransmit, which the tests skip (the bursts hold none).

The shortest last fragment the reference can emit has (mtu - 20) % 8 + 1 bytes: it sends what is
left as the last fragment as soon as that fits the MTU, so a rest of 1 ... (mtu - 20) % 8 bytes
beyond a whole number of rounded fragments rides in the fragment before. A last fragment of 1
byte exists only where (mtu - 20) % 8 == 0 (1500 here).

What the scenarios leave out, because a burst descriptor does not carry it: a
burst cut short by the send or congestion window, and a tail shorter than snd_mss that the
reference holds back while no push covers it. `_plan` keeps every burst within the window and
its tail pushed or whole; `generate` asserts that the stack sent all of each burst.

    python3 tests/golden/stack_tx_ref.py <reference tree>      # rewrites the fixture

Only `random.Random(seed).getrandbits` is used (a stable Mersenne Twister stream).
"""
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "stack_tx_ref_cases.json")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "stack_ref_gen")

LOCAL = 0x0A000001
UDP_MTUS = (256, 576, 1006, 1500)
STACK_MTU_TCP = 1500
CLOCK = 1000
MIN_MSS_PROBE = (215, 216)


class _Rng:
    def __init__(self, seed):
        self._r = random.Random(seed)

    def below(self, n):
        if n <= 1:
            return 0
        b = (n - 1).bit_length()
        while True:
            v = self._r.getrandbits(b)
            if v < n:
                return v


def fnv(data):
    f = 0xcbf29ce484222325
    for c in bytes(data):
        f = ((f ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return f


def udp_payload(D, salt, fix=-1):
    b = bytearray((salt + 3 * k) & 0xFF for k in range(D))
    if fix >= 0:
        b[0], b[1] = fix >> 8, fix & 0xFF
    return bytes(b)


def stream_bytes(start, n, salt):
    return bytes((salt + 3 * k) & 0xFF for k in range(start, start + n))


# ---- UDP scenarios --------------------------------------------------------------------------

def _zero_fix(src, dst, sport, dport, D, salt):
    """The two leading payload bytes that make pseudo-header + UDP header + payload sum to 0xFFFF."""
    P = 8 + D
    s = (src >> 16) + (src & 0xFFFF) + (dst >> 16) + (dst & 0xFFFF) + 17 + P + sport + dport + P
    data = udp_payload(D, salt)
    for k in range(2, D):
        s += data[k] << (8 if k % 2 == 0 else 0)
    return (-s) % 0xFFFF


def udp_scenarios():
    """[(mtu, sport, dport, dst, len0, len1, salt, fix)], grouped by mtu (one stack each, so the
    idents of a group run on)."""
    rng = _Rng(20261201)
    out = []
    for mtu in UDP_MTUS:
        M = mtu - 20
        F = M // 8 * 8
        one = lambda D, salt: out.append((mtu, 40000, 53, 0x0A000002, D, 0, salt, -1))   # noqa: E731
        for D in (0, 1, mtu - 29, mtu - 28, mtu - 27):
            one(D, 1 + D % 200)
        one(2 * F + M % 8 + 1 - 8, 11)      # the shortest last fragment: M % 8 + 1 bytes (see below)
        one(3 * F - 8, 12)                  # an exact multiple of the rounded fragment length
        one(F + M - 8, 13)                  # a last fragment of M bytes (longer than F where M % 8)
        one(F + M - 8 + 1, 14)
        one(20000 + mtu, 15)                # D >= 20000
        if mtu == 1500:
            one(65507, 16)
        # two pieces: the split on a fragment boundary, in a fragment's first 8 bytes, inside one
        D = 3 * F + 37 - 8
        for l0 in (F - 8, F - 8 + 3, F - 8 + 100, 2 * F - 8, 2 * F - 8 + 7, 1, D - 1, 0):
            out.append((mtu, 40001, 5353, 0x0A000003, l0, D - l0, 20 + l0 % 100, -1))
        out.append((mtu, 40001, 5353, 0x0A000003, 5, mtu - 28 - 5, 9, -1))       # two pieces, one packet
        # a UDP sum of 0, sent as 0xFFFF: one packet, fragmented, fragmented in two pieces
        for D, l0, salt in ((mtu - 100, mtu - 100, 31), (2 * F + 40, 2 * F + 40, 32), (2 * F + 41, F + 3, 33)):
            sport, dport, dst = 1000 + mtu, 2000 + D, 0x0A010203
            fix = _zero_fix(LOCAL, dst, sport, dport, D, salt)
            out.append((mtu, sport, dport, dst, l0, D - l0, salt, fix))
        for _ in range(25):
            D = rng.below(5 * M)
            l0 = rng.below(D + 1) if rng.below(3) else D
            out.append((mtu, rng.below(65536), rng.below(65536), 0x0A000000 | 2 + rng.below(1 << 24) % 0xFFFFF0,
                        l0, D - l0, rng.below(256), -1))
    return out


# ---- TCP scenarios --------------------------------------------------------------------------

def initial_cwnd(mss):
    return (2 if mss > 2190 else 3 if mss > 1095 else 4) * mss


def all_sent(D, push, mss):
    """Whether the reference sends all D bytes of a burst at once: it holds back a tail shorter
    than mss that no push covers (the loop condition of pcb_output_active)."""
    threshold = min(D - push, mss - 1)
    rem = D
    while rem > threshold:
        rem -= min(rem, mss)
    return rem == 0


class _Plan:
    """The bursts of one connection, each within the congestion window as the per-segment ACKs
    of the bursts before have grown it."""

    def __init__(self, peer_mss, ring, salt, dst, dport, wnd=65535, shift=4, clock=CLOCK, peer_isn=0x11223344):
        self.conn = (dst, dport, peer_mss, wnd, shift, ring, salt, clock, peer_isn)
        self.mss = min(peer_mss or 536, STACK_MTU_TCP - 40)
        self.ring, self.wnd = ring, wnd
        self.cwnd = initial_cwnd(self.mss)
        self.pos = 0
        self.bursts = []
        self.closed = False

    def room(self):
        return min(self.cwnd, self.wnd, self.ring)

    def burst(self, D, push="end", fin=False):
        """push: "end", "none", or an index in 1..D."""
        assert not self.closed and D <= self.room() and (D > 0 or fin)
        p = D if push == "end" or fin else 0 if push == "none" else push
        assert all_sent(D, p, self.mss), (D, p, self.mss)
        if fin:
            toks = ([str(D)] if D else []) + ["F"]
        elif p == 0:
            toks = [str(D)]
        else:
            toks = [str(p), "P"] + ([str(D - p)] if D > p else [])
        self.bursts.append(" ".join(toks))
        nseg = max(1, -(-D // self.mss))
        self.cwnd += sum(min(self.mss, min(self.mss, D - k * self.mss) + (fin and k == nseg - 1))
                         for k in range(nseg))
        self.pos += D
        self.closed = fin


def _fill(plan, rng, n, multiples_only=False):
    """n bursts of mixed shapes: sizes around the segment and window edges, pushes at the edges
    of a segment, in its middle, at the end and none."""
    m = plan.mss
    for i in range(n):
        room = plan.room()
        full = room // m
        kind = rng.below(10)
        if multiples_only or kind < 3:
            D = m * (1 + rng.below(full))
        elif kind == 3:
            D = m * rng.below(full) + 1                      # a last segment of 1 byte
        elif kind == 4:
            D = 1 + rng.below(m)                             # one segment
        elif kind == 5 and full >= 2:
            D = m * full - rng.below(2)                      # as long as the window allows
        else:
            D = 1 + rng.below(room)
        nseg = -(-D // m)
        r = D % m
        k = rng.below(nseg)
        opts = ["end"]
        if r == 0:
            opts += ["none", m * (k + 1), m * k + 1, m * k + 1 + rng.below(m)]
        else:
            last = m * (nseg - 1)
            opts += [last + 1, last + 1 + rng.below(r)]      # inside the short last segment
        push = opts[rng.below(len(opts))]
        plan.burst(D, push)


def tcp_plans():
    rng = _Rng(20261202)
    plans = []
    # snd_mss 536 (no MSS option: the default), a small ring with frequent wraps
    p = _Plan(0, 12007, 3, 0x0A000002, 80, shift=-1)
    p.burst(1)
    p.burst(536, "none")
    p.burst(537)
    p.burst(4 * 536, 536)                   # push on the first segment's last byte
    p.burst(4 * 536, 536 + 1)               # on the second segment's first byte
    p.burst(4 * 536, 536 + 200)             # in its middle
    _fill(p, rng, 22)
    p.burst(1000, fin=True)                 # FIN with data
    plans.append(p)
    # snd_mss 536 by option, the ring a multiple of it and every burst too: wraps on segment edges
    p = _Plan(536, 24 * 536, 77, 0x0A000005, 8080)
    for _ in range(3):
        p.burst(p.room() // 536 * 536, "none")
    _fill(p, rng, 20, multiples_only=True)
    p.burst(0, fin=True)                    # FIN alone
    plans.append(p)
    # snd_mss 1460, long bursts
    p = _Plan(1460, 50021, 200, 0x0A000002, 443)
    for _ in range(3):
        p.burst(p.room() // 1460 * 1460)
    p.burst(20 * 1460 + 1)
    p.burst(25 * 1460, "none")
    _fill(p, rng, 24)
    p.burst(3 * 1460, fin=True)             # FIN, the last segment full
    plans.append(p)
    # a peer MSS above the interface's: snd_mss stays 1460
    p = _Plan(9000, 33333, 5, 0x0A0000FE, 22, wnd=40000, shift=0)
    _fill(p, rng, 20)
    p.burst(1, fin=True)
    plans.append(p)
    # the smallest MSS the reference accepts
    p = _Plan(216, 7001, 9, 0x0A000002, 8000)
    p.burst(216, "none")
    p.burst(217)
    for _ in range(3):
        p.burst(p.room() // 216 * 216, 216 * 2)
    _fill(p, rng, 26)
    p.burst(0, fin=True)
    plans.append(p)
    # sequence numbers that pass 2^32: the initial sequence number is the clock's low 32 bits
    p = _Plan(1460, 40009, 41, 0x0A000002, 81, clock=(7 << 32) - 9000)
    _fill(p, rng, 14)
    p.burst(700, fin=True)
    plans.append(p)
    p = _Plan(536, 9973, 42, 0x0A000007, 82, clock=(1 << 32) - 537)           # a segment ends at 2^32
    p.burst(536, "none")
    p.burst(1072)
    _fill(p, rng, 14)
    p.burst(536, fin=True)
    plans.append(p)
    return plans


# ---- the generator --------------------------------------------------------------------------

def build_generator(reference):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/stack_ref_gen",
                    "REF_SRC=" + os.path.join(reference, "src")], check=True)
    return GEN_BIN


def run(requests):
    """The generator's answers: one list of lines per request."""
    out = subprocess.run([GEN_BIN], input="\n".join(requests) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert out[-1] == ""
    answers, cur = [], []
    for ln in out[:-1]:
        if ln == ".":
            answers.append(cur)
            cur = []
        else:
            cur.append(ln)
    assert not cur
    return answers


def _connect(conn):
    dst, dport, mss, wnd, shift, ring, salt, clock, pisn = conn
    return ["S %d %d %d" % (STACK_MTU_TCP, LOCAL, clock),
            "C %d %d %d %d %d %d %d %d" % (dst, dport, mss, wnd, shift, ring, salt, pisn)]


def generate(reference=None):
    """The fixture's text, from the reference's stack run on the scenarios above."""
    if reference is not None:
        build_generator(reference)
    doc = {"udp": [], "tcp": [], "min_mss": []}
    # UDP
    req, mtu = [], None
    scen = udp_scenarios()
    for s in scen:
        if s[0] != mtu:
            mtu = s[0]
            req.append("S %d %d %d" % (mtu, LOCAL, CLOCK))
        req.append("U " + " ".join(str(v) for v in s[1:]))
    ans = [a for a in run(req) if a]
    assert len(ans) == len(scen)
    for s, a in zip(scen, ans):
        assert a[0] == "U 0", a[0]
        doc["udp"].append(" ".join(str(v) for v in s) + "|" + ";".join(x[2:] for x in a[1:]))
    # TCP
    for plan in tcp_plans():
        req = _connect(plan.conn) + ["B " + b for b in plan.bursts]
        ans = run(req)
        hs = ans[1]
        assert hs[-1] == "C %d 1" % plan.mss, hs[-1]
        rows = []
        for toks, a in zip(plan.bursts, ans[2:]):
            info = a[0][2:]
            cut = a.index("I")
            assert a[cut + 1:] == [], "the stack answered an ACK with a packet: %r" % a[cut + 1:]
            segs = [x[2:] for x in a[1:cut]]
            f = info.split()
            sent = sum(int(x.split()[3]) for x in segs if x[0] == "D")
            assert sent == int(f[1]) + int(f[3]), "the stack held part of a burst back: %r" % toks
            rows.append(toks + "|" + info + "|" + ";".join(segs))
        doc["tcp"].append({"conn": " ".join(str(v) for v in plan.conn), "handshake": [x[2:] for x in hs[:-1]],
                           "snd_mss": plan.mss, "bursts": rows})
    for mss in MIN_MSS_PROBE:
        ans = run(_connect((0x0A000002, 80, mss, 65535, -1, 4096, 1, CLOCK, 1)))
        doc["min_mss"].append([mss, int(ans[1][-1].split()[2])])
    return json.dumps(doc, indent=0, separators=(",", ":")) + "\n"


def receive(local_addr, port, packet_lists):
    """Each list of IP packets injected into a fresh reference stack with a UdpListener on
    `port`: [[(length, fnv) per listener call]]."""
    req = []
    for pk in packet_lists:
        req.append("S 1500 %d %d" % (local_addr, CLOCK))
        req.append("R %d %d" % (port, len(pk)))
        req += [bytes(p).hex() for p in pk]
    out = []
    for a in run(req)[1::2]:
        assert a[0] == "R %d" % (len(a) - 1)
        out.append([(int(x.split()[1]), int(x.split()[2], 16)) for x in a[1:]])
    return out


# ---- the fixture ----------------------------------------------------------------------------

class Packet:
    """kind, ip (20 bytes), l4 (the UDP / TCP header bytes, b"" beyond a first fragment), length
    and fnv of the data."""

    def __init__(self, kind, ip, l4, length, h):
        self.kind, self.ip, self.l4, self.length, self.fnv = kind, ip, l4, length, h


def _packet(text, kind=None):
    f = text.split()
    if kind is None:
        kind, f = f[0], f[1:]
    return Packet(kind, bytes.fromhex(f[0]), b"" if f[1] == "-" else bytes.fromhex(f[1]), int(f[2]),
                  int(f[3], 16))


def load():
    """(udp, tcp, min_mss): udp = [dict(mtu, sport, dport, dst, len0, len1, salt, fix, frags)],
    tcp = [dict(dst, dport, peer_mss, wnd, shift, ring, salt, clock, peer_isn, handshake, snd_mss,
    bursts = [dict(tokens, off0, len0, off1, len1, mss, push, fin, seq, start, packets)])]."""
    with open(FIXTURE) as f:
        doc = json.load(f)
    udp = []
    for row in doc["udp"]:
        s, frags = row.split("|")
        d = dict(zip(("mtu", "sport", "dport", "dst", "len0", "len1", "salt", "fix"), map(int, s.split())))
        d["frags"] = [_packet(x, "F") for x in frags.split(";")]
        udp.append(d)
    tcp = []
    for c in doc["tcp"]:
        d = dict(zip(("dst", "dport", "peer_mss", "wnd", "shift", "ring", "salt", "clock", "peer_isn"),
                     map(int, c["conn"].split())))
        d["handshake"] = [_packet(x) for x in c["handshake"]]
        d["snd_mss"] = c["snd_mss"]
        d["bursts"] = []
        for row in c["bursts"]:
            toks, info, segs = row.split("|")
            b = dict(zip(("off0", "len0", "off1", "len1", "mss", "push", "fin", "seq", "start"),
                         map(int, info.split())))
            b["tokens"] = toks
            b["packets"] = [_packet(x) for x in segs.split(";")] if segs else []
            d["bursts"].append(b)
        tcp.append(d)
    return udp, tcp, [tuple(x) for x in doc["min_mss"]]


if __name__ == "__main__":
    text = generate(sys.argv[1])
    with open(FIXTURE, "w") as f:
        f.write(text)
    print("%s: %d bytes" % (FIXTURE, len(text)))
