"""TEST INFRASTRUCTURE -- reference-produced TCP segments without data (SYN, SYN-ACK, empty ACK,
window update, FIN, RST): the reference's own EthIpIface over its IpStack with IpTcpProto,
accepting TcpListeners and TcpConnections (tcp_ctl_ref_gen.cpp only includes reference headers;
the platform with its hand-moved clock and the capture driver are this project's), compiled from
the reference tree and driven by the scripted sessions below, one request at a time: a later
request is made from the answers before it (the peer acknowledges the ISS it was sent). What the
stack sent is recorded in tcp_ctl_ref_cases.json:

  {"sessions": [{"name": .., "addr": .., "prefix": .., "gateway": .., "mac": "<hex>",
                 "peer": .., "peer_mac": "<hex>",
                 "steps": [{"step": "<what was done>", "out": ["<hex frame>", ...]}]}]}

Only IPv4 TCP frames are kept (a timer may also send an ARP request, which takes no Ident); none
carries data, since no session ever gives a connection something to send. A session keeps one
stack, so its frames carry consecutive Idents from 0. Before the first frame an ARP reply makes the
peer's MAC known.

    python3 tests/golden/tcp_ctl_ref.py <reference tree>      # rewrites the fixture
"""
import json
import os
import struct
import subprocess
import sys

import icmp_ref as I
import tcp_rsp_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "tcp_ctl_ref_cases.json")
GEN_SRC = os.path.join(HERE, "tcp_ctl_ref_gen.cpp")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "tcp_ctl_ref_gen")

LOCAL_MAC, PEER_MAC = R.LOCAL_MAC, R.PEER_MAC
FIN, SYN, RST, PSH, ACK = R.FIN, R.SYN, R.RST, R.PSH, R.ACK
SMALL, LARGE = 80, 8080          # listeners: a 4096-byte and a 200000-byte receive buffer
SMALL_ROOM, LARGE_ROOM = 4096, 200000
WS_OPT = bytes([1, 3, 3, 7])


def build_generator(reference):
    os.makedirs(os.path.dirname(GEN_BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(reference, "src"), "-o", GEN_BIN,
                    GEN_SRC], check=True)
    return GEN_BIN


def is_tcp(f):
    return len(f) >= 54 and f[12:14] == b"\x08\x00" and f[23] == 6


def fields(f):
    """The TCP fields of a sent frame: (seq, ack, flags, window)."""
    t = 14 + (f[14] & 0xF) * 4
    seq, ack, of, wnd = struct.unpack(">IIHH", f[t + 4:t + 16])
    return seq, ack, of & 0xFF, wnd


class Session:
    """One stack in the generator process, and the record of what it sent."""

    def __init__(self, proc, name, local, prefix, peer, gateway, clock):
        self.proc, self.local, self.prefix, self.peer, self.gateway = proc, local, prefix, peer, gateway
        self.rec = {"name": name, "addr": local, "prefix": prefix, "gateway": gateway,
                    "mac": LOCAL_MAC.hex(), "peer": peer, "peer_mac": PEER_MAC.hex(), "steps": []}
        self.conns = 0
        self.say("S %d %d %d %s %d" % (local, prefix, gateway, LOCAL_MAC.hex(), clock))

    def say(self, line):
        self.proc.stdin.write(line + "\n")
        self.proc.stdin.flush()

    def ask(self, step, line):
        """The request `line`; the TCP frames it caused, recorded under `step`."""
        self.say(line)
        out = []
        while True:
            a = self.proc.stdout.readline().rstrip("\n")
            if a == ".":
                break
            assert a[:2] == "T ", a
            f = bytes.fromhex(a[2:])
            if is_tcp(f):
                out.append(f)
        self.rec["steps"].append({"step": step, "out": [f.hex() for f in out]})
        return out

    def listen(self, port, wnd, room):
        self.say("L %d %d %d %d" % (self.local, port, wnd, room))

    def frame(self, step, flags, **kw):
        for k in ("seq", "ack"):                         # the peer's arithmetic is mod 2^32
            kw[k] &= 0xFFFFFFFF
        f = R.frame(flags, src=self.peer, dst=self.local, **kw)
        if not self.rec["steps"]:
            self.say("Q " + R.next_hop_arp(f, self.local, self.prefix, self.gateway).hex())
        return self.ask(step, "F " + f.hex())

    def connect(self, step, port, wnd, room):
        if not self.rec["steps"]:
            f = R.frame(ACK, src=self.peer, dst=self.local)
            self.say("Q " + R.next_hop_arp(f, self.local, self.prefix, self.gateway).hex())
        self.conns += 1
        return self.ask(step, "C %d %d %d %d" % (self.peer, port, wnd, room))


def passive_syns():
    """[(step, port, source port, seq, options)] of the SYNs a passive session starts with."""
    syns = [("no option", b""), ("MSS 216", R.mss_opt(216)), ("MSS 536", R.mss_opt(536)),
            ("MSS 1460", R.mss_opt(1460)), ("MSS 1460 + window scale 7", R.mss_opt(1460) + WS_OPT),
            ("window scale alone", bytes([3, 3, 2, 1]))]
    return [("SYN with %s to the %s-buffer listener" % (oname, pname), port, 41000 + 100 * (port == LARGE) + k,
             0x10000000 * (k + 1) + port, opts)
            for port, pname in ((SMALL, "small"), (LARGE, "large")) for k, (oname, opts) in enumerate(syns)]


def syn_frames(session):
    """[(the SYN frame fed in, the SYN-ACK frame recorded for it)] of a passive session."""
    by = {st["step"]: st["out"] for st in session["steps"]}
    return [(R.frame(SYN, src=session["peer"], dst=session["addr"], sport=sport, dport=port, seq=iseq,
                     ack=0, opts=opts), bytes.fromhex(by[step][0]))
            for step, port, sport, iseq, opts in passive_syns()]


def passive(s):
    """Listeners: SYN-ACKs, their retransmission, handshakes, ACKs, window updates, RST, FIN."""
    s.listen(SMALL, SMALL_ROOM, SMALL_ROOM)
    s.listen(LARGE, LARGE_ROOM, LARGE_ROOM)
    pend = []
    for step, port, sport, iseq, opts in passive_syns():
        out = s.frame(step, SYN, sport=sport, dport=port, seq=iseq, ack=0, opts=opts)
        assert len(out) == 1 and fields(out[0])[2] == SYN | ACK
        pend.append((port, sport, iseq, fields(out[0])[0]))
    out = s.ask("1 s later: every SYN-ACK is retransmitted", "A 1000")
    assert len(out) == len(pend)
    est = []
    for port, sport, iseq, iss in pend[:4] + pend[6:10]:
        s.frame("ACK completes the handshake (port %d from %d); the listener accepts" % (port, sport),
                ACK, sport=sport, dport=port, seq=iseq + 1, ack=iss + 1)
        est.append((s.conns, port, sport, iseq + 1, iss + 1))
        s.conns += 1
    for c, port, sport, seq, ack in est:
        out = s.frame("100 bytes in order on connection %d" % c, PSH | ACK, sport=sport, dport=port,
                      seq=seq, ack=ack, data=I.pattern(100, c))
        assert len(out) == 1 and fields(out[0])[2] == ACK
    for c, port, sport, seq, ack in est:
        out = s.frame("a segment far beyond the window on connection %d" % c, ACK, sport=sport,
                      dport=port, seq=seq + 0x01000000, ack=ack, data=I.pattern(10, c))
        assert len(out) == 1 and fields(out[0])[2] == ACK
    for c, port, sport, seq, ack in est[:4]:
        for j in range(3):
            s.frame("1000 more bytes on connection %d (%d)" % (c, j), PSH | ACK, sport=sport,
                    dport=port, seq=seq + 100 + 1000 * j, ack=ack, data=I.pattern(1000, j))
        s.ask("the application of connection %d reads 3100 bytes: window update" % c, "X %d 3100" % c)
    for c, port, sport, seq, ack in est[:3]:
        out = s.ask("connection %d is reset with unread data: RST|ACK" % c, "R %d 1" % c)
        assert len(out) == 1 and fields(out[0])[2] == RST | ACK
    for c, port, sport, seq, ack in est[4:7]:
        s.ask("connection %d is abandoned" % c, "R %d 0" % c)
        out = s.ask("the output timer of abandoned connection %d: FIN|PSH|ACK" % c, "A 1")
        assert len(out) == 1 and fields(out[0])[2] == FIN | PSH | ACK, out
    s.ask("1 s later: retransmissions", "A 1000")


def active(s):
    """startConnection: SYN, its retransmission, the ACK of a SYN-ACK, the RST of a bad ACK."""
    syn = []
    for k, (wnd, room) in enumerate(((1000, 1000), (65535, 65535), (200000, 200000))):
        out = s.connect("startConnection with rcv_wnd %d" % wnd, 7000 + k, wnd, room)
        assert len(out) == 1 and fields(out[0])[2] == SYN
        syn.append(out[0])
    again = s.ask("1 s later: every SYN is retransmitted", "A 1000")
    assert len(again) == 3
    for a, b in zip(sorted(syn, key=lambda f: f[36:38]), sorted(again, key=lambda f: f[36:38])):
        assert a[18:20] != b[18:20] and a[38:42] == b[38:42]      # a new Ident, the same seq
    lport = [struct.unpack(">H", f[34:36])[0] for f in syn]
    iss = [fields(f)[0] for f in syn]
    out = s.frame("SYN-ACK with MSS 1460 + window scale for the first: its ACK", SYN | ACK, sport=7000,
                  dport=lport[0], seq=0x33330000, ack=iss[0] + 1, opts=R.mss_opt(1460) + WS_OPT)
    assert len(out) == 1 and fields(out[0])[2] == ACK
    out = s.frame("SYN-ACK without options for the second: its ACK", SYN | ACK, sport=7001,
                  dport=lport[1], seq=0xFFFFFFFF, ack=iss[1] + 1)
    assert len(out) == 1 and fields(out[0])[2] == ACK
    out = s.frame("an ACK of something never sent in SYN_SENT: RST without ACK", ACK, sport=7002,
                  dport=lport[2], seq=5, ack=iss[2] + 77)
    assert len(out) == 1 and fields(out[0])[2] == RST
    s.ask("the SYN_SENT connection is reset: nothing is sent", "R 2 1")
    out = s.ask("the first connection is reset with unread data: RST|ACK", "R 0 1")
    assert len(out) == 1 and fields(out[0])[2] == RST | ACK
    s.ask("the second connection is abandoned", "R 1 0")
    out = s.ask("the output timer of the abandoned connection: FIN|PSH|ACK", "A 1")
    assert len(out) == 1 and fields(out[0])[2] == FIN | PSH | ACK


def generate(reference):
    """The fixture's text, from the reference's code run on the sessions above."""
    gen = build_generator(reference)
    proc = subprocess.Popen([gen], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    sessions = []
    clock = 0x7FFFF000
    for n, (local, prefix, peer, gateway) in enumerate(R.STACKS):
        for name, script in (("passive", passive), ("active", active)):
            # the ISS is the clock: the second stack's sequence numbers wrap
            s = Session(proc, "%s_%d" % (name, n), local, prefix, peer, gateway,
                        clock if n == 0 else 0xFFFFFFFF)
            script(s)
            sessions.append(s.rec)
    proc.stdin.close()
    assert proc.wait() == 0
    return json.dumps({"sessions": sessions}, indent=0, separators=(",", ":")) + "\n"


def load():
    with open(FIXTURE) as f:
        return json.load(f)["sessions"]


def frames(session):
    """[(step, frame bytes)] of a session, in the order the stack sent them."""
    return [(st["step"], bytes.fromhex(h)) for st in session["steps"] for h in st["out"]]


if __name__ == "__main__":
    text = generate(sys.argv[1])
    with open(FIXTURE, "w") as f:
        f.write(text)
    print("%s: %d bytes" % (FIXTURE, len(text)))
