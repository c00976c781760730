"""TEST INFRASTRUCTURE -- shared by test_tcp_rsp_host.py and test_gpu_tcp_rsp.py: the model of
what tcp_rx_respond leaves, and the frame builders.

The model is a plain Python restatement, over the record the TCP Rx parse model (tcprx_cases.py)
gives for a frame, of what the reference does with a TCP datagram around find_pcb:
  1. the local-address test (tcp/IpTcpProto_input.h:72), checkUnicastSrcAddr and
     find_listener_for_rx (:132-151), the top of listen_input (:372-401) with CalcTcpSndMss;
  2. send_rst_reply / send_rst / send_tcp_nodata (tcp/IpTcpProto_output.h:989-1018, :1338-1404)
     through sendIp4Dgram (ip/IpStack.h:423-453) and the Ethernet header.
Both are pinned against the reference's own stack by tests/golden/tcp_rsp_ref_cases.json
(test_tcp_rsp_host.py).
"""
import struct

import numpy as np

import frame_cases as F
import tcp_rsp_ref as R
import tcprx_cases as T

NONE, NOT_LOCAL, PCB, DROP, SYN, RST = 31, 32, 33, 34, 35, 36
HEADER = 54
NO_LISTENER = 0xFFFFFFFF
NO_FRAME = 0xFFFFFFFFFFFFFFFF
ALL_ONES = 0xFFFFFFFF
MIN_MSS = 216
OPT_MSS = 1

SEG = np.dtype({"names": ["remote_addr", "local_addr", "remote_port", "local_port", "seq_num", "ack_num",
                          "flags", "window_size", "data_off", "data_len", "mss", "wnd_scale", "opts"],
                "formats": ["<u4", "<u4", "<u2", "<u2", "<u4", "<u4", "<u2", "<u2", "<u2", "<u2", "<u2",
                            "u1", "u1"],
                "offsets": [0, 4, 8, 10, 12, 16, 20, 22, 24, 26, 28, 30, 31], "itemsize": 32})
KEY = np.dtype({"names": ["local_addr", "remote_addr", "local_port", "remote_port", "cookie"],
                "formats": ["<u4", "<u4", "<u2", "<u2", "<u4"], "offsets": [0, 4, 8, 10, 12],
                "itemsize": 16})


def iface(*, local=R.STACKS[0][0], prefix=24, mac=R.LOCAL_MAC, ip_id=0, ttl=64, mtu=1500):
    mask = R.netmask(prefix)
    return dict(local=local, bcast=(local & mask) | (~mask & ALL_ONES), mac=bytes(mac), ip_id=ip_id,
                ttl=ttl, mtu=mtu)


def stack_iface(stack, ip_id=0):
    return iface(local=stack["addr"], prefix=stack["prefix"], mac=bytes.fromhex(stack["mac"]), ip_id=ip_id)


def stack_listeners(stack):
    """[(addr, port, cookie)] in table order: newest first; the cookie is the opening order."""
    return [(a, p, 100 + k) for k, (a, p) in enumerate(stack["listeners"])][::-1]


def stack_frames(stack):
    return [bytes.fromhex(c["in"]) for c in stack["cases"]]


# ---- step 1: the decision ------------------------------------------------------------------------

def find_listener(lis, dst, port):
    for addr, p, cookie in lis:
        if p == port and (addr == dst or addr == 0):
            return cookie
    return None


def decide(rec, has_pcb, req, ifc, lis):
    """(status, listener cookie) of a frame with the valid record `rec`."""
    src, dst, flags = rec["remote_addr"], rec["local_addr"], rec["flags"]
    if dst != ifc["local"]:
        return NOT_LOCAL, NO_LISTENER
    if has_pcb and not req:
        return PCB, NO_LISTENER
    if src == ALL_ONES or (src & 0xF0000000) == 0xE0000000 or src == ifc["bcast"]:
        return DROP, NO_LISTENER
    if req:
        return RST, NO_LISTENER
    cookie = find_listener(lis, dst, rec["local_port"])
    if cookie is None:
        return (DROP if flags & 0x04 else RST), NO_LISTENER
    if flags & 0x17 != 0x02:
        return (RST if flags & 0x14 == 0x10 else DROP), cookie
    req_mss = rec["mss"] if rec["opts"] & OPT_MSS else 536
    if min(ifc["mtu"] - 40, req_mss) < MIN_MSS:
        return RST, cookie
    return SYN, cookie


# ---- step 2: the bytes ---------------------------------------------------------------------------

def rst_tcp_checksum(*, local, remote, lport, rport, seq, ack, flags):
    hdr = struct.pack(">HHIIHHHH", lport, rport, seq, ack, flags, 0, 0, 0)
    return R.I.chksum(struct.pack(">IIHH", local, remote, 6, 20) + hdr)


def rst_frame(rec, src_mac, ident, ifc):
    """The 54 bytes of send_rst_reply for the segment `rec` received from `src_mac`."""
    if rec["flags"] & 0x10:
        seq, ack, fl = rec["ack_num"], 0, 0x5004
    else:
        seq_len = rec["data_len"] + (1 if rec["flags"] & 0x03 else 0)
        seq, ack, fl = 0, (rec["seq_num"] + seq_len) & ALL_ONES, 0x5014
    local, remote = rec["local_addr"], rec["remote_addr"]
    ck = rst_tcp_checksum(local=local, remote=remote, lport=rec["local_port"], rport=rec["remote_port"],
                          seq=seq, ack=ack, flags=fl)
    tcp = struct.pack(">HHIIHHHH", rec["local_port"], rec["remote_port"], seq, ack, fl, 0, ck, 0)
    ip = bytearray(struct.pack(">BBHHHBBHII", 0x45, 0, 40, ident & 0xFFFF, 0x4000, ifc["ttl"], 6, 0,
                               local, remote))
    struct.pack_into(">H", ip, 10, R.I.chksum(bytes(ip)))
    return src_mac + ifc["mac"] + b"\x08\x00" + bytes(ip) + tcp


class Expected:
    """verdict, segs, pcb (as tcprx_cases.expected), status (uint8), listener (uint32), hdr_len
    (uint32), headers ({frame: 54 bytes}), chunk_index (uint64, n + 1, zero), response_frame /
    syn_frame (uint64, n), counts."""


def respond(frames, verdicts, ifc, pcbs=None, lis=(), rst_request=None):
    """What tcp_rx_respond must leave for `frames` (list of bytes) whose Rx verify verdicts are
    `verdicts`, with the PCB table `pcbs` (a KEY array or None), the listeners `lis`
    ([(addr, port, cookie)] in table order) and the host's requests."""
    n = len(frames)
    e = T.expected(frames, verdicts, pcbs, SEG)
    e.status = np.full(n, NONE, dtype=np.uint8)
    e.listener = np.full(n, NO_LISTENER, dtype=np.uint32)
    e.hdr_len = np.zeros(n, dtype=np.uint32)
    e.chunk_index = np.zeros(n + 1, dtype=np.uint64)
    e.response_frame = np.full(n, NO_FRAME, dtype=np.uint64)
    e.syn_frame = np.full(n, NO_FRAME, dtype=np.uint64)
    e.headers = {}
    j = k = 0
    for i, f in enumerate(frames):
        if not e.segs["opts"][i] & 0x80:
            continue
        rec = {name: int(e.segs[name][i]) for name in SEG.names}
        req = rst_request is not None and bool(rst_request[i])
        st, cookie = decide(rec, int(e.pcb[i]) != T.NO_PCB, req, ifc, lis)
        e.status[i], e.listener[i] = st, cookie
        if st == RST:
            e.hdr_len[i] = HEADER
            e.headers[i] = rst_frame(rec, f[6:12], ifc["ip_id"] + j, ifc)
            e.response_frame[j] = i
            j += 1
        elif st == SYN:
            e.syn_frame[k] = i
            k += 1
    e.counts = np.array([j, k], dtype=np.uint64)
    return e


def verdicts_of(oracle, frames):
    buf, off = F.pack(frames)
    return oracle.rx_verify_batch(buf, off)


# ---- the fixture's events ------------------------------------------------------------------------

def sent(events):
    return [bytes.fromhex(e[2:]) for e in events if e.startswith("T ")]


# ---- crafted frames beyond the fixture -----------------------------------------------------------

LOCAL, PREFIX, PEER, GATEWAY = R.STACKS[0]
LISTENERS = [(LOCAL, 80, 7), (0, 8080, 8), (0, 443, 9), (LOCAL, 443, 10)]


def rst_due(k, **kw):
    """A segment that gets an RST; sender, ports, numbers and flags vary with k."""
    kw.setdefault("src", (LOCAL & 0xFFFFFF00) | (1 + k % 200))
    kw.setdefault("dst", LOCAL)
    kinds = ((R.SYN, R.CLOSED), (R.ACK, R.CLOSED), (R.ACK, R.SPECIFIC), (R.FIN | R.ACK, R.WILDCARD),
             (R.PSH, R.CLOSED), (R.SYN | R.FIN, R.CLOSED))
    flags, port = kinds[k % len(kinds)]
    return R.frame(flags, sport=1024 + k % 60000, dport=port, seq=(0x9E3779B1 * (k + 1)) & ALL_ONES,
                   ack=(0x85EBCA77 * (k + 3)) & ALL_ONES, data=R.I.pattern(k % 5, k), pad60=bool(k & 1),
                   **kw)


def no_rst(k, **kw):
    """TCP that gets no RST: to a PCB-less listener as a pure SYN, an RST segment, a bad source,
    another host's, a SYN+FIN to a listener."""
    kw.setdefault("dst", LOCAL)
    src = kw.pop("src", (LOCAL & 0xFFFFFF00) | (1 + k % 200))
    kinds = (dict(flags=R.SYN, dport=R.SPECIFIC, src=src), dict(flags=R.RST, src=src),
             dict(flags=R.SYN, src=0xE0000001), dict(flags=R.SYN, src=src, dst=LOCAL ^ 0x80),
             dict(flags=R.SYN | R.FIN, dport=R.WILDCARD, src=src),
             dict(flags=R.SYN, dport=R.SPECIFIC, src=src, opts=R.mss_opt(1460)))
    d = dict(kw, **kinds[k % len(kinds)])
    return R.frame(d.pop("flags"), sport=1024 + k % 60000, seq=k, pad60=bool(k & 1), **d)


def not_tcp(k):
    """Frames without a valid record: UDP, ICMP, ARP, short ones, a bad checksum, a bad offset."""
    peer = PEER
    kinds = (R.LOCAL_MAC + R.PEER_MAC + b"\x08\x00" + R.I.ip_packet(17, R.I.udp(R.I.pattern(k % 9, k))),
             R.LOCAL_MAC + R.PEER_MAC + b"\x08\x00" + R.I.echo(R.I.pattern(k % 23, k)),
             R.AR.arp(1, peer, LOCAL), R.LOCAL_MAC + R.PEER_MAC[:k % 7], b"",
             R.frame(R.SYN, src=peer, dst=LOCAL, bad=True),
             R.frame(R.SYN, src=peer, dst=LOCAL, doff=4), R.frame(R.ACK, src=peer, dst=LOCAL, doff=9))
    return kinds[k % len(kinds)]


def sized_batch(n, kind):
    """n frames: "all" get an RST, "none" does (TCP without one, and frames without a record), or
    "mixed" with RSTs at lanes 0 and 63 of a wave, at a block's first and last frame, in a block
    where every frame gets one (the third) and between blocks without one."""
    if kind == "all":
        return [rst_due(k) for k in range(n)]
    if kind == "none":
        return [no_rst(k) if k % 3 else not_tcp(k) for k in range(n)]
    places = {i for i in (0, 63, 64, 127, 255, 256, n - 1) if 0 <= i < n} | set(range(512, min(n, 768)))
    return [rst_due(k) if k in places else (no_rst(k // 3), not_tcp(k), no_rst(k // 3 + 3))[k % 3]
            for k in range(n)]


def pcb_table(count, *, port=5000):
    """`count` PCBs of LOCAL:port with distinct peers (unsorted; cookie = 1000 + index)."""
    t = np.zeros(count, dtype=KEY)
    for i in range(count):
        t[i] = (LOCAL, 0x0A141E00 + 1 + i % 200, port, 20000 + i, 1000 + i)
    return t


def pcb_frame(t, i, flags=R.ACK, **kw):
    """A segment of PCB i of `t`."""
    return R.frame(flags, src=int(t["remote_addr"][i]), dst=int(t["local_addr"][i]),
                   sport=int(t["remote_port"][i]), dport=int(t["local_port"][i]), **kw)


def random_batch(seed, n, table):
    """n frames drawn from every class above and segments of PCBs; (frames, rst_request)."""
    rng = np.random.default_rng(seed)
    picks = rng.integers(0, 10, n)
    ks = rng.integers(0, 1 << 20, n)
    frames = []
    for p, k in zip(picks.tolist(), ks.tolist()):
        if p < 3:
            frames.append(rst_due(k))
        elif p < 6:
            frames.append(no_rst(k))
        elif p < 8 and len(table):
            frames.append(pcb_frame(table, k % len(table), data=R.I.pattern(k % 40, k)))
        else:
            frames.append(not_tcp(k))
    req = (rng.integers(0, 8, n) == 0).astype(np.uint8)
    return frames, req
