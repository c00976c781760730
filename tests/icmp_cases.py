"""TEST INFRASTRUCTURE -- shared by test_icmp_host.py and test_gpu_icmp.py: the model of the ICMP
responder and the frame builders.

The model is a plain Python restatement, written independently of the kernel (it sums every
checksum over the bytes, where the kernel derives the echo checksum from the request's field), of
what the reference does with a received datagram that ends in an ICMP message of its own:
  1. recvIcmp4Dgram (ip/IpStack.h:1093-1148) with checkUnicastSrcAddr (:838-843);
  2. sendIp4DestUnreach (:869-887) under checkSendIp4Allowed (:666-690), for the frames the host
     asks one for;
  3. sendIcmp4Message (:1164-1190) and sendIp4Dgram (:423-453).
All three are pinned against the reference's own stack by tests/golden/icmp_ref_cases.json
(test_icmp_host.py); the verdicts rest on the frame oracle.
"""
import struct

import numpy as np

import frame_cases as F
import icmp_ref as R

ACCEPT, ACCEPT_NO_CHKSUM, ACCEPT_OTHER, FRAGMENT = 6, 7, 8, 3
NONE, ECHO_REPLY, UNREACH, TOO_LARGE = 23, 24, 25, 26
NO_UNREACH = 0xFF
PORT_UNREACH = 3
HEADER = 42
NO_FRAME = 0xFFFFFFFFFFFFFFFF

LOCAL_MAC = F.LOCAL_MAC
PEER_MAC = F.peer_mac(0)


def iface(*, local=R.LOCAL, bcast=R.BCAST, mtu=1500, ip_id=0, ttl=64, allow=False, mac=LOCAL_MAC):
    return dict(local=local, bcast=bcast, mtu=mtu, ip_id=ip_id & 0xFFFF, ttl=ttl, allow=bool(allow),
                mac=bytes(mac))


def eth(ip_packet, *, src_mac=PEER_MAC, pad60=False):
    f = LOCAL_MAC + src_mac + b"\x08\x00" + ip_packet
    if pad60 and len(f) < 60:
        f += bytes([0x5A]) * (60 - len(f))
    return f


def host_codes(frames):
    """What a host without any UDP listener asks for: Port Unreachable for every IPv4 UDP frame
    (udp/IpUdpProto.h:609-620 decides the rest), nothing for the others."""
    return [PORT_UNREACH if len(f) >= 34 and f[12:14] == b"\x08\x00" and f[23] == 17 else NO_UNREACH
            for f in frames]


# ---- steps 1 and 2: is a response due, and what is its data ----------------------------------

def plan(frame, verdict, code, ifc):
    """(status, data offset in the frame, data length) of one frame with Rx verify's verdict."""
    if verdict not in (ACCEPT, ACCEPT_NO_CHKSUM, ACCEPT_OTHER):
        return NONE, 0, 0
    hl = (frame[14] & 0xF) * 4
    total, = struct.unpack_from(">H", frame, 16)
    src, dst = struct.unpack_from(">II", frame, 26)
    payload = total - hl
    if verdict == ACCEPT and frame[23] == 1:                       # recvIcmp4Dgram
        unicast_src = src != 0xFFFFFFFF and (src >> 28) != 0xE and src != ifc["bcast"]
        if dst == ifc["local"]:
            dst_ok = True
        else:
            dst_ok = (dst == ifc["bcast"] or dst == 0xFFFFFFFF) and ifc["allow"]
        if unicast_src and dst_ok and frame[14 + hl] == 8:
            n = payload - 8
            return (TOO_LARGE if 28 + n > ifc["mtu"] else ECHO_REPLY), 14 + hl + 8, n
    if code != NO_UNREACH and dst == ifc["local"] and src != 0xFFFFFFFF and src != ifc["bcast"]:
        n = hl + min(8, payload)
        return (TOO_LARGE if 28 + n > ifc["mtu"] else UNREACH), 14, n
    return NONE, 0, 0


# ---- step 3: the bytes ---------------------------------------------------------------------------

def response_header(frame, status, data_off, data_len, code, ident, ifc):
    """The 42 header bytes of the response (Ethernet, IPv4, ICMP)."""
    data = frame[data_off:data_off + data_len]
    if status == ECHO_REPLY:
        t = 14 + (frame[14] & 0xF) * 4
        msg = bytearray(struct.pack(">BBH", 0, 0, 0) + frame[t + 4:t + 8])
    else:
        msg = bytearray(struct.pack(">BBHI", 3, code, 0, 0))
    struct.pack_into(">H", msg, 2, R.chksum(bytes(msg) + data))
    ip = bytearray(struct.pack(">BBHHHBBHI", 0x45, 0, 28 + data_len, ident & 0xFFFF, 0, ifc["ttl"], 1,
                               0, ifc["local"]) + frame[26:30])
    struct.pack_into(">H", ip, 10, R.chksum(bytes(ip)))
    return frame[6:12] + ifc["mac"] + b"\x08\x00" + bytes(ip) + bytes(msg)


class Expected:
    """status, hdr_len (uint32), headers ({frame: 42 bytes}), chunks ([(frame, offset in the
    frame, length)], compact), chunk_index (uint64, n + 1), response_frame (uint64, n), counts."""


def respond(frames, verdicts, codes, ifc):
    """What icmp_rx_respond must leave for `frames` (list of bytes) with Rx verify's `verdicts`
    and the host's unreach `codes` (None: no requests)."""
    n = len(frames)
    e = Expected()
    e.verdict = np.array(verdicts, dtype=np.uint8)
    e.status = np.full(n, NONE, dtype=np.uint8)
    e.hdr_len = np.zeros(n, dtype=np.uint32)
    e.chunk_index = np.zeros(n + 1, dtype=np.uint64)
    e.response_frame = np.full(n, NO_FRAME, dtype=np.uint64)
    e.headers, e.chunks = {}, []
    j = 0
    for i, f in enumerate(frames):
        code = NO_UNREACH if codes is None else int(codes[i])
        st, off, ln = plan(f, int(verdicts[i]), code, ifc)
        e.status[i] = st
        e.chunk_index[i] = len(e.chunks)
        if st in (ECHO_REPLY, UNREACH):
            e.hdr_len[i] = HEADER
            e.headers[i] = response_header(f, st, off, ln, code, ifc["ip_id"] + j, ifc)
            e.response_frame[j] = i
            j += 1
            if ln:
                e.chunks.append((i, off, ln))
    e.chunk_index[n] = len(e.chunks)
    e.counts = np.array([j, len(e.chunks)], dtype=np.uint64)
    return e


def response_packet(e, frames, i):
    """The IP packet of frame i's response: header bytes 14-41, then the chunk's bytes."""
    a, b = int(e.chunk_index[i]), int(e.chunk_index[i + 1])
    data = b"".join(frames[fi][off:off + ln] for fi, off, ln in e.chunks[a:b])
    return e.headers[i][14:] + data


# ---- a stack of the fixture, replayed as the host would -----------------------------------------

def stack_iface(stack, ip_id):
    return iface(local=stack["addr"], bcast=stack["addr"] | (0xFFFFFFFF >> stack["prefix"]),
                 mtu=stack["mtu"], ip_id=ip_id, allow=stack["allow"])


def stack_frames(stack):
    """The stack's injected packets as Ethernet frames; the echo_pad60 case as the 60-byte frame
    it stands for."""
    return [eth(bytes.fromhex(c["in"])) for c in stack["cases"]]


def stack_batches(stack, verdicts):
    """The stack's cases as the batches of a host that takes the slow path for a TOO_LARGE frame:
    a batch ends behind such a frame, and the next one starts one Ident later (the reference's
    fragmented send consumed it). [(first case, frames, verdicts, codes, iface, Expected)]"""
    frames = stack_frames(stack)
    codes = host_codes(frames)
    out, start, ip_id = [], 0, stack["warm"]
    while start < len(frames):
        ifc = stack_iface(stack, ip_id)
        e = respond(frames[start:], verdicts[start:], codes[start:], ifc)
        big = np.flatnonzero(e.status == TOO_LARGE)
        end = start + (int(big[0]) + 1 if big.size else len(frames) - start)
        e = respond(frames[start:end], verdicts[start:end], codes[start:end], ifc)
        out.append((start, frames[start:end], verdicts[start:end], codes[start:end], ifc, e))
        ip_id += int(e.counts[0]) + (1 if big.size else 0)
        start = end
    return out


# ---- crafted frames beyond the fixture -----------------------------------------------------------

def crafted_frames():
    """Echo requests and UDP datagrams at every IHL, with 0-9 data bytes and with trailing bytes,
    echo requests from several MACs, zero-class requests of every data length 0-9 and of 1472
    bytes (all zero, and zero but for the last byte pair), and other traffic in between."""
    out = []
    for ihl in range(5, 16):
        for n in (0, 1, 5, 9):
            out.append(eth(R.echo(R.pattern(n, ihl + n), ihl=ihl), pad60=bool(n & 1)))
            out.append(eth(R.ip_packet(17, R.udp(R.pattern(n, ihl)), ihl=ihl, trailing=bytes([0xEE]) * n)))
    for n in list(range(10)) + [1472]:
        out.append(eth(R.echo(bytes(n), rest=bytes(4)), src_mac=F.peer_mac(n % 4)))
        if n >= 2:
            out.append(eth(R.echo(bytes(n - 2) + b"\xff\xff", rest=bytes(4))))
    out.append(eth(R.echo(bytes([0xFF]) * 1472, rest=bytes([0xFF]) * 4)))
    out.append(eth(R.ip_packet(47, R.pattern(30, 1))))                  # ACCEPT_OTHER, no request
    out.append(eth(R.ip_packet(6, R.pattern(10, 2))))                   # TCP below 20 bytes
    out.append(LOCAL_MAC + PEER_MAC + b"\x08\x06" + bytes(28))          # ARP
    return out


def crafted_codes(frames):
    """Codes of every kind: the host's for UDP, and requests for an `other` protocol frame."""
    c = host_codes(frames)
    for i, f in enumerate(frames):
        if len(f) >= 34 and f[12:14] == b"\x08\x00" and f[23] == 47:
            c[i] = 2                                                   # Protocol Unreachable
    return c


def mixed_batch(n, responders, seed=20261020):
    """n frames of frame_cases.frames (TCP, UDP, ICMP, bad checksums, non-IP; their echo requests
    are addressed to LOCAL and answered too), with a fixture-style echo request at every index in
    `responders`."""
    fr = F.frames(seed=seed, n=n)
    for k, i in enumerate(sorted(responders)):
        fr[i] = eth(R.echo(R.pattern(k % 23, k), ident=k & 0xFFFF), pad60=bool(k & 1))
    return fr
