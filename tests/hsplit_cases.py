"""TEST INFRASTRUCTURE -- shared by test_hsplit_host.py and test_gpu_hsplit.py: split points
for the golden frames, hand-built exact-length segments, and the expected result of the
header-split Tx fill computed on the CPU: oracle.tx_fill_batch on the linearised copy plus the
layout rule of include/aipstack_amd/chksum.h, written out here independently of the kernels."""
import functools
import struct

import numpy as np

import frame_cases
from frame_cases import LOCAL_IP, LOCAL_MAC, be_sum, peer_ip, peer_mac

pack = frame_cases.pack

ACCEPT = 6
SPLIT_LAYOUT = 9
MAX_SPLIT_HEADER = 256

# (a) end of the fixed L4 header, (b) that +1 / +3, (c) end of the TCP options, (d) the whole
# frame in the slot, (e) 4 bytes short of (a)
SPLIT_CLASSES = ["l4_fixed", "l4_plus1", "l4_plus3", "tcp_opts", "whole", "short4"]


@functools.lru_cache(maxsize=None)
def golden_frames():
    return tuple(frame_cases.frames())


def _be16(f, o):
    return (f[o] << 8) | f[o + 1]


def _l4_fixed_end(f):
    """End of the fixed L4 header as the frame's own fields place it (any frame, however
    broken: the result only has to be a split point)."""
    hl = 20
    if len(f) > 14 and f[14] != 0x45:
        hl = max(20, (f[14] & 0xF) * 4)
    proto = f[23] if len(f) > 23 else 0
    return 14 + hl + {6: 20, 17: 8, 1: 8}.get(proto, 0), hl, proto


def split_points(frs, cls, stride):
    out = []
    for f in frs:
        a, hl, proto = _l4_fixed_end(f)
        at = a
        if cls == "l4_plus1" and len(f) >= a + 1:
            at = a + 1
        elif cls == "l4_plus3" and len(f) >= a + 3:
            at = a + 3
        elif cls == "tcp_opts" and proto == 6 and len(f) > 14 + hl + 12:
            at = max(a, 14 + hl + 4 * (f[14 + hl + 12] >> 4))
        elif cls == "whole" and len(f) <= min(stride, MAX_SPLIT_HEADER):
            at = len(f)
        elif cls == "short4":
            at = a - 4
        out.append(max(0, min(at, len(f), stride)))
    return out


def layout_ok(f, H, stride):
    """The layout rule: True when the header-split fill must treat the L-byte frame `f`, whose
    first H bytes lie in the slot, exactly as the linear fill does; False = status 9."""
    L = len(f)
    if H > min(stride, MAX_SPLIT_HEADER):
        return False
    if L < 14:
        return True                                  # NOT_IP4 by length alone
    if H < 14:
        return False
    if _be16(f, 12) != 0x0800:
        return True                                  # NOT_IP4
    plen = L - 14
    if plen < 20:
        return True                                  # IP malformed by length alone
    if H < 34:
        return False
    vihl = f[14]
    hl = 20 if vihl == 0x45 else (vihl & 0xF) * 4
    tot = _be16(f, 16)
    if (vihl >> 4) != 4 or hl < 20 or hl > plen or tot < hl or tot > plen:
        return True                                  # IP malformed
    if H < 14 + hl:
        return False
    if _be16(f, 20) & 0x3FFF:
        return True                                  # fragment: IPv4 field only
    proto, dlen, dg = f[23], tot - hl, 14 + hl
    if proto == 6:
        if dlen < 20:
            return True
        fixed, cover = 20, dlen
    elif proto == 17:
        if dlen < 8:
            return True
        if H < dg + 8:
            return False
        ulen = _be16(f, dg + 4)
        if ulen < 8 or ulen > dlen:
            return True
        fixed, cover = 8, ulen
    elif proto == 1:
        if dlen < 8:
            return True
        fixed, cover = 8, dlen
    else:
        return True
    if H < dg + fixed:
        return False
    return dg + cover == L                           # no trailing bytes


def expected(oracle, sp):
    """(headers, statuses, linear statuses, in-layout mask) the fill must leave for the
    SplitFrames layout `sp`; also checks that the oracle itself writes nothing past a header
    slot of an in-layout segment (the payload stays as it is)."""
    lin, off = sp.linearise()
    if lin.size == 0:
        lin = np.zeros(1, dtype=np.uint8)
    filled = lin.copy()
    st_lin = oracle.tx_fill_batch(filled, off)
    want_h = sp.headers.copy()
    want_st = np.empty(len(sp.chunks), dtype=np.uint8)
    ok = np.zeros(len(sp.chunks), dtype=bool)
    o = off.astype(np.int64)
    for i in range(len(sp.chunks)):
        H = int(sp.hdr_lens[i])
        f = lin[o[i]:o[i + 1]]
        ok[i] = layout_ok(bytes(f), H, sp.hdr_stride)
        if ok[i]:
            want_st[i] = st_lin[i]
            want_h[i * sp.hdr_stride:i * sp.hdr_stride + H] = filled[o[i]:o[i] + H]
            assert np.array_equal(filled[o[i] + H:o[i + 1]], f[H:]), i
        else:
            want_st[i] = SPLIT_LAYOUT
    return want_h, want_st, st_lin, ok


# ---- hand-built exact-length segments ---------------------------------------------------

def _eth():
    return LOCAL_MAC + peer_mac(1) + b"\x08\x00"


def _ip(proto, l4_len, ihl=5, src=None):
    opts = bytes((7 * k + 1) & 0xFF for k in range(4 * (ihl - 5)))
    return struct.pack(">BBHHHBBH4s4s", 0x40 | ihl, 0, 4 * ihl + l4_len, 0x1234, 0x4000, 64,
                       proto, 0xDEAD, src or peer_ip(1), LOCAL_IP) + opts


def tcp_segment(payload, ihl=5, doff=5, window=0x2000):
    """(frame, end of the fixed TCP header, end of the TCP options); fields hold junk"""
    opts = bytes([1]) * (4 * (doff - 5))
    tcp = struct.pack(">HHIIHHHH", 40000, 80, 0x01020304, 0x0A0B0C0D, (doff << 12) | 0x18, window,
                      0xBEEF, 0) + opts + bytes(payload)
    f = _eth() + _ip(6, len(tcp), ihl) + tcp
    return f, 14 + 4 * ihl + 20, 14 + 4 * ihl + 4 * doff


def udp_segment(payload, ihl=5, sport=40001):
    udp = struct.pack(">HHHH", sport, 53, 8 + len(payload), 0xBEEF) + bytes(payload)
    f = _eth() + _ip(17, len(udp), ihl) + udp
    return f, 14 + 4 * ihl + 8


def icmp_zero_segment(nbytes=40):
    """An ICMP datagram of all zero bytes: the sum is 0, the checksum 0xFFFF."""
    f = _eth() + _ip(1, nbytes) + bytes(nbytes)
    return f, 14 + 20 + 8


def tcp_inslot_ffff(payload, in_slot):
    """A TCP segment whose pseudo-header words plus its first `in_slot` L4 bytes (checksum field
    as 0; `in_slot` >= 20, the bytes past 20 taken from `payload`) sum to a nonzero multiple of
    0xFFFF: the seed of the payload pass folds to 0xFFFF. The window field absorbs the rest."""
    f, fixed_end, _ = tcp_segment(payload)
    dg = 34
    l4 = bytearray(f[dg:])
    struct.pack_into(">H", l4, 16, 0)
    struct.pack_into(">H", l4, 14, 0)
    s = be_sum(peer_ip(1)) + be_sum(LOCAL_IP) + 6 + len(l4) + be_sum(bytes(l4[:in_slot]))
    win = (-s) % 0xFFFF or 0xFFFF
    f, _, _ = tcp_segment(payload, window=win)
    l4 = bytearray(f[dg:])
    struct.pack_into(">H", l4, 16, 0)
    s = be_sum(peer_ip(1)) + be_sum(LOCAL_IP) + 6 + len(l4) + be_sum(bytes(l4[:in_slot]))
    assert s > 0 and s % 0xFFFF == 0
    return f, dg + in_slot


def ring_batch(n, seed, payload_len=1460, stride=64):
    """n exact-length TCP segments as a send path lays them out: 54-byte headers in `stride`-byte
    slots, payloads of `payload_len` bytes back to back in one ring; built with numpy.
    Returns (headers (n*stride), hdr_lens, payload, linear frames (n, 54 + payload_len))."""
    rng = np.random.default_rng(seed)
    f, _, _ = tcp_segment(bytes(payload_len))
    hdr = np.tile(np.frombuffer(f[:54], dtype=np.uint8), (n, 1))
    hdr[:, 18:20] = rng.integers(0, 256, (n, 2), dtype=np.uint8)    # IPv4 id
    hdr[:, 26:30] = rng.integers(1, 255, (n, 4), dtype=np.uint8)    # source address
    hdr[:, 34:46] = rng.integers(0, 256, (n, 12), dtype=np.uint8)   # ports, seq, ack
    hdr[:, 48:50] = rng.integers(0, 256, (n, 2), dtype=np.uint8)    # window
    payload = rng.integers(0, 256, n * payload_len, dtype=np.uint8)
    slots = np.full((n, stride), 0xEE, dtype=np.uint8)
    slots[:, :54] = hdr
    linear = np.concatenate([hdr, payload.reshape(n, payload_len)], axis=1)
    return (slots.reshape(-1), np.full(n, 54, dtype=np.uint32), payload,
            np.ascontiguousarray(linear))
