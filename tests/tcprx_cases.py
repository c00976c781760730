"""TEST INFRASTRUCTURE -- shared by test_tcprx_host.py and test_gpu_tcprx.py: the model of the TCP
Rx parse and the frame builders.

The model is a plain Python restatement, written independently of the kernel, of what the
reference does with a TCP datagram whose checksum is good (tcp/IpTcpProto_input.h:68-130):
  1. the six TcpSegMeta fields (:81-90, tcp/TcpMiscUtils.h:40-48);
  2. the data offset bound and the cut between options and data (:103-122);
  3. ParseTcpOptions (tcp/TcpOptions.h:63-125);
  4. find_pcb (tcp/IpTcpProto.h:806-820) over keys ordered by CompareKeys
     (tcp/TcpPcbKey.h:52-86).
Steps 3 and 4 are pinned against the reference's own code by tests/golden/tcp_rx_ref_cases.json
(test_tcprx_host.py). recvIp4Dgram itself needs the whole stack and cannot be compiled alone, so
steps 1 and 2 rest on this restatement, and the verdicts on the frame oracle.
"""
import struct

import numpy as np

import frame_cases as F

ACCEPT = 6
DROP_TCP_OFFSET = 11
NO_PCB = 0xFFFFFFFF
OPT_MSS, OPT_WND_SCALE, SEG_VALID = 1, 2, 0x80

LOCAL_IP = 0x0A141E28            # frame_cases.LOCAL_IP
PEER_IP = 0x0A141E64


# ---- step 3: ParseTcpOptions ----------------------------------------------------------------

def parse_options(buf, trace=None):
    """(flags, mss, wnd_scale) as ParseTcpOptions leaves them for the option bytes `buf` (mss and
    wnd_scale 0 unless set). `trace`: a list that receives the name of every branch taken."""
    note = trace.append if trace is not None else (lambda s: None)
    flags = mss = ws = 0
    pos, n = 0, len(buf)
    while pos < n:                                     # while (buf.tot_len > 0), :68
        kind = buf[pos]
        pos += 1
        if kind == 0:                                  # End, :73
            note("end")
            break
        if kind == 1:                                  # Nop, :76
            note("nop")
            continue
        if pos == n:                                   # no length byte, :81
            note("no_length_byte")
            break
        length = buf[pos]
        pos += 1
        if length < 2:                                 # :87
            note("length_below_2")
            break
        dlen = length - 2
        if n - pos < dlen:                             # :91
            note("length_beyond")
            break
        if kind == 2 and dlen == 2:                    # MSS, :98-106
            note("mss_again" if flags & OPT_MSS else "mss")
            flags |= OPT_MSS
            mss = buf[pos] << 8 | buf[pos + 1]
        elif kind == 3 and dlen == 1:                  # WndScale, :109-116
            note("wnd_scale_again" if flags & OPT_WND_SCALE else "wnd_scale")
            flags |= OPT_WND_SCALE
            ws = buf[pos]
        elif kind == 2:
            note("mss_bad_length")                     # goto skip_option, :99
        elif kind == 3:
            note("wnd_scale_bad_length")               # :110
        else:
            note("unknown")                            # default, :120
        pos += dlen
    return flags, mss, ws


STOP_SKIP_BRANCHES = ("end", "nop", "no_length_byte", "length_below_2", "length_beyond",
                      "mss_bad_length", "wnd_scale_bad_length", "unknown", "mss_again",
                      "wnd_scale_again")


# ---- step 4: CompareKeys and find_pcb ------------------------------------------------------

def compare_keys(a, b):
    """CompareKeys of (local_addr, remote_addr, local_port, remote_port) tuples, and the field
    that decided (None when equal)."""
    for f, name in ((3, "remote_port"), (1, "remote_addr"), (2, "local_port"), (0, "local_addr")):
        if a[f] < b[f]:
            return -1, name
        if a[f] > b[f]:
            return 1, name
    return 0, None


def sort_order(k):
    return (k[3], k[1], k[2], k[0])


def model_sort(keys):
    """A TCP_PCB_KEY_DTYPE array in the table's order."""
    idx = sorted(range(len(keys)), key=lambda i: sort_order(
        (int(keys["local_addr"][i]), int(keys["remote_addr"][i]), int(keys["local_port"][i]),
         int(keys["remote_port"][i]))))
    return keys[idx]


def table(entries, dtype):
    """[(local_addr, remote_addr, local_port, remote_port, cookie)] -> array (unsorted)."""
    t = np.zeros(len(entries), dtype=dtype)
    for i, (la, ra, lp, rp, ck) in enumerate(entries):
        t[i] = (la, ra, lp, rp, ck)
    return t


# ---- steps 1 and 2: the record of one frame ---------------------------------------------------

def model_frame(frame, verdict):
    """(verdict, record as a dict or None, key or None) of one frame with Rx verify's verdict."""
    if verdict != ACCEPT or frame[23] != 6:
        return verdict, None, None
    hl = (frame[14] & 0xF) * 4
    total, = struct.unpack_from(">H", frame, 16)
    dgram = total - hl                                     # dgram.tot_len
    T = 14 + hl
    sport, dport, seq, ack, flags, window = struct.unpack_from(">HHIIHH", frame, T)
    data_offset = (flags >> 12) * 4                         # :108
    if data_offset < 20 or data_offset - 20 > dgram - 20:   # opts_len > tcp_data.tot_len, :114
        return DROP_TCP_OFFSET, None, None
    src, dst = struct.unpack_from(">II", frame, 26)
    fl, mss, ws = parse_options(frame[T + 20:T + data_offset])
    rec = dict(remote_addr=src, local_addr=dst, remote_port=sport, local_port=dport, seq_num=seq,
               ack_num=ack, flags=flags, window_size=window, data_off=T + data_offset,
               data_len=dgram - data_offset, mss=mss, wnd_scale=ws, opts=fl | SEG_VALID)
    return verdict, rec, (dst, src, dport, sport)


class Expected:
    """verdict (uint8), segs (seg dtype), pcb (uint32)."""


def expected(frames, verdicts, tbl, seg_dtype):
    """What tcp_rx_parse must leave for `frames` (list of bytes) whose Rx verify verdicts are
    `verdicts`, with the (sorted or not: a dict lookup) table `tbl`."""
    lookup = {}
    if tbl is not None:
        for e in tbl:
            lookup[(int(e["local_addr"]), int(e["remote_addr"]), int(e["local_port"]),
                    int(e["remote_port"]))] = int(e["cookie"])
    e = Expected()
    n = len(frames)
    e.verdict = np.array(verdicts, dtype=np.uint8).copy()
    e.segs = np.zeros(n, dtype=seg_dtype)
    e.pcb = np.full(n, NO_PCB, dtype=np.uint32)
    for i, f in enumerate(frames):
        v, rec, key = model_frame(f, int(verdicts[i]))
        e.verdict[i] = v
        if rec is not None:
            for k, val in rec.items():
                e.segs[k][i] = val
            e.pcb[i] = lookup.get(key, NO_PCB)
    return e


# ---- frame builders ---------------------------------------------------------------------------

def tcp_frame(*, src=PEER_IP, dst=LOCAL_IP, sport=40000, dport=80, seq=0x01020304,
              ack=0x0A0B0C0D, flags=0x010, window=0x2000, ihl=5, doff=5, opts=None, payload=b"",
              trailing=b"", pad60=False, dgram_len=None):
    """An Ethernet + IPv4 + TCP frame with both checksum fields 0 (fill() writes them). `doff`
    is the header's data offset field, whatever follows the 20 header bytes: `opts` (default:
    Nops up to the offset, when it is 5 or more) then `payload`. IPv4 options are Nops.
    `dgram_len` overrides the datagram length the IPv4 total length announces."""
    if opts is None:
        opts = bytes([1]) * (4 * (doff - 5)) if doff > 5 else b""
    tcp = struct.pack(">HHIIHHHH", sport, dport, seq, ack, (doff << 12) | (flags & 0xFFF), window,
                      0, 0) + opts + payload
    dl = len(tcp) if dgram_len is None else dgram_len
    ip = struct.pack(">BBHHHBBHII", 0x40 | ihl, 0, 4 * ihl + dl, 0x4242, 0x4000, 64, 6, 0, src,
                     dst) + bytes([1]) * (4 * (ihl - 5))
    f = F.LOCAL_MAC + F.peer_mac(0) + b"\x08\x00" + ip + tcp + trailing
    if pad60 and len(f) < 60:
        f += bytes([0x5A]) * (60 - len(f))
    return f


def fill(oracle, frames):
    """The frames with valid checksums: the frame oracle's Tx fill. Returns (list of bytes,
    the oracle's Rx verify verdicts)."""
    buf, off = F.pack(frames)
    oracle.tx_fill_batch(buf, off)
    v = oracle.rx_verify_batch(buf, off)
    o = off.astype(np.int64)
    return [buf[o[i]:o[i + 1]].tobytes() for i in range(len(frames))], v


def key_of(frame):
    """The lookup tuple (local_addr, remote_addr, local_port, remote_port) of a TCP frame."""
    T = 14 + (frame[14] & 0xF) * 4
    src, dst = struct.unpack_from(">II", frame, 26)
    sport, dport = struct.unpack_from(">HH", frame, T)
    return dst, src, dport, sport


# ---- frame sets (unfilled; fill() gives them valid checksums) ---------------------------------

def _payload(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def geometry_frames():
    """Every IHL 5-15 x every data offset 5-15, with 0, 1 and 1460 data bytes; the options are
    Nops with an MSS option as the last four bytes (IHL 15, offset 15: it ends at header byte
    133)."""
    out = []
    for ihl in range(5, 16):
        for doff in range(5, 16):
            opts = bytes([1]) * (4 * (doff - 5))
            if doff > 5:
                opts = opts[:-4] + struct.pack(">BBH", 2, 4, 500 + ihl * 16 + doff)
            for dl in (0, 1, 1460):
                out.append(tcp_frame(ihl=ihl, doff=doff, opts=opts, payload=_payload(dl, ihl * 16 + doff),
                                     sport=1000 + len(out), seq=0x80000000 + len(out), pad60=True))
    return out


def padding_frames():
    """60-byte frames whose IPv4 total length is 40 (20 padding bytes that are not data), and
    frames with 1-17 trailing bytes after 0, 1 or 7 data bytes."""
    out = [tcp_frame(pad60=True, sport=2000 + j, flags=f) for j, f in enumerate((0x010, 0x002, 0x011))]
    for t in range(1, 18):
        out.append(tcp_frame(payload=_payload((0, 1, 7)[t % 3], t), trailing=bytes([0xEE]) * t,
                             sport=2100 + t))
        out.append(tcp_frame(doff=7, payload=_payload(100 + t, t), trailing=bytes([0xEE]) * t,
                             sport=2200 + t))
    return out


def bad_offset_frames():
    """[(frame, valid)]: data offset 0-4; 4*offset = datagram length + 4 (dropped), and
    4*offset = datagram length (valid, no data), for offsets 6-15 and IHL 5 and 7."""
    out = []
    for doff in range(0, 5):
        for dl in (0, 33):
            out.append((tcp_frame(doff=doff, payload=_payload(dl, doff), sport=3000 + doff), False))
    for ihl in (5, 7):
        for doff in range(6, 16):
            nops = bytes([1]) * (4 * doff - 20)
            out.append((tcp_frame(ihl=ihl, doff=doff, opts=nops[:-4], sport=3100 + doff), False))
            out.append((tcp_frame(ihl=ihl, doff=doff, opts=nops, sport=3200 + doff), True))
    return out


def option_frames(option_cases):
    """One frame per option buffer of the fixture: Nops in front (skipped, tcp/TcpOptions.h:76)
    bring it to a whole number of words, so that the record's opts / mss / wnd_scale must be
    the reference's recorded answer for the buffer itself."""
    out = []
    for j, (b, _, _, _) in enumerate(option_cases):
        pad = -len(b) % 4
        opts = bytes([1]) * pad + b
        out.append(tcp_frame(doff=5 + len(opts) // 4, opts=opts, payload=_payload(j % 5, j),
                             sport=1024 + j % 60000, seq=j, ihl=5 + (j % 3 == 0) * (j % 11)))
    return out


def mixed_frames(n=600):
    """frame_cases.frames: every verdict class of Rx verify (already filled and mutated)."""
    return F.frames(seed=20260903, n=n)
