"""TEST INFRASTRUCTURE -- shared by test_stack_tx_ref_host.py and test_gpu_stack_tx_ref.py: the
bursts and datagrams recorded from the reference stack (tests/golden/stack_tx_ref_cases.json) as
batches of tcpseg_cases / ipfrag_cases, with what the reference put on the wire for each.

Only the inputs a caller of ours would have go into a case: the ring range, snd_mss, the push
index, FIN, the sequence number; the template's untouched fields (addresses, ports, ack, window,
ttl, DSCP, the flags / offset word) and ip_id are the first captured packet's. Everything else
of the recorded headers is what the model and the kernels have to reproduce."""
import struct

import numpy as np

import ipfrag_cases as U
import stack_tx_ref as R
import tcpseg_cases as T

_cache = {}


def fixture():
    if "fixture" not in _cache:
        _cache["fixture"] = R.load()
    return _cache["fixture"]


def fnv(data):
    return R.fnv(data)


def _tcp_template(p):
    ip, t = p.ip, p.l4
    return T.template(src=struct.unpack_from(">I", ip, 12)[0], dst=struct.unpack_from(">I", ip, 16)[0],
                      sport=struct.unpack_from(">H", t, 0)[0], dport=struct.unpack_from(">H", t, 2)[0],
                      ack=struct.unpack_from(">I", t, 8)[0], window=struct.unpack_from(">H", t, 14)[0],
                      ttl=ip[8], dscp=ip[1], frag=struct.unpack_from(">H", ip, 6)[0],
                      urgent=struct.unpack_from(">H", t, 18)[0])


def _untouched_tcp(p):
    return p.ip[:2] + p.ip[6:10] + p.ip[12:20] + p.l4[0:4] + p.l4[8:12] + p.l4[14:16] + p.l4[18:20]


def tcp_batch():
    """(Batch, records): one case per recorded burst, in the fixture's order; records[b] is the
    list of captured segments of burst b. The payload buffer holds one image of the ring per
    burst, its stream bytes at their ring positions."""
    if "tcp" in _cache:
        return _cache["tcp"]
    _, tcp, _ = fixture()
    cases, records, parts, base = [], [], [], 0
    for c in tcp:
        for b in c["bursts"]:
            pk = [p for p in b["packets"] if p.kind == "D"]
            assert pk, "a burst without a segment"
            assert all(_untouched_tcp(p) == _untouched_tcp(pk[0]) for p in pk)
            ring = np.zeros(c["ring"], dtype=np.uint8)
            D = b["len0"] + b["len1"]
            data = np.frombuffer(R.stream_bytes(b["start"], D, c["salt"]), dtype=np.uint8)
            assert b["off0"] == b["start"] % c["ring"] or D == 0
            ring[b["off0"]:b["off0"] + b["len0"]] = data[:b["len0"]]
            ring[b["off1"]:b["off1"] + b["len1"]] = data[b["len0"]:]
            cases.append(T.burst((base + b["off0"], b["len0"]), (base + b["off1"], b["len1"]), mss=b["mss"],
                                 seq=b["seq"], psh_offset=b["push"], flags=T.FIN if b["fin"] else 0,
                                 ip_id=struct.unpack_from(">H", pk[0].ip, 4)[0], hdr=_tcp_template(pk[0])))
            records.append(pk)
            parts.append(ring)
            base += ring.size
    _cache["tcp"] = (T.Batch(cases, np.concatenate(parts)), records)
    return _cache["tcp"]


def udp_batch():
    """(Batch, records): one case per recorded datagram; records[d] is the list of its captured
    fragments. Piece 1 lies 7 bytes behind piece 0 in the payload buffer."""
    if "udp" in _cache:
        return _cache["udp"]
    udp, _, _ = fixture()
    cases, records, parts, base = [], [], [], 1
    parts.append(np.zeros(1, dtype=np.uint8))
    for d in udp:
        fr = d["frags"]
        data = np.frombuffer(R.udp_payload(d["len0"] + d["len1"], d["salt"], d["fix"]), dtype=np.uint8)
        o0, o1 = base, base + d["len0"] + 7
        parts += [data[:d["len0"]], np.full(7, 0xEE, dtype=np.uint8), data[d["len0"]:]]
        base = o1 + d["len1"]
        ip = fr[0].ip
        assert ip[6] & 0xDF == 0 and ip[7] == 0, "a first fragment with DF or an offset"
        cases.append(U.dgram((o0, d["len0"]), (o1, d["len1"]), mtu=d["mtu"],
                             ip_id=struct.unpack_from(">H", ip, 4)[0], src=R.LOCAL, dst=d["dst"],
                             sport=d["sport"], dport=d["dport"], ttl=ip[8], dscp=ip[1]))
        records.append(fr)
    _cache["udp"] = (U.Batch(cases, np.concatenate(parts)), records)
    return _cache["udp"]


def flat(records):
    """The recorded packets of all cases in order, and the index of each case's first."""
    index = np.cumsum([0] + [len(r) for r in records])
    return [p for r in records for p in r], index


def chunk_bytes(payload, chunks):
    return b"".join(payload[o:o + l].tobytes() for o, l in chunks)
