"""TEST INFRASTRUCTURE -- the seeded scenarios of test_gpu_rx_loop.py: one mixed batch of frames for
the whole receive loop of INTEGRATION.md section 2 (Rx verify, ARP, UDP demux, ICMP responder, TCP
parse, reassembly, and the two linearise calls that turn the responses into frames of one send
ring), and what the loop must do with it. They need no GPU: test_rx_loop_cases.py runs every seed
with the CPU oracle and checks what the scenarios cover.

The setting (interface, tables, batch size, layout) comes from ``np.random.default_rng(BASE +
seed)``, and the frames from the same generator as it goes on; the second batch of the same
setting that the graph test copies in place (``variant=1``) draws its frames from
``default_rng(BASE + 500 + seed)``. Every frame comes from a builder of an existing case module
(arp_cases / arp_ref, icmp_cases / icmp_ref, udp_rx_cases / udp_rx_ref, tcprx_cases, ipreass_cases,
frame_cases.frames) with every argument that shapes it passed explicitly; every expectation comes
from those modules' models and the CPU oracle, none from the library under test. A scenario never
drops a frame after drawing it.

Not drawn: batches below 1,100 or above 1,400 frames, frames above 1,514 bytes, slot strides
other than 2048, an interface without an address, an MTU of 1500 (every scenario has one echo
request whose reply is TOO_LARGE, which needs a smaller one), listeners of port 0, more than 64
listeners, unsorted tables, handlers that reject (the delivery list is taken as the deliveries),
IPv4 options other than Nops in the crafted frames, VLAN tags, datagrams completed by reassembly
fed back into the demux or the responder (the documents give them to the host), fragment trains
above five fragments, TCP state.
"""
import hashlib
import struct

import numpy as np

import aipstack_amd as A

import arp_cases as AC
import arp_ref as AR
import frame_cases as F
import icmp_cases as IC
import icmp_ref as IR
import ipreass_cases as RC
import tcprx_cases as TC
import udp_rx_cases as UC

BASE = 31000
SEEDS = 12
SLOT = 2048
TILE = 256
KEY, LIS, DGRAM, SEG = A.TCP_PCB_KEY_DTYPE, A.UDP_LISTENER_DTYPE, A.UDP_RX_DGRAM_DTYPE, A.TCP_RX_SEG_DTYPE
AUX_BLOCKS = (-1, 1, 2)

LOCAL = IR.LOCAL
PEERS = tuple(IR.PEER + p for p in range(4))
OTHER_HOST = LOCAL + 1                      # a unicast address of the subnet that is not ours
ALL_ONES = 0xFFFFFFFF

OWNERS = ("ARP", "ICMP_ECHO", "UDP_DELIVER", "UDP_UNREACH", "TCP", "REASS_MEMBER", "HOST", "DROP")
ARP, ICMP_ECHO, UDP_DELIVER, UDP_UNREACH, TCP, REASS_MEMBER, HOST, DROP = range(8)
HOST_SORTS = ("fragment", "too_large", "other_proto", "icmp_type")
RESPONDING = ("arp_req", "echo", "udp_closed", "udp_assoc")     # the kinds that feed a list each
PLACES = (0, 63, 64, 255)                                       # lanes of a tile


# ---- the layouts: balanced over the seeds -------------------------------------------------------

def _layouts():
    """Per seed (slotted, lead, hdr_shift, rec_shift, aux_blocks), drawn once from a seeded
    generator out of lists in which every value stands at least twice: 8 seeds of 12 are CSR, so
    that each lead 0-3 occurs twice."""
    rng = np.random.default_rng(BASE - 1)
    slotted = rng.permutation([False] * 8 + [True] * 4)
    leads = list(rng.permutation([0, 1, 2, 3] * 2))
    hdr = rng.permutation([0, 8] * 6)
    rec = rng.permutation([0, 8] * 6)
    aux = rng.permutation(list(AUX_BLOCKS) * 4)
    return [(bool(slotted[s]), 0 if slotted[s] else int(leads.pop()), int(hdr[s]), int(rec[s]), int(aux[s]))
            for s in range(SEEDS)]


LAYOUTS = _layouts()


class Scenario:
    """seed, n, frames, kinds (what each frame was drawn as); ifc (icmp_cases.iface), arp_ifc
    (arp_cases.iface), assocs / listeners / pcbs (tables, or None); slotted, lead, hdr_shift,
    rec_shift, aux_blocks; verdicts (the oracle's Rx verify); e_arp, e_udp, e_icmp, e_tcp, e_reass
    (the models' Expected objects); owner, host_sort (the dispatch table); wire ({frame: the bytes
    that leave for the wire because of it}); special (None, or (tile, "all" / "none"))."""


# ---- the dispatch table, from the outputs of the calls as the host loop reads them ---------------

def dispatch(frames, verdict, arp_status, icmp_status, delivered, tcp_valid, reass_verdict):
    """(owner, number of stages that claim the frame, host sort or -1) per frame, from what the
    loop of INTEGRATION.md section 2 reads: `verdict` Rx verify's, `arp_status` and `icmp_status`
    the two responders', `delivered` a bool per frame (it stands in the delivery list), `tcp_valid`
    a bool per frame (AIPSTACK_TCP_SEG_VALID), `reass_verdict` the reassembly's verdicts. The same
    function reads the models' outputs (the dispatch table) and the device's (the partition)."""
    n = len(frames)
    claims = np.stack([np.asarray(arp_status) != AC.NONE, np.asarray(icmp_status) == IC.ECHO_REPLY,
                       np.asarray(delivered, dtype=bool), np.asarray(icmp_status) == IC.UNREACH,
                       np.asarray(tcp_valid, dtype=bool), np.asarray(reass_verdict) == RC.MEMBER])
    count = claims.sum(axis=0)
    owner = np.full(n, DROP, dtype=np.int8)
    host_sort = np.full(n, -1, dtype=np.int8)
    for i in range(n):
        if count[i]:
            owner[i] = int(np.argmax(claims[:, i]))
            continue
        f = frames[i]
        if reass_verdict[i] == RC.FRAGMENT:
            host_sort[i] = 0
        elif icmp_status[i] == IC.TOO_LARGE:
            host_sort[i] = 1
        elif verdict[i] == RC.OTHER:
            host_sort[i] = 2
        elif verdict[i] == RC.ACCEPT and f[23] == 1 and f[14 + (f[14] & 0xF) * 4] != 8:
            host_sort[i] = 3
        if host_sort[i] >= 0:
            owner[i] = HOST
    return owner, count, host_sort


def verdicts_agree(verdict, icmp, udp, tcp, reass):
    """The five verdict arrays are equal element for element but for the rewrites chksum.h
    documents: 11 from tcp_rx_parse where Rx verify gives 6, and 14 / 15 from ip4_rx_reassemble
    where it gives 3. Returns how many rewrites there were."""
    verdict = np.asarray(verdict)
    assert np.array_equal(icmp, verdict) and np.array_equal(udp, verdict)
    t = np.asarray(tcp) != verdict
    assert (np.asarray(tcp)[t] == TC.DROP_TCP_OFFSET).all() and (verdict[t] == TC.ACCEPT).all()
    r = np.asarray(reass) != verdict
    assert np.isin(np.asarray(reass)[r], (RC.MEMBER, RC.DROP_FRAG)).all() and (verdict[r] == RC.FRAGMENT).all()
    return int(t.sum()), int(r.sum())


def delivered_mask(deliver_frame, count, n):
    m = np.zeros(n, dtype=bool)
    m[np.asarray(deliver_frame[:int(count)], dtype=np.int64)] = True
    return m


def send_ring(sc, slot=SLOT, poison=0xC3):
    """The expected send ring: slot i holds frame i's response from its first byte, every other
    byte is `poison`; and the frame lengths."""
    ring = np.full((sc.n, slot), poison, dtype=np.uint8)
    lens = np.zeros(sc.n, dtype=np.uint32)
    for i, w in sc.wire.items():
        ring[i, :len(w)] = np.frombuffer(w, dtype=np.uint8)
        lens[i] = len(w)
    return ring, lens


def digest(frames):
    h = hashlib.sha256()
    for f in frames:
        h.update(struct.pack("<I", len(f)) + f)
    return h.hexdigest()


# ---- the frames -----------------------------------------------------------------------------------

def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _bad_ip(frame):
    f = bytearray(frame)
    f[24] ^= 0x40
    return bytes(f)


class _Builder:
    """The frame builders of one scenario; every one takes the frame's running number k."""

    def __init__(self, rng, sc, lis_ports):
        self.rng, self.sc, self.lis_ports = rng, sc, lis_ports
        self.tcp_at = []          # (unfilled TCP frames get their checksums from the oracle's fill)
        self.ident = 0x3000

    def peer(self, k):
        p = k % 4
        return PEERS[p], F.peer_mac(p)

    def echo_frame(self, k, *, dst=LOCAL, bad=False, ihl=5, n=None, src=None):
        rng = self.rng
        ip, mac = self.peer(k)
        n = int(rng.choice([0, 1, 2, 17, 18, 56, 301])) if n is None else n
        data = _bytes(rng, n)
        rest = struct.pack(">HH", int(rng.integers(0, 65536)), k & 0xFFFF)
        pkt = IR.ip_packet(1, IR.icmp(8, 0, rest, data, bad=bad), src=ip if src is None else src, dst=dst,
                           ihl=ihl, flags_off=0, ident=k & 0xFFFF, ttl=61, trailing=b"")
        return IC.eth(pkt, src_mac=mac, pad60=bool(k & 1))

    def udp_frame(self, k, dport, *, dst=LOCAL, chk="good", src=None, sport=UC.R.SPORT, ihl=5):
        ip, mac = self.peer(k)
        data = IR.pattern(int(self.rng.choice([0, 1, 3, 18, 19, 200])), k & 0xFF)
        pkt = UC.R.packet(data, src=ip if src is None else src, dst=dst, ihl=ihl, ttl=61, sport=sport,
                          dport=dport, chk=chk, udp_len=None, extra=b"")
        return IC.eth(pkt, src_mac=mac, pad60=bool(k & 2))

    def tcp_frame(self, k, key, *, doff=5):
        la, ra, lp, rp = key
        return TC.tcp_frame(src=ra, dst=la, sport=rp, dport=lp, seq=k, ack=0x0A0B0C0D, flags=0x010,
                            window=0x2000, ihl=5, doff=doff, opts=None,
                            payload=_bytes(self.rng, int(self.rng.choice([0, 1, 40, 700]))), trailing=b"",
                            pad60=True, dgram_len=None)

    def train(self, k, complete):
        """[frames] of one UDP or protocol-47 datagram cut into 2-5 fragments; incomplete: one
        fragment is left out."""
        rng = self.rng
        ip, _ = self.peer(k)
        self.ident += 1
        pieces_n = int(rng.integers(2, 6))
        body_len = 8 * (pieces_n - 1) * int(rng.integers(1, 30)) + int(rng.integers(1, 40))
        if k % 3:
            proto, body = 17, RC.udp_body(ip, LOCAL, 7, 5000, _bytes(rng, body_len), ulen=None, chk=None)
        else:
            proto, body = 47, _bytes(rng, body_len + 8)
        step = (len(body) - 1) // pieces_n // 8 * 8 or 8
        cuts = [step * j for j in range(1, pieces_n) if step * j < len(body)]
        pieces = RC.cut(body, cuts)
        if not complete:
            del pieces[int(rng.integers(0, len(pieces)))]
        return RC.frag_frames(ip, LOCAL, self.ident, proto, pieces, ihl=5, ttl=64, pad=0, total=None)

    def build(self, kind, k):
        """[frames] of one drawn kind."""
        rng, sc = self.rng, self.sc
        ip, mac = self.peer(k)
        if kind == "arp_req":
            return [AC.request(k, sc.arp_ifc, pad=(0, 18)[k & 1])]
        if kind == "arp_other":
            return [AC.other(k, sc.arp_ifc)]
        if kind == "arp_bad":
            full = AR.arp(1, ip, LOCAL, sha=mac, tha=bytes(6), eth_src=mac, eth_dst=AR.BCAST_MAC,
                          ethertype=0x0806, hwtype=1, ptype=0x0800, hlen=6 + (k % 3 == 1), plen=4 + (k % 3 == 2),
                          pad=0)
            return [full[:41] if k % 3 == 0 else full]
        if kind == "echo":
            return [self.echo_frame(k)]
        if kind == "echo_bcast":
            return [self.echo_frame(k, dst=(sc.ifc["bcast"], ALL_ONES)[k & 1])]
        if kind == "echo_bad":
            return [self.echo_frame(k, bad=True)]
        if kind == "echo_opts":
            return [self.echo_frame(k, ihl=6 + k % 10)]
        if kind == "echo_big":
            return [self.echo_frame(k, n=sc.ifc["mtu"] - 27)]
        if kind == "icmp_other":
            pkt = IR.ip_packet(1, IR.icmp((0, 3, 13, 11)[k % 4], k % 5, _bytes(rng, 4), _bytes(rng, 8 + k % 30),
                                          bad=False), src=ip, dst=LOCAL, ihl=5, flags_off=0, ident=k & 0xFFFF,
                               ttl=61, trailing=b"")
            return [IC.eth(pkt, src_mac=mac, pad60=True)]
        if kind == "udp_assoc":
            la, ra, lp, rp = self.assoc_keys[k % len(self.assoc_keys)]
            return [self.udp_frame(k, lp, dst=la, src=ra, sport=rp)]
        if kind == "udp_lis":
            return [self.udp_frame(k, self.lis_ports[k % len(self.lis_ports)])]
        if kind == "udp_closed":
            return [self.udp_frame(k, 9000 + k % 500, ihl=5 + (k % 7 == 0) * (k % 10))]
        if kind == "udp_bcast":
            return [self.udp_frame(k, 9000 + k % 500, dst=(sc.ifc["bcast"], ALL_ONES)[k & 1])]
        if kind == "udp_zero":
            port = (9000 + k % 500, self.lis_ports[k % len(self.lis_ports)])[k & 1]
            return [self.udp_frame(k, port, chk="zero")]
        if kind == "udp_bad":
            return [self.udp_frame(k, self.lis_ports[k % len(self.lis_ports)], chk="bad")]
        if kind in ("tcp_pcb", "tcp_none", "tcp_badoff"):
            key = self.pcb_keys[k % len(self.pcb_keys)]
            if kind == "tcp_none":
                key = (key[0], key[1], key[2], key[3] + 1000)
            self.tcp_at.append(k)
            return [self.tcp_frame(k, key, doff=(5, 6, 8)[k % 3] if kind != "tcp_badoff" else k % 5)]
        if kind == "train":
            return self.train(k, True)
        if kind == "train_cut":
            return self.train(k, False)
        if kind == "lone_frag":
            self.ident += 1
            return RC.frag_frames(ip, LOCAL, self.ident, 17, [(8 * (1 + k % 50), _bytes(rng, 24), bool(k & 1))],
                                  ihl=5, ttl=64, pad=0, total=None)
        if kind == "other_proto":
            pkt = IR.ip_packet((47, 50, 132)[k % 3], _bytes(rng, k % 40), src=ip, dst=LOCAL, ihl=5, flags_off=0,
                               ident=k & 0xFFFF, ttl=61, trailing=b"")
            return [IC.eth(pkt, src_mac=mac, pad60=bool(k & 1))]
        if kind == "bad_ip":
            return [_bad_ip(self.echo_frame(k) if k & 1 else self.udp_frame(k, 5000))]
        if kind == "runt":
            return [(F.LOCAL_MAC + mac + b"\x08\x00")[:1 + k % 13]]
        assert kind == "empty"
        return [b""]


# frames of each kind per 1,000 frames of the pool (a train counts once here), and the least number
GENERAL = (("arp_req", 35, 8), ("arp_other", 30, 8), ("arp_bad", 30, 8), ("echo", 45, 10), ("echo_bcast", 15, 4),
           ("echo_bad", 15, 4), ("echo_opts", 15, 4), ("echo_big", 2, 1), ("icmp_other", 25, 6),
           ("udp_assoc", 50, 25), ("udp_lis", 45, 10), ("udp_closed", 45, 22), ("udp_bcast", 25, 6),
           ("udp_zero", 15, 4), ("udp_bad", 15, 4), ("tcp_pcb", 35, 14), ("tcp_none", 25, 10),
           ("tcp_badoff", 25, 8), ("train", 20, 10), ("train_cut", 12, 6), ("lone_frag", 12, 4),
           ("other_proto", 25, 6), ("bad_ip", 25, 6), ("runt", 15, 4), ("empty", 4, 1))
ALL_RESPOND = ("arp_req", "echo", "udp_closed", "echo_opts")
NONE_RESPOND = ("arp_other", "arp_bad", "udp_assoc", "tcp_pcb", "other_proto", "bad_ip", "icmp_other",
                "echo_bad", "runt", "lone_frag")


def _setting(rng, seed, sc):
    sc.seed = seed
    sc.n = int(rng.integers(1100, 1401))
    sc.slotted, sc.lead, sc.hdr_shift, sc.rec_shift, sc.aux_blocks = LAYOUTS[seed]
    prefix = int(rng.choice([16, 24]))
    bcast = LOCAL | (ALL_ONES >> prefix)
    mac = bytes([2 * int(rng.integers(0, 128))]) + _bytes(rng, 5)
    ip_id = 0x10000 - int(rng.integers(1, 200)) if seed % 3 == 0 else int(rng.integers(0, 65536))
    sc.prefix = prefix
    sc.ifc = IC.iface(local=LOCAL, bcast=bcast, mtu=int(rng.choice([576, 1006, 1400])), ip_id=ip_id,
                      ttl=int(rng.integers(1, 256)), allow=bool(rng.integers(0, 2)), mac=mac)
    sc.arp_ifc = AC.iface(local=LOCAL, prefix=prefix, have=True, mac=mac)
    # the tables
    assoc_keys = [(LOCAL, PEERS[j % 4], 6000 + j, 30000 + j) for j in range(6)]
    sc.assocs = UC.assocs([k + (False, 100 + j) for j, k in enumerate(assoc_keys)], KEY)
    n_lis = (0, 1, 3, 8, 33, 64)[seed % 6]
    rows = []
    for j in range(n_lis):
        r = rng.random()
        rows.append((0 if r < 0.7 else LOCAL if r < 0.9 else OTHER_HOST, 5000 + j // 3,
                     bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), int(rng.integers(0, 1 << 32))))
    sc.listeners = UC.listeners(rows, LIS, dirty=False) if rows else None
    lis_ports = [5000 + j for j in range(max(1, (n_lis + 2) // 3))]
    pcb_keys = [(LOCAL, PEERS[j % 4], 80 + j, 40000 + j) for j in range(8)]
    sc.pcbs = TC.model_sort(TC.table([k + (500 + j,) for j, k in enumerate(pcb_keys)], KEY))
    return assoc_keys, pcb_keys, lis_ports


def scenario(oracle, seed, variant=0):
    """One interface and one batch of 1,100 to 1,400 frames (module docstring: what is drawn and
    what is not). Frames of each responding kind (a request for the interface's address, an echo
    request, a datagram to a closed port, a datagram for an association) stand at lanes 0, 63, 64
    and 255 of a tile of their own, and one of them, by the seed, at the batch's last index; seeds
    that are 1 mod 3 have a tile whose frames all respond, seeds that are 2 mod 3 one in which none
    does. `variant` 1: other frames in the same setting and layout."""
    rng = np.random.default_rng(BASE + seed)
    sc = Scenario()
    assoc_keys, pcb_keys, lis_ports = _setting(rng, seed, sc)
    if variant:
        rng = np.random.default_rng(BASE + 500 * variant + seed)
    n = sc.n
    b = _Builder(rng, sc, lis_ports)
    b.assoc_keys, b.pcb_keys = assoc_keys, pcb_keys
    # the places that are fixed: index -> kind
    fixed = {}
    sc.special = None
    if seed % 3:
        tile = (seed % 4) if seed % 3 == 1 else (3 + seed) % 4
        pool = ALL_RESPOND if seed % 3 == 1 else NONE_RESPOND
        sc.special = (tile, "all" if seed % 3 == 1 else "none")
        for i in range(tile * TILE, (tile + 1) * TILE):
            fixed[i] = pool[int(rng.integers(0, len(pool)))]
    for j, kind in enumerate(RESPONDING):
        tile = (j + seed) % 4
        for lane in PLACES:
            fixed[tile * TILE + lane] = kind
    fixed[n - 1] = RESPONDING[seed % 4]
    # the pool: every other frame, in a seeded order
    room = n - len(fixed)
    kinds = []
    for kind, per_thousand, least in GENERAL:
        kinds += [kind] * max(least, room * per_thousand // 1000)
    kinds = [kinds[int(j)] for j in rng.permutation(len(kinds))]
    pool, pool_kinds, k = [], [], 0
    for kind in kinds:
        for f in b.build(kind, k):
            pool.append(f)
            pool_kinds.append(kind)
        k += 1
    rest = room - len(pool)
    assert rest >= 50, rest
    pool += F.frames(seed=BASE + 500 * variant + seed, n=rest)
    pool_kinds += ["frame_cases"] * rest
    order = rng.permutation(room)
    frames, sc.kinds, at = [], [], 0
    for i in range(n):
        if i in fixed:
            got = b.build(fixed[i], k)
            assert len(got) == 1
            frames.append(got[0])
            sc.kinds.append(fixed[i])
            k += 1
        else:
            frames.append(pool[int(order[at])])
            sc.kinds.append(pool_kinds[int(order[at])])
            at += 1
    assert at == room and len(frames) == n
    # the crafted TCP frames get their checksums from the oracle's Tx fill
    tcp_idx = [i for i, kd in enumerate(sc.kinds) if kd.startswith("tcp_")]
    filled, _ = TC.fill(oracle, [frames[i] for i in tcp_idx])
    for i, f in zip(tcp_idx, filled):
        frames[i] = f
    sc.frames = frames
    _expect(oracle, sc)
    return sc


def _expect(oracle, sc):
    """The models' answers and the dispatch table."""
    frames, n = sc.frames, sc.n
    buf, off = F.pack(frames)
    sc.verdicts = oracle.rx_verify_batch(buf, off)
    sc.e_arp = AC.respond(frames, sc.arp_ifc)
    sc.e_udp = UC.expected(frames, sc.verdicts, sc.ifc, sc.assocs, sc.listeners, DGRAM)
    sc.codes = [int(c) for c in sc.e_udp.unreach]
    sc.e_icmp = IC.respond(frames, sc.verdicts, sc.codes, sc.ifc)
    sc.e_tcp = TC.expected(frames, sc.verdicts, sc.pcbs, SEG)
    sc.e_reass = RC.model(oracle, RC.Batch(frames), RC.MAX_REASS)
    sc.owner, sc.claims, sc.host_sort = dispatch(
        frames, sc.verdicts, sc.e_arp.status, sc.e_icmp.status,
        delivered_mask(sc.e_udp.deliver_frame, sc.e_udp.counts[0], n),
        (sc.e_tcp.segs["opts"] & TC.SEG_VALID) != 0, sc.e_reass.verdict)
    sc.wire = {}
    for i, h in sc.e_arp.headers.items():
        sc.wire[i] = h
    for i, h in sc.e_icmp.headers.items():
        assert i not in sc.wire
        sc.wire[i] = h[:14] + IC.response_packet(sc.e_icmp, frames, i)
    sc.responds = np.zeros(n, dtype=bool)
    sc.responds[list(sc.wire)] = True


_cache = {}


def cached(oracle, seed, variant=0):
    """scenario(), computed once per process and left unchanged."""
    if (seed, variant) not in _cache:
        _cache[(seed, variant)] = scenario(oracle, seed, variant)
    return _cache[(seed, variant)]


# ---- the sessions recorded from the reference (tests/golden/rx_loop_ref_cases.json) ---------------

def session_cuts(s):
    """The session as two or three batches cut at seeded places: [(start, end)]."""
    rng = np.random.default_rng(BASE + 900 + s["seed"])
    n = len(s["frames"])
    at = sorted(int(x) for x in rng.choice(np.arange(40, n - 40), 2 + s["seed"] % 2, replace=False))
    return list(zip([0] + at, at + [n]))


def session_batch(oracle, s, start, end, ip_id, slotted):
    """Frames [start, end) of a session as a Scenario whose interface starts at the Ident `ip_id`,
    with the models' answers; the layout follows the session's seed."""
    import udp_rx_ref as UR
    sc = Scenario()
    sc.seed, sc.n, sc.special = s["seed"], end - start, None
    sc.frames = [bytes.fromhex(row[0]) for row in s["frames"][start:end]]
    sc.kinds = ["session"] * sc.n
    sc.slotted, sc.lead, sc.aux_blocks = slotted, s["seed"] % 4, AUX_BLOCKS[s["seed"] % 3]
    sc.hdr_shift, sc.rec_shift = 8 * (s["seed"] & 1), 8 * (s["seed"] >> 1 & 1)
    sc.prefix = s["prefix"]
    mac = bytes.fromhex(s["mac"])
    sc.ifc = IC.iface(local=s["addr"], bcast=s["addr"] | (ALL_ONES >> s["prefix"]), mtu=1500, ip_id=ip_id,
                      ttl=64, allow=bool(s["allow"]), mac=mac)
    sc.arp_ifc = AC.iface(local=s["addr"], prefix=s["prefix"], have=True, mac=mac)
    sc.assocs = UC.assocs([tuple(r) + (k,) for k, r in enumerate(s["assocs"])], KEY)
    sc.listeners = UC.listeners([tuple(r) + (k,) for k, r in UR.listener_table(s)], LIS)
    sc.pcbs = None
    _expect(oracle, sc)
    return sc


def session_sent(s, start, end):
    """{frame of the batch: the one frame the reference sent because of it}."""
    out = {}
    for i, row in enumerate(s["frames"][start:end]):
        assert len(row[1]) <= 1
        if row[1]:
            out[i] = bytes.fromhex(row[1][0])
    return out


def calls_of(dgram, listeners):
    """The handler calls one demux record stands for, as the fixture writes them: the association
    first, then the listeners in table order (the order the reference walks them in)."""
    if not dgram["flags"] & UC.VALID:
        return []
    out = []
    if dgram["assoc"] != UC.NO_ASSOC:
        out.append("A%d %d" % (int(dgram["assoc"]), int(dgram["data_len"])))
    for k in range(len(listeners)):
        if (int(dgram["listeners"]) >> k) & 1:
            out.append("L%d %d" % (int(listeners["cookie"][k]), int(dgram["data_len"])))
    return out


def session_calls_match(s, start, sc, dgrams, deliver_frame, count):
    """The delivery list and the records (the models' or the device's) name exactly the handler
    calls the reference made for frames [start, start + n) of the session; returns how many."""
    delivered = delivered_mask(deliver_frame, count, sc.n)
    calls = 0
    for i in range(sc.n):
        want = s["frames"][start + i][2]
        got = calls_of(dgrams[i], sc.listeners) if delivered[i] else []
        assert got == want, (start + i, got, want)
        calls += len(want)
    return calls
