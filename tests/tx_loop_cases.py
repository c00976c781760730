"""TEST INFRASTRUCTURE -- shared by test_tx_loop_cases.py and test_gpu_tx_loop.py: the whole send
loop of INTEGRATION.md ("Tx resolve: route and next-hop MAC between the producers and the
lineariser") played by a host that knows nothing but what the calls return.

Part 1, play(): the command sequences of tests/golden/tx_resolve_ref_cases.json, recorded from the
reference's own IpStack and EthIpIface, in batches. A maximal run of sends is one tx_resolve batch
against the sorted snapshot of the keeper's tables; a maximal run of injected frames is one
arp_rx_respond batch per interface. Between the calls the host (the same code for every backend)
makes one Query entry per distinct new (interface, next hop) of the held list and notes one
request, and folds the ARP records into the keeper (tx_resolve_cases.Keeper.learned). What the
calls return is held to the recording: the IpErr of every send, the frame's 14 bytes, the ARP
requests (the "Q" events) at their first holders, the stack's ARP replies. A backend supplies the
two calls: ModelBackend here (tx_resolve_cases.expected, arp_cases.respond), the device in
test_gpu_tx_loop.py.

Resolving a run of sends against the table at its start differs from the reference's one-by-one
order in one thing only: the second and later holders of a pair that had no entry carry
_ROUTE_NEW_ENTRY too (sequentially they find the Query entry the first one made). The host makes
the entry once per pair, so the requests are the same. test_tx_loop_cases.py asserts that this is
the only difference.
"""
import struct

import numpy as np

import aipstack_amd as A

import arp_cases as AC
import arp_ref as AR
import icmp_cases as IC
import icmp_ref as IR
import ipfrag_cases as IF
import tcp_rsp_cases as TRC
import tcpseg_cases as TS
import tx_resolve_cases as C
import tx_resolve_ref as R

SENTINEL = 0xC3
FRAME_SLOT = 64          # the send ring of part 1: 42-byte frames in 64-byte slots
HEADER = 42              # 8 payload bytes, as the generator sends


# ---- the host between the calls ------------------------------------------------------------------

def snapshot(keeper):
    """The ARP snapshot of the next tx_resolve call: the keeper's entries handed over in the
    wrong order, so that aipstack_arp_table_sort is what orders them."""
    return A.arp_table_sort(keeper.table()[::-1].copy())


def after_resolve(keeper, r):
    """The host's walk over the held list of one tx_resolve call (r: status, routes, held,
    counts): a Query entry and one request per distinct pair that has no entry yet. Returns the
    requests [(interface in table order, target address, first holder)]."""
    requests = []
    for i in r.held[:int(r.counts[0])].tolist():
        route = r.routes[i]
        key = (int(route["iface"]), int(route["next_hop"]))
        if int(route["flags"]) & C.NEW_ENTRY:
            if key not in keeper.entries:
                keeper.entries[key] = (C.QUERY, bytes(6))
                requests.append((key[0], key[1], i))
        assert keeper.entries[key][0] == C.QUERY, key
    return requests


def after_arp(keeper, k, h):
    """The host's walk over the records of one arp_rx_respond call on interface k, in frame
    order."""
    for rec in h.records:
        keeper.learned(k, (int(rec["status"]), int(rec["sender_addr"]), rec["sender_mac"].tobytes(),
                           int(rec["flags"])))


# ---- the model's backend -------------------------------------------------------------------------

def linearised(ring, stride, send_len, slot=FRAME_SLOT):
    """The send ring a lineariser leaves for header-only segments: (frames (n, slot), lens)."""
    n = len(send_len)
    frames = np.full((n, slot), SENTINEL, dtype=np.uint8)
    for i in range(n):
        ln = int(send_len[i])
        frames[i, :ln] = ring[i * stride:i * stride + ln]
    return frames, np.asarray(send_len, dtype=np.uint32).copy()


class ModelBackend:
    """resolve(): tx_resolve_cases.expected plus the send ring (`frames`, `frame_lens`) that
    tx_linearise_slotted makes of it with send_len. arp(): arp_cases.respond plus `sent`, {frame:
    the reply as it leaves through tx_resolve (nothing to resolve) and the lineariser}."""

    def resolve(self, ring, stride, hdr_len, ifaces, table, send_flags, force, seg_status=None, where=0):
        e = C.expected(ring, stride, hdr_len, ifaces, table, seg_status=seg_status, send_flags=send_flags,
                       force=force)
        if seg_status is None:              # part 1: header-only segments, linearised here
            e.frames, e.frame_lens = linearised(e.ring, stride, e.send_len)
        return e

    def arp(self, frames, k, keeper, table, where=0):
        e = AC.respond(frames, keeper.arp_iface(k))
        e.sent = dict(e.headers)
        return e


# ---- part 1: the recorded sequences --------------------------------------------------------------

def batches(stack):
    """[("D", None, [step numbers]) or ("F", interface in table order, [step numbers])]: a
    maximal run of sends is one batch, a maximal run of injected frames one batch per interface,
    order kept."""
    n = len(stack["ifaces"])
    out, at, steps = [], 0, stack["steps"]
    while at < len(steps):
        end = at
        while end < len(steps) and steps[end]["op"] == steps[at]["op"]:
            end += 1
        if steps[at]["op"] == "D":
            out.append(("D", None, list(range(at, end))))
        else:
            for k in sorted({steps[j]["iface"] for j in range(at, end)}):
                out.append(("F", n - 1 - k, [j for j in range(at, end) if steps[j]["iface"] == k]))
        at = end
    return out


class Played:
    """What play() saw: route ({send's step number: its aipstack_tx_route as a numpy record}),
    requests ([(step number of the first holder, interface in table order, target)]), pinned
    (steps held to the recording), q_consumed ("Q" events matched), later_holders (held segments
    with _NEW_ENTRY beyond the first of their pair, per batch), resolved_rounds (resolve batches
    that sent to a pair an earlier batch held), most_entries (the fullest ARP table of one
    interface), n_batches."""

    def __init__(self):
        self.route, self.requests, self.later_holders = {}, [], []
        self.pinned = self.q_consumed = self.resolved_rounds = self.most_entries = self.n_batches = 0


def _events(step):
    sent = [e.split() for e in step["out"] if e.startswith("T ")]
    asked = [e.split() for e in step["out"] if e.startswith("Q ")]
    assert len(sent) + len(asked) == len(step["out"]), step["out"]      # no other kind of event
    return sent, asked


def _pin_sends(name, steps, js, r, requests, ifaces, stride):
    """Every send of one resolve batch against the recording. Returns the "Q" events matched."""
    n, consumed = len(ifaces), 0
    for i, (j, s) in enumerate(zip(js, steps)):
        where = (name, s["name"])
        st = int(r.status[i])
        assert s["err"] == C.IP_ERR[st], where
        sent, asked = _events(s)
        k = int(r.routes[i]["iface"])
        if st == C.SENT:
            assert sent == [["T", str(n - 1 - k), r.ring[i * stride:i * stride + 14].tobytes().hex()]], where
            assert r.frames[i, :14].tobytes() == r.ring[i * stride:i * stride + 14].tobytes(), where
            assert int(r.frame_lens[i]) == HEADER and (r.frames[i, HEADER:] == SENTINEL).all(), where
        else:
            assert not sent, where
            assert int(r.frame_lens[i]) == 0 and (r.frames[i] == SENTINEL).all(), where
        noted = [(q, hop) for q, hop, holder in requests if holder == i]
        recorded = []
        for _, kq, hx in asked:
            q = bytes.fromhex(hx)
            f = ifaces[n - 1 - int(kq)]
            assert q[:6] == b"\xff" * 6 and q[6:12] == f["mac"] and q[12:14] == b"\x08\x06", where
            assert struct.unpack_from(">H", q, 20)[0] == 1 and struct.unpack_from(">I", q, 28)[0] == f["addr"], where
            recorded.append((n - 1 - int(kq), struct.unpack_from(">I", q, 38)[0]))
        assert noted == recorded, (where, noted, recorded)     # a request exactly where one was recorded
        consumed += len(asked)
    return consumed


def _pin_frames(name, steps, k, h, n):
    """Every injected frame of one ARP batch against the recording: the stack's reply, or none."""
    consumed = 0
    for i, s in enumerate(steps):
        sent, asked = _events(s)
        assert not sent, (name, i)
        if i in h.sent:
            assert [(int(kq), bytes.fromhex(hx)) for _, kq, hx in asked] == [(n - 1 - k, h.sent[i])], (name, i)
        else:
            assert not asked, (name, i)
        consumed += len(asked)
    return consumed


def play(stack, backend, stride=64):
    """The stack's steps in batches through `backend`, the host in between, every step held to
    the recording. Returns a Played."""
    ifaces = C.stack_ifaces(stack)
    n = len(ifaces)
    keeper = C.Keeper(ifaces)
    p = Played()
    was_held = set()
    for b, (op, k, js) in enumerate(batches(stack)):
        steps = [stack["steps"][j] for j in js]
        table = snapshot(keeper)
        if op == "D":
            ring, lens = C.ring_of([C.header(s["src"], s["dst"], length=HEADER) for s in steps], stride)
            sf = np.array([s["flags"] for s in steps], dtype=np.uint8)
            force = np.array([C.ROUTE_ANY if s["iface"] < 0 else n - 1 - s["iface"] for s in steps], dtype=np.uint16)
            r = backend.resolve(ring, stride, lens, ifaces, table, sf, force, where=b)
            requests = after_resolve(keeper, r)
            p.q_consumed += _pin_sends(stack["name"], steps, js, r, requests, ifaces, stride)
            new = [i for i in r.held[:int(r.counts[0])].tolist() if int(r.routes[i]["flags"]) & C.NEW_ENTRY]
            p.later_holders.append(len(new) - len(requests))
            pairs = lambda idx: {(int(r.routes[i]["iface"]), int(r.routes[i]["next_hop"])) for i in idx}  # noqa: E731
            sent_to = pairs(i for i in range(len(js)) if r.status[i] == C.SENT)
            p.resolved_rounds += bool(sent_to & was_held)
            was_held |= pairs(r.held[:int(r.counts[0])].tolist())
            for i, j in enumerate(js):
                p.route[j] = r.routes[i].copy()
            p.requests += [(js[holder], q, hop) for q, hop, holder in requests]
        else:
            h = backend.arp([bytes.fromhex(s["in"]) for s in steps], k, keeper, table, where=b)
            after_arp(keeper, k, h)
            p.q_consumed += _pin_frames(stack["name"], steps, k, h, n)
        p.pinned += len(js)
        p.n_batches += 1
        for q in range(n):
            p.most_entries = max(p.most_entries, sum(1 for key in keeper.entries if key[0] == q))
    return p


# ---- part 2: one mixed batch from the real producers, two rounds with a retry ---------------------
#
# Two interfaces: the /24 with a gateway of tx_resolve_cases.LAN, constructed first, and a /16
# without one, constructed second, so the table (the order the stack's list iterates) has the /16
# first. With these two (the gateway lies inside its subnet and has an entry) no route can end in
# _NO_HW_ROUTE: a next hop is the destination inside a subnet, the all-ones address of a named
# interface, or that gateway. The scenario therefore reaches the statuses 41..45 and 47; _NO_ROUTE
# needs a named interface (one burst names the /16 for an outside address), every other segment of
# the producers is routed with _ROUTE_ANY. The answers of icmp_rx_respond and tcp_rx_respond to one
# small batch received on the /24 name that interface; they leave with the interface's own address
# for a unicast peer through an interface that has a gateway, so none of them can fail.

K_B, K_LAN = 0, 1
IFACE_B = C.iface(R.ip(10, 21, 0, 5), 16, None, R.mac_of(1))
IFACES = [IFACE_B, C.LAN[0]]
OWN, OWN_B, GW = C.LAN[0]["addr"], IFACE_B["addr"], C.LAN[0]["gateway"]
PEER_SILENT, PEER_B_VALID, PEER_B_NEW = R.ip(10, 20, 30, 103), R.ip(10, 21, 7, 7), R.ip(10, 21, 9, 9)
SUBNET_BCAST = C.bcast_of(C.LAN[0])
SEEDS = (0, 1, 2)
LAYOUTS = ((64, 0, -1), (128, 2, 1), (64, 4, 2))          # (hdr_stride, ring shift, aux_blocks) per seed
SEND_SLOT = 2048
TILE = 256
ICMP_ID, RST_ID = 0x7000, 0x7100                          # the responders' first Idents
FILL = 0x5E                                               # what the ring holds before the producers run


class Scenario:
    """seed, stride, shift, aux_blocks; tcp / udp (the producers' Batch, index arrays and model
    Expected: *_batch, *_si, *_cb, e_*), rx_frames with e_icmp and e_rst (the batch received on the
    /24 that both responders answer), arp_frames and e_arp (the received ARP batch on the /24 whose
    replies ride along); at (dict: first slot of the "tcp", "icmp", "rst", "arp", "udp" slice), n;
    per slot hdr_len, seg_status, send_flags, force, group (the burst, or 1000 + the datagram, a
    slot belongs to; -1 for ARP, -2 for a responder's answer), body ({slot: the frame's bytes from 14 on by the producers' models}), chunks ({slot: number
    of chunks}); ring (the model's header ring: the models' header bytes over FILL)."""


def start_keeper():
    k = C.Keeper(IFACES)
    k.entries[(K_LAN, C.PEER_SENT)] = (C.VALID, R.peer_mac(C.PEER_SENT))
    k.entries[(K_LAN, C.PEER_QUERY)] = (C.QUERY, bytes(6))
    k.entries[(K_LAN, GW)] = (C.REFRESHING, R.peer_mac(GW))
    k.entries[(K_B, PEER_B_VALID)] = (C.VALID, R.peer_mac(PEER_B_VALID))
    return k


def _tcp_cases(rng):
    """[(burst, force)]: held and failed bursts first, then a seeded mix."""
    def b(src, dst, d, mss, two=False):
        o = int(rng.integers(0, 20000))
        a = int(rng.integers(1, d)) if two and d > 1 else d
        return TS.burst((o, a), (int(rng.integers(30000, 40000)), d - a), mss=mss, seq=int(rng.integers(0, 1 << 32)),
                        psh_offset=d, ip_id=int(rng.integers(0, 1 << 16)), flags=int(rng.integers(0, 2)),
                        hdr=TS.template(src=src, dst=dst, sport=int(rng.integers(1024, 65536))))
    out = [(b(OWN, C.PEER_NEW, 5 * 536 + 77, 536, True), C.ROUTE_ANY),          # held, two-chunk segments
           (b(OWN + 1, C.PEER_SENT, 900, 300), C.ROUTE_ANY),                     # _NONLOCAL_SRC
           (b(OWN_B, R.OUTSIDE + 1, 700, 100), K_B),                             # the /16 has no gateway: _NO_ROUTE
           (b(OWN, PEER_SILENT, 3000, 1460, True), C.ROUTE_ANY)]
    dests = ((OWN, C.PEER_SENT), (OWN, C.PEER_QUERY), (OWN, C.PEER_NEW), (OWN, R.OUTSIDE), (OWN, PEER_SILENT),
             (OWN_B, PEER_B_VALID), (OWN_B, PEER_B_NEW), (OWN, C.PEER_SENT))
    for j in range(100):
        src, dst = dests[j % len(dests)]
        mss = (100, 536, 1460)[j % 3]
        out.append((b(src, dst, min(int(rng.integers(1, 40 * mss)), 24000), mss, j % 2 == 0), C.ROUTE_ANY))
    out.insert(9, (TS.burst((0, 50), mss=0, give=(3, 3)), C.ROUTE_ANY))          # breaks the contract
    return out


def _udp_cases(rng):
    """[(datagram, send_flags)]: a seeded mix, then held and failed datagrams last."""
    def d(dst, size, mtu, src=OWN):
        o = int(rng.integers(0, 30000))
        a = int(rng.integers(0, size + 1))
        return IF.dgram((o, a), (int(rng.integers(40000, 60000)), size - a), mtu=mtu, ip_id=int(rng.integers(0, 1 << 16)),
                        src=src, dst=dst, sport=int(rng.integers(1024, 65536)))
    out = []
    dests = (C.PEER_SENT, C.PEER_NEW, PEER_SILENT, SUBNET_BCAST, SUBNET_BCAST, C.PEER_SENT)
    for j in range(66):
        dst = dests[j % len(dests)]
        mtu = (576, 1500)[j % 2]
        size = int(rng.integers(0, mtu - 28)) if j % 3 == 0 else int(rng.integers(2 * mtu, 6 * mtu))
        out.append((d(dst, size, mtu), C.ALLOW_BROADCAST if j % len(dests) == 3 else 0))
    out.insert(11, (IF.dgram((0, 100), mtu=100, ip_id=999, give=(2, 2)), 0))     # mtu below the minimum
    out += [(d(SUBNET_BCAST, 4000, 1500), 0), (d(PEER_SILENT, 5000, 1500), 0), (d(C.PEER_NEW, 20, 1500), 0),
            (d(SUBNET_BCAST, 10, 1500), 0)]
    return out


RX_PEERS = (C.PEER_SENT, C.PEER_NEW, PEER_SILENT, R.OUTSIDE + 2, C.PEER_QUERY)


def _rx_frames():
    """60 frames received on the /24: echo requests and SYNs to a closed port from a Valid peer, a
    peer without an entry, the silent peer, an outside address (answered through the gateway) and
    the peer in Query state; every seventh frame is ARP, which neither responder answers."""
    lan = IFACES[K_LAN]
    out = []
    for k in range(60):
        src = RX_PEERS[k % 5]
        if k % 7 == 3:
            out.append(AC.other(k, start_keeper().arp_iface(K_LAN)))
        elif k % 2 == 0:
            out.append(lan["mac"] + R.peer_mac(src) + b"\x08\x00" + IR.echo(IR.pattern(9 + k % 40, k), src=src, dst=OWN))
        else:
            out.append(TRC.rst_due(6 * k, src=src, dst=OWN))
    return out


def scenario(oracle, seed):
    rng = np.random.default_rng(47000 + seed)
    sc = Scenario()
    sc.seed = seed
    sc.stride, sc.shift, sc.aux_blocks = LAYOUTS[seed]
    tcp, udp = _tcp_cases(rng), _udp_cases(rng)
    sc.tcp_batch = TS.Batch([c for c, _ in tcp], TS.payload_bytes(1 << 16, seed=100 + seed))
    sc.tcp_si, sc.tcp_cb = TS.caller_index(sc.tcp_batch.cases)
    sc.udp_batch = IF.Batch([c for c, _ in udp], IF.payload_bytes(1 << 17, seed=200 + seed))
    sc.e_tcp = TS.expected(oracle, sc.tcp_batch, sc.tcp_si, sc.tcp_cb)
    for batch in (sc.tcp_batch, sc.udp_batch):          # every piece lies inside its payload buffer
        assert all(o + ln <= len(batch.payload) for c in batch.cases for o, ln in c["pieces"])
    sc.udp_si, sc.udp_cb = IF.caller_index(sc.udp_batch.cases)
    sc.e_udp = IF.expected(oracle, sc.udp_batch, sc.udp_si, sc.udp_cb)
    ifc = start_keeper().arp_iface(K_LAN)
    sc.arp_frames = [AC.request(k, ifc, pad=(0, 18)[k & 1]) if k % 3 != 1 else AC.other(k, ifc) for k in range(37)]
    sc.e_arp = AC.respond(sc.arp_frames, ifc)
    lan = IFACES[K_LAN]
    sc.rx_frames = _rx_frames()
    verdicts = TRC.verdicts_of(oracle, sc.rx_frames)
    sc.e_icmp = IC.respond(sc.rx_frames, verdicts, None,
                           IC.iface(local=OWN, bcast=SUBNET_BCAST, ip_id=ICMP_ID, mac=lan["mac"]))
    sc.e_rst = TRC.respond(sc.rx_frames, verdicts, TRC.iface(local=OWN, prefix=24, mac=lan["mac"], ip_id=RST_ID))
    nt, nr, na, nu = len(sc.e_tcp.status), len(sc.rx_frames), len(sc.arp_frames), len(sc.e_udp.status)
    sc.at = dict(tcp=0, icmp=nt, rst=nt + nr, arp=nt + 2 * nr, udp=nt + 2 * nr + na)
    sc.n = n = nt + 2 * nr + na + nu
    sc.hdr_len = np.concatenate([np.full(nt, TS.HDR), sc.e_icmp.hdr_len, sc.e_rst.hdr_len, sc.e_arp.hdr_len,
                                 sc.e_udp.hdr_len]).astype(np.uint32)
    sc.seg_status = np.concatenate([sc.e_tcp.status, sc.e_icmp.status, sc.e_rst.status, sc.e_arp.status,
                                    sc.e_udp.status]).astype(np.uint8)
    sc.send_flags = np.zeros(n, dtype=np.uint8)
    sc.force = np.full(n, C.ROUTE_ANY, dtype=np.uint16)
    sc.group = np.full(n, -1, dtype=np.int64)
    sc.group[:nt] = sc.e_tcp.seg_case
    sc.group[nt:nt + 2 * nr] = -2
    sc.force[nt:nt + 2 * nr] = K_LAN                    # the receive interface
    sc.group[sc.at["udp"]:] = 1000 + sc.e_udp.frag_case
    for i in range(nt):
        sc.force[i] = tcp[int(sc.e_tcp.seg_case[i])][1]
    for i in range(nu):
        sc.send_flags[sc.at["udp"] + i] = udp[int(sc.e_udp.frag_case[i])][1]
    sc.ring = np.full(n * sc.stride, FILL, dtype=np.uint8)
    sc.body, sc.chunks = {}, {}

    def put(i, hdr, data, chunks):
        sc.ring[i * sc.stride:i * sc.stride + len(hdr)] = np.frombuffer(hdr, dtype=np.uint8)
        sc.body[i], sc.chunks[i] = hdr[14:] + data, chunks

    for i in np.flatnonzero(sc.e_tcp.status == TS.ACCEPT).tolist():
        ch = sc.e_tcp.seg_chunks[i]
        put(i, sc.e_tcp.headers[i].tobytes(), b"".join(sc.tcp_batch.payload[o:o + l].tobytes() for o, l in ch), len(ch))
    for i, h in sc.e_icmp.headers.items():
        data = IC.response_packet(sc.e_icmp, sc.rx_frames, i)[len(h) - 14:]
        put(sc.at["icmp"] + i, h, data, 1 if data else 0)
    for i, h in sc.e_rst.headers.items():
        put(sc.at["rst"] + i, h, b"", 0)
    for i, h in sc.e_arp.headers.items():
        put(sc.at["arp"] + i, h, b"", 0)
    for i in np.flatnonzero(sc.e_udp.status == IF.ACCEPT).tolist():
        f = IF.frame_of(sc.e_udp, sc.udp_batch.payload, i)
        put(sc.at["udp"] + i, f[:int(sc.e_udp.hdr_len[i])], f[int(sc.e_udp.hdr_len[i]):], len(sc.e_udp.frag_chunks[i]))
    return sc


_scenarios = {}


def cached(oracle, seed):
    """scenario(), computed once per process and left unchanged."""
    if seed not in _scenarios:
        _scenarios[seed] = scenario(oracle, seed)
    return _scenarios[seed]


def answers(requests):
    """The ARP frames that arrive between the rounds, [(interface, frame)] in order: a reply to
    every request but the silent peer's, a late reply of the peer that was in Query state, a
    broadcast request of the Valid peer under a new MAC, and a reply from an address outside
    every subnet (never learned)."""
    out = []
    for k, target, _ in requests:
        if target != PEER_SILENT:
            f = IFACES[k]
            out.append((k, AR.arp(2, target, f["addr"], sha=R.peer_mac(target), tha=f["mac"],
                                  eth_src=R.peer_mac(target), eth_dst=f["mac"])))
    lan = IFACES[K_LAN]
    out.append((K_LAN, AR.arp(2, C.PEER_QUERY, OWN, sha=R.peer_mac(C.PEER_QUERY), tha=lan["mac"],
                              eth_src=R.peer_mac(C.PEER_QUERY), eth_dst=lan["mac"])))
    out.append((K_LAN, AR.arp(1, C.PEER_SENT, OWN ^ 0x80, sha=R.peer_mac(C.PEER_SENT, 1),
                              eth_src=R.peer_mac(C.PEER_SENT, 1))))
    out.append((K_LAN, AR.arp(2, R.OUTSIDE, OWN, sha=R.peer_mac(R.OUTSIDE), tha=lan["mac"],
                              eth_src=R.peer_mac(R.OUTSIDE), eth_dst=lan["mac"])))
    return out


class Loop:
    """The two rounds and the fresh send of one scenario through a backend, the host in between.
    After run(): r1, r2 (the two tx_resolve results over the ring), requests1, requests2,
    hdr_len2 (the retry's lengths: hdr_len where round 1 held, else 0), table1, table2, keeper."""

    def __init__(self, sc, backend, ring0):
        self.sc, self.backend, self.ring0 = sc, backend, ring0
        self.keeper = start_keeper()

    def round1(self):
        sc = self.sc
        self.table1 = snapshot(self.keeper)
        self.r1 = self.backend.resolve(self.ring0, sc.stride, sc.hdr_len, IFACES, self.table1, sc.send_flags,
                                       sc.force, seg_status=sc.seg_status, where=1)
        self.requests1 = after_resolve(self.keeper, self.r1)
        return self.r1

    def between(self):
        frames = answers(self.requests1)
        for k in sorted({k for k, _ in frames}):
            h = self.backend.arp([f for q, f in frames if q == k], k, self.keeper, snapshot(self.keeper), where=k)
            after_arp(self.keeper, k, h)

    def round2(self):
        sc = self.sc
        held = self.r1.held[:int(self.r1.counts[0])].astype(np.int64)
        self.hdr_len2 = np.zeros(sc.n, dtype=np.uint32)
        self.hdr_len2[held] = sc.hdr_len[held]
        self.table2 = snapshot(self.keeper)
        self.r2 = self.backend.resolve(self.r1.ring, sc.stride, self.hdr_len2, IFACES, self.table2, sc.send_flags,
                                       sc.force, seg_status=sc.seg_status, where=2)
        self.requests2 = after_resolve(self.keeper, self.r2)
        return self.r2

    def run(self):
        self.round1()
        self.between()
        self.round2()
        return self


def check_rounds(sc, lp):
    """What both rounds must show, from the results alone (the models' or the device's)."""
    r1, r2 = lp.r1, lp.r2
    valid = np.zeros(sc.n, dtype=bool)
    valid[list(sc.body)] = True
    for r in (r1, r2):                                  # a datagram is never half-sent
        for g in np.unique(sc.group[sc.group >= 1000]):
            assert len(set(r.status[sc.group == g].tolist())) == 1, g
    arp = np.arange(sc.at["arp"], sc.at["udp"])
    assert (r1.status[arp] == C.NONE).all() and np.array_equal(r1.send_len[arp], sc.hdr_len[arp])
    held1 = set(r1.held[:int(r1.counts[0])].tolist())
    sent2 = set(np.flatnonzero((r2.status == C.SENT)).tolist())
    held2 = set(r2.held[:int(r2.counts[0])].tolist())
    assert sent2 | held2 == held1 and not sent2 & held2 and int(r2.counts[1]) == 0
    for i in held2:                                     # the silent peer: held again, no new request
        assert int(r2.routes[i]["next_hop"]) == PEER_SILENT and not int(r2.routes[i]["flags"]) & C.NEW_ENTRY
    assert not lp.requests2 and {t for _, t, _ in lp.requests1} == {C.PEER_NEW, PEER_SILENT, PEER_B_NEW}
    assert len(lp.requests1) == 3
    for i in sent2:
        hop, k = int(r2.routes[i]["next_hop"]), int(r2.routes[i]["iface"])
        assert r2.ring[i * sc.stride:i * sc.stride + 14].tobytes() == R.peer_mac(hop) + IFACES[k]["mac"] + b"\x08\x00"
    sent1 = set(np.flatnonzero((r1.status == C.SENT) & valid).tolist())
    want = set(np.flatnonzero(valid & (sc.hdr_len >= 34) & (sc.group != -1)).tolist()) - \
        set(r1.failed[:int(r1.counts[1])].tolist()) - held2
    assert sent1 | sent2 == want and not sent1 & sent2           # once and only once
    # the responders' answers: all through the receive interface; sent at once to the Valid peer and,
    # through the gateway, to the outside one; held and retried for the others; the silent peer's stay
    rsp = [i for i in sc.body if sc.group[i] == -2]
    for i in rsp:
        assert int(r1.routes[i]["flags"]) & C.FORCED and int(r1.routes[i]["iface"]) == K_LAN, i
    by_peer = {p: [i for i in rsp if int.from_bytes(sc.body[i][16:20], "big") == p] for p in RX_PEERS}
    assert all(len(v) >= 8 for v in by_peer.values()) and sum(map(len, by_peer.values())) == len(rsp)
    assert set(by_peer[C.PEER_SENT]) | set(by_peer[R.OUTSIDE + 2]) <= sent1
    assert all(int(r1.routes[i]["flags"]) & C.GATEWAY and int(r1.routes[i]["next_hop"]) == GW
               for i in by_peer[R.OUTSIDE + 2])
    assert set(by_peer[C.PEER_NEW]) | set(by_peer[C.PEER_QUERY]) <= sent2 and set(by_peer[PEER_SILENT]) <= held2
    assert (K_LAN, R.OUTSIDE) not in lp.keeper.entries
    assert lp.keeper.entries[(K_LAN, C.PEER_SENT)] == (C.VALID, R.peer_mac(C.PEER_SENT, 1))
    return sent1, sent2, held2
