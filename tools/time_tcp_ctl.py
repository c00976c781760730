#!/usr/bin/env python3
"""tcp_tx_control against tx_resolve of the same slots and against a plain device copy of the
header ring's bytes, in ONE process.

Workload: n empty-ACK descriptors (default 1,048,576; one connection each towards 4,096 peers of
one /16, no options: 54-byte headers) into a ring of 64-byte slots on a 64-byte boundary. Three
resident batches (descriptors and ring) take turns so that no launch finds its bytes in the
Infinity Cache. Routes, alternating step by step, each launch timed with its own HIP event pair
(5 warm-up + 20 timed steps): tcp_tx_control; tx_resolve of the slots it emitted (every peer Valid
in the ARP table); torch's device-to-device copy of the ring's n * 64 bytes. Before timing, batch
0's ring is checked whole against the rules of chksum.h in numpy (below), with both checksums
verified by summation. One JSON line per route (us min / median), then the ratios; the call moves
32 bytes in and 64 bytes + 13 bytes of per-descriptor outputs out per descriptor. Informational;
not part of the product.

    python tools/time_tcp_ctl.py [--descriptors 1048576] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOT, PEERS, LOCAL, TTL = 64, 4096, 10 << 24 | 20 << 16 | 1, 64
MAC = bytes([2, 0, 0x5E, 0x10, 0x20, 0x30])


def peer_addr(j):
    return (np.uint32(10 << 24 | 20 << 16) | (1 + j // 250).astype(np.uint32) << 8 |
            (2 + j % 250).astype(np.uint32))


def build(A, n, r):
    rng = np.random.default_rng(1700 + r)
    c = np.zeros(n, dtype=A.TCP_CTL_DTYPE)
    c["local_addr"], c["remote_addr"] = LOCAL, peer_addr(rng.integers(0, PEERS, n))
    c["local_port"], c["remote_port"] = 80, rng.integers(1024, 65536, n)
    c["seq"], c["ack"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 32, n)
    c["window"], c["flags"] = rng.integers(0, 65536, n), 0x10
    return c


def sum16(words):
    s = words.astype(np.uint64).sum(axis=1)
    for _ in range(3):
        s = (s & 0xFFFF) + (s >> 16)
    return s


def check_ring(ring, c, ip_id):
    """The ring of batch `c` by the rules of chksum.h: the fields in place, both checksums good."""
    n = c.size
    g = ring.reshape(n, SLOT)
    be = g[:, 14:54].reshape(n, 20, 2).astype(np.uint32)
    w = be[:, :, 0] << 8 | be[:, :, 1]
    ok = not g[:, 0:6].any() and (g[:, 6:12] == np.frombuffer(MAC, dtype=np.uint8)).all()
    ok = ok and (g[:, 12:14] == (8, 0)).all() and not g[:, 54:].any()
    ok = ok and (w[:, 0] == 0x4500).all() and (w[:, 1] == 40).all() and (w[:, 3] == 0x4000).all()
    ok = ok and (w[:, 2] == (ip_id + np.arange(n)) & 0xFFFF).all() and (w[:, 4] == (TTL << 8 | 6)).all()
    ok = ok and ((w[:, 6] << 16 | w[:, 7]) == c["local_addr"]).all()
    ok = ok and ((w[:, 8] << 16 | w[:, 9]) == c["remote_addr"]).all()
    ok = ok and (w[:, 10] == c["local_port"]).all() and (w[:, 11] == c["remote_port"]).all()
    ok = ok and ((w[:, 12] << 16 | w[:, 13]) == c["seq"]).all() and ((w[:, 14] << 16 | w[:, 15]) == c["ack"]).all()
    ok = ok and (w[:, 16] == 0x5010).all() and (w[:, 17] == c["window"]).all() and (w[:, 19] == 0).all()
    ok = ok and (sum16(w[:, :10]) == 0xFFFF).all()
    pseudo = np.concatenate([w[:, 6:10], np.full((n, 1), 6 + 20, dtype=np.uint32), w[:, 10:]], axis=1)
    return bool(ok and (sum16(pseudo) == 0xFFFF).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--descriptors", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    import aipstack_amd as A

    dev = torch.device("cuda", 0)
    n, ip_id = args.descriptors, 0xFF00
    iface = A.icmp_iface(LOCAL, LOCAL | 0xFFFF, MAC, ip_id=ip_id)
    d_ifaces = torch.from_numpy(A.tx_ifaces([(LOCAL, 16, None, MAC)]).view(np.uint8)).to(dev)
    table = np.zeros(PEERS, dtype=A.ARP_ENTRY_DTYPE)
    table["addr"], table["state"] = peer_addr(np.arange(PEERS)), A.AIPSTACK_ARP_STATE_VALID
    table["mac"][:, 0] = 2
    table["mac"][:, 2:6] = table["addr"].astype(">u4").view(np.uint8).reshape(-1, 4)
    d_table = torch.from_numpy(A.arp_table_sort(table).view(np.uint8)).to(dev)
    host = [build(A, n, r) for r in range(args.rotate)]
    ctl = [torch.from_numpy(c.view(np.uint8).copy()).to(dev) for c in host]
    rings = [torch.zeros(n * SLOT, dtype=torch.uint8, device=dev) for _ in host]
    assert all(t.data_ptr() % 64 == 0 for t in rings)
    ws = torch.empty(max(A.tcp_tx_control_workspace_bytes(n), A.tx_resolve_workspace_bytes(n)),
                     dtype=torch.uint8, device=dev)
    copy_dst = torch.empty(n * SLOT, dtype=torch.uint8, device=dev)
    res = [None] * args.rotate
    out = dict(status=torch.empty(n, dtype=torch.uint8, device=dev),
               routes=torch.empty(16 * n, dtype=torch.uint8, device=dev),
               send_lens=torch.empty(n, dtype=torch.int32, device=dev),
               arp_used=torch.empty(PEERS, dtype=torch.uint8, device=dev),
               held_seg=torch.empty(n, dtype=torch.int64, device=dev),
               failed_seg=torch.empty(n, dtype=torch.int64, device=dev),
               counts=torch.empty(2, dtype=torch.int64, device=dev))

    def control(step):
        r = step % args.rotate
        res[r] = A.tcp_tx_control(ctl[r], iface, tcp_ttl=TTL, headers=rings[r], workspace=ws)

    def resolve(step):
        r = step % args.rotate
        A.tx_resolve(rings[r], SLOT, res[r].hdr_lens, d_ifaces, d_table, workspace=ws, **out)

    def copy(step):
        copy_dst.copy_(rings[step % args.rotate])

    for r in range(args.rotate):
        control(r)
    torch.cuda.synchronize()
    parity = check_ring(rings[0].cpu().numpy(), host[0], ip_id) and \
        res[0].counts.cpu().numpy().tolist() == [n, 0] and \
        bool((res[0].hdr_lens == 54).all()) and not bool(res[0].chunk_index.any())
    resolve(0)
    torch.cuda.synchronize()
    parity = parity and bool((out["status"] == A.AIPSTACK_TX_RES_SENT).all())
    if not parity:
        print(json.dumps({"error": "tcp_tx_control differs from the rules of chksum.h"}))
        return 1

    routes = [("tcp_tx_control", control), ("tx_resolve", resolve), ("device_copy", copy)]
    times = {name: [] for name, _ in routes}
    for step in range(args.warmup + args.steps):
        for name, fn in routes:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(step)
            b.record()
            b.synchronize()
            if step >= args.warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
    lines = [dict(route=name, descriptors=n, us_min=round(min(t), 1), us_median=round(statistics.median(t), 1),
                  steps=len(t), parity=True) for name, t in times.items()]
    med = {ln["route"]: ln["us_median"] for ln in lines}
    lines.append(dict(ratio_control_to_copy=round(med["tcp_tx_control"] / med["device_copy"], 2),
                      ratio_control_to_resolve=round(med["tcp_tx_control"] / med["tx_resolve"], 2),
                      bytes_in=32 * n, bytes_out=(SLOT + 13) * n + 24))
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
