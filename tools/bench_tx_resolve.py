#!/usr/bin/env python3
"""Tx resolve against tx_linearise_slotted over the same segments and against a plain device copy
of the header ring's bytes, in ONE process.

Workload: n segments (default 1,048,576) of 54-byte headers in 64-byte slots, sent from four
interfaces (a /16 each) to peers of a 4,096-entry ARP table (1,024 Valid entries per interface);
one segment in 64 goes to an address the table lacks and is held (_ARP_QUERY with _NEW_ENTRY).
Three resident batches take turns so that no launch finds its bytes in the Infinity Cache (the
held segment's place in a group of 64 and the peers move with the batch). Routes, alternating step
by step, each launch timed with its own HIP event pair (5 warm-up + 20 timed steps): tx_resolve;
tx_linearise_slotted of the same header slots (no chunks) into 64-byte frame slots; torch's
device-to-device copy of the ring's n * 64 bytes. tx_resolve is checked on rotation batch 0
against the rules of chksum.h in numpy (below) before timing: status, records, send_len, arp_used,
both lists, the counts and every slot of the ring. One JSON line per route (us min / median), then
the ratios. Not part of the product.

    python tools/bench_tx_resolve.py [--segments 1048576] [--out FILE]
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

HDR, SLOT, GROUP, IFACES, PER_IFACE = 54, 64, 64, 4, 1024


def entry_addr(k, j):
    """Peer j of interface k: 10.(20+k).(1 + j // 250).(1 + j % 250)."""
    return (np.uint32(10 << 24) | (np.uint32(20) + k.astype(np.uint32)) << 16 |
            (1 + j // 250).astype(np.uint32) << 8 | (1 + j % 250).astype(np.uint32))


def mac_of(addr):
    m = np.zeros((addr.size, 6), dtype=np.uint8)
    m[:, 0], m[:, 1] = 2, 0x77
    m[:, 2:6] = addr.astype(">u4").view(np.uint8).reshape(-1, 4)
    return m


def build(A, n, r):
    """One batch: the ring (n, 64), and what tx_resolve must leave for it."""
    rng = np.random.default_rng(1200 + r)
    i = np.arange(n)
    k = ((i + r) % IFACES).astype(np.uint32)
    j = rng.integers(0, PER_IFACE, n)
    held = i % GROUP == (7 * r + 3) % GROUP
    dst = entry_addr(k, j)
    dst[held] = (np.uint32(10 << 24) | (np.uint32(20) + k[held]) << 16 | np.uint32(200) << 8 |
                 (1 + i[held] % 250).astype(np.uint32))
    src = (np.uint32(10 << 24) | (np.uint32(20) + k) << 16 | np.uint32(1))
    ring = rng.integers(0, 256, (n, SLOT), dtype=np.uint8)
    ring[:, 12:14] = (8, 0)
    ring[:, 14] = 0x45
    ring[:, 26:30] = src.astype(">u4").view(np.uint8).reshape(n, 4)
    ring[:, 30:34] = dst.astype(">u4").view(np.uint8).reshape(n, 4)
    want = ring.copy()
    sent = ~held
    want[sent, 0:6] = mac_of(dst[sent])
    own = np.zeros((n, 6), dtype=np.uint8)
    own[:, 0:5], own[:, 5] = (2, 0, 0x5E, 0x10, 0x20), 0x30 + k
    want[sent, 6:12] = own[sent]
    routes = np.zeros(n, dtype=A.TX_ROUTE_DTYPE)
    routes["next_hop"], routes["iface"] = dst, k
    routes["arp_index"] = np.where(held, A.AIPSTACK_TX_NO_ARP_ENTRY, k * PER_IFACE + j)
    routes["status"] = np.where(held, A.AIPSTACK_TX_RES_ARP_QUERY, A.AIPSTACK_TX_RES_SENT)
    routes["flags"] = np.where(held, A.AIPSTACK_TX_ROUTE_NEW_ENTRY, 0)
    used = np.zeros(IFACES * PER_IFACE, dtype=np.uint8)
    used[(k * PER_IFACE + j)[sent]] = 1
    lst = np.full(n, -1, dtype=np.int64)
    lst[:int(held.sum())] = np.flatnonzero(held)
    return ring, dict(ring=want, routes=routes, status=routes["status"].copy(),
                      send_len=np.where(held, 0, HDR).astype(np.int32), used=used, held=lst,
                      failed=np.full(n, -1, dtype=np.int64),
                      counts=np.array([int(held.sum()), 0], dtype=np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    import aipstack_amd as A

    dev = torch.device("cuda", 0)
    n = args.segments // GROUP * GROUP
    ifaces = A.tx_ifaces([(int(10 << 24 | (20 + k) << 16 | 1), 16, None, bytes([2, 0, 0x5E, 0x10, 0x20, 0x30 + k]))
                          for k in range(IFACES)])
    kk, jj = np.repeat(np.arange(IFACES), PER_IFACE), np.tile(np.arange(PER_IFACE), IFACES)
    table = np.zeros(IFACES * PER_IFACE, dtype=A.ARP_ENTRY_DTYPE)
    table["addr"], table["iface"], table["state"] = entry_addr(kk, jj), kk, A.AIPSTACK_ARP_STATE_VALID
    table["mac"] = mac_of(table["addr"])
    assert A.arp_table_sort(table).tobytes() == table.tobytes()          # already in the lookup's order
    d_ifaces = torch.from_numpy(ifaces.view(np.uint8)).to(dev)
    d_table = torch.from_numpy(table.view(np.uint8)).to(dev)
    ws = torch.empty(A.tx_resolve_workspace_bytes(n), dtype=torch.uint8, device=dev)
    lens = torch.full((n,), HDR, dtype=torch.int32, device=dev)
    out = dict(status=torch.empty(n, dtype=torch.uint8, device=dev),
               routes=torch.empty(16 * n, dtype=torch.uint8, device=dev),
               send_lens=torch.empty(n, dtype=torch.int32, device=dev),
               arp_used=torch.empty(len(table), dtype=torch.uint8, device=dev),
               held_seg=torch.empty(n, dtype=torch.int64, device=dev),
               failed_seg=torch.empty(n, dtype=torch.int64, device=dev),
               counts=torch.empty(2, dtype=torch.int64, device=dev))
    batches, want0 = [], None
    for r in range(args.rotate):
        ring, want = build(A, n, r)
        batches.append(torch.from_numpy(ring.reshape(-1)).to(dev))
        want0 = want if r == 0 else want0
    frames = torch.empty(n * SLOT, dtype=torch.uint8, device=dev)
    copy_dst = torch.empty(n * SLOT, dtype=torch.uint8, device=dev)
    no_addr = torch.empty(0, dtype=torch.int64, device=dev)
    no_len = torch.empty(0, dtype=torch.int32, device=dev)
    index = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    lin_lens = torch.empty(n, dtype=torch.int32, device=dev)
    lin_status = torch.empty(n, dtype=torch.uint8, device=dev)

    def resolve(step):
        A.tx_resolve(batches[step % args.rotate], SLOT, lens, d_ifaces, d_table, workspace=ws, **out)

    def linearise(step):
        A.tx_linearise_slotted(frames, SLOT, headers=batches[step % args.rotate], hdr_stride=SLOT, hdr_lens=lens,
                               chunk_addr=no_addr, chunk_len=no_len, chunk_index=index, frame_max=SLOT,
                               lens=lin_lens, status=lin_status)

    def copy(step):
        copy_dst.copy_(batches[step % args.rotate])

    routes = [("tx_resolve", resolve), ("tx_linearise_slotted", linearise), ("device_copy", copy)]

    for t in out.values():
        t.view(torch.uint8).fill_(0xC3)
    resolve(0)
    torch.cuda.synchronize()
    w = want0
    parity = bool(
        np.array_equal(out["status"].cpu().numpy(), w["status"])
        and out["routes"].cpu().numpy().tobytes() == w["routes"].tobytes()
        and np.array_equal(out["send_lens"].cpu().numpy(), w["send_len"])
        and np.array_equal(out["arp_used"].cpu().numpy(), w["used"])
        and np.array_equal(out["held_seg"].cpu().numpy(), w["held"])
        and np.array_equal(out["failed_seg"].cpu().numpy(), w["failed"])
        and np.array_equal(out["counts"].cpu().numpy(), w["counts"])
        and batches[0].cpu().numpy().tobytes() == w["ring"].tobytes())

    times = {name: [] for name, _ in routes}
    events = []
    for step in range(args.warmup + args.steps):
        for name, fn in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(step)
            e1.record()
            if step >= args.warmup:
                events.append((name, e0, e1))
    torch.cuda.synchronize()
    for name, e0, e1 in events:
        times[name].append(e0.elapsed_time(e1) * 1e3)

    lines = [{"route": name, "n": n, "ring_bytes": n * SLOT, "arp_entries": len(table), "ifaces": IFACES,
              "held": int(w["counts"][0]) if name == "tx_resolve" else None,
              "us_min": round(min(times[name]), 1), "us_median": round(statistics.median(times[name]), 1),
              "model_parity": ("ok" if parity else "MISMATCH") if name == "tx_resolve" else None}
             for name, _ in routes]
    med = {name: statistics.median(times[name]) for name, _ in routes}
    lines.append({"tx_resolve_over_tx_linearise_median": round(med["tx_resolve"] / med["tx_linearise_slotted"], 3),
                  "tx_resolve_over_device_copy_median": round(med["tx_resolve"] / med["device_copy"], 3)})
    for l in lines:
        print(json.dumps(l))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")
    return 0 if parity else 1


if __name__ == "__main__":
    sys.exit(main())
