#!/usr/bin/env python3
"""Received ICMP Destination Unreachable against Rx verify alone on the same frames, in ONE
process.

Workload: n frames (default 1,048,576) in 2 KiB ring slots: one frame in eight is a 70-byte
frag-needed message (ICMP type 3 code 4) that quotes an IPv4 header and the first 8 bytes of a TCP
segment, the other seven are UDP frames of 42 + 1472 bytes with valid checksums (the product's own
Tx fill). The PCB table has 4,096 entries; every second quoted connection is in it.

Three resident batches take turns so that no launch finds its bytes in the Infinity Cache (the
message's place in a group of eight moves with the batch). Two routes, alternating step by step,
each launch timed with its own HIP event pair (5 warm-up + 20 timed steps):
icmp_rx_unreach_slotted, and rx_verify_slotted alone on the same frames: the yardstick.
icmp_rx_unreach_slotted is checked on rotation batch 0 against the rules of chksum.h in numpy
(below; the messages have one shape) before timing: verdicts, statuses, records, the list, the
counts. One JSON line per route (us min / median), then the ratio to rx_verify. Not part of the
product.

    python tools/bench_icmp_rx_unreach.py [--frames 1048576] [--out FILE]
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

from bench_udp_rx_demux import make_headers  # noqa: E402  (tools/: the UDP frames' 42 header bytes)

UDP, MSG, SLOT, GROUP, PCBS = 1514, 70, 2048, 8, 4096
LOCAL_IP, BCAST, PEER = 0x0A141E28, 0x0A141EFF, 0x0A141E64
LOCAL_MAC = bytes([2, 0, 0x5E, 0x10, 0x20, 0x30])


def be(values, width):
    v = np.asarray(values, dtype=np.uint64)
    return np.stack([(v >> (8 * (width - 1 - k)) & 0xFF).astype(np.uint8) for k in range(width)], axis=1)


def chksum(rows):
    """The Internet checksum of each row (an even number of bytes) as (m, 2) big-endian bytes."""
    w = rows.reshape(rows.shape[0], -1, 2).astype(np.uint64)
    s = (w[:, :, 0] << 8 | w[:, :, 1]).sum(axis=1)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    return be(~s & 0xFFFF, 2)


def table(A):
    """4,096 connections of LOCAL_IP; cookie = index + 1."""
    i = np.arange(PCBS)
    t = np.zeros(PCBS, dtype=A.TCP_PCB_KEY_DTYPE)
    t["local_addr"], t["remote_addr"] = LOCAL_IP, 0xC0A80000 + i
    t["local_port"], t["remote_port"], t["cookie"] = 5000 + i % 1000, 20000 + i, i + 1
    return t


def messages(m, seed):
    """(m, 70) frag-needed messages; message k quotes connection (k + seed) // 2 mod 4096 of the
    table when k + seed is even and a connection that is not in it otherwise. Also the record
    fields: connection index, hit, sequence number, next-hop MTU."""
    rng = np.random.default_rng(seed)
    k = np.arange(m) + seed
    conn, hit = (k // 2) % PCBS, k % 2 == 0
    seq = rng.integers(0, 1 << 32, m, dtype=np.uint64)
    mtu = rng.integers(576, 1500, m, dtype=np.uint64)
    f = np.zeros((m, MSG), dtype=np.uint8)
    f[:, 0:6] = np.frombuffer(LOCAL_MAC, dtype=np.uint8)
    f[:, 6:14] = (2, 0x11, 0x22, 0x33, 0x44, 0x50, 8, 0)
    f[:, 14:24] = (0x45, 0, 0, MSG - 14, 0, 0, 0, 0, 64, 1)
    f[:, 26:30], f[:, 30:34] = be([PEER] * m, 4), be([LOCAL_IP] * m, 4)
    f[:, 24:26] = chksum(f[:, 14:34])
    f[:, 34:36] = (3, 4)
    f[:, 40:42] = be(mtu, 2)
    f[:, 42:52] = (0x45, 0, 0x05, 0xDC, 0x12, 0x34, 0x40, 0, 63, 6)
    f[:, 54:58], f[:, 58:62] = be([LOCAL_IP] * m, 4), be(0xC0A80000 + conn, 4)
    f[:, 62:64] = be(5000 + conn % 1000 + np.where(hit, 0, 30000), 2)
    f[:, 64:66], f[:, 66:70] = be(20000 + conn, 2), be(seq, 4)
    f[:, 36:38] = chksum(f[:, 34:70])
    return f, conn, hit, seq, mtu


def model(A, n, rows, conn, hit, seq, mtu):
    """What icmp_rx_unreach leaves for n frames whose `rows` are the messages above and whose
    other frames are UDP."""
    rec = np.zeros(n, dtype=A.ICMP_DU_RECORD_DTYPE)
    r = rec[rows]
    r["local_addr"], r["remote_addr"] = LOCAL_IP, 0xC0A80000 + conn
    r["local_port"], r["remote_port"] = 5000 + conn % 1000 + np.where(hit, 0, 30000), 20000 + conn
    r["seq"], r["rest"], r["pcb"] = seq, mtu, np.where(hit, conn + 1, A.AIPSTACK_TCP_NO_PCB)
    r["ip_off"], r["l4_len"], r["code"], r["proto"], r["ttl"], r["hl"] = 42, 8, 4, 6, 63, 20
    rec[rows] = r
    status = np.full(n, A.AIPSTACK_ICMP_DU_NONE, dtype=np.uint8)
    status[rows] = np.where(hit, A.AIPSTACK_ICMP_DU_TCP_PCB, A.AIPSTACK_ICMP_DU_TCP_NO_PCB)
    lst = np.full(n, -1, dtype=np.int64)
    lst[:int(hit.sum())] = rows[hit]
    return rec, status, lst, np.array([int(hit.sum()), rows.size], dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    import aipstack_amd as A
    from aipstack_amd import synth

    dev = torch.device("cuda", 0)
    n = args.frames // GROUP * GROUP
    g = n // GROUP
    iface = A.icmp_iface(LOCAL_IP, BCAST, LOCAL_MAC)
    pcbs = torch.from_numpy(A.tcp_pcb_table_sort(table(A)).view(np.uint8).copy()).to(dev)
    ws = torch.empty(A.icmp_rx_unreach_workspace_bytes(n), dtype=torch.uint8, device=dev)
    verdict_only = torch.empty(n, dtype=torch.uint8, device=dev)
    out = dict(verdict=torch.empty(n, dtype=torch.uint8, device=dev),
               status=torch.empty(n, dtype=torch.uint8, device=dev),
               records=torch.empty(n * 32, dtype=torch.uint8, device=dev),
               pcb_frame=torch.empty(n, dtype=torch.int64, device=dev),
               counts=torch.empty(2, dtype=torch.int64, device=dev))

    def build(r):
        rows = np.arange(g) * GROUP + r % GROUP
        msg, conn, hit, seq, mtu = messages(g, 900 + 10 * r)
        ring = torch.empty(n * SLOT, dtype=torch.uint8, device=dev)
        synth.fill_device(ring, synth.SEED_DATA + 90 + r)
        ring.view(n, SLOT)[:, :42] = torch.from_numpy(make_headers(n, 950 + r)[0]).to(dev)
        full = torch.full((n,), UDP, dtype=torch.int32, device=dev)
        assert bool((A.tx_fill_slotted(ring, SLOT, full) == 6).all())          # valid checksums
        ring.view(n, SLOT)[torch.from_numpy(rows).to(dev), :MSG] = torch.from_numpy(msg).to(dev)
        lens = np.full(n, UDP, dtype=np.int32)
        lens[rows] = MSG
        return dict(ring=ring, lens=torch.from_numpy(lens).to(dev), rows=rows, conn=conn, hit=hit, seq=seq,
                    mtu=mtu)

    batches = [build(r) for r in range(args.rotate)]

    def unreach(step):
        b = batches[step % args.rotate]
        A.icmp_rx_unreach_slotted(b["ring"], SLOT, b["lens"], iface, pcbs, workspace=ws, **out)

    def verify(step):
        b = batches[step % args.rotate]
        A.rx_verify_slotted(b["ring"], SLOT, b["lens"], out=verdict_only)

    routes = [("icmp_rx_unreach", unreach), ("rx_verify", verify)]

    b = batches[0]
    for t in out.values():
        t.view(torch.uint8).fill_(0xC3)
    unreach(0)
    verify(0)
    torch.cuda.synchronize()
    rec, status, lst, counts = model(A, n, b["rows"], b["conn"], b["hit"], b["seq"], b["mtu"])
    v = verdict_only.cpu().numpy()
    parity = {"rx_verify": bool((v == 6).all()),
              "icmp_rx_unreach": bool(
                  np.array_equal(out["verdict"].cpu().numpy(), v)
                  and np.array_equal(out["status"].cpu().numpy(), status)
                  and out["records"].cpu().numpy().tobytes() == rec.tobytes()
                  and np.array_equal(out["pcb_frame"].cpu().numpy(), lst)
                  and np.array_equal(out["counts"].cpu().numpy(), counts))}

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

    lines = []
    for name, _ in routes:
        t = times[name]
        lines.append({"route": name, "layout": "slots", "n": n, "unreach_frames": g, "pcbs": PCBS,
                      "pcb_hits": int(b["hit"].sum()), "us_min": round(min(t), 1),
                      "us_median": round(statistics.median(t), 1),
                      "model_parity": "ok" if parity[name] else "MISMATCH"})
    lines.append({"icmp_rx_unreach_over_rx_verify_median": round(
        statistics.median(times["icmp_rx_unreach"]) / statistics.median(times["rx_verify"]), 3)})
    for l in lines:
        print(json.dumps(l))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")
    return 0 if all(parity.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
