#!/usr/bin/env python3
"""ARP on receive against Rx verify alone on the same frames, in ONE process.

Workload: n frames (default 1,048,576) in two mixes, each in 2 KiB ring slots and as CSR frames
back to back:

  udp8   one frame in eight is a 60-byte ARP request for the interface's address (sender MAC and
         address vary per frame), the other seven are UDP frames of 42 + 1472 bytes with valid
         checksums (the product's own Tx fill);
  arp60  every frame is such a 60-byte ARP request.

Three resident batches per mix and layout take turns so that no launch finds its bytes in the
Infinity Cache (the ARP frame's place in a group of eight moves with the batch). Routes,
alternating step by step, each launch timed with its own HIP event pair (5 warm-up + 20 timed
steps): arp_rx_respond / _slotted, and rx_verify / _slotted alone on the same frames: the
yardstick. arp_rx_respond is checked on rotation batch 0 of every mix and layout against the
model before timing: status, records, header lengths, the chunk index, both lists, the counts
and every reply slot, by the rules of chksum.h in numpy (below; the ARP frames have one shape).
One JSON line per route (us min / median), then per mix and layout the ratio to rx_verify. Not
part of the product.

    python tools/bench_arp_rx.py [--frames 1048576] [--out FILE]
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

UDP, ARP, SLOT, GROUP = 1514, 60, 2048, 8
LOCAL_IP, NETMASK = 0x0A141E28, 0xFFFFFF00
LOCAL_MAC = bytes([2, 0, 0x5E, 0x10, 0x20, 0x30])


def arp_requests(m, seed):
    """(m, 60) ARP requests for LOCAL_IP with 18 padding bytes, their sender MACs (m, 6) and
    sender addresses (in the subnet, neither network nor broadcast address)."""
    rng = np.random.default_rng(seed)
    mac = rng.integers(0, 256, (m, 6), dtype=np.uint8)
    mac[:, 0] = 2
    ip = (np.uint32(LOCAL_IP & NETMASK) + rng.integers(1, 255, m).astype(np.uint32)).astype(np.uint32)
    f = np.zeros((m, ARP), dtype=np.uint8)
    f[:, 0:6] = 0xFF
    f[:, 6:12] = (2, 0x11, 0x22, 0x33, 0x44, 0x51)                     # Ethernet source: another MAC
    f[:, 12:22] = (8, 6, 0, 1, 8, 0, 6, 4, 0, 1)
    f[:, 22:28] = mac
    f[:, 28:32] = ip.astype(">u4").view(np.uint8).reshape(m, 4)
    f[:, 38:42] = np.frombuffer(LOCAL_IP.to_bytes(4, "big"), dtype=np.uint8)
    return f, mac, ip


def model(A, n, rows, mac, ip):
    """What arp_rx_respond leaves for n frames whose `rows` are the requests of arp_requests and
    whose other frames are IPv4."""
    m = rows.size
    rec = np.zeros(n, dtype=A.ARP_RECORD_DTYPE)
    rec["status"] = A.AIPSTACK_ARP_NONE
    rec["sender_addr"][rows], rec["sender_mac"][rows], rec["op"][rows] = ip, mac, 1
    rec["flags"][rows] = (A.AIPSTACK_ARP_REC_LEARN | A.AIPSTACK_ARP_REC_NEW_OK | A.AIPSTACK_ARP_REC_NOTIFY |
                          A.AIPSTACK_ARP_REC_REPLY)
    rec["status"][rows] = A.AIPSTACK_ARP_REPLY
    hdr_len = np.zeros(n, dtype=np.int32)
    hdr_len[rows] = 42
    lst = np.full(n, -1, dtype=np.int64)
    lst[:m] = rows
    slots = np.zeros((m, 64), dtype=np.uint8)
    own = np.frombuffer(LOCAL_MAC, dtype=np.uint8)
    slots[:, 0:6], slots[:, 6:12] = mac, own
    slots[:, 12:22] = (8, 6, 0, 1, 8, 0, 6, 4, 0, 2)
    slots[:, 22:28] = own
    slots[:, 28:32] = np.frombuffer(LOCAL_IP.to_bytes(4, "big"), dtype=np.uint8)
    slots[:, 32:38] = mac
    slots[:, 38:42] = ip.astype(">u4").view(np.uint8).reshape(m, 4)
    return rec, hdr_len, lst, np.array([m, m], dtype=np.int64), slots


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
    iface = A.arp_iface(LOCAL_IP, NETMASK, LOCAL_MAC)
    ws = torch.empty(A.arp_rx_respond_workspace_bytes(n), dtype=torch.uint8, device=dev)
    verdict_only = torch.empty(n, dtype=torch.uint8, device=dev)

    def outputs():
        return A.ArpResponses(torch.empty(n * 64, dtype=torch.uint8, device=dev), 64,
                              torch.empty(n, dtype=torch.int32, device=dev),
                              torch.empty(n + 1, dtype=torch.int64, device=dev),
                              torch.empty(n, dtype=torch.uint8, device=dev),
                              torch.empty(n * 16, dtype=torch.uint8, device=dev),
                              torch.empty(n, dtype=torch.int64, device=dev),
                              torch.empty(n, dtype=torch.int64, device=dev),
                              torch.empty(2, dtype=torch.int64, device=dev))

    def build(mix, r):
        """One batch in both layouts: (ring, lens), (flat, offsets), and the rows, MACs and
        addresses of its ARP frames."""
        rows = np.arange(n) if mix == "arp60" else np.arange(g) * GROUP + r % GROUP
        arp, mac, ip = arp_requests(rows.size, 900 + 10 * r + (mix == "arp60"))
        d_arp, d_rows = torch.from_numpy(arp).to(dev), torch.from_numpy(rows).to(dev)
        ring = torch.empty(n * SLOT, dtype=torch.uint8, device=dev)
        lens = np.full(n, ARP if mix == "arp60" else UDP, dtype=np.int32)
        lens[rows] = ARP
        if mix == "udp8":
            synth.fill_device(ring, synth.SEED_DATA + 90 + r)
            ring.view(n, SLOT)[:, :42] = torch.from_numpy(make_headers(n, 950 + r)[0]).to(dev)
            full = torch.full((n,), UDP, dtype=torch.int32, device=dev)
            assert bool((A.tx_fill_slotted(ring, SLOT, full) == 6).all())          # valid checksums
        ring.view(n, SLOT)[d_rows, :ARP] = d_arp
        d_lens = torch.from_numpy(lens).to(dev)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        flat = torch.empty(int(off[-1]), dtype=torch.uint8, device=dev)
        if mix == "arp60":
            flat.view(n, ARP).copy_(d_arp)
        else:                                             # groups of eight: seven UDP frames, one ARP
            at, grp = 0, int(off[GROUP])
            for j in range(GROUP):
                ln = ARP if j == r % GROUP else UDP
                flat.view(g, grp)[:, at:at + ln] = ring.view(g, GROUP, SLOT)[:, j, :ln]
                at += ln
        return dict(ring=ring, lens=d_lens, flat=flat, off=torch.from_numpy(off).to(dev),
                    out=outputs(), rows=rows, mac=mac, ip=ip)

    mixes = {mix: [build(mix, r) for r in range(args.rotate)] for mix in ("udp8", "arp60")}

    def route(mix, layout, what):
        bs = mixes[mix]

        def run(step):
            b = bs[step % args.rotate]
            if what == "arp" and layout == "slots":
                A.arp_rx_respond_slotted(b["ring"], SLOT, b["lens"], iface, out=b["out"], workspace=ws)
            elif what == "arp":
                A.arp_rx_respond(b["flat"], b["off"], iface, out=b["out"], workspace=ws)
            elif layout == "slots":
                A.rx_verify_slotted(b["ring"], SLOT, b["lens"], out=verdict_only)
            else:
                A.rx_verify(b["flat"], b["off"], out=verdict_only)
        return run

    routes = [(mix, layout, what, route(mix, layout, what)) for mix in ("udp8", "arp60")
              for layout in ("slots", "csr") for what in ("arp", "rx_verify")]

    parity = {}
    for mix, layout, what, fn in routes:
        b = mixes[mix][0]
        if what == "rx_verify":                                  # the UDP frames are good, ARP is not IPv4
            fn(0)
            v = verdict_only.cpu().numpy()
            is_arp = np.zeros(n, dtype=bool)
            is_arp[b["rows"]] = True
            parity[(mix, layout, what)] = bool((v[is_arp] == 0).all() and (v[~is_arp] == 6).all())
            continue
        o = b["out"]
        for t in (o.headers, o.hdr_lens, o.chunk_index, o.status, o.records, o.reply_frame, o.seen_frame,
                  o.counts):
            t.view(torch.uint8).fill_(0xC3)
        fn(0)
        torch.cuda.synchronize()
        rec, hdr_len, lst, counts, slots = model(A, n, b["rows"], b["mac"], b["ip"])
        d_rows = torch.from_numpy(b["rows"]).to(dev)
        ring = o.headers.view(n, 64)
        got_slots = ring[d_rows].cpu().numpy()
        ring[d_rows] = 0xC3                                       # every other slot is untouched
        parity[(mix, layout, what)] = bool(
            o.records.cpu().numpy().tobytes() == rec.tobytes()
            and np.array_equal(o.status.cpu().numpy(), rec["status"])
            and np.array_equal(o.hdr_lens.cpu().numpy(), hdr_len)
            and not bool(o.chunk_index.any())
            and np.array_equal(o.reply_frame.cpu().numpy(), lst)
            and np.array_equal(o.seen_frame.cpu().numpy(), lst)
            and np.array_equal(o.counts.cpu().numpy(), counts)
            and np.array_equal(got_slots, slots) and bool((o.headers == 0xC3).all()))

    times = {r[:3]: [] for r in routes}
    events = []
    for step in range(args.warmup + args.steps):
        for mix, layout, what, fn in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(step)
            e1.record()
            if step >= args.warmup:
                events.append(((mix, layout, what), e0, e1))
    torch.cuda.synchronize()
    for key, e0, e1 in events:
        times[key].append(e0.elapsed_time(e1) * 1e3)

    lines = []
    for mix, layout, what, _ in routes:
        t = times[(mix, layout, what)]
        b = mixes[mix][0]
        lines.append({"route": what, "mix": mix, "layout": layout, "n": n, "arp_frames": int(b["rows"].size),
                      "frame_bytes": int(b["flat"].numel()), "us_min": round(min(t), 1),
                      "us_median": round(statistics.median(t), 1),
                      "model_parity": "ok" if parity[(mix, layout, what)] else "MISMATCH"})
    for mix in ("udp8", "arp60"):
        for layout in ("slots", "csr"):
            a = statistics.median(times[(mix, layout, "arp")])
            v = statistics.median(times[(mix, layout, "rx_verify")])
            lines.append({"mix": mix, "layout": layout, "arp_over_rx_verify_median": round(a / v, 3)})
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
