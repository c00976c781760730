#!/usr/bin/env python3
"""IPv4 reassembly on receive against Rx verify alone and the chained-batch floor, in ONE process.

Workload: what udp_tx_fragment's benchmark emits, as received: B datagrams of S full fragments
each (default 16,384 x 44 x 1480 bytes of IP payload) as back-to-back 1514-byte frames, the
fragments of a datagram in order, the datagrams interleaved four at a time (frame i belongs to
datagram 4 * (i // 4S) + i % 4, fragment (i % 4S) // 4). Three resident batches take turns so that
no launch finds its bytes in the Infinity Cache. Routes, alternating step by step, each launch
timed with its own HIP event pair (5 warm-up + 20 timed steps):

  reassemble  ip4_rx_reassemble: Rx verify, classify, insert, the chained batch, link, finish
  rxverify    rx_verify alone on the same frames (fragments: headers only)
  chain       chksum_batch_chain over the same one-chunk-per-frame table: the floor, it reads the
              same payload once

The new route is checked bit-exact on rotation batch 0 against the model in closed form: every
frame verdict 14, its chunk the 1480 bytes at frame byte 34, head / next by the interleaving, one
record per datagram at its first fragment (44 fragments, 65,120 bytes, UDP, ACCEPT: the UDP
checksum is made here from torch sums of the payload, not by the library). One JSON line per
route (us min / median, bytes read and written, the fraction of 8 TB/s), then the gate line: the
new call's overhead over the chain floor is no worse than tcp_rx_parse's measured overhead over
rx_verify (53 % at the median), within the min-to-median spread of the alternation.
Bytes: reassemble reads each frame's payload once (chain), its 34 header bytes twice (verify,
classify), the offsets twice, and the workspace records three times; it writes the six outputs
(37 B per frame), the workspace (30 B per frame) and the cleared tables (16 B per slot). Not part
of the product.

    python tools/bench_ip_reassemble.py [--dgrams 16384] [--frags 44] [--out FILE]
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

FRAME, HDR, F = 1514, 34, 1480
PEAK = 8e12  # bytes per second
PARSE_OVER_VERIFY = 0.53


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dgrams", type=int, default=16384)
    ap.add_argument("--frags", type=int, default=44)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    import aipstack_amd as A
    from aipstack_amd import synth

    dev = torch.device("cuda", 0)
    nd, S = args.dgrams, args.frags
    assert nd % 4 == 0 and 2 <= S and S * F <= 65531
    n = nd * S
    P = S * F                                            # the reassembled length: UDP header + data

    i = torch.arange(n, dtype=torch.int64, device=dev)
    dg = 4 * (i // (4 * S)) + i % 4                      # datagram of frame i
    k = (i % (4 * S)) // 4                               # its fragment number
    first = (dg // 4) * (4 * S) + dg % 4                 # frame of the datagram's fragment 0

    def be16(t, col, val):
        t[:, col] = (val >> 8).to(torch.uint8)
        t[:, col + 1] = (val & 0xFF).to(torch.uint8)

    def words(t):                                        # big-endian 16-bit word sums per row
        w = t.to(torch.int64)
        return (w[:, 0::2] * 256 + w[:, 1::2]).sum(dim=1)

    def fold(x):
        for _ in range(3):
            x = (x & 0xFFFF) + (x >> 16)
        return x

    batches = []
    offsets = (torch.arange(n + 1, dtype=torch.int64, device=dev) * FRAME)
    for r in range(args.rotate):
        buf = torch.empty(n * FRAME, dtype=torch.uint8, device=dev)
        synth.fill_device(buf, synth.SEED_DATA + 40 + r)
        fr = buf.view(n, FRAME)
        g = torch.Generator(device="cpu").manual_seed(900 + r)
        src = torch.randint(1, 255, (nd, 4), generator=g, dtype=torch.int64).to(torch.uint8).to(dev)
        ident = torch.randint(0, 1 << 16, (nd,), generator=g, dtype=torch.int64).to(dev)
        hdr = torch.zeros((n, HDR), dtype=torch.uint8, device=dev)
        hdr[:, 0:12] = torch.tensor([2, 0, 0x5E, 0x10, 0x20, 0x30, 2, 0x11, 0x22, 0x33, 0x44, 0x51],
                                    dtype=torch.uint8, device=dev)
        hdr[:, 12], hdr[:, 14] = 0x08, 0x45
        be16(hdr, 16, torch.full_like(i, 20 + F))
        be16(hdr, 18, ident[dg])
        be16(hdr, 20, torch.where(k < S - 1, 0x2000, 0) | (k * (F // 8)))
        hdr[:, 22], hdr[:, 23] = 64, 17
        hdr[:, 26:30] = src[dg]
        hdr[:, 30:34] = torch.tensor([10, 20, 30, 40], dtype=torch.uint8, device=dev)
        be16(hdr, 24, 0xFFFF - fold(words(hdr[:, 14:34])))
        fr[:, :HDR] = hdr
        # the UDP header in fragment 0: ports as they fell, length P, checksum over the datagram
        f0 = first[::1].unique()
        head = fr[f0]
        head[:, HDR + 4], head[:, HDR + 5] = P >> 8, P & 0xFF
        head[:, HDR + 6:HDR + 8] = 0
        fr[f0] = head
        pay = torch.zeros(n, dtype=torch.int64, device=dev)
        slab = 1 << 16
        for lo in range(0, n, slab):
            pay[lo:lo + slab] = words(fr[lo:lo + slab, HDR:])
        per = torch.zeros(nd, dtype=torch.int64, device=dev).index_add_(0, dg, pay)
        d0 = dg[f0]
        seed = words(fr[f0][:, 26:34]) + 17 + P
        chk = 0xFFFF - fold(per[d0] + seed)
        chk = torch.where(chk == 0, torch.full_like(chk, 0xFFFF), chk)
        head = fr[f0]
        be16(head, HDR + 6, chk)
        fr[f0] = head
        mk = lambda cnt, dt: torch.zeros(cnt, dtype=dt, device=dev)      # noqa: E731
        batches.append(dict(buf=buf, verdict=mk(n, torch.uint8), chunk_addr=mk(n, torch.int64),
                            chunk_len=mk(n, torch.int32), next=mk(n, torch.int32),
                            head=mk(n, torch.int32), dgram=mk(n * 16, torch.uint8)))
        del hdr, pay

    ws = torch.empty(A.ip4_reass_workspace_bytes(n), dtype=torch.uint8, device=dev)
    slots = 64
    while slots < 4 * n:
        slots *= 2
    vout = torch.empty(n, dtype=torch.uint8, device=dev)
    sums = torch.empty(n, dtype=torch.uint16, device=dev)
    index = torch.arange(n + 1, dtype=torch.int64, device=dev)

    def run_reassemble(b):
        A.ip4_rx_reassemble(b["buf"], offsets, verdict=b["verdict"], chunk_addr=b["chunk_addr"],
                            chunk_len=b["chunk_len"], next=b["next"], head=b["head"],
                            dgram=b["dgram"], workspace=ws)

    def run_rxverify(b):
        A.rx_verify(b["buf"], offsets, out=vout)

    def run_chain(b):
        A.chksum_batch_chain(b["chunk_addr"], b["chunk_len"], index, out=sums)

    pay_bytes = n * F
    routes = [("reassemble", run_reassemble, pay_bytes + n * (2 * HDR + 2 * 8 + 3 * 16 + 8 + 8 + 4 + 4 + 2),
               n * (37 + 30) + 16 * slots),
              ("rxverify", run_rxverify, n * (HDR + 8), n),
              ("chain", run_chain, pay_bytes + n * (8 + 4 + 8), n * 2)]

    b0 = batches[0]
    run_reassemble(b0)
    torch.cuda.synchronize()
    want_next = torch.where(k < S - 1, i + 4, torch.full_like(i, -1)).to(torch.int32)
    dgr = b0["dgram"].cpu().numpy().view(A.IP4_DGRAM_DTYPE)
    want_d = np.zeros(n, dtype=A.IP4_DGRAM_DTYPE)
    heads = (k == 0).cpu().numpy()
    hi = np.nonzero(heads)[0]
    want_d["n_frags"][hi], want_d["last_frame"][hi] = S, hi + 4 * (S - 1)
    want_d["data_len"][hi], want_d["proto"][hi], want_d["verdict"][hi] = P, 17, 6
    parity = {"reassemble": bool(
        (b0["verdict"] == 14).all() and torch.equal(b0["next"], want_next)
        and torch.equal(b0["head"], first.to(torch.int32))
        and torch.equal(b0["chunk_addr"], b0["buf"].data_ptr() + i * FRAME + HDR)
        and (b0["chunk_len"] == F).all() and dgr.tobytes() == want_d.tobytes())}
    run_rxverify(b0)
    torch.cuda.synchronize()
    parity["rxverify"] = bool((vout == 3).all())
    run_chain(b0)
    torch.cuda.synchronize()
    want_s = fold(torch.cat([words(b0["buf"].view(n, FRAME)[lo:lo + (1 << 16), HDR:])
                             for lo in range(0, n, 1 << 16)]))
    parity["chain"] = bool(torch.equal(sums.to(torch.int64) & 0xFFFF, want_s))
    for b in batches[1:]:                                # the chain route reads each batch's table
        run_reassemble(b)
    torch.cuda.synchronize()

    times = {name: [] for name, *_ in routes}
    events = []
    for step in range(args.warmup + args.steps):
        b = batches[step % args.rotate]
        for name, fn, _, _ in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(b)
            e1.record()
            if step >= args.warmup:
                events.append((name, e0, e1))
    torch.cuda.synchronize()
    for name, e0, e1 in events:
        times[name].append(e0.elapsed_time(e1) * 1e3)

    lines = []
    for name, _, rd, wr in routes:
        t = times[name]
        lo, med = min(t), statistics.median(t)
        lines.append({"route": name, "dgrams": nd, "frags_per_dgram": S, "n": n, "us_min": round(lo, 1),
                      "us_median": round(med, 1), "bytes_read": rd, "bytes_written": wr,
                      "frac_8TBs_median": round((rd + wr) / (med * 1e-6) / PEAK, 3),
                      "model_parity": "ok" if parity[name] else "MISMATCH"})
    by = {l["route"]: l for l in lines}
    new, floor, ver = (by[r]["us_median"] for r in ("reassemble", "chain", "rxverify"))
    spread = max(by[r]["us_median"] - by[r]["us_min"] for r in ("reassemble", "chain"))
    over = (new - floor) / floor
    lines.append({"gate": "overhead over the chain floor <= tcp_rx_parse's over rx_verify (0.53), "
                          "within the alternation's spread",
                  "reassemble_us_median": new, "chain_us_median": floor, "rxverify_us_median": ver,
                  "overhead_over_floor": round(over, 3), "spread_us": round(spread, 1),
                  "lane_passes_us_by_subtraction": round(new - floor - ver, 1),
                  "holds": bool(new <= floor * (1 + PARSE_OVER_VERIFY) + spread)})
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
