#!/usr/bin/env python3
"""Header-split Tx fill against the two routes a caller had before it, in ONE process.

Workload: N TCP segments as a send path holds them -- 54-byte headers (Ethernet + IPv4 + TCP)
in 64-byte slots of a header ring, 1460-byte payloads back to back in a send ring. Three
resident batches take turns so that no launch finds its bytes in the Infinity Cache. Routes,
alternating step by step, each launch timed with its own HIP event pair (5 warm-up + 20 timed
steps by default):

  hsplit     tx_fill_header_split on the split layout where it lies (both fields)
  linear     the in-place tx_fill on linearised copies of the same segments (both fields)
  chainfill  chksum_chain_fill on header node + payload chains (the L4 field only, host-made
             pseudo-header states, the field zeroed by the caller)

One JSON line per route: us min / median, bytes read, the fraction of 8 TB/s, ns per packet
byte, and an oracle parity word for rotation batch 0; then the gate line: the split fill's
time per packet byte must not exceed the linear fill's beyond the min-to-median spread the
alternation itself shows. Not part of the product.

    python tools/bench_tx_split.py [--n 1048576] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HDR, SLOT, PAY = 54, 64, 1460
PEAK = 8e12  # bytes per second


def make_headers(n, seed):
    """(n, 54) headers of exact-length TCP segments with 1460-byte payloads; junk in both
    checksum fields (the fills take them as 0)."""
    rng = np.random.default_rng(seed)
    eth = bytes([2, 0, 0x5E, 0x10, 0x20, 0x30, 2, 0x11, 0x22, 0x33, 0x44, 0x51, 8, 0])
    ip = struct.pack(">BBHHHBBH4s4s", 0x45, 0, 40 + PAY, 0, 0x4000, 64, 6, 0,
                     bytes([10, 20, 30, 101]), bytes([10, 20, 30, 40]))
    tcp = struct.pack(">HHIIHHHH", 40000, 80, 0, 0, (5 << 12) | 0x18, 0x2000, 0, 0)
    hdr = np.tile(np.frombuffer(eth + ip + tcp, dtype=np.uint8), (n, 1))
    hdr[:, 18:20] = rng.integers(0, 256, (n, 2), dtype=np.uint8)
    hdr[:, 26:30] = rng.integers(1, 255, (n, 4), dtype=np.uint8)
    hdr[:, 34:46] = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    hdr[:, 48:50] = rng.integers(0, 256, (n, 2), dtype=np.uint8)
    return hdr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    import aipstack_amd as A
    from aipstack_amd import _lib, synth

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    n = args.n
    orc = ctypes.CDLL(os.path.join(ROOT, "oracle", "build", "libchksum_oracle.so"))
    orc.oracle_tx_fill_batch.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint64, ctypes.c_void_p]

    lens = torch.full((n,), HDR, dtype=torch.int32, device=dev)
    clen1 = torch.full((n,), PAY, dtype=torch.int32, device=dev)
    index1 = torch.arange(n + 1, dtype=torch.int64, device=dev)
    lin_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * (HDR + PAY)
    clen2 = torch.tensor([20, PAY], dtype=torch.int32, device=dev).repeat(n)
    index2 = torch.arange(n + 1, dtype=torch.int64, device=dev) * 2
    ar = torch.arange(n, dtype=torch.int64, device=dev)

    batches = []
    for r in range(args.rotate):
        hdr = make_headers(n, 700 + r)
        slots = np.full((n, SLOT), 0xEE, dtype=np.uint8)
        slots[:, :HDR] = hdr
        d_slots = torch.from_numpy(slots.reshape(-1)).to(dev)
        d_pay = torch.empty(n * PAY, dtype=torch.uint8, device=dev)
        synth.fill_device(d_pay, synth.SEED_DATA + r)
        d_lin = torch.cat([d_slots.view(n, SLOT)[:, :HDR], d_pay.view(n, PAY)], dim=1).contiguous().view(-1)
        # route chainfill: its own header ring, L4 field zeroed; states = pseudo-header words
        d_slots_c = d_slots.clone()
        d_slots_c.view(n, SLOT)[:, 50:52] = 0
        h16 = hdr[:, 26:34].astype(np.uint32)
        states = (h16[:, 0::2] << 8 | h16[:, 1::2]).sum(axis=1) + 6 + 20 + PAY
        b = dict(
            slots=d_slots, pay=d_pay, lin=d_lin, slots_c=d_slots_c,
            addr1=d_pay.data_ptr() + ar * PAY,
            addr2=torch.stack([d_slots_c.data_ptr() + ar * SLOT + 34,
                               d_pay.data_ptr() + ar * PAY], dim=1).contiguous().view(-1),
            fields=d_slots_c.data_ptr() + ar * SLOT + 50,
            states=torch.from_numpy(states.astype(np.uint32).view(np.int32)).to(dev))
        batches.append(b)
    # the oracle's answer for rotation batch 0
    want = batches[0]["lin"].cpu().numpy().copy()
    want_st = np.empty(n, dtype=np.uint8)
    o64 = (np.arange(n + 1, dtype=np.uint64) * np.uint64(HDR + PAY))
    orc.oracle_tx_fill_batch(want.ctypes.data, o64.ctypes.data, n, want_st.ctypes.data)
    want2 = want.reshape(n, HDR + PAY)

    status = torch.empty(n, dtype=torch.uint8, device=dev)
    sums = torch.empty(n, dtype=torch.uint16, device=dev)
    ws = torch.empty(int(lib.aipstack_chksum_tx_fill_hsplit_workspace_bytes(n)), dtype=torch.uint8,
                     device=dev)

    def run_hsplit(b):
        A.tx_fill_header_split(b["slots"], SLOT, lens, b["addr1"], clen1, index1, out=status,
                               workspace=ws)

    def run_linear(b):
        A.tx_fill(b["lin"], lin_off, out=status)

    def run_chainfill(b):
        A.chksum_chain_fill(b["addr2"], clen2, index2, b["states"], b["fields"], out=sums)

    routes = [("hsplit", run_hsplit, n * (SLOT + PAY)), ("linear", run_linear, n * (HDR + PAY)),
              ("chainfill", run_chainfill, n * (20 + PAY))]

    # parity on rotation batch 0, one call each (chainfill needs its zeroed field: first call)
    parity = {}
    b0 = batches[0]
    run_hsplit(b0)
    torch.cuda.synchronize()
    got = b0["slots"].cpu().numpy().reshape(n, SLOT)
    parity["hsplit"] = bool(np.array_equal(status.cpu().numpy(), want_st)
                            and np.array_equal(got[:, :HDR], want2[:, :HDR])
                            and (got[:, HDR:] == 0xEE).all())
    run_linear(b0)
    torch.cuda.synchronize()
    parity["linear"] = bool(np.array_equal(status.cpu().numpy(), want_st)
                            and np.array_equal(b0["lin"].cpu().numpy(), want))
    run_chainfill(b0)
    torch.cuda.synchronize()
    got = b0["slots_c"].cpu().numpy().reshape(n, SLOT)
    parity["chainfill"] = bool(np.array_equal(got[:, 50:52], want2[:, 50:52]))
    del want, want2

    times = {name: [] for name, _, _ in routes}
    events = []
    for step in range(args.warmup + args.steps):
        b = batches[step % args.rotate]
        for name, fn, _ in routes:
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
    pkt_bytes = n * (HDR + PAY)
    for name, _, nbytes in routes:
        t = times[name]
        lo, med = min(t), statistics.median(t)
        lines.append({"route": name, "n": n, "us_min": round(lo, 1), "us_median": round(med, 1),
                      "bytes_read": nbytes, "frac_8TBs_median": round(nbytes / (med * 1e-6) / PEAK, 3),
                      "ns_per_packet_byte_median": round(med * 1e3 / pkt_bytes, 6),
                      "oracle_parity": "ok" if parity[name] else "MISMATCH"})
    by = {l["route"]: l for l in lines}
    spread = max(by[r]["us_median"] - by[r]["us_min"] for r in ("hsplit", "linear"))
    lines.append({"gate": "hsplit time per packet byte <= linear's, within the alternation's spread",
                  "hsplit_us_median": by["hsplit"]["us_median"],
                  "linear_us_median": by["linear"]["us_median"], "spread_us": round(spread, 1),
                  "holds": bool(by["hsplit"]["us_median"] <= by["linear"]["us_median"] + spread)})
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
