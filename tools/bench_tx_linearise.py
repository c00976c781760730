#!/usr/bin/env python3
"""Linearising header-split Tx segments against a contiguous copy of the same bytes, in ONE
process.

Workload: N TCP segments as tcp_tx_segment leaves them -- 54-byte headers in 64-byte slots of a
header ring, 1460-byte payloads back to back in a send ring. Three resident batches take turns
so that no launch finds its bytes in the Infinity Cache. Routes, alternating step by step, each
launch timed with its own HIP event pair (5 warm-up + 20 timed steps by default):

  slots     (a) tx_linearise_slotted into 2048-byte slots
  csr       (b) tx_linearise to back-to-back CSR frames
  memcpy    (c) the yardstick of the same run: one contiguous device-to-device copy of the same
                number of bytes (hipMemcpyAsync through torch's copy_)
  tcpseg    (d) tcp_tx_segment alone
  tcpseg+csr (e) tcp_tx_segment + tx_linearise: descriptors to linear frames

One JSON line per route: us min / median, bytes read and written, (a) and (b) as a ratio of (c),
and a model parity word for rotation batch 0 (plain concatenation of header and payload); then
the statement under test: route (b)'s median is within the min-to-median spread of (c) plus what
64 MB of extra header-slot reads cost at the copy's own rate. Not part of the product.

    python tools/bench_tx_linearise.py [--bursts 16384] [--segs 64] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

HDR, SLOT, PAY, RING = 54, 64, 1460, 2048
L = HDR + PAY


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bursts", type=int, default=16384)
    ap.add_argument("--segs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    import aipstack_amd as A
    from aipstack_amd import _lib, synth
    from bench_tcp_segment import make_bursts

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    nb, segs = args.bursts, args.segs
    n = nb * segs
    ws = torch.empty(int(lib.aipstack_tcp_tx_segment_workspace_bytes(n)), dtype=torch.uint8,
                     device=dev)

    def new_segments():
        return A.TcpSegments(torch.full((n * SLOT,), 0xEE, dtype=torch.uint8, device=dev), SLOT,
                             torch.zeros(n, dtype=torch.int64, device=dev),
                             torch.zeros(n, dtype=torch.int32, device=dev),
                             torch.zeros(n + 1, dtype=torch.int64, device=dev),
                             torch.zeros(n, dtype=torch.uint8, device=dev))

    batches = []
    for r in range(args.rotate):
        d = make_bursts(nb, segs, 900 + r, A.TCP_BURST_DTYPE)
        d_pay = torch.empty(n * PAY, dtype=torch.uint8, device=dev)
        synth.fill_device(d_pay, synth.SEED_DATA + r)
        d["data_addr"][:, 0] += np.uint64(d_pay.data_ptr())
        si, cb = A.tcp_burst_layout(d)
        assert int(si[-1]) == n and int(cb[-1]) == n
        b = dict(bursts=torch.from_numpy(d.view(np.uint8).copy()).to(dev),
                 si=torch.from_numpy(si.view(np.int64)).to(dev),
                 cb=torch.from_numpy(cb.view(np.int64)).to(dev), pay=d_pay, seg=new_segments(),
                 src=torch.empty(n * L, dtype=torch.uint8, device=dev))
        A.tcp_tx_segment(b["bursts"], b["si"], b["cb"], out=b["seg"], workspace=ws, n_segments=n,
                         n_chunks=n)
        synth.fill_device(b["src"], synth.SEED_DATA + 10 + r)
        batches.append(b)
    torch.cuda.synchronize()
    assert (batches[0]["seg"].status.cpu().numpy() == 6).all()

    ring = torch.empty(n * RING, dtype=torch.uint8, device=dev)
    flat = torch.empty(n * L, dtype=torch.uint8, device=dev)
    flat2 = torch.empty(n * L, dtype=torch.uint8, device=dev)
    offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)

    def run_slots(b):
        A.tx_linearise_slotted(ring, RING, b["seg"], frame_max=L, lens=lens, status=status)

    def run_csr(b):
        A.tx_linearise(flat, offsets, b["seg"], frame_max=L, lens=lens, status=status)

    def run_memcpy(b):
        flat2.copy_(b["src"])

    def run_tcpseg(b):
        A.tcp_tx_segment(b["bursts"], b["si"], b["cb"], out=b["seg"], workspace=ws, n_segments=n,
                         n_chunks=n)

    def run_both(b):
        run_tcpseg(b)
        run_csr(b)

    rd_lin, wr_lin = n * (SLOT + PAY + 4 + 4 + 8 + 8 + 4), n * (L + 4 + 1)
    routes = [("slots", run_slots, rd_lin, wr_lin), ("csr", run_csr, rd_lin + 8 * n, wr_lin),
              ("memcpy", run_memcpy, n * L, n * L), ("tcpseg", run_tcpseg, None, None),
              ("tcpseg+csr", run_both, None, None)]

    # parity on rotation batch 0: plain concatenation of each header with its payload
    b0 = batches[0]
    want = np.concatenate([b0["seg"].headers.cpu().numpy().reshape(n, SLOT)[:, :HDR],
                           b0["pay"].cpu().numpy().reshape(n, PAY)], axis=1)
    parity = {}
    ring.fill_(0xA5)
    run_slots(b0)
    torch.cuda.synchronize()
    ok = bool((status.cpu().numpy() == A.AIPSTACK_TX_LIN_WRITTEN).all()
              and (lens.cpu().numpy() == L).all())
    for lo in range(0, n, 1 << 16):   # in pieces: the ring is 2 GiB
        got = ring[lo * RING:(lo + (1 << 16)) * RING].cpu().numpy().reshape(-1, RING)
        ok = ok and np.array_equal(got[:, :L], want[lo:lo + got.shape[0]]) \
            and bool((got[:, L:] == 0xA5).all())
    parity["slots"] = ok
    flat.fill_(0xA5)
    run_csr(b0)
    torch.cuda.synchronize()
    parity["csr"] = bool((status.cpu().numpy() == A.AIPSTACK_TX_LIN_WRITTEN).all()
                         and np.array_equal(flat.cpu().numpy().reshape(n, L), want))
    run_memcpy(b0)
    torch.cuda.synchronize()
    parity["memcpy"] = bool(torch.equal(flat2, b0["src"]))
    run_both(b0)
    torch.cuda.synchronize()
    parity["tcpseg"] = parity["tcpseg+csr"] = bool(
        np.array_equal(flat.cpu().numpy().reshape(n, L), want))
    del want

    times = {name: [] for name, *_ in routes}
    events = []
    for step in range(args.warmup + args.steps):
        b = batches[step % args.rotate]
        for name, fn, *_ in routes:
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
        line = {"route": name, "n": n, "us_min": round(min(t), 1),
                "us_median": round(statistics.median(t), 1),
                "model_parity": "ok" if parity[name] else "MISMATCH"}
        if rd is not None:
            line.update(bytes_read=rd, bytes_written=wr)
        lines.append(line)
    by = {l["route"]: l for l in lines}
    c = by["memcpy"]
    for r in ("slots", "csr"):
        by[r]["ratio_to_memcpy_median"] = round(by[r]["us_median"] / c["us_median"], 3)
    spread = c["us_median"] - c["us_min"]
    extra = 64e6 / ((c["bytes_read"] + c["bytes_written"]) / c["us_median"])
    lines.append({"statement": "csr median <= memcpy median + memcpy's min-to-median spread + "
                               "64 MB of reads at the copy's rate",
                  "csr_us_median": by["csr"]["us_median"], "memcpy_us_median": c["us_median"],
                  "spread_us": round(spread, 1), "extra_reads_us": round(extra, 1),
                  "holds": bool(by["csr"]["us_median"] <= c["us_median"] + spread + extra)})
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
