#!/usr/bin/env python3
"""TCP burst segmentation against the parent's way to the same bytes, in ONE process.

Workload: B bursts of S full segments each (default 16,384 x 64 x 1460 bytes): 54-byte headers
in 64-byte slots of a header ring, the payload back to back in a send ring. Three resident
batches take turns so that no launch finds its bytes in the Infinity Cache. Routes, alternating
step by step, each launch timed with its own HIP event pair (5 warm-up + 20 timed steps):

  tcpseg     tcp_tx_segment: descriptors resident; emits headers, chunk table, both checksums
  hsplit     tx_fill_header_split on the same segments with host-built headers and the chunk
             table already resident (the header upload is not counted)
  chainfill  chksum_chain_fill on header node + payload chains (the L4 field only): the floor

Every route is checked bit-exact on rotation batch 0 against the model: the per-segment fields
by the reference's rules (numpy, below), both checksums by the CPU oracle's Tx fill of the
linearised frames. One JSON line per route (us min / median, bytes read and written, the
fraction of 8 TB/s), then the gate line: the new route is no slower than the header-split fill
beyond the min-to-median spread of the alternation. Not part of the product.

    python tools/bench_tcp_segment.py [--bursts 16384] [--segs 64] [--out FILE]
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


def make_bursts(nb, segs, seed, dtype):
    """nb descriptors (data addresses still relative to the payload buffer) of `segs` full
    segments each; every third burst ends with FIN, PSH lies at the end of every burst."""
    rng = np.random.default_rng(seed)
    d = np.zeros(nb, dtype=dtype)
    per = segs * PAY
    d["data_addr"][:, 0] = np.arange(nb, dtype=np.uint64) * np.uint64(per)
    d["data_len"][:, 0] = per
    d["seq"] = rng.integers(0, 1 << 32, nb, dtype=np.uint64).astype(np.uint32)
    d["psh_offset"] = per
    d["mss"] = PAY
    d["ip_id"] = rng.integers(0, 1 << 16, nb).astype(np.uint16)
    d["flags"] = (np.arange(nb) % 3 == 0).astype(np.uint8)
    eth = bytes([2, 0, 0x5E, 0x10, 0x20, 0x30, 2, 0x11, 0x22, 0x33, 0x44, 0x51, 8, 0])
    ip = struct.pack(">BBHHHBBH4s4s", 0x45, 0, 0xA5A5, 0xA5A5, 0x4000, 64, 6, 0xA5A5,
                     bytes([10, 20, 30, 101]), bytes([10, 20, 30, 40]))
    tcp = struct.pack(">HHIIHHHH", 40000, 80, 0xA5A5A5A5, 0, 0xA5A5, 0x2000, 0xA5A5, 0)
    hdr = np.tile(np.frombuffer(eth + ip + tcp + b"\xA5\xA5", dtype=np.uint8), (nb, 1))
    hdr[:, 26:30] = rng.integers(1, 255, (nb, 4), dtype=np.uint8)    # source address
    hdr[:, 34:38] = rng.integers(0, 256, (nb, 4), dtype=np.uint8)    # ports
    hdr[:, 42:46] = rng.integers(0, 256, (nb, 4), dtype=np.uint8)    # ack
    hdr[:, 48:50] = rng.integers(0, 256, (nb, 2), dtype=np.uint8)    # window
    d["hdr"] = hdr
    return d


def model_headers(d, segs):
    """(n, 54) headers by the reference's per-segment rules (tcp/IpTcpProto_output.h:1079-1102,
    ip/IpStack.h:640-653) for bursts of `segs` full segments; both checksum fields 0."""
    nb = d.size
    k = np.tile(np.arange(segs, dtype=np.uint64), nb)
    rep = lambda a: np.repeat(a, segs, axis=0)                       # noqa: E731
    h = rep(d["hdr"][:, :HDR]).copy()
    start = k * np.uint64(PAY)
    seq = (rep(d["seq"]).astype(np.uint64) + start) & np.uint64(0xFFFFFFFF)
    psh = rep(d["psh_offset"]).astype(np.uint64)
    last = k == segs - 1
    fl = np.full(k.size, 0x5010, dtype=np.uint32)
    fl |= np.where((start < psh) & (psh <= start + np.uint64(PAY)), 0x08, 0).astype(np.uint32)
    fl |= np.where(last & (rep(d["flags"]) & 1).astype(bool), 0x09, 0).astype(np.uint32)
    ident = (rep(d["ip_id"]).astype(np.uint64) + k) & np.uint64(0xFFFF)

    def put(col, val, nbytes):
        for j in range(nbytes):
            h[:, col + j] = (val >> np.uint64(8 * (nbytes - 1 - j))).astype(np.uint64) & np.uint64(0xFF)
    put(16, np.full(k.size, 40 + PAY, dtype=np.uint64), 2)
    put(18, ident, 2)
    put(24, np.zeros(k.size, dtype=np.uint64), 2)
    put(38, seq, 4)
    put(46, fl.astype(np.uint64), 2)
    put(50, np.zeros(k.size, dtype=np.uint64), 2)
    return h


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

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    nb, segs = args.bursts, args.segs
    n = nb * segs
    orc = ctypes.CDLL(os.path.join(ROOT, "oracle", "build", "libchksum_oracle.so"))
    orc.oracle_tx_fill_batch.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint64, ctypes.c_void_p]

    lens = torch.full((n,), HDR, dtype=torch.int32, device=dev)
    clen1 = torch.full((n,), PAY, dtype=torch.int32, device=dev)
    index1 = torch.arange(n + 1, dtype=torch.int64, device=dev)
    clen2 = torch.tensor([20, PAY], dtype=torch.int32, device=dev).repeat(n)
    index2 = torch.arange(n + 1, dtype=torch.int64, device=dev) * 2
    ar = torch.arange(n, dtype=torch.int64, device=dev)

    batches = []
    want = None
    for r in range(args.rotate):
        d = make_bursts(nb, segs, 900 + r, A.TCP_BURST_DTYPE)
        d_pay = torch.empty(n * PAY, dtype=torch.uint8, device=dev)
        synth.fill_device(d_pay, synth.SEED_DATA + r)
        hdr = model_headers(d, segs)
        d["data_addr"][:, 0] += np.uint64(d_pay.data_ptr())
        si, cb = A.tcp_burst_layout(d)
        assert int(si[-1]) == n and int(cb[-1]) == n
        slots = np.full((n, SLOT), 0xEE, dtype=np.uint8)
        slots[:, :HDR] = hdr
        slots[:, 24:26] = 0xA5                                      # junk: the fill takes them as 0
        slots[:, 50:52] = 0xA5
        d_slots = torch.from_numpy(slots.reshape(-1)).to(dev)
        d_slots_c = d_slots.clone()
        d_slots_c.view(n, SLOT)[:, 50:52] = 0
        h16 = hdr[:, 26:34].astype(np.uint32)
        states = (h16[:, 0::2] << 8 | h16[:, 1::2]).sum(axis=1) + 6 + 20 + PAY
        b = dict(
            bursts=torch.from_numpy(d.view(np.uint8).copy()).to(dev),
            si=torch.from_numpy(si.view(np.int64)).to(dev), cb=torch.from_numpy(cb.view(np.int64)).to(dev),
            seg=A.TcpSegments(torch.full((n * SLOT,), 0xEE, dtype=torch.uint8, device=dev), SLOT,
                              torch.zeros(n, dtype=torch.int64, device=dev),
                              torch.zeros(n, dtype=torch.int32, device=dev),
                              torch.zeros(n + 1, dtype=torch.int64, device=dev),
                              torch.zeros(n, dtype=torch.uint8, device=dev)),
            slots=d_slots, pay=d_pay, slots_c=d_slots_c, addr1=d_pay.data_ptr() + ar * PAY,
            addr2=torch.stack([d_slots_c.data_ptr() + ar * SLOT + 34,
                               d_pay.data_ptr() + ar * PAY], dim=1).contiguous().view(-1),
            fields=d_slots_c.data_ptr() + ar * SLOT + 50,
            states=torch.from_numpy(states.astype(np.uint32).view(np.int32)).to(dev))
        batches.append(b)
        if r == 0:  # the model's answer for rotation batch 0: the oracle fills the linear frames
            lin = np.concatenate([hdr, d_pay.cpu().numpy().reshape(n, PAY)], axis=1).reshape(-1)
            st = np.empty(n, dtype=np.uint8)
            o64 = np.arange(n + 1, dtype=np.uint64) * np.uint64(HDR + PAY)
            orc.oracle_tx_fill_batch(lin.ctypes.data, o64.ctypes.data, n, st.ctypes.data)
            assert (st == 6).all()
            want = lin.reshape(n, HDR + PAY)[:, :HDR].copy()
            del lin

    status = torch.empty(n, dtype=torch.uint8, device=dev)
    sums = torch.empty(n, dtype=torch.uint16, device=dev)
    ws = torch.empty(max(int(lib.aipstack_chksum_tx_fill_hsplit_workspace_bytes(n)),
                         int(lib.aipstack_tcp_tx_segment_workspace_bytes(n))), dtype=torch.uint8,
                     device=dev)

    def run_tcpseg(b):
        A.tcp_tx_segment(b["bursts"], b["si"], b["cb"], out=b["seg"], workspace=ws, n_segments=n,
                         n_chunks=n)

    def run_hsplit(b):
        A.tx_fill_header_split(b["slots"], SLOT, lens, b["addr1"], clen1, index1, out=status,
                               workspace=ws)

    def run_chainfill(b):
        A.chksum_chain_fill(b["addr2"], clen2, index2, b["states"], b["fields"], out=sums)

    desc_bytes = nb * 96 + 2 * (nb + 1) * 8
    routes = [("tcpseg", run_tcpseg, n * PAY + desc_bytes, n * (SLOT + 8 + 4 + 8 + 1)),
              ("hsplit", run_hsplit, n * (SLOT + PAY + 4 + 8 + 4 + 8), n * (2 + 2 + 1)),
              ("chainfill", run_chainfill, n * (20 + PAY + 2 * (8 + 4) + 8 + 4 + 8), n * (2 + 2))]

    parity = {}
    b0 = batches[0]
    run_tcpseg(b0)
    torch.cuda.synchronize()
    got = b0["seg"].headers.cpu().numpy().reshape(n, SLOT)
    parity["tcpseg"] = bool(
        (b0["seg"].status.cpu().numpy() == 6).all() and np.array_equal(got[:, :HDR], want)
        and (got[:, HDR:] == 0).all()
        and np.array_equal(b0["seg"].chunk_addr.cpu().numpy(), b0["addr1"].cpu().numpy())
        and np.array_equal(b0["seg"].chunk_len.cpu().numpy(), clen1.cpu().numpy())
        and np.array_equal(b0["seg"].chunk_index.cpu().numpy(), index1.cpu().numpy()))
    run_hsplit(b0)
    torch.cuda.synchronize()
    got = b0["slots"].cpu().numpy().reshape(n, SLOT)
    parity["hsplit"] = bool((status.cpu().numpy() == 6).all() and np.array_equal(got[:, :HDR], want)
                            and (got[:, HDR:] == 0xEE).all())
    run_chainfill(b0)
    torch.cuda.synchronize()
    got = b0["slots_c"].cpu().numpy().reshape(n, SLOT)
    parity["chainfill"] = bool(np.array_equal(got[:, 50:52], want[:, 50:52]))

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
        lines.append({"route": name, "bursts": nb, "n": n, "us_min": round(lo, 1),
                      "us_median": round(med, 1), "bytes_read": rd, "bytes_written": wr,
                      "frac_8TBs_median": round((rd + wr) / (med * 1e-6) / PEAK, 3),
                      "model_parity": "ok" if parity[name] else "MISMATCH"})
    by = {l["route"]: l for l in lines}
    spread = max(by[r]["us_median"] - by[r]["us_min"] for r in ("tcpseg", "hsplit"))
    lines.append({"gate": "tcpseg is no slower than hsplit, within the alternation's spread",
                  "tcpseg_us_median": by["tcpseg"]["us_median"],
                  "hsplit_us_median": by["hsplit"]["us_median"], "spread_us": round(spread, 1),
                  "holds": bool(by["tcpseg"]["us_median"] <= by["hsplit"]["us_median"] + spread)})
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
