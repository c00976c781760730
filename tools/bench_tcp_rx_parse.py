#!/usr/bin/env python3
"""TCP Rx parse against Rx verify alone, in ONE process.

Workload: n TCP frames (default 1,048,576) of 54 + 1460 bytes back to back with valid checksums
(the product's own Tx fill; batch 0 re-verified by the CPU oracle). A tenth of them carry 12
option bytes (MSS, Nop, window scale, four Nops) in front of 1448 data bytes. The PCB table has
65,536 entries; the frames belong to 72,818 connections chosen uniformly, the first 65,536 of
which are in the table, so about 90 % of the frames hit. Three resident batches take turns so
that no launch finds its bytes in the Infinity Cache. Routes, alternating step by step, each
launch timed with its own HIP event pair (5 warm-up + 20 timed steps):

  rx_parse   tcp_rx_parse: Rx verify, then the parse pass (records, options, PCB lookup)
  rx_verify  rx_verify alone on the same frames: the yardstick

rx_parse is checked on rotation batch 0 against the model before timing: verdicts by the CPU
oracle, the record fields, the options and the cookies by the reference's rules in numpy (below;
the frames have two fixed shapes). One JSON line per route (us min / median), then a line with
the added time as a fraction of rx_verify's median. Not part of the product.

    python tools/bench_tcp_rx_parse.py [--frames 1048576] [--out FILE]
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

HDR, PAY, FRAME = 54, 1460, 1514
OPTS = bytes([2, 4, 0x05, 0xB4, 1, 3, 3, 7, 1, 1, 1, 1])
LOCAL_IP, LOCAL_PORT = 0x0A141E28, 80
TABLE, CONNS = 65536, 72818


def make_connections(seed):
    """CONNS distinct (remote_addr, remote_port) pairs; the first TABLE of them are PCBs."""
    rng = np.random.default_rng(seed)
    ra = rng.permutation(1 << 20)[:CONNS].astype(np.uint32) + np.uint32(0x0B000000)
    rp = rng.integers(1024, 65536, CONNS).astype(np.uint16)
    return ra, rp


def make_headers(n, ra, rp, seed):
    """(n, 66) header bytes (54, plus the 12 option bytes of every tenth frame), checksum fields
    0, and the connection of each frame."""
    rng = np.random.default_rng(seed)
    conn = rng.integers(0, CONNS, n)
    has_opt = np.arange(n) % 10 == 3
    h = np.zeros((n, HDR + 12), dtype=np.uint8)
    eth = bytes([2, 0, 0x5E, 0x10, 0x20, 0x30, 2, 0x11, 0x22, 0x33, 0x44, 0x51, 8, 0])
    ip = struct.pack(">BBHHHBBHII", 0x45, 0, 20 + 20 + PAY, 0, 0x4000, 64, 6, 0, 0, LOCAL_IP)
    h[:, :34] = np.frombuffer(eth + ip, dtype=np.uint8)

    def put(col, val, nbytes):
        v = val.astype(np.uint64)
        for j in range(nbytes):
            h[:, col + j] = (v >> np.uint64(8 * (nbytes - 1 - j))) & np.uint64(0xFF)
    f = dict(ident=rng.integers(0, 1 << 16, n), seq=rng.integers(0, 1 << 32, n, dtype=np.uint64),
             ack=rng.integers(0, 1 << 32, n, dtype=np.uint64), window=rng.integers(0, 1 << 16, n),
             flags=np.where(has_opt, 0x8012, 0x5010) | (rng.integers(0, 2, n) << 3))
    put(18, f["ident"], 2)
    put(26, ra[conn], 4)
    put(34, rp[conn], 2)
    put(36, np.full(n, LOCAL_PORT), 2)
    put(38, f["seq"], 4)
    put(42, f["ack"], 4)
    put(46, f["flags"], 2)
    put(48, f["window"], 2)
    h[has_opt, HDR:] = np.frombuffer(OPTS, dtype=np.uint8)
    return h, conn, has_opt, f


def model_records(dtype, ra, rp, conn, has_opt, f):
    """The records and cookies by the reference's rules for the two frame shapes
    (tcp/IpTcpProto_input.h:81-126, tcp/TcpOptions.h:63-125): offset 5 without options, offset 8
    with MSS 1460 and window scale 7; cookie = 1 + the connection's number when it is a PCB."""
    n = conn.size
    s = np.zeros(n, dtype=dtype)
    s["remote_addr"], s["local_addr"] = ra[conn], LOCAL_IP
    s["remote_port"], s["local_port"] = rp[conn], LOCAL_PORT
    s["seq_num"], s["ack_num"] = f["seq"], f["ack"]
    s["flags"], s["window_size"] = f["flags"], f["window"]
    s["data_off"] = np.where(has_opt, HDR + 12, HDR)
    s["data_len"] = np.where(has_opt, PAY - 12, PAY)
    s["mss"] = np.where(has_opt, 1460, 0)
    s["wnd_scale"] = np.where(has_opt, 7, 0)
    s["opts"] = np.where(has_opt, 0x83, 0x80)
    pcb = np.where(conn < TABLE, conn + 1, 0xFFFFFFFF).astype(np.uint32)
    return s, pcb


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
    n = args.frames
    orc = ctypes.CDLL(os.path.join(ROOT, "oracle", "build", "libchksum_oracle.so"))
    orc.oracle_rx_verify_batch.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint64, ctypes.c_void_p]

    ra, rp = make_connections(77)
    keys = np.zeros(TABLE, dtype=A.TCP_PCB_KEY_DTYPE)
    keys["local_addr"], keys["local_port"] = LOCAL_IP, LOCAL_PORT
    keys["remote_addr"], keys["remote_port"] = ra[:TABLE], rp[:TABLE]
    keys["cookie"] = np.arange(TABLE) + 1
    d_table = torch.from_numpy(A.tcp_pcb_table_sort(keys).view(np.uint8).copy()).to(dev)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(FRAME)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)

    batches, want = [], None
    for r in range(args.rotate):
        h, conn, has_opt, f = make_headers(n, ra, rp, 500 + r)
        d_fr = torch.empty(n * FRAME, dtype=torch.uint8, device=dev)
        synth.fill_device(d_fr, synth.SEED_DATA + 40 + r)
        v = d_fr.view(n, FRAME)
        d_h = torch.from_numpy(h).to(dev)
        v[:, :HDR] = d_h[:, :HDR]
        idx = torch.from_numpy(np.nonzero(has_opt)[0]).to(dev)
        v[idx, HDR:HDR + 12] = d_h[idx, HDR:]
        st = A.tx_fill(d_fr, d_off)                                 # valid checksums
        assert bool((st == 6).all())
        batches.append(dict(frames=d_fr, out=A.TcpRxParsed(
            torch.empty(n, dtype=torch.uint8, device=dev),
            torch.empty(n * 32, dtype=torch.uint8, device=dev),
            torch.empty(n, dtype=torch.int32, device=dev))))
        if r == 0:
            host = d_fr.cpu().numpy()
            verdict = np.empty(n, dtype=np.uint8)
            orc.oracle_rx_verify_batch(host.ctypes.data, off.ctypes.data, n, verdict.ctypes.data)
            del host
            want = (verdict,) + model_records(A.TCP_RX_SEG_DTYPE, ra, rp, conn, has_opt, f)
        del d_h, h
    verdict_only = torch.empty(n, dtype=torch.uint8, device=dev)

    def run_parse(b):
        o = b["out"]
        A.tcp_rx_parse(b["frames"], d_off, d_table, verdict=o.verdict, segs=o.segs, pcb=o.pcb)

    def run_verify(b):
        A.rx_verify(b["frames"], d_off, out=verdict_only)

    routes = [("rx_parse", run_parse), ("rx_verify", run_verify)]

    b0 = batches[0]
    run_parse(b0)
    torch.cuda.synchronize()
    o = b0["out"]
    hits = float((want[2] != 0xFFFFFFFF).mean())
    parity = bool((want[0] == 6).all() and np.array_equal(o.verdict.cpu().numpy(), want[0])
                  and o.segs_numpy().tobytes() == want[1].tobytes()
                  and np.array_equal(o.pcb_numpy(), want[2]))

    times = {name: [] for name, _ in routes}
    events = []
    for step in range(args.warmup + args.steps):
        b = batches[step % args.rotate]
        for name, fn in routes:
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
    for name, _ in routes:
        t = times[name]
        lines.append({"route": name, "n": n, "pcbs": TABLE, "hit_fraction": round(hits, 3),
                      "us_min": round(min(t), 1), "us_median": round(statistics.median(t), 1),
                      "model_parity": ("ok" if parity else "MISMATCH") if name == "rx_parse" else "n/a"})
    by = {l["route"]: l for l in lines}
    added = by["rx_parse"]["us_median"] - by["rx_verify"]["us_median"]
    lines.append({"added_us_median": round(added, 1),
                  "added_fraction_of_rx_verify": round(added / by["rx_verify"]["us_median"], 3),
                  "within_25_percent": bool(added <= 0.25 * by["rx_verify"]["us_median"])})
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
