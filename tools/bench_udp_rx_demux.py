#!/usr/bin/env python3
"""UDP Rx demux against Rx verify alone and against TCP Rx parse, in ONE process.

Workload: n UDP frames (default 1,048,576) of 42 + 1472 bytes back to back with valid checksums
(the product's own Tx fill; batch 0 re-verified by the CPU oracle), all for the interface's
address. Half go to open ports: three in eight of all frames to one of 8 listeners, one in eight
to one of 4,096 associations; half go to closed ports and ask for a port unreachable. Three
resident batches take turns so that no launch finds its bytes in the Infinity Cache. Routes,
alternating step by step, each launch timed with its own HIP event pair (5 warm-up + 20 timed
steps):

  udp_demux  udp_rx_demux: Rx verify, then the demux, scan and emit passes
  rx_verify  rx_verify alone on the same frames: the yardstick
  tcp_parse  tcp_rx_parse on the same number of TCP frames of the same size with a 65,536-entry
             table (one resident batch set of its own): the neighbour the extra is set beside

udp_demux is checked on rotation batch 0 against the model before timing: verdicts by the CPU
oracle; records, codes, delivery list and counts by the rules in numpy (below; the frames have
one shape). One JSON line per route (us min / median), then a line with the extras over
rx_verify. Not part of the product.

    python tools/bench_udp_rx_demux.py [--frames 1048576] [--out FILE]
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

HDR, PAY, FRAME = 42, 1472, 1514
LOCAL_IP, BCAST_IP = 0x0A141E28, 0x0A141EFF
LISTENERS, ASSOCS = 8, 4096
LIS_PORT, ASSOC_PORT, CLOSED_PORT = 5000, 6000, 20000
TCP_TABLE = 65536


def make_headers(n, seed):
    """(n, 42) header bytes with checksum fields 0, and per frame its class (0 closed, 1
    listener, 2 association), remote address and ports."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    cls = np.where(k % 2 == 0, 0, np.where(k % 8 == 7, 2, 1))
    peer = rng.integers(0, ASSOCS, n)
    ra = (np.uint32(0x0B000000) + peer).astype(np.uint32)
    sport = np.where(cls == 2, 30000 + peer % 1000, rng.integers(1024, 65536, n))
    dport = np.where(cls == 0, CLOSED_PORT + rng.integers(0, 30000, n),
                     np.where(cls == 1, LIS_PORT + k // 2 % LISTENERS, ASSOC_PORT))
    h = np.zeros((n, HDR), dtype=np.uint8)
    eth = bytes([2, 0, 0x5E, 0x10, 0x20, 0x30, 2, 0x11, 0x22, 0x33, 0x44, 0x51, 8, 0])
    ip = struct.pack(">BBHHHBBHII", 0x45, 0, 20 + 8 + PAY, 0, 0x4000, 64, 17, 0, 0, LOCAL_IP)
    h[:, :34] = np.frombuffer(eth + ip, dtype=np.uint8)

    def put(col, val, nbytes):
        v = np.asarray(val).astype(np.uint64)
        for j in range(nbytes):
            h[:, col + j] = (v >> np.uint64(8 * (nbytes - 1 - j))) & np.uint64(0xFF)
    put(18, rng.integers(0, 1 << 16, n), 2)
    put(26, ra, 4)
    put(34, sport, 2)
    put(36, dport, 2)
    put(38, np.full(n, 8 + PAY), 2)
    return h, cls, peer, ra, sport, dport


def make_tables(A):
    lis = np.zeros(LISTENERS, dtype=A.UDP_LISTENER_DTYPE)
    lis["port"], lis["cookie"] = LIS_PORT + np.arange(LISTENERS), 1 + np.arange(LISTENERS)
    keys = np.zeros(ASSOCS, dtype=A.TCP_PCB_KEY_DTYPE)
    p = np.arange(ASSOCS)
    keys["local_addr"], keys["local_port"] = LOCAL_IP, ASSOC_PORT
    keys["remote_addr"], keys["remote_port"] = 0x0B000000 + p, 30000 + p % 1000
    keys["cookie"] = p
    return lis, A.tcp_pcb_table_sort(keys)


def model(A, cls, peer, ra, sport, dport):
    """Records, codes, delivery list and counts by the rules of chksum.h for the one frame shape."""
    n = cls.size
    d = np.zeros(n, dtype=A.UDP_RX_DGRAM_DTYPE)
    d["remote_addr"], d["local_addr"], d["remote_port"], d["local_port"] = ra, LOCAL_IP, sport, dport
    d["data_off"], d["data_len"], d["ttl"] = HDR, PAY, 64
    d["flags"] = A.AIPSTACK_UDP_DGRAM_VALID | A.AIPSTACK_UDP_DGRAM_HAS_CHKSUM | A.AIPSTACK_UDP_DGRAM_DST_LOCAL
    d["listeners"] = np.where(cls == 1, np.uint64(1) << (dport - LIS_PORT).clip(0, 63).astype(np.uint64), 0)
    d["assoc"] = np.where(cls == 2, peer, 0xFFFFFFFF)
    code = np.where(cls == 0, 3, 0xFF).astype(np.uint8)
    deliver = np.full(n, -1, dtype=np.int64)
    idx = np.flatnonzero(cls != 0)
    deliver[:idx.size] = idx
    return d, code, deliver, np.array([idx.size, n - idx.size], dtype=np.int64)


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

    lis, keys = make_tables(A)
    d_lis = torch.from_numpy(lis.view(np.uint8).copy()).to(dev)
    d_keys = torch.from_numpy(keys.view(np.uint8).copy()).to(dev)
    iface = A.icmp_iface(LOCAL_IP, BCAST_IP, bytes([2, 0, 0x5E, 0x10, 0x20, 0x30]))
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(FRAME)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    ws = torch.empty(A.udp_rx_demux_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def filled(h, seed):
        d_fr = torch.empty(n * FRAME, dtype=torch.uint8, device=dev)
        synth.fill_device(d_fr, seed)
        d_fr.view(n, FRAME)[:, :h.shape[1]] = torch.from_numpy(h).to(dev)
        assert bool((A.tx_fill(d_fr, d_off) == 6).all())           # valid checksums
        return d_fr

    batches, want = [], None
    for r in range(args.rotate):
        h, cls, peer, ra, sport, dport = make_headers(n, 700 + r)
        d_fr = filled(h, synth.SEED_DATA + 60 + r)
        batches.append(dict(frames=d_fr, out=A.UdpRxDemuxed(
            torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n * 32, dtype=torch.uint8, device=dev),
            torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
            torch.empty(2, dtype=torch.int64, device=dev))))
        if r == 0:
            host = d_fr.cpu().numpy()
            verdict = np.empty(n, dtype=np.uint8)
            orc.oracle_rx_verify_batch(host.ctypes.data, off.ctypes.data, n, verdict.ctypes.data)
            del host
            want = (verdict,) + model(A, cls, peer, ra, sport, dport)
        del h
    verdict_only = torch.empty(n, dtype=torch.uint8, device=dev)

    # the neighbour: TCP frames of the same size, one in TCP_TABLE + a tenth connections
    rng = np.random.default_rng(9)
    conns = TCP_TABLE + TCP_TABLE // 9
    t_ra = rng.permutation(1 << 20)[:conns].astype(np.uint32) + np.uint32(0x0B000000)
    t_rp = rng.integers(1024, 65536, conns).astype(np.uint16)
    tkeys = np.zeros(TCP_TABLE, dtype=A.TCP_PCB_KEY_DTYPE)
    tkeys["local_addr"], tkeys["local_port"] = LOCAL_IP, 80
    tkeys["remote_addr"], tkeys["remote_port"], tkeys["cookie"] = t_ra[:TCP_TABLE], t_rp[:TCP_TABLE], 1 + np.arange(TCP_TABLE)
    d_tkeys = torch.from_numpy(A.tcp_pcb_table_sort(tkeys).view(np.uint8).copy()).to(dev)
    tcp_batches = []
    for r in range(args.rotate):
        conn = np.random.default_rng(800 + r).integers(0, conns, n)
        h = np.zeros((n, 54), dtype=np.uint8)
        eth = bytes([2, 0, 0x5E, 0x10, 0x20, 0x30, 2, 0x11, 0x22, 0x33, 0x44, 0x51, 8, 0])
        h[:, :34] = np.frombuffer(eth + struct.pack(">BBHHHBBHII", 0x45, 0, 1500, 0, 0x4000, 64, 6, 0, 0,
                                                     LOCAL_IP), dtype=np.uint8)
        h[:, 26:30] = t_ra[conn].astype(">u4").view(np.uint8).reshape(n, 4)
        h[:, 34:36] = t_rp[conn].astype(">u2").view(np.uint8).reshape(n, 2)
        h[:, 36:38] = (0, 80)
        h[:, 46:48] = (0x50, 0x10)
        tcp_batches.append(dict(frames=filled(h, synth.SEED_DATA + 80 + r), out=A.TcpRxParsed(
            torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n * 32, dtype=torch.uint8, device=dev),
            torch.empty(n, dtype=torch.int32, device=dev))))
        del h

    def run_demux(step):
        b = batches[step % args.rotate]
        o = b["out"]
        A.udp_rx_demux(b["frames"], d_off, iface, d_keys, d_lis, verdict=o.verdict, dgrams=o.dgrams,
                       unreach_code=o.unreach_code, deliver_frame=o.deliver_frame, counts=o.counts,
                       workspace=ws)

    def run_verify(step):
        A.rx_verify(batches[step % args.rotate]["frames"], d_off, out=verdict_only)

    def run_tcp(step):
        b = tcp_batches[step % args.rotate]
        o = b["out"]
        A.tcp_rx_parse(b["frames"], d_off, d_tkeys, verdict=o.verdict, segs=o.segs, pcb=o.pcb)

    def run_tcp_verify(step):
        A.rx_verify(tcp_batches[step % args.rotate]["frames"], d_off, out=verdict_only)

    routes = [("udp_demux", run_demux), ("rx_verify", run_verify), ("tcp_parse", run_tcp),
              ("tcp_rx_verify", run_tcp_verify)]

    run_demux(0)
    torch.cuda.synchronize()
    o = batches[0]["out"]
    parity = bool((want[0] == 6).all() and np.array_equal(o.verdict.cpu().numpy(), want[0])
                  and o.dgrams_numpy().tobytes() == want[1].tobytes()
                  and np.array_equal(o.unreach_code.cpu().numpy(), want[2])
                  and np.array_equal(o.deliver_frame.cpu().numpy(), want[3])
                  and np.array_equal(o.counts.cpu().numpy(), want[4]))

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
        lines.append({"route": name, "n": n, "frame_bytes": FRAME, "listeners": LISTENERS, "assocs": ASSOCS,
                      "us_min": round(min(t), 1), "us_median": round(statistics.median(t), 1),
                      "model_parity": ("ok" if parity else "MISMATCH") if name == "udp_demux" else "n/a"})
    by = {l["route"]: l["us_median"] for l in lines}
    udp_extra = by["udp_demux"] - by["rx_verify"]
    tcp_extra = by["tcp_parse"] - by["tcp_rx_verify"]
    lines.append({"udp_extra_us_median": round(udp_extra, 1), "tcp_extra_us_median": round(tcp_extra, 1),
                  "udp_extra_fraction_of_rx_verify": round(udp_extra / by["rx_verify"], 3),
                  "udp_extra_over_tcp_extra": round(udp_extra / tcp_extra, 2) if tcp_extra > 0 else None})
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
