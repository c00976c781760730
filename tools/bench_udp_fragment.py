#!/usr/bin/env python3
"""UDP send with IPv4 fragmentation against the TCP burst segmentation of the same payload bytes
and the chain-fill floor, in ONE process.

Workload: B datagrams of S full fragments each on mtu 1500 (default 16,384 x 44 x 1480 bytes of IP
payload: 8 + D <= 65535 admits at most 44 full fragments of 1480 bytes, so the 64 of a TCP burst
cannot be had), headers in 64-byte slots of a header ring, the payload back to back. Three
resident batches take turns so that no launch finds its bytes in the Infinity Cache. Routes,
alternating step by step, each launch timed with its own HIP event pair (5 warm-up + 20 timed
steps):

  udpfrag    udp_tx_fragment: descriptors resident; emits headers, chunk table, every IPv4 header
             checksum and one UDP checksum per datagram
  tcpseg     tcp_tx_segment over the same payload bytes at mss 1480 (one TCP checksum per segment)
  chainfill  chksum_chain_fill over the same payload, one chain per datagram with the UDP header
             node in front (the L4 field only): the floor

The new route is checked bit-exact on rotation batch 0 against the model: the per-fragment fields
by the reference's rules and the IPv4 header checksums in numpy, the UDP checksum as the
big-endian word sum of pseudo-header, UDP header and payload. One JSON line per route (us min /
median, bytes read and written, the fraction of 8 TB/s), then the gate line: the new route's
median is no worse than tcp_tx_segment's beyond the min-to-median spread of the alternation. Not
part of the product.

    python tools/bench_udp_fragment.py [--dgrams 16384] [--frags 44] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOT, MTU, F = 64, 1500, 1480
PEAK = 8e12  # bytes per second


def fold(x):
    x = (x & 0xFFFF) + (x >> 16)
    x = (x & 0xFFFF) + (x >> 16)
    return (x & 0xFFFF) + (x >> 16)


def make_dgrams(nd, D, seed, dtype):
    """nd descriptors (data addresses still relative to the payload buffer) of D payload bytes."""
    rng = np.random.default_rng(seed)
    g = np.zeros(nd, dtype=dtype)
    g["data_addr"][:, 0] = np.arange(nd, dtype=np.uint64) * np.uint64(D)
    g["data_len"][:, 0] = D
    g["mtu"] = MTU
    g["ip_id"] = rng.integers(0, 1 << 16, nd).astype(np.uint16)
    eth = bytes([2, 0, 0x5E, 0x10, 0x20, 0x30, 2, 0x11, 0x22, 0x33, 0x44, 0x51, 8, 0])
    ip = struct.pack(">BBHHHBBH4s4s", 0x45, 0, 0xA5A5, 0xA5A5, 0, 64, 17, 0xA5A5,
                     bytes([10, 20, 30, 101]), bytes([10, 20, 30, 40]))
    udp = struct.pack(">HHHH", 40000, 53, 0xA5A5, 0xA5A5)
    hdr = np.tile(np.frombuffer(eth + ip + udp + b"\xA5" * 6, dtype=np.uint8), (nd, 1))
    hdr[:, 26:30] = rng.integers(1, 255, (nd, 4), dtype=np.uint8)    # source address
    hdr[:, 34:38] = rng.integers(0, 256, (nd, 4), dtype=np.uint8)    # ports
    g["hdr"] = hdr
    return g


def model_slots(g, S, D, pay):
    """(nd * S, 64) slots by the reference's rules for datagrams of S full fragments."""
    nd = g.size
    n = nd * S
    k = np.tile(np.arange(S, dtype=np.uint64), nd)
    rep = lambda a: np.repeat(a, S, axis=0)                          # noqa: E731
    s = np.zeros((n, SLOT), dtype=np.uint8)
    s[:, :34] = rep(g["hdr"][:, :34])

    def be(col, val):
        s[:, col] = (val >> np.uint64(8)).astype(np.uint8)
        s[:, col + 1] = (val & np.uint64(0xFF)).astype(np.uint8)
    be(16, np.full(n, 20 + F, dtype=np.uint64))
    be(18, rep(g["ip_id"]).astype(np.uint64))
    be(20, np.where(k < S - 1, 0x2000, 0).astype(np.uint64) | (k * np.uint64(F // 8)))
    s[:, 24:26] = 0
    w = s[:, 14:34].astype(np.uint64)
    be(24, np.uint64(0xFFFF) - fold((w[:, 0::2] << np.uint64(8) | w[:, 1::2]).sum(axis=1)))
    first = np.arange(nd) * S
    P = 8 + D
    s[first, 34:38] = g["hdr"][:, 34:38]
    s[first, 38], s[first, 39] = P >> 8, P & 0xFF
    a = g["hdr"][:, 26:38].astype(np.uint64)
    seed = (a[:, 0::2] << np.uint64(8) | a[:, 1::2]).sum(axis=1) + np.uint64(17 + 2 * P)
    data = np.zeros(nd, dtype=np.uint64)
    slab = 1024
    for lo in range(0, nd, slab):
        blk = pay[lo * D:min(nd, lo + slab) * D].reshape(-1, D)
        data[lo:lo + blk.shape[0]] = blk.view(">u2").sum(axis=1, dtype=np.uint64)
    chk = np.uint64(0xFFFF) - fold(seed + data)
    chk = np.where(chk == 0, np.uint64(0xFFFF), chk)
    s[first, 40], s[first, 41] = (chk >> np.uint64(8)).astype(np.uint8), (chk & np.uint64(0xFF)).astype(np.uint8)
    return s, seed, chk


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
    from aipstack_amd import _lib, synth

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    nd, S = args.dgrams, args.frags
    D = S * F - 8
    assert 2 <= S and 8 + D <= 65535 and D % 2 == 0
    n = nd * S

    batches, want = [], None
    clen2 = torch.tensor([8, D], dtype=torch.int32, device=dev).repeat(nd)
    index2 = torch.arange(nd + 1, dtype=torch.int64, device=dev) * 2
    ar = torch.arange(nd, dtype=torch.int64, device=dev)
    for r in range(args.rotate):
        g = make_dgrams(nd, D, 700 + r, A.UDP_DGRAM_DTYPE)
        d_pay = torch.empty(nd * D, dtype=torch.uint8, device=dev)
        synth.fill_device(d_pay, synth.SEED_DATA + r)
        slots = seed = None
        if r == 0:
            slots, seed, _ = model_slots(g, S, D, d_pay.cpu().numpy())
            want = slots
        g["data_addr"][:, 0] += np.uint64(d_pay.data_ptr())
        fi, cb, st = A.udp_dgram_layout(g)
        assert int(fi[-1]) == n and int(cb[-1]) == n and (st == 6).all()
        # the TCP route: one burst per datagram over the same bytes at mss 1480
        t = np.zeros(nd, dtype=A.TCP_BURST_DTYPE)
        t["data_addr"], t["data_len"] = g["data_addr"], g["data_len"]
        t["mss"], t["ip_id"], t["psh_offset"] = F, g["ip_id"], D
        th = np.zeros((nd, 56), dtype=np.uint8)
        th[:, :34] = g["hdr"][:, :34]
        th[:, 23] = 6
        th[:, 34:38] = g["hdr"][:, 34:38]
        t["hdr"] = th
        si, tcb = A.tcp_burst_layout(t)
        assert int(si[-1]) == n and int(tcb[-1]) == n
        # the floor: per datagram a chain of its 8 UDP header bytes (length set, field 0) and payload
        uh = np.zeros((nd, 8), dtype=np.uint8)
        uh[:, :4] = g["hdr"][:, 34:38]
        uh[:, 4], uh[:, 5] = (8 + D) >> 8, (8 + D) & 0xFF
        d_uh = torch.from_numpy(uh.reshape(-1)).to(dev)
        a16 = g["hdr"][:, 26:34].astype(np.uint32)
        states = (a16[:, 0::2] << 8 | a16[:, 1::2]).sum(axis=1) + 17 + 8 + D
        mk = lambda cnt, dt: torch.zeros(cnt, dtype=dt, device=dev)      # noqa: E731
        batches.append(dict(
            dgrams=torch.from_numpy(g.view(np.uint8).copy()).to(dev),
            fi=torch.from_numpy(fi.view(np.int64)).to(dev), cb=torch.from_numpy(cb.view(np.int64)).to(dev),
            frags=A.UdpFragments(torch.full((n * SLOT,), 0xEE, dtype=torch.uint8, device=dev), SLOT,
                                 mk(n, torch.int32), mk(n, torch.int64), mk(n, torch.int32),
                                 mk(n + 1, torch.int64), mk(n, torch.uint8), mk(nd, torch.uint8)),
            bursts=torch.from_numpy(t.view(np.uint8).copy()).to(dev),
            si=torch.from_numpy(si.view(np.int64)).to(dev), tcb=torch.from_numpy(tcb.view(np.int64)).to(dev),
            seg=A.TcpSegments(torch.full((n * SLOT,), 0xEE, dtype=torch.uint8, device=dev), SLOT,
                              mk(n, torch.int64), mk(n, torch.int32), mk(n + 1, torch.int64),
                              mk(n, torch.uint8)),
            pay=d_pay, uh=d_uh,
            addr2=torch.stack([d_uh.data_ptr() + ar * 8, d_pay.data_ptr() + ar * D], dim=1).contiguous().view(-1),
            fields=d_uh.data_ptr() + ar * 8 + 6,
            states=torch.from_numpy(states.astype(np.uint32).view(np.int32)).to(dev)))

    sums = torch.empty(nd, dtype=torch.uint16, device=dev)
    ws = torch.empty(max(int(lib.aipstack_udp_tx_fragment_workspace_bytes(nd, n)),
                         int(lib.aipstack_tcp_tx_segment_workspace_bytes(n))), dtype=torch.uint8,
                     device=dev)

    def run_udpfrag(b):
        A.udp_tx_fragment(b["dgrams"], b["fi"], b["cb"], out=b["frags"], workspace=ws, n_frags=n,
                          n_chunks=n)

    def run_tcpseg(b):
        A.tcp_tx_segment(b["bursts"], b["si"], b["tcb"], out=b["seg"], workspace=ws, n_segments=n,
                         n_chunks=n)

    def run_chainfill(b):
        b["uh"].view(nd, 8)[:, 6:8] = 0          # (the field is summed: as the reference zeroes it)
        A.chksum_chain_fill(b["addr2"], clen2, index2, b["states"], b["fields"], out=sums,
                            zero_as_ffff=True)

    pay_bytes = nd * D
    routes = [("udpfrag", run_udpfrag, pay_bytes + nd * 80 + 2 * (nd + 1) * 8,
               n * (SLOT + 4 + 8 + 4 + 8 + 1) + nd),
              ("tcpseg", run_tcpseg, pay_bytes + nd * 96 + 2 * (nd + 1) * 8, n * (SLOT + 8 + 4 + 8 + 1)),
              ("chainfill", run_chainfill, pay_bytes + nd * (8 + 2 * (8 + 4) + 8 + 4 + 8), nd * (2 + 2))]

    b0 = batches[0]
    run_udpfrag(b0)
    torch.cuda.synchronize()
    f = b0["frags"]
    got = f.headers.cpu().numpy().reshape(n, SLOT)
    k = np.tile(np.arange(S), nd)
    want_addr = b0["pay"].data_ptr() + np.repeat(np.arange(nd, dtype=np.int64) * D, S) + \
        np.where(k == 0, 0, k * F - 8)
    parity = {"udpfrag": bool(
        (f.status.cpu().numpy() == 6).all() and (f.dgram_status.cpu().numpy() == 6).all()
        and np.array_equal(got, want)
        and np.array_equal(f.hdr_lens.cpu().numpy(), np.where(k == 0, 42, 34))
        and np.array_equal(f.chunk_addr.cpu().numpy(), want_addr)
        and np.array_equal(f.chunk_len.cpu().numpy(), np.where(k == 0, F - 8, F))
        and np.array_equal(f.chunk_index.cpu().numpy(), np.arange(n + 1)))}
    run_tcpseg(b0)
    torch.cuda.synchronize()
    parity["tcpseg"] = bool((b0["seg"].status.cpu().numpy() == 6).all())
    run_chainfill(b0)
    torch.cuda.synchronize()
    first = np.arange(nd) * S
    parity["chainfill"] = bool(np.array_equal(b0["uh"].cpu().numpy().reshape(nd, 8)[:, 6:8],
                                              want[first, 40:42]))

    times = {name: [] for name, *_ in routes}
    events = []
    for step in range(args.warmup + args.steps):
        b = batches[step % args.rotate]
        for name, fn, _, _ in routes:
            if name == "chainfill":
                b["uh"].view(nd, 8)[:, 6:8] = 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if name == "chainfill":
                A.chksum_chain_fill(b["addr2"], clen2, index2, b["states"], b["fields"], out=sums,
                                    zero_as_ffff=True)
            else:
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
    spread = max(by[r]["us_median"] - by[r]["us_min"] for r in ("udpfrag", "tcpseg"))
    lines.append({"gate": "udpfrag is no slower than tcpseg, within the alternation's spread",
                  "udpfrag_us_median": by["udpfrag"]["us_median"],
                  "tcpseg_us_median": by["tcpseg"]["us_median"], "spread_us": round(spread, 1),
                  "holds": bool(by["udpfrag"]["us_median"] <= by["tcpseg"]["us_median"] + spread)})
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
