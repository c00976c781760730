"""TEST INFRASTRUCTURE -- reference-produced answers for the TCP Rx parse: the reference's own
ParseTcpOptions (tcp/TcpOptions.h:63-125) and TcpPcbKeyCompare::CompareKeys
(tcp/TcpPcbKey.h:52-86), compiled from the reference tree (tcp_rx_ref_gen.cpp only includes the
two headers) and run on the inputs below. The answers are recorded in tcp_rx_ref_cases.json:

  {"options": ["<hex option bytes>:<flags>:<mss>:<wnd_scale>", ...],
   "keys": ["<la> <ra> <lp> <rp> <la> <ra> <lp> <rp>:<CompareKeys>", ...]}   (hex fields)

    python3 tests/golden/tcp_rx_ref.py <reference tree>      # rewrites the fixture

Only `random.Random(seed).getrandbits` is used (a stable Mersenne Twister stream).
"""
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "tcp_rx_ref_cases.json")
GEN_SRC = os.path.join(HERE, "tcp_rx_ref_gen.cpp")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "tcp_rx_ref_gen")

MSS = bytes([2, 4, 0x05, 0xB4])
WS = bytes([3, 3, 7])

# One or more buffers per branch of ParseTcpOptions.
CRAFTED = [
    b"",                                   # nothing
    bytes([0]),                            # End alone
    bytes([1]),                            # Nop alone
    bytes([1, 1, 1, 1]),                   # Nops
    MSS,                                   # MSS
    WS + bytes([1]),                       # window scale, Nop
    MSS + bytes([1]) + WS,                 # both (the form WriteTcpOptions sends)
    WS + bytes([0]) + MSS,                 # End before MSS: only the window scale
    bytes([0]) + MSS,                      # End first: nothing
    bytes([1, 1]) + MSS + bytes([0, 0]),   # Nops, MSS, End padding
    bytes([2]),                            # MSS kind, no length byte left
    bytes([3]),                            # window-scale kind, no length byte left
    bytes([1, 1, 1, 8]),                   # unknown kind as the last byte
    MSS + bytes([3]),                      # flag set, then no length byte: the flag stays
    bytes([2, 0, 5, 0xB4]),                # length 0: stop
    bytes([2, 1, 5, 0xB4]),                # length 1: stop
    bytes([8, 1]),                         # unknown kind, length 1: stop
    WS + bytes([2, 1]) + MSS,              # flag set, then a stop: later MSS never read
    bytes([2, 4, 5]),                      # MSS data beyond the bytes left: stop
    bytes([3, 3]),                         # window-scale data beyond the bytes left
    bytes([8, 10, 1, 2, 3, 4, 5, 6, 7]),   # unknown option one byte short: stop
    bytes([8, 10, 1, 2, 3, 4, 5, 6, 7, 8]),  # unknown option that just fits
    bytes([2, 3, 9]) + MSS,                # MSS with 1 data byte: skipped; then a good one
    bytes([2, 5, 9, 9, 9]) + WS,           # MSS with 3 data bytes: skipped
    bytes([2, 2]) + MSS,                   # MSS with no data: skipped
    bytes([3, 2]) + WS,                    # window scale with no data: skipped
    bytes([3, 4, 9, 9]) + MSS,             # window scale with 2 data bytes: skipped
    bytes([3, 4, 9, 9]),                   # ... and nothing else
    bytes([8, 2]) + MSS,                   # unknown option without data
    bytes([8, 10, 1, 2, 3, 4, 5, 6, 7, 8]) + MSS + WS + bytes([0]),   # timestamps-like, then both
    bytes([4, 2, 5, 10, 1, 2, 3, 4, 1, 2, 3, 4]) + WS + bytes([1]),   # SACK-permitted, SACK
    MSS + bytes([2, 4, 0x02, 0x18]),       # a later MSS overrides
    WS + bytes([3, 3, 14]),                # a later window scale overrides
    MSS + WS + bytes([2, 4, 0xFF, 0xFF, 3, 3, 0]),   # both overridden, extreme values
    MSS + bytes([2, 3, 9]),                # a later MSS of the wrong length does not override
    bytes([2, 4, 0, 0]),                   # MSS 0
    bytes([3, 3, 255]),                    # window scale 255
    bytes([1] * 36) + MSS,                 # the last option bytes of 40
    bytes([1] * 37) + WS,                  # window scale ending at byte 39
    bytes([1] * 38) + bytes([2, 4]),       # MSS cut by the end of 40 bytes
    bytes([8, 40] + [0xAA] * 38),          # one option of all 40 bytes
    bytes([8, 41] + [0xAA] * 38),          # ... one byte too long
    bytes([8, 255, 1, 2]),                 # length 255
    bytes([2, 4, 1, 0, 0, 2, 4, 9, 9]),    # End after the first MSS
]

ALPHABET = [0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 8, 2, 3, 4, 40, 255, 7]
N_RANDOM = 2000
N_KEY_RANDOM = 380


class _Rng:
    def __init__(self, seed):
        self._r = random.Random(seed)

    def below(self, n):
        if n <= 1:
            return 0
        b = (n - 1).bit_length()
        while True:
            v = self._r.getrandbits(b)
            if v < n:
                return v


def option_inputs():
    rng = _Rng(20260901)
    out = list(CRAFTED)
    for i in range(N_RANDOM):
        n = rng.below(41)
        kind = i % 4
        if kind == 0:      # bytes of the small alphabet
            b = bytes(ALPHABET[rng.below(len(ALPHABET))] for _ in range(n))
        elif kind == 1:    # well-formed options back to back, cut at n bytes
            parts = []
            while sum(map(len, parts)) < n:
                parts.append([MSS, WS, bytes([1]), bytes([1]), bytes([8, 4, 1, 2]),
                              bytes([2, 4, rng.below(256), rng.below(256)]),
                              bytes([3, 3, rng.below(256)]), bytes([4, 2]),
                              bytes([2, 2 + rng.below(4)]), bytes([3, 2 + rng.below(3)]),
                              bytes([0])][rng.below(11)] if rng.below(12) else bytes([rng.below(256)]))
            b = b"".join(parts)[:n]
        elif kind == 2:    # well-formed with one byte changed
            b = bytearray((MSS + bytes([1]) + WS + bytes([8, 6, 1, 2, 3, 4]) + MSS + WS +
                           bytes([1]) * 40)[:n])
            if n:
                b[rng.below(n)] = ALPHABET[rng.below(len(ALPHABET))]
            b = bytes(b)
        else:              # any bytes
            b = bytes(rng.below(256) for _ in range(n))
        out.append(b)
    return out


def key_inputs():
    """Pairs (la, ra, lp, rp) x 2: equal keys, keys that differ in exactly one field (both ways,
    with the other fields pulling the other way where they are compared later), random pairs
    from a small set of values (equal fields are likely), random 32/16-bit values."""
    rng = _Rng(20260902)
    base = (0x0A141E28, 0x0A141E64, 0x1234, 40000)
    out = [(base, base)]
    for f in range(4):
        for d in (1, -1, 0x100, -0x100):
            k = list(base)
            k[f] += d
            out.append((base, tuple(k)))
            out.append((tuple(k), base))
            for g in range(4):        # a second field differs the other way
                if g != f:
                    k2 = list(k)
                    k2[g] -= d
                    out.append((base, tuple(k2)))
    addrs = [0, 1, 0x0A141E28, 0x0A141E64, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    ports = [0, 1, 80, 255, 256, 0x7FFF, 0x8000, 0xFFFF]
    while len(out) < 120 + N_KEY_RANDOM:
        if rng.below(4):
            a = (addrs[rng.below(7)], addrs[rng.below(7)], ports[rng.below(8)], ports[rng.below(8)])
            b = (addrs[rng.below(7)], addrs[rng.below(7)], ports[rng.below(8)], ports[rng.below(8)])
            if rng.below(2):
                b = (a[0], b[1], a[2], a[3]) if rng.below(2) else (b[0], a[1], b[2], a[3])
        else:
            a = (rng.below(1 << 32), rng.below(1 << 32), rng.below(1 << 16), rng.below(1 << 16))
            b = (rng.below(1 << 32), rng.below(1 << 32), rng.below(1 << 16), rng.below(1 << 16))
        out.append((a, b))
    return out


def build_generator(reference):
    os.makedirs(os.path.dirname(GEN_BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(reference, "src"), "-o", GEN_BIN,
                    GEN_SRC], check=True)
    return GEN_BIN


def generate(reference):
    """The fixture's text, from the reference's code run on the inputs above."""
    gen = build_generator(reference)
    opts, keys = option_inputs(), key_inputs()
    req = ["O " + (b.hex() or "-") for b in opts]
    req += ["K " + " ".join("%x" % v for v in a + b) for a, b in keys]
    ans = subprocess.run([gen], input="\n".join(req) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert len(ans) == len(req) + 1 and ans[-1] == ""
    doc = {"options": [], "keys": []}
    for b, line in zip(opts, ans):
        fl, mss, ws = line.split()
        doc["options"].append("%s:%s:%s:%s" % (b.hex(), fl, mss, ws))
    for (a, b), line in zip(keys, ans[len(opts):]):
        doc["keys"].append(" ".join("%x" % v for v in a + b) + ":" + line.strip())
    return json.dumps(doc, indent=0, separators=(",", ":")) + "\n"


def load():
    """(options [(bytes, flags, mss, wnd_scale)], keys [((la, ra, lp, rp), (..), result)])."""
    with open(FIXTURE) as f:
        doc = json.load(f)
    opts = []
    for s in doc["options"]:
        h, fl, mss, ws = s.split(":")
        opts.append((bytes.fromhex(h), int(fl), int(mss), int(ws)))
    keys = []
    for s in doc["keys"]:
        k, r = s.split(":")
        v = [int(x, 16) for x in k.split()]
        keys.append((tuple(v[:4]), tuple(v[4:]), int(r)))
    return opts, keys


if __name__ == "__main__":
    text = generate(sys.argv[1])
    with open(FIXTURE, "w") as f:
        f.write(text)
    print("%s: %d bytes" % (FIXTURE, len(text)))
