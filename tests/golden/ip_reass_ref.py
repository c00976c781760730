"""TEST INFRASTRUCTURE -- reference-produced answers for IPv4 reassembly: the reference's own
IpReassembly::reassembleIp4 (ip/IpReassembly.h:181-386), compiled from the reference tree
(ip_reass_ref_gen.cpp only includes that header; the platform is a stub of this project's: a clock
that stands still, a timer that does nothing) and run on the arrival sequences below. The answers
are recorded in ip_reass_ref_cases.json:

  {"sequences": ["<config>|<ident> <src> <dst> <ttl> <proto> <mf> <offset> <len> <salt>;...|<answer>;...", ...]}

one answer per call: "0" (false) or "1 <length> <FNV-1a 64 of the reassembled bytes>". A
fragment's payload byte k is (salt + 3 * (offset + k)) & 0xFF, so the fixture holds no payload.
Configs: (MaxReassSize, MaxReassHoles) = CONFIGS[config], 8 entries each.

    python3 tests/golden/ip_reass_ref.py <reference tree>      # rewrites the fixture

Only `random.Random(seed).getrandbits` is used (a stable Mersenne Twister stream).
"""
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "ip_reass_ref_cases.json")
GEN_SRC = os.path.join(HERE, "ip_reass_ref_gen.cpp")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "ip_reass_ref_gen")

CONFIGS = ((65531, 250), (2000, 250), (576, 250), (2000, 2))
N_RANDOM = 320


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

    def shuffle(self, xs):
        for i in range(len(xs) - 1, 0, -1):
            j = self.below(i + 1)
            xs[i], xs[j] = xs[j], xs[i]


def payload(off, ln, salt):
    return bytes((salt + 3 * (off + k)) & 0xFF for k in range(ln))


def fnv(data):
    f = 0xcbf29ce484222325
    for c in data:
        f = ((f ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return f


def _cut(total, cuts, salt=1):
    """[(mf, offset, len, salt)] of a datagram of `total` bytes cut at `cuts`."""
    e = [0] + list(cuts) + [total]
    return [(int(b != total), a, b - a, salt) for a, b in zip(e, e[1:])]


def _seq(cfg, frags, ident=7, src=0x0A000001, dst=0x0A000002, proto=17):
    return (cfg, [(ident, src, dst, 64, proto) + f for f in frags])


def crafted():
    """Arrival orders, duplicates, overlaps, oversize, small holes, last-fragment rules, the hole
    bound, an empty fragment, two keys that differ in one field only."""
    out = []
    p = _cut(100, [40, 80])
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2)):
        out.append(_seq(0, [p[i] for i in order]))
    out.append(_seq(0, [p[0], p[1], (1, 40, 40, 9), p[2]]))             # duplicate, other bytes
    out.append(_seq(0, [p[0], p[0], p[1], p[2], p[2]]))                 # a last fragment twice: late
    out.append(_seq(0, [p[0], p[1], (1, 32, 16, 5), p[2]]))             # overlap, then complete
    out.append(_seq(0, [p[0], (1, 32, 16, 5), p[1], p[2]]))
    out.append(_seq(0, [p[2], (0, 80, 21, 1), p[0], p[1]]))             # a second last, other end
    out.append(_seq(0, [p[2], (1, 96, 8, 1), p[0], p[1]]))              # data beyond the last
    out.append(_seq(0, [(1, 96, 8, 1), p[2], p[0], p[1]]))              # the last ends before data
    out.append(_seq(0, [(1, 0, 38, 1), p[1], p[2]]))                    # a hole of 2 bytes
    out.append(_seq(0, [p[1], (1, 0, 37, 1), p[2]]))                    # a hole of 3, on the left
    out.append(_seq(0, [(1, 0, 36, 1), p[1], p[2], (1, 32, 8, 2)]))     # a hole of 4 is kept, filled
    out.append(_seq(0, [p[0], (1, 16, 0, 1), p[1], p[2]]))              # an empty fragment
    out.append(_seq(0, [p[0], p[1], (0, 65528, 3, 1)]))                 # ends at MaxReassSize
    out.append(_seq(0, [p[0], p[1], (0, 65528, 4, 1), p[2]]))           # one byte past it
    for cfg, size in ((1, 2000), (2, 576)):
        q = _cut(size, [size // 2 & ~7])
        out.append(_seq(cfg, q))
        out.append(_seq(cfg, _cut(size + 1, [size // 2 & ~7])))
        out.append(_seq(cfg, [q[0], (0, size, 1, 1), q[1]]))            # offset = size, one byte
        out.append(_seq(cfg, [q[0], (0, size + 8, 1, 1), q[1]]))        # offset > size
        out.append(_seq(cfg, [q[0], (1, (size & ~7) - 8, 0, 1), q[1]]))
    # MaxReassHoles 2: two holes pass, a third invalidates
    out.append(_seq(3, [(1, 16, 8, 1), (1, 0, 16, 1), (0, 24, 5, 1)]))
    out.append(_seq(3, [(1, 16, 8, 1), (1, 48, 8, 1), (1, 0, 16, 1), (1, 24, 24, 1), (0, 56, 5, 1)]))
    out.append(_seq(1, [(1, 16, 8, 1), (1, 48, 8, 1), (1, 0, 16, 1), (1, 24, 24, 1), (0, 56, 5, 1)]))
    # keys that differ only in ident / source / destination / protocol interleave
    base = dict(ident=7, src=0x0A000001, dst=0x0A000002, proto=17)
    for field, val in (("ident", 8), ("src", 0x0A000003), ("dst", 0x0A000004), ("proto", 6)):
        a = _seq(0, _cut(100, [40, 80], 1), **base)[1]
        b = _seq(0, _cut(90, [24], 2), **dict(base, **{field: val}))[1]
        out.append((0, [a[0], b[1], a[2], b[0], a[1]]))
    return out


def randomised():
    rng = _Rng(20261101)
    out = []
    for s in range(N_RANDOM):
        cfg = rng.below(4)
        size = CONFIGS[cfg][0]
        calls = []
        for key in range(1 + rng.below(3)):
            total = 9 + rng.below(600 if rng.below(8) else min(size, 3000))
            if rng.below(40) == 0:
                total = size - rng.below(3)
            k = 1 + rng.below(6)
            cuts = sorted({8 * (1 + rng.below(max(1, (total - 1) // 8))) for _ in range(k)})
            cuts = [c for c in cuts if c < total] or ([8] if total > 8 else [])
            fr = _cut(total, cuts, 1 + rng.below(250))
            m = rng.below(10)
            if m == 0 and len(fr) > 1:
                del fr[rng.below(len(fr))]                                   # a piece missing
            elif m == 1:
                f = fr[rng.below(len(fr))]
                fr.insert(rng.below(len(fr) + 1), f[:3] + (rng.below(256),))  # duplicate
            elif m == 2:
                f = fr[rng.below(len(fr))]
                fr.append((1, max(0, f[1] - 8 * rng.below(3)), 8 + rng.below(40), rng.below(256)))
            elif m == 3:
                i = rng.below(len(fr))
                f = fr[i]
                fr[i] = (f[0], f[1], max(1, f[2] - 1 - rng.below(7)), f[3])  # a small hole
            elif m == 4:
                fr.append((rng.below(2), (size & ~7) + 8 * rng.below(3) if size < 60000 else 65528,
                           1 + rng.below(16), 3))                            # oversize
            elif m == 5:
                fr.append((0, fr[-1][1] + 8 * (1 + rng.below(4)), 1 + rng.below(30), 4))
            if rng.below(4):
                rng.shuffle(fr)
            proto = (17, 6, 1, 47)[rng.below(4)]
            calls.append([(100 + key, 0x0A000000 + s, 0x0B000000 + key, 1 + rng.below(255), proto) + f
                          for f in fr])
        merged = []
        while any(calls):                                                    # interleave the keys
            c = [x for x in calls if x][rng.below(len([x for x in calls if x]))]
            merged.append(c.pop(0))
        out.append((cfg, merged))
    return out


def sequences():
    return crafted() + randomised()


def build_generator(reference):
    os.makedirs(os.path.dirname(GEN_BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(reference, "src"), "-o", GEN_BIN,
                    GEN_SRC], check=True)
    return GEN_BIN


def generate(reference):
    """The fixture's text, from the reference's code run on the sequences above."""
    gen = build_generator(reference)
    seqs = sequences()
    req = []
    for cfg, calls in seqs:
        req.append("S %d" % cfg)
        req += ["F " + " ".join(str(v) for v in c) for c in calls]
    ans = subprocess.run([gen], input="\n".join(req) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert ans[-1] == "" and len(ans) - 1 == sum(len(c) for _, c in seqs)
    rows, at = [], 0
    for cfg, calls in seqs:
        rows.append("%d|%s|%s" % (cfg, ";".join(" ".join(str(v) for v in c) for c in calls),
                                   ";".join(ans[at:at + len(calls)])))
        at += len(calls)
    return json.dumps({"sequences": rows}, indent=0, separators=(",", ":")) + "\n"


def load():
    """[(config, [(ident, src, dst, ttl, proto, mf, offset, len, salt)], [None | (length, fnv)])]"""
    with open(FIXTURE) as f:
        doc = json.load(f)
    out = []
    for row in doc["sequences"]:
        cfg, calls, ans = row.split("|")
        calls = [tuple(int(v) for v in c.split()) for c in calls.split(";")]
        res = []
        for a in ans.split(";"):
            p = a.split()
            res.append(None if p[0] == "0" else (int(p[1]), int(p[2], 16)))
        out.append((int(cfg), calls, res))
    return out


if __name__ == "__main__":
    text = generate(sys.argv[1])
    with open(FIXTURE, "w") as f:
        f.write(text)
    print("%s: %d bytes" % (FIXTURE, len(text)))
