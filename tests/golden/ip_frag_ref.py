"""TEST INFRASTRUCTURE -- reference-produced answers for the UDP send with IPv4 fragmentation:
the reference's own Ip4RoundFragLen (proto/Ip4Proto.h:71-73), IpChksum over 20-byte fragment
headers (infra/Chksum.h:122-125, as send_fragmented calls it, ip/IpStack.h:510-515) and the UDP
checksum sequence of udp/IpUdpProto.h:163-179 on IpChksumAccumulator, compiled from the reference
tree (ip_frag_ref_gen.cpp only includes the two headers) and run on the inputs below. The answers
are recorded in ip_frag_ref_cases.json:

  {"round": ["<mtu>:<Ip4RoundFragLen(20, mtu)>", ...],
   "headers": ["<40 hex digits>:<IpChksum>", ...],
   "udp": ["<src> <dst> <sport> <dport> <hex payload or ->:<checksum>", ...]}   (hex fields)

    python3 tests/golden/ip_frag_ref.py <reference tree>      # rewrites the fixture

Only `random.Random(seed).getrandbits` is used (a stable Mersenne Twister stream).
"""
import json
import os
import random
import struct
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "ip_frag_ref_cases.json")
GEN_SRC = os.path.join(HERE, "ip_frag_ref_gen.cpp")
GEN_BIN = os.path.join(ROOT, "oracle", "_ref", "ip_frag_ref_gen")

N_MTU_RANDOM = 200
N_HEADERS = 300
N_UDP = 300


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


def mtu_inputs():
    """Every residue mod 8 round the MTUs in use, both ends of the range (the smallest MTU the
    reference allows, 256, and 65535), then random ones."""
    out = []
    for lo in (256, 568, 1000, 1492, 8996, 65520):
        out += list(range(lo, lo + 16))
    rng = _Rng(20261001)
    out += [256 + rng.below(65536 - 256) for _ in range(N_MTU_RANDOM)]
    return out


def header_inputs():
    """20-byte IPv4 headers as the fragments carry them (checksum field 0): random total length,
    ident, flags / offset, TTL, protocol and addresses; a few extreme ones."""
    rng = _Rng(20261002)
    out = [bytes(20), b"\xff" * 10 + b"\x00\x00" + b"\xff" * 8,
           struct.pack(">BBHHHBBHII", 0x45, 0, 20, 0, 0, 0, 0, 0, 0, 0)]
    while len(out) < N_HEADERS:
        fo = rng.below(1 << 13) | (0x2000 if rng.below(2) else 0)
        out.append(struct.pack(">BBHHHBBHII", 0x45, rng.below(256) if rng.below(4) == 0 else 0,
                               20 + rng.below(65516), rng.below(1 << 16), fo, rng.below(256),
                               17 if rng.below(4) else rng.below(256), 0, rng.below(1 << 32),
                               rng.below(1 << 32)))
    return out


def udp_inputs():
    """(src, dst, sport, dport, payload): small datagrams of every length 0..40 and random ones up
    to 200 bytes, random and extreme addresses and ports."""
    rng = _Rng(20261003)
    out = [(0, 0, 0, 0, b""), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFF, 0xFFFF, b"\xff" * 7)]
    for i in range(N_UDP - 2):
        n = i if i <= 40 else rng.below(201)
        out.append((rng.below(1 << 32), rng.below(1 << 32), rng.below(1 << 16), rng.below(1 << 16),
                    bytes(rng.below(256) for _ in range(n))))
    return out


def build_generator(reference):
    os.makedirs(os.path.dirname(GEN_BIN), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(reference, "src"), "-o", GEN_BIN,
                    GEN_SRC], check=True)
    return GEN_BIN


def generate(reference):
    """The fixture's text, from the reference's code run on the inputs above."""
    gen = build_generator(reference)
    mtus, hdrs, udps = mtu_inputs(), header_inputs(), udp_inputs()
    udp_keys = ["%x %x %x %x %s" % (s, d, sp, dp, p.hex() or "-") for s, d, sp, dp, p in udps]
    req = ["R %d" % m for m in mtus] + ["H " + h.hex() for h in hdrs] + ["U " + k for k in udp_keys]
    ans = subprocess.run([gen], input="\n".join(req) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    assert len(ans) == len(req) + 1 and ans[-1] == ""
    a, b = len(mtus), len(mtus) + len(hdrs)
    doc = {"round": ["%d:%s" % (m, v) for m, v in zip(mtus, ans[:a])],
           "headers": ["%s:%s" % (h.hex(), v) for h, v in zip(hdrs, ans[a:b])],
           "udp": ["%s:%s" % (k, v) for k, v in zip(udp_keys, ans[b:])]}
    return json.dumps(doc, indent=0, separators=(",", ":")) + "\n"


def load():
    """(round [(mtu, value)], headers [(20 bytes, checksum)], udp [(src, dst, sport, dport,
    payload, checksum)])."""
    with open(FIXTURE) as f:
        doc = json.load(f)
    rnd = [tuple(int(x) for x in s.split(":")) for s in doc["round"]]
    hdrs = [(bytes.fromhex(s.split(":")[0]), int(s.split(":")[1])) for s in doc["headers"]]
    udps = []
    for s in doc["udp"]:
        k, v = s.split(":")
        src, dst, sp, dp, p = k.split()
        udps.append((int(src, 16), int(dst, 16), int(sp, 16), int(dp, 16),
                     b"" if p == "-" else bytes.fromhex(p), int(v)))
    return rnd, hdrs, udps


if __name__ == "__main__":
    text = generate(sys.argv[1])
    with open(FIXTURE, "w") as f:
        f.write(text)
    print("%s: %d bytes" % (FIXTURE, len(text)))
