"""TEST INFRASTRUCTURE -- seeded random scenarios of the UDP send with IPv4 fragmentation, for
test_gpu_random_ipfrag.py (the GPU against the model of ipfrag_cases.py) and
test_random_ipfrag_cases.py (what the scenarios cover, from the model alone, on the CPU)."""
import numpy as np

import ipfrag_cases as T

SEEDS = 40
MAX_FRAGS = 1500
STRIDES = (42, 48, 64, 80, 128)


class Scenario:
    pass


def _random_dgram(rng, kind):
    mtu = T.MTUS[int(rng.integers(0, 5))]
    M, F = mtu - 20, ((mtu - 20) // 8) * 8
    if kind == "small":                      # fits, or nearly
        D = int(rng.integers(0, M + 8))
    elif kind == "long":                     # more than 64 fragments
        mtu, M, F = 256, 236, 232
        D = int(rng.integers(64 * F, 90 * F))
    else:
        mtu = T.MTUS[int(rng.integers(0, 4))]
        M, F = mtu - 20, ((mtu - 20) // 8) * 8
        D = int(rng.integers(M - 8, 6 * M))
    two = rng.integers(0, 3) != 0
    l0 = int(rng.integers(0, D + 1)) if two else (D if rng.integers(0, 2) else 0)
    if two and rng.integers(0, 4) == 0 and D > F:    # the boundary on or next to a fragment edge
        l0 = min(D, max(0, int(rng.integers(1, D // F + 1)) * F - 8 + int(rng.integers(-1, 2))))
    return T.dgram((int(rng.integers(0, 20000)), l0), (int(rng.integers(66000, 90000)), D - l0),
                   mtu=mtu, ip_id=int(rng.integers(0, 65536)), ttl=int(rng.integers(1, 256)),
                   df=bool(rng.integers(0, 5) == 0), src=int(rng.integers(0, 1 << 32)),
                   dst=int(rng.integers(0, 1 << 32)), sport=int(rng.integers(0, 65536)),
                   dport=int(rng.integers(0, 65536)),
                   dscp=int(rng.integers(0, 256)) if rng.integers(0, 3) == 0 else 0)


def scenario(oracle, seed):
    """Scenario `seed`: datagrams of every kind in random order (a datagram of more than 64
    fragments in every fourth), the clamped straddle, a datagram whose UDP sum is 0, datagrams
    that break the contract or whose counts disagree, the slot stride, the ring's alignment and
    the JUST_WRITTEN hint; the model's expectation."""
    rng = np.random.default_rng(9000 + seed)
    pay = T.payload_bytes(seed=100 + seed).copy()
    cs, total = [], 0
    want = int(rng.integers(1, 60)) if seed % 3 else int(rng.integers(1, 8))

    def add(c):
        nonlocal total
        ns = c["give"][0] if "give" in c else T.counts_of(c)[0]
        if total + ns <= MAX_FRAGS:
            cs.append(c)
            total += ns

    if seed % 4 == 0:
        add(_random_dgram(rng, "long"))
    if seed % 5 == 1:
        add(T.clamp_case(256 if seed % 2 else 1006, S=int(rng.integers(2, 6)), back=1,
                         ip_id=seed))
    if seed % 5 == 2:                       # the UDP sum comes out 0: sent as 0xFFFF
        ln = 2 * int(rng.integers(1, 1500))
        o = 30000 + (seed & 1)
        c = T.dgram((o, ln), mtu=T.MTUS[seed % 4], ip_id=seed, sport=seed)
        pay[o + ln - 2:o + ln] = 0
        chk = T.udp_checksum(oracle, c, pay)
        pay[o + ln - 2], pay[o + ln - 1] = chk >> 8, chk & 0xFF
        add(c)
    while len(cs) < want:
        r = int(rng.integers(0, 20))
        if r == 0:
            add(T.invalid_case(T.INVALID_CLASSES[int(rng.integers(0, len(T.INVALID_CLASSES)))]))
        elif r == 1:
            c = _random_dgram(rng, "mid")
            ns, nc = T.counts_of(c)
            c["give"] = (max(0, ns + int(rng.integers(-1, 2))), max(0, nc + int(rng.integers(-1, 3))))
            if c["give"] != (ns, nc):
                add(c)
        else:
            add(_random_dgram(rng, "small" if r < 9 else "mid"))
    if total == 0:
        add(T.dgram((1, 10), mtu=576))
    order = rng.permutation(len(cs))
    sc = Scenario()
    sc.seed = seed
    sc.batch = T.Batch([cs[j] for j in order], pay)
    sc.fi, sc.cb = T.caller_index(sc.batch.cases)
    sc.e = T.expected(oracle, sc.batch, sc.fi, sc.cb)
    sc.stride = STRIDES[seed % len(STRIDES)] if seed % 3 else 64
    sc.shift = 0 if seed % 3 == 0 else int(rng.integers(0, 64))
    sc.just_written = bool(seed & 1)
    return sc
