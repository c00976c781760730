"""TEST INFRASTRUCTURE -- the inputs of test_gpu_tx_fill_cut.py: the frames of rx_cut_cases.py as the
linear Tx fills get them. Family A of the rx-verify, TCP, UDP and ICMP stages (every seed and
companion cut at every length, with both tails) and family C's 513-frame mixed batch in its plain
and inverted-surroundings layouts; each as built ("raw"), with the checksum fields zeroed (before
the fill) and already filled; in the CSR form and in ring slots of 256 and 2048 bytes (on the
128-byte grid, so that line stores are taken) and 264 bytes (off it); the buffer shifted by
SHIFTS bytes, so that both checksum fields meet every position within a 32-byte sector.

Expectations: oracle.tx_fill_batch / tx_fill_slotted on a copy. Nothing here needs a GPU or torch."""
import copy

import rx_cut_cases as X

STAGES = ("rx_verify", "tcp_rx_parse", "udp_rx_demux", "icmp_rx_respond")
LAYOUTS = {"csr": None, "slots256": 256, "slots2048": 2048, "slots264": 264}
SHIFTS = {"csr": (0, 1, 14, 31), "slots256": tuple(range(32)), "slots2048": (0, 7, 30), "slots264": (0, 5, 30)}
VARIANTS = ("raw", "zeroed", "filled")
TX_STATUSES = {0, 1, 3, 4, 6, 8}     # NOT_IP4, IP_MALFORMED, FRAGMENT, L4_MALFORMED, ACCEPT, ACCEPT_OTHER


def is_ip(f):
    return len(f) >= 34 and f[12:14] == b"\x08\x00"


def l4_field(f):
    """The offset of the L4 checksum field of an IPv4 frame that holds it whole, or None."""
    if not is_ip(f):
        return None
    at = 14 + (f[14] & 15) * 4 + {6: 16, 17: 6, 1: 2}.get(f[23], -1000)
    return at if 34 <= at and at + 2 <= len(f) else None


def fill(oracle, lay, buf):
    """The frame oracle's Tx fill of the layout's frames in buf, in place; returns the statuses."""
    if lay.slotted:
        return oracle.tx_fill_slotted(buf[X.GUARD:], lay.stride, lay.lens)
    return oracle.tx_fill_batch(buf, lay.offsets)


def laid_out(oracle, name, family, layout, alt, variant):
    """(the layout, its host buffer in this variant, the expected buffer, the expected statuses)."""
    b = X.cached(oracle, name, family)
    stride = LAYOUTS[layout]
    if stride is not None:
        b = copy.copy(b)
        need = max(len(f) + (X.EXTRA if family == "C" else len(t)) for f, t in b.cases)
        b.stride = stride if need <= stride else 2048 + stride % 128
    lay = X.lay_out(b, stride is not None, alt)
    host = lay.host.copy()
    if variant != "raw":
        for s, f in zip(lay.start.tolist(), lay.frames):
            if is_ip(f):
                host[s + 24:s + 26] = 0
                at = l4_field(f)
                if at is not None:
                    host[s + at:s + at + 2] = 0
    if variant == "filled":
        fill(oracle, lay, host)
    want = host.copy()
    return lay, host, want, fill(oracle, lay, want)


_c = {}


def cached(oracle, *key):
    """laid_out(), computed once per process and left unchanged."""
    if key not in _c:
        _c[key] = laid_out(oracle, *key)
    return _c[key]
