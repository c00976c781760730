"""Linearise (aipstack_tx_linearise / _slotted) without a GPU: the argument checks of the two
entry points, what the seeded generator of linearise_cases covers (so that the GPU tests cannot
pass vacuously), and the shared rule and piece lookup under ASan + UBSan as a stand-alone
program."""
import ctypes
import os
import subprocess

import numpy as np

import aipstack_amd as A
from aipstack_amd import _lib
from conftest import ROOT

import linearise_cases as LC

EINVAL = A.AIPSTACK_CHKSUM_EINVAL


def _calls():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def slotted(hdr=p, hs=64, hl=p, ca=p, cl=p, ci=p, n=1, ss=None, fr=p, stride=2048, fmax=1514,
                fl=p, st=p):
        return lib.aipstack_tx_linearise_slotted(hdr, hs, hl, ca, cl, ci, n, ss, fr, stride, fmax,
                                                 fl, st, 0, None)

    def csr(hdr=p, hs=64, hl=p, ca=p, cl=p, ci=p, n=1, ss=None, fr=p, off=p, fmax=1514, fl=p, st=p):
        return lib.aipstack_tx_linearise(hdr, hs, hl, ca, cl, ci, n, ss, fr, off, fmax, fl, st, 0,
                                         None)
    return slotted, csr


def test_argument_rules_without_gpu():
    slotted, csr = _calls()
    for call in (slotted, csr):
        for name in ("hdr", "hl", "ca", "cl", "ci", "fr", "fl", "st"):
            assert call(**{name: None}) == EINVAL, name
        assert call(hs=0) == EINVAL
        assert call(fmax=0) == EINVAL and call(fmax=65536) == EINVAL
        assert call(n=(1 << 40) + 1) == EINVAL
        # n == 0 is a no-op, whatever else is passed
        assert call(n=0) == 0 and call(n=0, hdr=None, fmax=0) == 0
    assert csr(off=None) == EINVAL
    assert slotted(stride=0) == EINVAL and slotted(stride=65537) == EINVAL
    assert slotted(stride=1513) == EINVAL            # frame_max > slot_stride
    assert slotted(stride=65536, fmax=65535, n=0) == 0


def test_status_codes_follow_the_header():
    text = open(os.path.join(ROOT, "include", "aipstack_amd", "chksum.h")).read()
    for name, value in (("WRITTEN", LC.WRITTEN), ("SKIPPED", LC.SKIPPED), ("INVALID", LC.INVALID),
                        ("TOO_SHORT", LC.TOO_SHORT), ("TOO_LARGE", LC.TOO_LARGE),
                        ("WRONG_ROOM", LC.WRONG_ROOM)):
        assert f"#define AIPSTACK_TX_LIN_{name}" in text
        assert getattr(A, f"AIPSTACK_TX_LIN_{name}") == value >= 17


def test_generator_coverage():
    """Over the seeded set each outcome occurs at least 20 times, and frames with >= 65 pieces,
    with 0 chunks, with L = 14, L = frame_max and L = frame_max + 1 all occur."""
    count = {o: 0 for o in LC.OUTCOMES}
    many = nochunk = l14 = lmax = lmax1 = 0
    forms = set()
    for seed in range(LC.N_SCENARIOS):
        sc = LC.scenario(seed)
        forms.add((seed % 2, sc.form))
        dest, lens, status = sc.expected()
        assert dest.size == sc.dest_bytes()
        for o in LC.OUTCOMES:
            count[o] += int((status == o).sum())
        for i in np.nonzero(status == LC.WRITTEN)[0]:
            many += sc.pieces(i) >= 65
            nochunk += sc.index[i] == sc.index[i + 1]
        l14 += int((lens == 14).sum())
        lmax += int((lens == sc.frame_max).sum())
        lmax1 += sum(t == "lmax1" and s == LC.TOO_LARGE for t, s in zip(sc.tags, status))
        # the sentinel survives outside the written frames
        written = int(lens.sum())
        assert (dest != LC.SENTINEL).sum() <= written
    assert forms == {(0, "slots"), (1, "csr")}
    assert all(c >= 20 for c in count.values()), count
    assert min(many, nochunk, l14, lmax, lmax1) >= 20, (many, nochunk, l14, lmax, lmax1)


def test_shared_rule_and_lookup_under_asan_ubsan():
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "linearise.mk"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "linearise_plan_test")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
