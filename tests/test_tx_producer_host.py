"""The owner search the Tx producers share (aipstack_amd/csrc/tx_producer_common.h: upper_bound
and owner_of, behind tcp_tx_segment and udp_tx_fragment) under ASan/UBSan as a stand-alone program
(tests/cpp/tx_producer_test.cpp): every element against a linear scan, on indices that are proper
running sums and on indices that lie, with no read outside the index."""
import os
import subprocess

from conftest import ROOT


def test_owner_search_under_asan_ubsan():
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "tx_producer.mk"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "build", "asan", "tx_producer_test")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
