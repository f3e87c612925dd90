"""The record arrays' owner (PcrRecordArrays) and the record slice copy (pcr_records_slice) of
sharkmer_amd/csrc/shk_products.h without a GPU: slices at the start, in the middle, at the end and empty ones, every
optional destination pointer absent, capacities short by one, grow-then-fits, each against pcr_records_store on the same
records — under a stand-alone program (tests/native/pcr_records_driver.cpp) built with AddressSanitizer and UBSan, the
runtimes linked statically.  Nothing is preloaded and no sanitized code is loaded into the interpreter."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sharkmer_amd", "csrc")


def test_pcr_records_driver_clean_under_asan_ubsan():
    subprocess.check_call(["make", "-C", CSRC, "pcr_records_driver"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=0:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "pcr_records_driver")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 10_000, r.stdout
