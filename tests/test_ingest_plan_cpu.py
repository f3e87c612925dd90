"""A host-buffer ingest's plan without a GPU: the slice cuts, the ring of staging sets, a slice's extents in the packed
streams, the host packer's staging layout, the list form of a sparse N mask and the packer thread
(sharkmer_amd/csrc/shk_ingest_plan.h) against linear-scan models in a stand-alone program
(tests/native/ingest_plan_driver.cpp) — under AddressSanitizer and UBSan, and under ThreadSanitizer for the packer
thread's handshake.  Nothing is preloaded and no sanitized code is loaded into the interpreter."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sharkmer_amd", "csrc")


def run_driver(target, runtime, env_extra):
    probe = subprocess.run(["g++", f"-print-file-name={runtime}"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip(f"no {runtime} in this toolchain")
    subprocess.check_call(["make", "-C", CSRC, target], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([os.path.join(CSRC, target)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 50_000, r.stdout


def test_ingest_plan_driver_clean_under_asan_ubsan():
    run_driver("ingest_plan_driver", "libasan.so",
               {"ASAN_OPTIONS": "halt_on_error=1:abort_on_error=0:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})


def test_ingest_plan_driver_clean_under_tsan():
    run_driver("ingest_plan_driver_tsan", "libtsan.so", {"TSAN_OPTIONS": "halt_on_error=1:exitcode=66"})

