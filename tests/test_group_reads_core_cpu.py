"""The retained reads of a multi-device context without a GPU: the flag is declared and the ABI version stays; the run
directory and the host merges (sharkmer_amd/csrc/shk_group_reads_core.h) run clean against their linear models under
AddressSanitizer and UBSan as a stand-alone program (tests/native/group_reads_driver.cpp; the runtimes are linked
statically, nothing is preloaded and no sanitized code is loaded into the interpreter)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sharkmer_amd", "csrc")


def test_the_flag_is_declared_and_the_abi_version_stays():
    import sharkmer_amd as sa
    src = open(os.path.join(ROOT, "include", "shk.h")).read()
    assert "#define SHK_FLAG_GROUP_READS 64u" in src and "#define SHK_ABI_VERSION 2" in src
    assert sa.FLAG_GROUP_READS == 64 and sa.FLAG_GROUP_GRAPH == 32


def test_the_core_header_is_plain_cpp():
    src = open(os.path.join(CSRC, "shk_group_reads_core.h")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower()


def test_group_reads_driver_clean_under_asan_ubsan():
    subprocess.check_call(["make", "-C", CSRC, "group_reads_driver"], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    env["ASAN_OPTIONS"] = "halt_on_error=1:abort_on_error=0:detect_leaks=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([os.path.join(CSRC, "group_reads_driver")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    m = re.fullmatch(r"ok (\d+) (\d+) (\d+)\n", r.stdout)
    assert m and int(m.group(1)) >= 4 * 34 and int(m.group(2)) > 100_000 and int(m.group(3)) > 100_000, r.stdout
