"""The bodies of the K_FASTQ kernels (sharkmer_amd/csrc/shk_fastq_text_core.h) on the host, one lane in the wave's
place, under AddressSanitizer and UBSan: a stand-alone program (tests/native/fastq_text_driver.cpp; runtimes linked
statically, nothing preloaded) that frames every text of tests/fastq_text_cases.py at byte alignments 0, 1 and 7 with
guard bytes round every output and must give exactly what tests/fastq_text_ref.py answers, and that holds the CRC-32
core — 64 shares combined by x^(8·len) mod P, conditioned once — to crc32_update over random extents of 0..70000 bytes
(CPU only)."""
import os
import subprocess

import pytest

import fastq_text_cases as fc

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sharkmer_amd", "csrc")


@pytest.fixture(scope="module")
def driver():
    r = subprocess.run(["make", "-C", CSRC, "fastq_text_driver"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(CSRC, "fastq_text_driver")


def test_core_frames_every_text_like_the_helper(driver, tmp_path):
    path = os.path.join(tmp_path, "cases.bin")
    n = fc.write_case_file(path, fc.all_cases(fc.tile_bytes()))
    r = subprocess.run([driver, "parse", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"parse ok: {n} cases" in r.stdout


def test_crc_core_against_crc32_update(driver):
    r = subprocess.run([driver, "crc", "20261020", "400"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "crc ok: 421 extents" in r.stdout
