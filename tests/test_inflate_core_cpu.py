"""shk_inflate_core.h — the decode K_INFLATE runs, one wave per BGZF member — compiled for the host with one lane in the
wave's place and run by a stand-alone driver (tests/native/inflate_core_driver.cpp) under AddressSanitizer and UBSan:
every clean member gives zlib's bytes; every truncation of three members, and thousands of bit flips and random
overwrites, give a status — never a sanitizer report, a write outside the output slot, a read outside the stated
slack, or more decode steps than a fixed multiple of the bytes in and out.  CPU only; nothing is preloaded."""
import os
import subprocess

import pytest

import bgzf_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sharkmer_amd", "csrc")
DRIVER = os.path.join(CSRC, "inflate_core_driver")


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-C", CSRC, "inflate_core_driver"], stdout=subprocess.DEVNULL)
    return DRIVER


def run(*args):
    r = subprocess.run(list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_every_clean_member_decodes_to_zlibs_bytes(driver, tmp_path):
    files, n_members = [], 0
    for name, (data, n, _env, text) in bc.clean_cases().items():
        p = tmp_path / f"{name}.gz"
        p.write_bytes(data)
        (tmp_path / f"{name}.gz.raw").write_bytes(text)   # (checked against zlib where the case is made)
        files.append(str(p))
        n_members += n
    out = run(driver, "clean", *files)
    assert out.startswith(f"clean ok: {n_members} members"), out


@pytest.mark.parametrize("level,strategy", [(6, "default"), (1, "default"), (0, "default"), (6, "fixed")])
def test_damaged_members_give_a_status(driver, tmp_path, level, strategy):
    """Small members, so that every truncation length of three of them is a few thousand decodes."""
    import zlib
    strat = zlib.Z_FIXED if strategy == "fixed" else zlib.Z_DEFAULT_STRATEGY
    ms = bc.bgzf(bc.SMALL[:30000], 1500, level=level, strategy=strat) + [bc.bgzf_member(bc.SMALL[:4000], level=level, flush_at=1234)]
    p = tmp_path / "members.gz"
    p.write_bytes(b"".join(ms))
    out = run(driver, "damage", "20261020", "1500", str(p))
    assert out.startswith("damage ok:"), out


def test_rejected_crafted_members_give_their_status(driver, tmp_path):
    """bgzf_cases.rejected_members(): every one the status it was built for, at all four alignments — and the lenient
    members, which the core takes or refuses as the table says."""
    lines = []
    for name, (member, status) in bc.rejected_members().items():
        p = tmp_path / f"{name}.gz"
        p.write_bytes(member)
        lines.append(f"{p} 0 {status}")
    for name, (data, at, decodes) in bc.lenient_cases().items():
        p = tmp_path / f"lenient_{name}.gz"
        p.write_bytes(data)
        lines.append(f"{p} {at} {bc.INFC_OK if decodes else bc.INFC_CORRUPT}")
    lst = tmp_path / "expect.txt"
    lst.write_text("\n".join(lines) + "\n")
    out = run(driver, "expect", str(lst))
    assert out.splitlines()[-1].startswith(f"expect ok: {len(lines)} members"), out
    for want, n in ((bc.INFC_CORRUPT, 14), (bc.INFC_INPUT_EXHAUSTED, 2), (bc.INFC_OUTPUT_OVER, 3), (bc.INFC_OUTPUT_SHORT, 1), (bc.INFC_INPUT_LEFT, 1)):
        assert sum(1 for _m, s in bc.rejected_members().values() if s == want) == n


def test_damaged_crafted_members_give_a_status(driver, tmp_path):
    """Truncations, bit flips and overwrites of the crafted valid members: the damage lands in 15-bit code words, maximal
    headers and chains of stored blocks.  Small members only for the every-truncation part (the driver takes the first,
    a middle and the last member of the file)."""
    order = ["craft_max_header", "craft_no_dist_code", "craft_one_dist_code", "craft_stage_borders", "craft_overlap", "craft_block_mix",
             "craft_all_symbols", "craft_deep_codes"]
    ms = [m for name in order for m in bc.crafted_members()[name][0]]
    p = tmp_path / "crafted.gz"
    p.write_bytes(b"".join(ms))
    out = run(driver, "damage", "20261020", "600", str(p))
    assert out.startswith("damage ok:"), out
