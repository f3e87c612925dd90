"""The BGZF batched route on host threads (FastqReader(bgzf="host"), SHK_FASTQ_BGZF_BATCH) against the existing
all-members reader and the oracle (CPU only).

Clean files: the same reads in the same order, the same counts and n_reads_read / n_bases_read, every member decoded
in a batch.  Damaged files: the error code and text and the reads handed out before it are the all-members reader's,
and exactly the members in front of the damage were decoded in batches.  Flags 0 and 1 are untouched."""
import ctypes
import os

import pytest

import sharkmer_amd as sa

import bgzf_cases as bc
from bgzf_checks import CLEAN, DAMAGED, LENIENT, check_clean, check_damaged, check_interleaved, check_lenient, read_all

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROUTE, STAT = "host", "host_batch"


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.mark.parametrize("name", sorted(CLEAN))
def test_clean_file_reads_the_same_in_host_batches(orc, tmp_path, monkeypatch, name):
    check_clean(orc, tmp_path, monkeypatch, name, ROUTE, STAT)


@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_damaged_file_fails_the_same_in_host_batches(tmp_path, monkeypatch, name):
    check_damaged(tmp_path, monkeypatch, name, ROUTE, STAT)


def test_reads_before_a_late_error_are_handed_out(tmp_path, monkeypatch):
    """More than 1000 reads in front of the damage (the reference drains 1000 at a time): they come out, then the error."""
    text = bc.fastq_text(2600, seed=21)
    ms = bc.bgzf(text, 20000)
    bad = bytearray(ms[-3])
    bad[-8] ^= 1
    p = str(tmp_path / "late.fastq.gz")
    open(p, "wb").write(b"".join(ms[:-3]) + bytes(bad) + b"".join(ms[-2:]))
    monkeypatch.setenv("SHK_BGZF_BATCH_KB", "50")
    want = read_all(p, gzip_all_members=True)
    got = read_all(p, bgzf=ROUTE)
    assert want[1] is not None and len(want[0]) >= 2000
    assert got[:3] == want[:3] and got[3][STAT] == len(ms) - 3 and got[3]["sequential"] == 1


def test_flags_0_and_1_are_untouched():
    """The committed two-member fixture: 5 reads as the reference reads it, 12 with every member — by the decoder that
    takes one member after the other, as before."""
    p = os.path.join(G, "reads_two_members.fastq.gz")
    first = read_all(p)
    every = read_all(p, gzip_all_members=True)
    assert first[2][0] == 5 and first[3] == {"device": 0, "host_batch": 0, "sequential": 0}
    assert every[2][0] == 12 and every[3] == {"device": 0, "host_batch": 0, "sequential": 2}
    # (plain gzip members are not BGZF: the batched route hands them over at once, and reads the same)
    assert read_all(p, bgzf=ROUTE)[:3] == every[:3]


def test_bgzf_argument_is_checked():
    with pytest.raises(ValueError):
        sa.FastqReader([os.path.join(G, "reads_two_members.fastq.gz")], bgzf="gpu")


def test_new_symbols_are_exported_and_listed():
    from sharkmer_amd.engine import ABI_SYMBOLS, FRONT_SYMBOLS, lib_path
    L = ctypes.CDLL(lib_path())
    for s in ("shk_fastq_open_device", "shk_fastq_member_stats", "shk_bgzf_device_totals"):
        assert s in ABI_SYMBOLS and getattr(L, s)
    assert "shk_fastq_open_device" in FRONT_SYMBOLS and "shk_fastq_member_stats" in FRONT_SYMBOLS
    hdr = open(os.path.join(os.path.dirname(G), "..", "include", "shk.h")).read()
    assert "#define SHK_FASTQ_BGZF_BATCH 2u" in hdr and "#define SHK_FASTQ_BGZF_DEVICE 4u" in hdr
    assert sa.engine.FASTQ_BGZF_BATCH == 2 and sa.engine.FASTQ_BGZF_DEVICE == 4


@pytest.mark.parametrize("name", sorted(LENIENT))
def test_lenient_stream_reads_the_same_in_host_batches(tmp_path, monkeypatch, name):
    check_lenient(tmp_path, monkeypatch, name, ROUTE, STAT)


@pytest.mark.parametrize("batch_kb", [7, None])
def test_crafted_members_among_ordinary_ones_in_host_batches(orc, tmp_path, monkeypatch, batch_kb):
    check_interleaved(orc, tmp_path, monkeypatch, ROUTE, STAT, batch_kb)
