"""The BGZF batched route on the device (FastqReader(bgzf="device"), SHK_FASTQ_BGZF_DEVICE: K_INFLATE, one wave per
member) against the existing all-members reader and the oracle.

Clean files: the same reads, order, counts and totals, and EVERY member decoded on the device — the fallback to the
one-after-the-other decoder must not be able to hide a kernel that does not work.  Damaged files: the all-members
reader's error and reads, with the members in front of the damage decoded on the device.  Two device readers in
lockstep; run_files and shk_count end to end, byte for byte the all-members run's files; sPCR over retained reads."""
import os
import subprocess

import pytest
import yaml

import bgzf_cases as bc
import sharkmer_amd as sa
from bgzf_checks import CLEAN, DAMAGED, LENIENT, check_clean, check_damaged, check_interleaved, check_lenient, read_all

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "sharkmer_amd", "csrc", "shk_count")
ROUTE, STAT = "device", "device"


@pytest.mark.parametrize("name", sorted(CLEAN))
def test_clean_file_reads_the_same_on_the_device(orc, tmp_path, monkeypatch, name):
    check_clean(orc, tmp_path, monkeypatch, name, ROUTE, STAT)


@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_damaged_file_fails_the_same_on_the_device(tmp_path, monkeypatch, name):
    check_damaged(tmp_path, monkeypatch, name, ROUTE, STAT)


def test_device_totals_count_what_was_decoded(tmp_path):
    L = sa.engine.load_library()
    import ctypes as C

    def totals():
        v = [C.c_uint64(0) for _ in range(4)]
        assert L.shk_bgzf_device_totals(*[C.byref(x) for x in v]) == 0
        return [int(x.value) for x in v]
    data, n_members, _env, text = CLEAN["level6"]
    p = str(tmp_path / "t.fastq.gz")
    open(p, "wb").write(data)
    before = totals()
    got = read_all(p, bgzf="device")
    after = totals()
    assert got[3]["device"] == n_members and after[0] - before[0] == n_members
    assert after[1] > before[1]                                    # the kernel's time
    assert after[2] - before[2] >= len(data) - 28 and after[3] - before[3] >= len(text)   # bytes up and down


def test_a_device_that_is_not_there_fails_at_open(tmp_path):
    p = str(tmp_path / "x.fastq.gz")
    open(p, "wb").write(CLEAN["members2"][0])
    with pytest.raises(sa.ShkError) as e:
        sa.FastqReader([p], bgzf="device", device=4096)
    assert e.value.code == -9 and "no HIP device 4096" in e.value.msg


def test_two_device_readers_in_lockstep(tmp_path, monkeypatch):
    """R1 / R2: two readers open at once, each with a device decoder of its own, consumed in turn by one thread."""
    monkeypatch.setenv("SHK_BGZF_BATCH_KB", "40")
    monkeypatch.setenv("SHK_FASTQ_WINDOW_KB", "32")
    ta, tb = bc.fastq_text(1500, seed=31), bc.fastq_text(1400, seed=32)
    pa, pb = str(tmp_path / "r1.fastq.gz"), str(tmp_path / "r2.fastq.gz")
    open(pa, "wb").write(b"".join(bc.bgzf(ta, 9000)))
    open(pb, "wb").write(b"".join(bc.bgzf(tb, 7000)))
    want_a, want_b = read_all(pa, gzip_all_members=True)[0], read_all(pb, gzip_all_members=True)[0]
    ra, rb = sa.FastqReader([pa], bgzf="device"), sa.FastqReader([pb], bgzf="device")
    got_a, got_b = [], []

    def take(r, out):
        b, o = r.next_batch(max_seqs=100, max_bases=1 << 16)
        out += [b[int(o[i]):int(o[i + 1])].tobytes() for i in range(len(o) - 1)]
        return r.stats()["done"]
    done_a = done_b = False
    while not (done_a and done_b):
        if not done_a:
            done_a = take(ra, got_a)
        if not done_b:
            done_b = take(rb, got_b)
    sa_, sb_ = ra.member_stats(), rb.member_stats()
    ra.close()
    rb.close()
    assert got_a == want_a and got_b == want_b and len(want_a) == 1500 and len(want_b) == 1400
    assert sa_["sequential"] == 0 and sb_["sequential"] == 0 and sa_["device"] > 30 and sb_["device"] > 30


@pytest.fixture(scope="module")
def file300(tmp_path_factory):
    text = bc.fastq_text(4000, seed=41)
    ms = bc.bgzf(text, -(-len(text) // 299))
    assert len(ms) == 300
    p = tmp_path_factory.mktemp("bgzf300") / "reads.fastq.gz"
    p.write_bytes(b"".join(ms))
    return str(p)


def outputs(d, sample):
    doc = yaml.safe_load((d / f"{sample}.stats.yaml").read_text())
    doc.pop("command", None)
    doc.pop("peak_memory_bytes", None)
    return (d / f"{sample}.histo").read_bytes(), (d / f"{sample}.final.histo").read_bytes(), doc


def test_run_files_and_shk_count_write_the_all_members_runs_files(file300, tmp_path):
    for d in ("all", "dev", "cli"):
        (tmp_path / d).mkdir()
    kw = dict(k=21, chunks=3, sample="s", histo_max=60)
    st_all = sa.run_files([file300], outdir=str(tmp_path / "all"), gzip_all_members=True, **kw)
    st_dev = sa.run_files([file300], outdir=str(tmp_path / "dev"), bgzf="device", **kw)
    for st in (st_all, st_dev):
        st.pop("peak_memory_bytes")   # (the process's high-water mark: not the run's result)
    assert st_all == st_dev and st_all["n_reads_read"] == 4000
    want = outputs(tmp_path / "all", "s")
    assert outputs(tmp_path / "dev", "s") == want
    r = subprocess.run([EXE, "-k", "21", "--chunks", "3", "--histo-max", "60", "-s", "s", "-o", str(tmp_path / "cli"), "--bgzf-device", file300],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert outputs(tmp_path / "cli", "s") == want
    # (the first member alone — what the run reads without any of the flags — is not the same run)
    (tmp_path / "first").mkdir()
    assert sa.run_files([file300], outdir=str(tmp_path / "first"), **kw)["n_reads_read"] < 4000


def test_retained_reads_see_the_same_reads(tmp_path, orc):
    """run_files(pcr_primers=…, read_threading=True): the reads kept in HBM at ingest are the ones the device decoded."""
    import pcr_run_cases as cases
    import pcr_run_ref as ref
    _seq, bases, offsets, _gene, _keys, _counts = cases.case_18s(orc)
    text = "".join(f"@r{i}\n{s.decode()}\n+\n{'I' * len(s)}\n" for i, s in enumerate(ref.split_reads(bases, offsets))).encode()
    p = str(tmp_path / "reads.fastq.gz")
    open(p, "wb").write(b"".join(bc.bgzf(text, 20000)))
    spec = f"forward={cases.FWD_18S.lower()},reverse={cases.REV_18S},name=18s,max-length=2500,min-count=3"
    for d, kw in (("all", dict(gzip_all_members=True)), ("dev", dict(bgzf="device"))):
        (tmp_path / d).mkdir()
        sa.run_files([p], k=21, chunks=2, histo_max=50, sample="s", outdir=str(tmp_path / d), read_threading=True, pcr_primers=[spec], **kw)
    assert (tmp_path / "dev" / "s_18s.fasta").read_bytes() == (tmp_path / "all" / "s_18s.fasta").read_bytes()
    assert len((tmp_path / "dev" / "s_18s.fasta").read_bytes()) > 100
    assert outputs(tmp_path / "dev", "s") == outputs(tmp_path / "all", "s")


def test_crafted_members_at_every_alignment_decode_on_the_device(orc, tmp_path, monkeypatch):
    """bgzf_cases.alignment_members: the deep-code and the block-mix member at file offsets ≡ 0, 1, 2, 3 (mod 4) in one
    batch.  bgzf_plan_batch does not re-align bodies — a job's in_offset is the body's offset from the batch's first
    byte — so these offsets are what the kernel's dword loads and its seek after a stored block see."""
    data, n_members, _env, _text = CLEAN["craft_alignment"]
    offs, at = set(), 0
    for m in bc.alignment_members()[0]:
        if len(m) > 600:
            offs.add((len(m) > 5000, at % 4))
        at += len(m)
    assert offs == {(big, r) for big in (False, True) for r in range(4)}
    p = str(tmp_path / "alignment.fastq.gz")
    open(p, "wb").write(data)
    monkeypatch.delenv("SHK_BGZF_BATCH_KB", raising=False)
    got = read_all(p, bgzf="device")
    assert got[1] is None and got[3]["device"] == n_members and got[3]["sequential"] == 0
    check_clean(orc, tmp_path, monkeypatch, "craft_alignment", ROUTE, STAT)


@pytest.mark.parametrize("name", sorted(LENIENT))
def test_lenient_stream_reads_the_same_on_the_device(tmp_path, monkeypatch, name):
    check_lenient(tmp_path, monkeypatch, name, ROUTE, STAT)


@pytest.mark.parametrize("batch_kb", [7, None])
def test_crafted_members_among_ordinary_ones_on_the_device(orc, tmp_path, monkeypatch, batch_kb):
    check_interleaved(orc, tmp_path, monkeypatch, ROUTE, STAT, batch_kb)
