"""FASTQ text framed on the device (K_FASTQ): KmerEngine.parse_fastq_text against tests/fastq_text_ref.py
byte for byte, crc32_members against zlib.crc32, and the route that keeps a bgzip'd file's text in device memory —
ingest_fastq_files, run_files(bgzf="device", parse="device"), shk_count --device-parse — against the existing
all-members reader and the oracle.

Every clean file must go through with gave_up == 0 and every record framed on the device: a give-up followed by the
existing reader cannot stand in for a parser that does not work.  Damaged files end exactly as the bgzf="device" run
does, after one give-up."""
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch
import yaml

import bgzf_cases as bc
import fastq_text_cases as fc
import fastq_text_ref as ref
import sharkmer_amd as sa
from bgzf_checks import CLEAN, DAMAGED, oracle_counts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "sharkmer_amd", "csrc", "shk_count")
T = sa.fastq_parse_geometry()
CASES = fc.all_cases(T)
SMALL_NAMES = [n for n in CASES if not n.startswith("text_padded_")]
ROOM = 1 << 20  # device bytes for a text, its bases and offsets (the largest text is ≈ 330 KB)


def test_tile_is_the_core_headers():
    assert T == fc.tile_bytes() and T % 256 == 0


@pytest.fixture(scope="module")
def dev():
    eng = sa.KmerEngine(k=11, chunks=2, histo_max=50)
    d = {"eng": eng, "text": torch.zeros(ROOM + 64, dtype=torch.uint8, device="cuda"), "bases": torch.zeros(ROOM, dtype=torch.uint8, device="cuda"),
         "offs": torch.zeros(ROOM // 8, dtype=torch.int64, device="cuda")}
    assert d["text"].data_ptr() % 256 == 0
    yield d
    eng.close()


def parse_on_device(dev, text: bytes, p: dict, align: int, bases_cap=None, offsets_cap=None):
    n = len(text)
    if n:
        dev["text"][align:align + n] = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy())
    dev["bases"].fill_(0xEE)
    dev["offs"].fill_(-1)
    torch.cuda.synchronize()  # (torch's copies run on torch's stream, the engine's kernels on its own)
    r = dev["eng"].parse_fastq_text(dev["text"].data_ptr() + align, n, dev["bases"].data_ptr(), ROOM if bases_cap is None else bases_cap,
                                    dev["offs"].data_ptr(), ROOM // 8 if offsets_cap is None else offsets_cap, **p)
    r["bases"] = dev["bases"][:r["n_bases"]].cpu().numpy()
    r["offsets"] = dev["offs"][:r["n_records"] + 1].cpu().numpy().astype(np.uint64)
    return r


def same(got: dict, want: dict, what):
    for f in ("n_records", "n_bases", "bytes_consumed", "anomaly_record", "anomaly_kind"):
        assert got[f] == want[f], (what, f, got[f], want[f])
    assert np.array_equal(got["offsets"], want["offsets"]), what
    assert np.array_equal(got["bases"], want["bases"]), what


@pytest.mark.parametrize("name", SMALL_NAMES)
def test_parse_is_the_helpers(dev, name):
    """bases, offsets, n_records, n_bases, bytes_consumed and the anomaly, at byte offsets 0, 1 and 7 of an aligned
    allocation."""
    text, p = CASES[name]
    want = ref.parse(text, **p)
    for align in (0, 1, 7):
        same(parse_on_device(dev, text, p, align), want, (name, align))


def test_parse_every_residue_of_the_line_ends(dev):
    """bgzf_cases.TEXT with its first header padded by 0..255 bytes (the text's start cycles through 0, 1, 7 as well)."""
    for pad in range(256):
        text, p = CASES[f"text_padded_{pad}"]
        same(parse_on_device(dev, text, p, (0, 1, 7)[pad % 3]), ref.parse(text, **p), pad)


def test_parse_capacities(dev):
    """Too few offsets or bases: SHK_ERR_BAD_ARG, what the text needs comes back, nothing is written beyond a capacity."""
    text, p = CASES["max_records_12_of_12"]
    want = ref.parse(text, **p)
    with pytest.raises(sa.ShkError) as e:
        parse_on_device(dev, text, p, 0, offsets_cap=want["n_records"])
    assert e.value.code == -2 and e.value.needed["n_records"] == want["n_records"] and e.value.needed["n_bases"] == want["n_bases"]
    assert int(dev["offs"][0].item()) == -1 and int(dev["bases"][0].item()) == 0xEE
    with pytest.raises(sa.ShkError) as e:
        parse_on_device(dev, text, p, 0, bases_cap=want["n_bases"] - 1)
    assert e.value.code == -2 and e.value.needed["n_bases"] == want["n_bases"]
    assert int(dev["bases"][want["n_bases"] - 1].item()) == 0xEE and int(dev["bases"][want["n_bases"] - 2].item()) != 0xEE
    same(parse_on_device(dev, text, p, 0, bases_cap=want["n_bases"], offsets_cap=want["n_records"] + 1), want, "exact capacities")


def test_crc32_members_is_zlibs(dev):
    lens = [0, 1, 63, 64, 65, 255, 4095, 65279, 65280, 65536]
    lens += [int(x) for x in np.random.default_rng(5).integers(0, 3000, 300 - len(lens))]   # 300 members in one call
    data = np.random.default_rng(6).integers(0, 256, sum(lens) + 3, dtype=np.uint8)
    jobs = np.zeros((len(lens), 2), dtype=np.uint64)
    at = 3  # (the first member starts at an odd address)
    for i, n in enumerate(lens):
        jobs[i] = (at, n)
        at += n
    want = np.array([zlib.crc32(data[int(o):int(o) + int(n)].tobytes()) for o, n in jobs], dtype=np.uint32)
    d_text = torch.from_numpy(data).cuda()
    d_jobs = torch.from_numpy(jobs.view(np.int64)).cuda()
    d_crc = torch.full((len(lens),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev["eng"].crc32_members(d_text.data_ptr(), d_jobs.data_ptr(), len(lens), d_crc.data_ptr())
    got = d_crc.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want)
    assert got[0] == 0


# ---- the route ---------------------------------------------------------------------------------------------------------
def reference_run(paths, k=11, chunks=2, histo_max=50, **kw):
    """The existing all-members reader feeding ingest_reads: (histograms, counters, n_reads_read, n_bases_read)."""
    eng = sa.KmerEngine(k=k, chunks=chunks, histo_max=histo_max)
    r = sa.FastqReader(paths, gzip_all_members=True, **kw)
    try:
        while True:
            b, o = r.next_batch(max_seqs=2000, max_bases=1 << 20)
            if len(o) > 1:
                eng.ingest_reads(b, o)
            if r.stats()["done"]:
                break
        st = r.stats()
        eng.finalize()
        return eng.histograms().copy(), results(eng.counters()), st["n_reads_read"], st["n_bases_read"]
    finally:
        r.close()
        eng.close()


def results(cnt: dict) -> dict:
    """The counters that are the run's result (capacity, growth and spills depend on how the reads were batched)."""
    return {f: v for f, v in cnt.items() if f not in ("table_capacity", "n_grows", "n_spilled")}


def device_run(paths, k=11, chunks=2, histo_max=50, **kw):
    eng = sa.KmerEngine(k=k, chunks=chunks, histo_max=histo_max)
    try:
        st = eng.ingest_fastq_files(paths, **kw)
        if st["gave_up"]:
            return None, None, st
        eng.finalize()
        return eng.histograms().copy(), results(eng.counters()), st
    finally:
        eng.close()


def write_case(tmp_path, monkeypatch, name):
    data, n_members, env, text = CLEAN[name]
    monkeypatch.delenv("SHK_BGZF_BATCH_KB", raising=False)
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    p = str(tmp_path / f"{name}.fastq.gz")
    open(p, "wb").write(data)
    return p, n_members


@pytest.mark.parametrize("name", sorted(n for n in CLEAN if n not in ("payload1", "payload2")))
def test_route_counts_what_the_reader_route_counts(orc, tmp_path, monkeypatch, name):
    p, n_members = write_case(tmp_path, monkeypatch, name)
    before = sa.fastq_device_totals()
    hist, cnt, st = device_run([p])
    down = sa.fastq_device_totals()["bytes_down"] - before["bytes_down"]
    assert st["gave_up"] == 0, st
    want_hist, want_cnt, n_reads, n_bases = reference_run([p])
    assert st["n_records"] == n_reads and st["n_bases"] == n_bases and st["n_members"] == n_members   # every record framed on the device
    assert np.array_equal(hist, want_hist) and cnt == want_cnt
    assert ("ok", hist.tobytes(), st["n_records"], st["n_bases"]) == oracle_counts(orc, p)
    # two status/CRC words per member; per framed batch the control words in front of n_bases_look and the result words
    assert st["bytes_down"] == 8 * st["n_members"] + 64 * st["n_batches"] == down, st
    assert st["bytes_up"] >= os.path.getsize(p) - 28 * n_members and st["kernel_ns"] > 0


@pytest.mark.parametrize("name", ["payload1", "payload2"])
def test_route_gives_up_on_a_file_that_ends_inside_a_record(tmp_path, monkeypatch, name):
    p, _ = write_case(tmp_path, monkeypatch, name)
    before = sa.fastq_device_totals()
    hist, cnt, st = device_run([p])
    assert st["gave_up"] == 1 and hist is None
    assert sa.fastq_device_totals()["give_ups"] == before["give_ups"] + 1
    # the rerun through run_files is the existing route's outcome: its files, or its error and text
    outs = []
    for d, kw in (("dev", dict(bgzf="device")), ("par", dict(bgzf="device", parse="device"))):
        (tmp_path / d).mkdir()
        try:
            sa.run_files([p], k=11, chunks=2, histo_max=50, sample="s", outdir=str(tmp_path / d), **kw)
            outs.append(outputs(tmp_path / d, "s"))
        except sa.ShkError as e:
            outs.append((e.code, e.msg))
    assert outs[0] == outs[1]
    assert (name == "payload2") == (isinstance(outs[0][1], str) and "Truncated FASTQ record" in outs[0][1])


def test_route_gives_up_and_leaves_an_empty_engine(tmp_path, monkeypatch):
    """After a give-up the engine is as new: the reader route into the same engine counts what it always counts."""
    p, _ = write_case(tmp_path, monkeypatch, "level6")
    bad = str(tmp_path / "bad.fastq.gz")
    text = bc.TEXT[:200000] + b"@x\nACgT\n+\nIIII\n" + bc.TEXT[200000:]   # (an anomaly in the fourth member, behind whole batches of ingested reads)
    monkeypatch.setenv("SHK_BGZF_BATCH_KB", "64")
    open(bad, "wb").write(b"".join(bc.bgzf(text)))
    eng = sa.KmerEngine(k=11, chunks=2, histo_max=50)
    st = eng.ingest_fastq_files([bad])
    assert st["gave_up"] == 1 and st["give_up_reason"] == 5 and st["n_batches"] > 2
    assert eng.ingest_fastq_files([p])["gave_up"] == 0     # (the same engine, after the reset of the give-up)
    eng.finalize()
    want = reference_run([p])
    assert np.array_equal(eng.histograms(), want[0]) and results(eng.counters()) == want[1]
    eng.close()


@pytest.fixture(scope="module")
def growing_file(tmp_path_factory):
    """≈ 12 MiB of text in level-6 members, then ≈ 12 MiB in stored ones: with 6000 KiB batches the compressed bytes of a
    batch go from well under 4 MiB to about 6 MiB, so both slots' upload blocks step from 4 to 8 MiB after use."""
    reps = -(-(12 << 20) // len(bc.TEXT))
    part = {level: b"".join(bc.bgzf(bc.TEXT, level=level, eof=False)) for level in (6, 0)}
    assert len(part[6]) * 6000 * 1024 < 3 * (1 << 20) * len(bc.TEXT) and len(part[0]) > len(bc.TEXT)
    p = tmp_path_factory.mktemp("bgzf_grow") / "reads.fastq.gz"
    p.write_bytes(part[6] * reps + part[0] * reps + bc.EOF_MEMBER)
    return str(p)


def test_route_slot_blocks_grow_while_the_other_slot_is_in_flight(growing_file, monkeypatch):
    monkeypatch.setenv("SHK_BGZF_BATCH_KB", "6000")
    hist, cnt, st = device_run([growing_file])
    assert st["gave_up"] == 0 and st["n_batches"] >= 4, st
    want_hist, want_cnt, n_reads, n_bases = reference_run([growing_file])
    assert st["n_records"] == n_reads and st["n_bases"] == n_bases
    assert np.array_equal(hist, want_hist) and cnt == want_cnt
    # the same file through the reader whose batches the device decodes: the all-members reader's reads, none one by one
    got, want = [], []
    for out, kw in ((got, dict(bgzf="device")), (want, dict(gzip_all_members=True))):
        r = sa.FastqReader([growing_file], **kw)
        try:
            while True:
                b, o = r.next_batch(max_seqs=1 << 20, max_bases=64 << 20)
                out.append((b.copy(), o.copy()))
                if r.stats()["done"]:
                    break
            if out is got:
                assert r.member_stats()["sequential"] == 0 and r.member_stats()["device"] > 0
        finally:
            r.close()
    assert np.array_equal(np.concatenate([b for b, _ in got]), np.concatenate([b for b, _ in want]))
    assert np.array_equal(np.concatenate([np.diff(o.astype(np.int64)) for _, o in got]), np.concatenate([np.diff(o.astype(np.int64)) for _, o in want]))


def test_route_two_files_max_reads_and_cadence(tmp_path, monkeypatch):
    monkeypatch.setenv("SHK_BGZF_BATCH_KB", "64")
    pa, pb = str(tmp_path / "a.fastq.gz"), str(tmp_path / "b.fastq.gz")
    open(pa, "wb").write(b"".join(bc.bgzf(bc.TEXT, 30000)))          # 1500 reads, several batches
    open(pb, "wb").write(b"".join(bc.bgzf(bc.SMALL, 9000)))          # 260 reads
    for kw in (dict(), dict(max_reads=1000), dict(max_reads=1001), dict(max_reads=37), dict(max_reads=1600), dict(validate_every=100),
               dict(max_reads=1501, validate_every=100)):
        hist, cnt, st = device_run([pa, pb], **kw)
        want = reference_run([pa, pb], **kw)
        assert st["gave_up"] == 0, (kw, st)
        assert (st["n_records"], st["n_bases"]) == want[2:], kw
        assert np.array_equal(hist, want[0]) and cnt == want[1], kw
    assert device_run([pa, pb])[2]["n_records"] == 1760
    # a FASTA-like header on a validated record of the second file (global index 1600): an anomaly; unvalidated: none
    t = bytearray(bc.SMALL)
    at = t.index(b"@read100 ")
    t[at] = ord(">")
    open(pb, "wb").write(b"".join(bc.bgzf(bytes(t), 9000)))
    assert device_run([pa, pb], validate_every=100)[2]["give_up_reason"] == 5
    assert device_run([pa, pb], validate_every=7)[2]["gave_up"] == 0
    assert device_run([pa, pb], validate_every=100, max_reads=1600)[2]["gave_up"] == 0      # (behind max_reads: never read)


def test_route_is_not_for_this_input(tmp_path):
    plain = str(tmp_path / "plain.fastq")
    open(plain, "wb").write(bc.SMALL)
    gz = str(tmp_path / "one.fastq.gz")
    open(gz, "wb").write(bc.plain_gzip_member(bc.SMALL))
    eng = sa.KmerEngine(k=11, chunks=2, histo_max=50)
    for paths in ([plain], [gz], [str(tmp_path / "missing.fastq.gz")], [str(tmp_path)], []):
        st = eng.ingest_fastq_files(paths)
        assert st["gave_up"] == 2 and st["n_batches"] == 0, paths
    assert eng.counters()["n_reads_ingested"] == 0
    eng.close()


def outputs(d, sample):
    doc = yaml.safe_load((d / f"{sample}.stats.yaml").read_text())
    doc.pop("command", None)
    doc.pop("peak_memory_bytes", None)
    return (d / f"{sample}.histo").read_bytes(), (d / f"{sample}.final.histo").read_bytes(), doc


@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_damaged_file_ends_as_the_device_decode_run_does(tmp_path, monkeypatch, name):
    monkeypatch.delenv("SHK_BGZF_BATCH_KB", raising=False)
    p = str(tmp_path / "damaged.fastq.gz")
    open(p, "wb").write(DAMAGED[name][0])
    outs = []
    for d, kw in (("dev", dict(bgzf="device")), ("par", dict(bgzf="device", parse="device"))):
        (tmp_path / d).mkdir()
        before = sa.fastq_device_totals()
        try:
            sa.run_files([p], k=11, chunks=2, histo_max=50, sample="s", outdir=str(tmp_path / d), **kw)
            outs.append(outputs(tmp_path / d, "s"))
        except sa.ShkError as e:
            outs.append((e.code, e.msg, sorted(os.listdir(tmp_path / d))))
        give_ups = sa.fastq_device_totals()["give_ups"] - before["give_ups"]
        assert give_ups == (1 if d == "par" else 0)
    assert outs[0] == outs[1]


@pytest.fixture(scope="module")
def file300(tmp_path_factory):
    text = bc.fastq_text(4000, seed=41)
    ms = bc.bgzf(text, -(-len(text) // 299))
    assert len(ms) == 300
    p = tmp_path_factory.mktemp("bgzf300") / "reads.fastq.gz"
    p.write_bytes(b"".join(ms))
    return str(p)


def test_run_files_and_shk_count_write_the_all_members_runs_files(file300, tmp_path):
    for d in ("all", "par", "cli"):
        (tmp_path / d).mkdir()
    kw = dict(k=21, chunks=3, sample="s", histo_max=60)
    st_all = sa.run_files([file300], outdir=str(tmp_path / "all"), gzip_all_members=True, **kw)
    before = sa.fastq_device_totals()
    st_par = sa.run_files([file300], outdir=str(tmp_path / "par"), bgzf="device", parse="device", **kw)
    after = sa.fastq_device_totals()
    assert after["records"] - before["records"] == 4000 and after["give_ups"] == before["give_ups"] and after["batches"] > before["batches"]
    for st in (st_all, st_par):
        st.pop("peak_memory_bytes")
    assert st_all == st_par and st_all["n_reads_read"] == 4000
    want = outputs(tmp_path / "all", "s")
    assert outputs(tmp_path / "par", "s") == want
    r = subprocess.run([EXE, "-k", "21", "--chunks", "3", "--histo-max", "60", "-s", "s", "-o", str(tmp_path / "cli"), "--bgzf-device", "--device-parse", file300],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert outputs(tmp_path / "cli", "s") == want


def test_retained_reads_are_the_device_parsed_ones(tmp_path, orc):
    """run_files(pcr_primers=…, read_threading=True, parse="device"): the reads kept in HBM at ingest are the ones the
    device framed; the FASTA and pcr_results are the all-members run's."""
    import pcr_run_cases as cases
    import pcr_run_ref as pref
    _seq, bases, offsets, _gene, _keys, _counts = cases.case_18s(orc)
    text = "".join(f"@r{i}\n{s.decode()}\n+\n{'I' * len(s)}\n" for i, s in enumerate(pref.split_reads(bases, offsets))).encode()
    p = str(tmp_path / "reads.fastq.gz")
    open(p, "wb").write(b"".join(bc.bgzf(text, 20000)))
    spec = f"forward={cases.FWD_18S.lower()},reverse={cases.REV_18S},name=18s,max-length=2500,min-count=3"
    before = sa.fastq_device_totals()
    for d, kw in (("all", dict(gzip_all_members=True)), ("par", dict(bgzf="device", parse="device"))):
        (tmp_path / d).mkdir()
        sa.run_files([p], k=21, chunks=2, histo_max=50, sample="s", outdir=str(tmp_path / d), read_threading=True, pcr_primers=[spec], **kw)
    after = sa.fastq_device_totals()
    assert after["give_ups"] == before["give_ups"] and after["records"] - before["records"] == len(offsets) - 1
    assert (tmp_path / "par" / "s_18s.fasta").read_bytes() == (tmp_path / "all" / "s_18s.fasta").read_bytes()
    assert len((tmp_path / "par" / "s_18s.fasta").read_bytes()) > 100
    got, want = outputs(tmp_path / "par", "s"), outputs(tmp_path / "all", "s")
    assert got == want and "pcr_results" in got[2]
    # … and through the command: shk_count --pcr-primers … --read-threading --bgzf-device --device-parse
    (tmp_path / "cli").mkdir()
    r = subprocess.run([EXE, "-k", "21", "--chunks", "2", "--histo-max", "50", "-s", "s", "-o", str(tmp_path / "cli"), "--pcr-primers", spec,
                        "--read-threading", "--bgzf-device", "--device-parse", p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "cli" / "s_18s.fasta").read_bytes() == (tmp_path / "all" / "s_18s.fasta").read_bytes()
    assert outputs(tmp_path / "cli", "s") == want


def test_flag_errors(tmp_path, file300):
    import ctypes as C
    with pytest.raises(sa.ShkError) as e:
        sa.run_files([file300], k=21, chunks=2, sample="s", outdir=str(tmp_path), parse="device")
    assert e.value.code == -2 and "SHK_FASTQ_DEVICE_PARSE needs SHK_FASTQ_BGZF_DEVICE" in e.value.msg
    with pytest.raises(sa.ShkError) as e:
        sa.run_files([file300], k=21, chunks=2, sample="s", outdir=str(tmp_path), bgzf="host", parse="device")
    assert e.value.code == -2
    assert not os.listdir(tmp_path)
    with pytest.raises(ValueError):
        sa.run_files([file300], k=21, chunks=2, sample="s", outdir=str(tmp_path), bgzf="device", parse="gpu")
    L = sa.engine.load_library()
    arr = (C.c_char_p * 1)(os.fsencode(file300))
    h = C.c_void_p()
    assert L.shk_fastq_open_ex(arr, 1, 0, 0, sa.engine.FASTQ_BGZF_DEVICE | sa.engine.FASTQ_DEVICE_PARSE, C.byref(h)) == -2 and not h.value
    assert b"SHK_FASTQ_DEVICE_PARSE" in L.shk_run_error()
    eng = sa.KmerEngine(k=21, chunks=2, histo_max=50)
    eng.ingest_seqs([b"ACGTACGTACGTACGTACGTACGTACGT"])
    with pytest.raises(sa.ShkError) as e:
        eng.ingest_fastq_files([file300])
    assert e.value.code == -11 and "holds reads already" in e.value.msg
    eng.reset()
    assert eng.ingest_fastq_files([file300])["n_records"] == 4000
    eng.close()
