"""tests/fastq_text_ref.py — the framing and anomaly rules that shk_fastq_parse_device is held to — pinned against the
project's host reader (sa.FastqReader over the same text as a plain file), for every text of tests/fastq_text_cases.py
(CPU only).

A text whose first record has the global index f is read behind f clean records; a text that does not end with a
whole record up to where the helper says the whole records end.  Where the helper reports no anomaly the reader hands
out exactly the helper's sequences and no error; where it reports one, the reader fails there: a framing error names
the record, an invalid base comes with exactly the reads in front of it (one read to a call)."""
import os
import re

import numpy as np
import pytest

import bgzf_cases as bc
import fastq_text_cases as fc
import fastq_text_ref as ref
import sharkmer_amd as sa

T = fc.tile_bytes()
CASES = fc.all_cases(T)
NAMES = list(CASES)


def read_all(path, max_reads, validate_every):
    """(sequences handed out one to a call through the packed route, error text or None, stats)"""
    r = sa.FastqReader([path], max_reads=max_reads, validate_every=validate_every)
    n, err = 0, None
    try:
        while True:
            b = r.next_batch_packed(max_seqs=1, max_bases=1 << 16)
            n += len(b.offsets) - 1
            if r.stats()["done"]:
                break
    except sa.ShkError as e:
        err = str(e)
    st = r.stats()
    r.close()
    return n, err, st


def read_ascii(path, max_reads, validate_every):
    r = sa.FastqReader([path], max_reads=max_reads, validate_every=validate_every)
    seqs = []
    while True:
        b, o = r.next_batch(max_seqs=4096, max_bases=1 << 20)
        seqs += [bytes(b[int(o[i]):int(o[i + 1])]) for i in range(len(o) - 1)]
        if r.stats()["done"]:
            break
    r.close()
    return seqs


@pytest.mark.parametrize("name", NAMES)
def test_helper_is_the_host_reader(name, tmp_path):
    text, p = CASES[name]
    e = ref.parse(text, **p)
    f = p["first_record"]
    if not p["last"]:
        assert e["anomaly_record"] == ref.NO_ANOMALY
    if e["anomaly_record"] == ref.NO_ANOMALY and not p["max_records"]:
        text = text[:e["bytes_consumed"]]  # (what lies behind the whole records is the caller's: a file that ended there is an error of the reader's)
    front = fc.records(f).encode()
    path = os.path.join(tmp_path, "t.fastq")
    with open(path, "wb") as fh:
        fh.write(front + text)
    max_reads = f + p["max_records"] if p["max_records"] else 0
    n, err, st = read_all(path, max_reads, p["validate_every"])
    a = e["anomaly_record"]
    if a == ref.NO_ANOMALY:
        assert err is None, err
        assert n == f + e["n_records"] and st["n_reads_read"] == n
        got = read_ascii(path, max_reads, p["validate_every"])[f:]
        want = [bytes(e["bases"][int(e["offsets"][i]):int(e["offsets"][i + 1])]) for i in range(e["n_records"])]
        assert got == want
        assert st["n_bases_read"] == e["n_bases"] + sum(len(s) for s in read_ascii(path, max_reads, p["validate_every"])[:f])
        return
    assert err is not None
    assert e["n_records"] == a
    if e["anomaly_kind"] == ref.BASE:
        assert "Invalid character" in err and n == f + a
    else:
        m = re.search(r"record (\d+)", err)
        assert m and int(m.group(1)) == f + a + 1, err
        word = {ref.HIGH_BYTE: "Failed to read", ref.HEADER: "header", ref.SEPARATOR: "separator", ref.QUALITY_LEN: "mismatched"}[e["anomaly_kind"]]
        assert word in err or (e["anomaly_kind"] == ref.HEADER and "FASTA" in err), err


def test_expected_anomalies():
    """What the cases are there to show (the pin above says that the reader agrees)."""
    A = {n: ref.parse(t, **p) for n, (t, p) in fc.anomaly_cases().items()}
    want = {"fasta_header_validated": (5, ref.HEADER), "fasta_header_unvalidated": None, "empty_header": (0, ref.HEADER),
            "bad_separator": (5, ref.SEPARATOR), "quality_one_short": (5, ref.QUALITY_LEN), "quality_one_short_unvalidated": None,
            "high_byte_in_quality": (2, ref.HIGH_BYTE), "lowercase_base": (2, ref.BASE), "two_anomalies": (2, ref.BASE),
            "anomaly_behind_max_records": None, "anomaly_at_max_records_minus_1": (6, ref.BASE)}
    for n, w in want.items():
        got = None if A[n]["anomaly_record"] == ref.NO_ANOMALY else (A[n]["anomaly_record"], A[n]["anomaly_kind"])
        assert got == w, n
    F = fc.framing_cases(T)
    assert ref.parse(*F["cadence_bad_header_on_0_unvalidated"][:1], **F["cadence_bad_header_on_0_unvalidated"][1])["anomaly_record"] == ref.NO_ANOMALY
    assert ref.parse(*F["cadence_bad_header_on_5_validated"][:1], **F["cadence_bad_header_on_5_validated"][1])["anomaly_record"] == 5
    for name, where in (("newline_at_T_minus_1", T - 1), ("newline_at_T", T), ("cr_at_T_minus_1_newline_at_T", T)):
        assert F[name][0][where] == 10 and (name[0] != "c" or F[name][0][T - 1] == 13)


def test_clean_bgzf_texts_have_no_anomaly():
    """No anomaly in any text of bgzf_cases.clean_cases(), and all of them whole records up to a final '\n': the route
    must not give up on them — except payload1 / payload2, which end inside a record (inside its quality line, which
    the reader takes as it is on a record it does not validate; inside its sequence line)."""
    for name, (_, _, _, text) in bc.clean_cases().items():
        e = ref.parse(text, validate_every=100)
        assert e["anomaly_record"] == ref.NO_ANOMALY, name
        assert (not text.endswith(b"\n")) == (name in ("payload1", "payload2")), name
        assert e["bytes_consumed"] == len(text) or name == "payload2", name
        # and record by record, whatever the batch borders: a text cut anywhere leaves the same records
        if len(text) < 100000:
            cut = len(text) // 3
            a = ref.parse(text[:cut], validate_every=100, last=False)
            b = ref.parse(text[a["bytes_consumed"]:], first_record=a["n_records"], validate_every=100)
            assert a["anomaly_record"] == b["anomaly_record"] == ref.NO_ANOMALY
            assert np.array_equal(np.concatenate([a["bases"], b["bases"]]), e["bases"]) and a["n_records"] + b["n_records"] == e["n_records"]
