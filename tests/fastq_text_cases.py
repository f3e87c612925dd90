"""The texts that the FASTQ framing on the device is held to (tests/test_fastq_text_ref_cpu.py pins the Python
restatement against the host reader over them, tests/test_fastq_text_core_cpu.py runs the kernels' core over them on
the host, tests/test_gpu_fastq_device.py the kernels): name → (text, parameters).  T is the tile of the framing passes
(shk_fastq_parse_geometry; FQ_TILE in shk_fastq_text_core.h).  No GPU, no product code."""
import os
import re
import struct

import bgzf_cases as bc
import fastq_text_ref as ref

_CORE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sharkmer_amd", "csrc", "shk_fastq_text_core.h")


def tile_bytes() -> int:
    with open(_CORE) as f:
        return int(re.search(r"constexpr uint32_t FQ_TILE = (\d+);", f.read()).group(1))


def rec(i: int, seq: str, header=None, sep: str = "+", qual=None, eol: str = "\n") -> str:
    return eol.join([f"@r{i}" if header is None else header, seq, sep, "I" * len(seq) if qual is None else qual]) + eol


def _seq(i: int, n: int) -> str:
    return "".join("ACGTN"[(i * 7 + j * j + j // 3) % 5] for j in range(n))


def records(n: int, over=None) -> str:
    """n records of 20..59 bases; over: index → keyword arguments of rec for that record."""
    return "".join(rec(i, _seq(i, 20 + (i * 13) % 40), **(over or {}).get(i, {})) for i in range(n))


def P(first_record=0, validate_every=0, max_records=0, last=True) -> dict:
    return {"first_record": first_record, "validate_every": validate_every, "max_records": max_records, "last": last}


def framing_cases(T: int) -> dict:
    c = {}

    def add(name, text, **p):
        c[name] = (text if isinstance(text, bytes) else text.encode("latin-1"), P(**p))

    one = rec(0, "ACGTNACGT")
    add("empty", b"")
    add("one_record", one)
    add("one_record_no_final_newline_last", one[:-1])
    add("one_record_no_final_newline_not_last", one[:-1], last=False)
    add("crlf", bc.CRLF)
    add("empty_sequence_lines", rec(0, "") + rec(1, "") + rec(2, "ACG") + rec(3, ""))
    add("final_bare_cr_validated", one[:-1] + "\r")                         # quality "IIIIIIIII\r": one longer, record 0 is validated
    add("final_bare_cr_unvalidated", one + rec(1, "ACGT")[:-1] + "\r")      # … record 1 is not
    add("final_bare_cr_not_last", one + rec(1, "ACGT")[:-1] + "\r", last=False)
    for n in (63, 64, 65):
        add(f"lines{n}_in_one_tile", "".join(("@", "A", "+", "I")[i % 4] + "\n" for i in range(n)))
    tail = records(5)
    add("newline_at_T_minus_1", "@" + "h" * (T - 2) + "\n" + tail[tail.index("\n") + 1:])
    add("newline_at_T", "@" + "h" * (T - 1) + "\n" + tail[tail.index("\n") + 1:])
    crlf_tail = records(5, {i: {"eol": "\r\n"} for i in range(5)})
    add("cr_at_T_minus_1_newline_at_T", "@" + "h" * (T - 2) + "\r\n" + crlf_tail[crlf_tail.index("\n") + 1:])
    long = 5 * T // 2
    add("sequence_of_2.5_tiles", records(2) + rec(2, _seq(2, long)) + records(3))
    add("header_of_2.5_tiles", records(2) + rec(2, "ACGT", header="@" + "x" * (long - 1)) + records(3))
    nl = bc.TEXT.index(b"\n")
    for pad in range(256):  # every residue of the line ends mod 256
        c[f"text_padded_{pad}"] = (bc.TEXT[:nl] + b"p" * pad + bc.TEXT[nl:], P())
    for r in range(1, 16):
        add(f"tail_bytes_{r}", bc.SMALL[:16 * 200 + r], last=False)
    n = 12
    for m in (1, n - 1, n, n + 1):
        add(f"max_records_{m}_of_{n}", records(n), max_records=m)
    # cadence: with first_record 7 and validate_every 4, local record 0 (global 7) is not validated, 1 (global 8) and 5 are
    add("cadence_clean", records(8), first_record=7, validate_every=4)
    add("cadence_bad_header_on_0_unvalidated", records(8, {0: {"header": ">r0"}}), first_record=7, validate_every=4)
    add("cadence_bad_header_on_5_validated", records(8, {5: {"header": ">r5"}}), first_record=7, validate_every=4)
    return c


def anomaly_cases() -> dict:
    """Eight records, validated: 0 and 5 (validate_every 5)."""
    c = {}

    def add(name, text, **p):
        p.setdefault("validate_every", 5)
        c[name] = (text if isinstance(text, bytes) else text.encode("latin-1"), P(**p))

    s = lambda i: _seq(i, 20 + (i * 13) % 40)  # noqa: E731
    add("fasta_header_validated", records(8, {5: {"header": ">r5"}}))
    add("fasta_header_unvalidated", records(8, {3: {"header": ">r3"}}))          # NOT an anomaly
    add("empty_header", records(8, {0: {"header": ""}}))
    add("bad_separator", records(8, {5: {"sep": "-"}}))
    add("quality_one_short", records(8, {5: {"qual": "I" * (len(s(5)) - 1)}}))
    add("quality_one_short_unvalidated", records(8, {4: {"qual": "I" * (len(s(4)) - 1)}}))  # NOT an anomaly
    add("high_byte_in_quality", records(8, {2: {"qual": "I" * (len(s(2)) - 1) + "\xc3"}}))
    add("lowercase_base", rec(0, "ACGT") + rec(1, "ACGT") + rec(2, "ACgT") + records(5))
    add("two_anomalies", rec(0, "ACGT") + rec(1, "ACGT") + rec(2, "ACgT") + records(3) + rec(6, "AcGT") + rec(7, "A"))
    add("anomaly_behind_max_records", records(6) + rec(6, "AcGT") + rec(7, "A"), max_records=6)   # NOT reported
    add("anomaly_at_max_records_minus_1", records(6) + rec(6, "AcGT") + rec(7, "A"), max_records=7)
    return c


def all_cases(T: int) -> dict:
    c = framing_cases(T)
    c.update(anomaly_cases())
    return c


def write_case_file(path: str, cases: dict, aligns=(0, 1, 7)) -> int:
    """The cases with what fastq_text_ref answers, for tests/native/fastq_text_driver.cpp: u32 count, then per case
    u32 name length, name, 4 u64 parameters (first_record, validate_every, max_records, last), u64 alignment, u64 n,
    the expected n_records, n_bases, bytes_consumed, anomaly_record (u64), anomaly_kind (u64), the text, the expected
    offsets (n_records + 1 u64) and bases."""
    blobs = []
    for k, (name, (text, p)) in enumerate(cases.items()):
        e = ref.parse(text, **p)
        nm = name.encode()
        blobs.append(struct.pack("<I", len(nm)) + nm +
                     struct.pack("<11Q", p["first_record"], p["validate_every"], p["max_records"], int(p["last"]), aligns[k % len(aligns)], len(text),
                                 e["n_records"], e["n_bases"], e["bytes_consumed"], e["anomaly_record"], e["anomaly_kind"]) +
                     text + e["offsets"].tobytes() + e["bases"].tobytes())
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blobs)) + b"".join(blobs))
    return len(blobs)
