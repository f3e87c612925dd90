"""FASTQ framing over a text of whole lines, restated in plain Python: what shk_fastq_parse_device (K_FASTQ, DESIGN.md
§20) must answer, byte for byte.  The rules are read_fastq / BufRead::lines / validate_fastq_record's (io.rs:161-198,
271-352); tests/test_fastq_text_ref_cpu.py pins this file against the project's host reader.  No GPU, no product code.

  * a line ends with '\\n'; a '\\r' directly in front of that '\\n' is not part of the line; with last=True an
    unterminated rest is a line too and keeps a '\\r' at its end;
  * record j is lines 4j .. 4j+3, its sequence line 4j+1;
  * the records looked at are [0, min(whole records, max_records or all));
  * an anomaly: a byte >= 0x80 in one of the record's four lines (kind 1); for a record whose global index g =
    first_record + j is validated (g == 0, or validate_every and g % validate_every == 0) a header that does not start
    with '@' (2), a separator that does not start with '+' (3), a quality line of another length than the sequence (4);
    a sequence byte outside ACGTN (5).  The lowest record wins, and within it the lowest kind;
  * emitted are the records in front of the first anomaly; bytes_consumed is where the last emitted record ends."""
import numpy as np

NO_ANOMALY = (1 << 64) - 1
HIGH_BYTE, HEADER, SEPARATOR, QUALITY_LEN, BASE = 1, 2, 3, 4, 5
_NOT_ACGTN = bytes(b for b in range(256) if b not in b"ACGTN")
_LOW = bytes(range(128))


def lines_of(text: bytes, last: bool):
    """[(start, end of content, end of line incl. terminator)]"""
    out, pos, n = [], 0, len(text)
    while True:
        i = text.find(b"\n", pos)
        if i < 0:
            break
        e = i - 1 if i > pos and text[i - 1] == 13 else i
        out.append((pos, e, i + 1))
        pos = i + 1
    if last and pos < n:
        out.append((pos, n, n))
    return out


def validates(g: int, validate_every: int) -> bool:
    return g == 0 or (validate_every > 0 and g % validate_every == 0)


def parse(text: bytes, first_record: int = 0, validate_every: int = 0, max_records: int = 0, last: bool = True) -> dict:
    ln = lines_of(text, last)
    n_look = len(ln) // 4
    if max_records:
        n_look = min(n_look, max_records)
    seqs, anomaly, kind, consumed = [], NO_ANOMALY, 0, 0
    for j in range(n_look):
        h, s, p, q = ln[4 * j:4 * j + 4]
        kinds = []
        if text[h[0]:q[2]].translate(None, _LOW):
            kinds.append(HIGH_BYTE)
        if validates(first_record + j, validate_every):
            if text[h[0]:h[1]][:1] != b"@":
                kinds.append(HEADER)
            if text[p[0]:p[1]][:1] != b"+":
                kinds.append(SEPARATOR)
            if q[1] - q[0] != s[1] - s[0]:
                kinds.append(QUALITY_LEN)
        seq = text[s[0]:s[1]]
        if seq.translate(None, b"ACGTN"):
            kinds.append(BASE)
        if kinds:
            anomaly, kind = j, min(kinds)
            break
        seqs.append(seq)
        consumed = q[2]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        offsets[1:] = np.cumsum([len(s) for s in seqs])
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    return {"bases": bases, "offsets": offsets, "n_records": len(seqs), "n_bases": int(offsets[-1]), "bytes_consumed": consumed,
            "anomaly_record": anomaly, "anomaly_kind": kind}
