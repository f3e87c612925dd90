"""BGZF files for the batched member decode (tests/test_bgzf_cpu.py, test_inflate_core_cpu.py, test_gpu_bgzf.py): a
writer, the clean cases — one FASTQ text cut and compressed in different ways — and the damaged variants of one
20-member file.  No GPU, no product code."""
import struct
import zlib

import numpy as np

MEMBER_MAX = 65280  # what bgzip puts into a member


def bgzf_member(payload: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, flush_at=None) -> bytes:
    """One BGZF member: the 18-byte header with the BC subfield, a raw DEFLATE body, CRC-32 and ISIZE.  flush_at: a
    Z_FULL_FLUSH there, so that the body holds several blocks."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        body = c.compress(payload) + c.flush()
    else:
        body = c.compress(payload[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(payload[flush_at:]) + c.flush()
    assert len(payload) <= 65536 and len(body) + 26 <= 65536
    head = struct.pack("<4BI2BH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(body) + 25)
    return head + body + struct.pack("<II", zlib.crc32(payload), len(payload))


EOF_MEMBER = bgzf_member(b"")
assert len(EOF_MEMBER) == 28


def bgzf(text: bytes, size: int = MEMBER_MAX, eof: bool = True, **kw) -> list:
    """The members of `text` cut every `size` bytes (a list, so that a case can damage or count them)."""
    ms = [bgzf_member(text[i:i + size], **kw) for i in range(0, len(text), size)]
    return ms + ([EOF_MEMBER] if eof else [])


def cut_at(text: bytes, cuts, **kw) -> list:
    edges = [0] + sorted(cuts) + [len(text)]
    return [bgzf_member(text[a:b], **kw) for a, b in zip(edges, edges[1:])]


def fastq_text(n: int, seed: int = 3, eol: str = "\n", length=(30, 160)) -> bytes:
    """Synthetic reads: N's, now and then a read shorter than any k in use, a long homopolymer stretch."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = 7 if i % 53 == 5 else int(rng.integers(*length))
        seq = "".join(rng.choice(list("ACGTN"), size=L, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
        if i % 41 == 9:
            seq = seq[:10] + "A" * 90 + seq[10:]
        out.append(eol.join([f"@read{i} lane:{i % 7}", seq, "+", "I" * len(seq)]) + eol)
    return "".join(out).encode()


def homopolymer_text(n: int = 40, run: int = 1500) -> bytes:
    """Long runs of one base: matches of 258 at distance 1."""
    return "".join(f"@h{i}\n{'ACGT'[i % 4] * run}\n+\n{'F' * run}\n" for i in range(n)).encode()


def repeat_32768_text() -> bytes:
    """Whole FASTQ records that fill exactly 32768 bytes, twice: with 65280-byte members the first one holds matches at
    the largest distance DEFLATE has."""
    rng = np.random.default_rng(17)
    recs, size = [], 0
    while True:
        L = int(rng.integers(80, 150))
        name = f"@p{len(recs)}"
        room = 32768 - size - (len(name) + 1 + 2 + 2)   # what is left for seq + qual of a last record
        if room < 2 * 200:
            L = room // 2
            if room % 2:
                name += "x"
                L = (room - 1) // 2
        seq = "".join(rng.choice(list("ACGT"), size=L))
        recs.append(f"{name}\n{seq}\n+\n{'I' * L}\n")
        size += len(recs[-1])
        if size == 32768:
            break
        assert size < 32768
    block = "".join(recs).encode()
    return block + block


TEXT = fastq_text(1500)          # ≈ 330 KB: five members of 65280 and a short one
SMALL = fastq_text(260, seed=5)  # ≈ 57 KB
CRLF = fastq_text(200, seed=6, eol="\r\n")


def _find(text: bytes, what: bytes, start: int = 1000) -> int:
    i = text.index(what, start)
    assert i > 0
    return i


def clean_cases() -> dict:
    """name → (file bytes, n_members, env).  env: SHK_BGZF_BATCH_KB where the case sets it."""
    c = {}

    def add(name, members, text, **env):
        assert b"".join(zlib.decompress(m[18:-8], -15) for m in members) == text, name
        c[name] = (b"".join(members), len(members), {k: str(v) for k, v in env.items()}, text)

    for level in (0, 1, 6, 9):
        add(f"level{level}", bgzf(TEXT, level=level), TEXT)
    for nm, strat in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        add(nm, bgzf(TEXT, 20000, strategy=strat), TEXT)
    add("payload1", bgzf(SMALL[:1500], 1), SMALL[:1500])   # (ends inside a record: the same parse error on every route)
    add("payload2", bgzf(SMALL[:3000], 2), SMALL[:3000])
    add("payload255", bgzf(SMALL, 255), SMALL)
    add("payload65279", bgzf(TEXT, 65279), TEXT)
    add("payload65280", bgzf(TEXT, 65280), TEXT)
    add("full_flush", [bgzf_member(SMALL[:30000], flush_at=11111), bgzf_member(SMALL[30000:], level=1, flush_at=7)] + [EOF_MEMBER], SMALL)
    h = homopolymer_text()
    add("homopolymer", bgzf(h), h)
    r = repeat_32768_text()
    add("repeat32768", bgzf(r, 65280, level=9), r)
    # member borders: inside a header line, inside a sequence, directly behind a '\n', between '\r' and '\n'
    hdr = _find(CRLF, b"@read50 ") + 3
    seq = _find(CRLF, b"\r\n", hdr) + 2 + 11
    nl = _find(CRLF, b"\r\n", seq + 400) + 2
    crlf = _find(CRLF, b"\r\n", nl + 700) + 1
    assert CRLF[crlf - 1:crlf + 1] == b"\r\n" and CRLF[nl - 1] == 10
    add("borders", cut_at(CRLF, [hdr, seq, nl, crlf]) + [EOF_MEMBER], CRLF)
    parts = bgzf(SMALL, 9000, eof=False)
    add("empty_members", [EOF_MEMBER] + parts[:3] + [EOF_MEMBER] + parts[3:5] + [EOF_MEMBER, EOF_MEMBER] + parts[5:] + [EOF_MEMBER], SMALL)
    add("no_eof_marker", bgzf(SMALL, 9000, eof=False), SMALL)
    for n in (1, 2, 63, 64, 65, 300):
        ms = bgzf(SMALL, -(-len(SMALL) // n), eof=False)
        assert len(ms) == n
        add(f"members{n}", ms, SMALL)
    add("batch_kb1", bgzf(SMALL, 700), SMALL, SHK_BGZF_BATCH_KB=1)
    add("batch_kb64", bgzf(TEXT, 30000), TEXT, SHK_BGZF_BATCH_KB=64)
    # 3 KB batches of 1000-byte members: a batch border every 3000 bytes, inside a record almost every time
    assert SMALL[2999] != 10 and SMALL[5999] != 10
    add("batch_border_in_record", bgzf(SMALL, 1000), SMALL, SHK_BGZF_BATCH_KB=3)
    return c


def plain_gzip_member(data: bytes) -> bytes:
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    return co.compress(data) + co.flush()


def damaged_cases() -> dict:
    """name → (file bytes, members in front of the damage).  One 20-member file (19 of 3000 bytes and the end-of-file
    marker); each kind of damage in member 0, in member 9 and in the last member that has a body (18)."""
    ms = bgzf(SMALL, 3000)
    assert len(ms) == 20
    c = {}

    def put(name, at, member):
        c[f"{name}@{at}"] = (b"".join(ms[:at] + [member] + ms[at + 1:]), at)

    for at in (0, 9, 18):
        m = bytearray(ms[at])
        x = bytearray(m)
        x[18 + (len(m) - 26) // 2] ^= 0x10
        put("bitflip", at, bytes(x))
        x = bytearray(m)
        x[-8] ^= 0xFF
        put("crc", at, bytes(x))
        isize = struct.unpack("<I", m[-4:])[0]
        put("isize_small", at, bytes(m[:-4]) + struct.pack("<I", isize - 1))
        put("isize_large", at, bytes(m[:-4]) + struct.pack("<I", isize + 1))
        bsize = struct.unpack("<H", m[16:18])[0]
        put("bsize_plus", at, bytes(m[:16]) + struct.pack("<H", bsize + 1) + bytes(m[18:]))
        put("bsize_minus", at, bytes(m[:16]) + struct.pack("<H", bsize - 1) + bytes(m[18:]))
        front = b"".join(ms[:at])
        c[f"cut_in_body@{at}"] = (front + bytes(m[:18 + (len(m) - 26) // 2]), at)
        c[f"cut_in_trailer@{at}"] = (front + bytes(m[:-3]), at)
        # FNAME set: a valid gzip member that is not a BGZF one (flags FEXTRA | FNAME, the name behind the extra field)
        put("fname", at, bytes(m[:3]) + b"\x0c" + bytes(m[4:18]) + b"reads.fq\0" + bytes(m[18:]))
    c["junk_at_end@20"] = (b"".join(ms) + b"\x01\x02\x03\x04\x05", 20)
    extra = fastq_text(30, seed=9)
    c["plain_gzip_in_the_middle@10"] = (b"".join(ms[:10]) + plain_gzip_member(extra) + b"".join(ms[10:]), 10)
    c["plain_gzip_at_the_end@20"] = (b"".join(ms) + plain_gzip_member(extra), 20)
    return c
