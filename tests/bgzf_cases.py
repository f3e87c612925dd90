"""BGZF files for the batched member decode (tests/test_bgzf_cpu.py, test_inflate_core_cpu.py, test_gpu_bgzf.py): a
writer, the clean cases — one FASTQ text cut and compressed in different ways — and the damaged variants of one
20-member file; then members that zlib's encoder never writes, built token by token with tests/deflate_craft.py
(crafted_members, rejected_members, lenient_cases), which join the same tables.  No GPU, no product code."""
import functools
import struct
import zlib

import numpy as np

import deflate_craft as dc

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
    for name, (members, text) in crafted_members().items():
        add(name, members + [EOF_MEMBER], text)
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
    for i, (name, (member, _status)) in enumerate(rejected_members().items()):
        put(name, (0, 9, 18)[i % 3], member)
    return c


# ---- members that zlib's encoder never writes (tests/deflate_craft.py) -------------------------------------------------
# Every valid one holds whole FASTQ records, so that the reads — not only the member counts — are compared on every
# route.  The token list defines the payload: a match copies bases into a sequence line out of an earlier stretch of
# bases (Composer.place looks for a position where that is so), quality lines are 'I' literals or distance-1 matches.

def raw_member(body: bytes, payload: bytes) -> bytes:
    """A BGZF member round a DEFLATE body made elsewhere; the trailer is `payload`'s: what the member claims to hold."""
    assert len(payload) <= 65536 and len(body) + 26 <= 65536
    head = struct.pack("<4BI2BH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(body) + 25)
    return head + body + struct.pack("<II", zlib.crc32(payload), len(payload))


def crafted(body: bytes, payload: bytes) -> bytes:
    """A valid crafted member: zlib reads the body as the payload."""
    assert zlib.decompress(body, -15) == payload
    return raw_member(body, payload)


class Composer:
    """FASTQ records as DEFLATE tokens.  `out` is what the tokens expand to, `base[i]` whether out[i] is a base of a
    sequence line — what a match into a sequence line may copy."""

    def __init__(self, seed: int, tag: str):
        self.rng = np.random.default_rng(seed)
        self.tag, self.n = tag, 0
        self.tokens, self.out, self.base = [], bytearray(), bytearray()
        self.seq_start = None   # where the open record's sequence line begins

    def lit(self, data: bytes, is_base: bool = False):
        self.tokens += list(data)
        self.out += data
        self.base += bytes([is_base]) * len(data)

    def match(self, length: int, dist: int, via284: bool = False):
        assert dist <= len(self.out)
        self.tokens.append((length, dist, "via284") if via284 else (length, dist))
        for _ in range(length):
            self.out.append(self.out[-dist])
            self.base.append(self.base[-dist])

    def begin(self):
        assert self.seq_start is None
        self.lit(f"@{self.tag}{self.n}\n".encode())
        self.n += 1
        self.seq_start = len(self.out)

    def seq_len(self) -> int:
        return len(self.out) - self.seq_start

    def bases(self, n: int):
        if self.seq_start is None:
            self.begin()
        self.lit("".join(self.rng.choice(list("ACGTN"), size=n, p=[0.24, 0.24, 0.24, 0.24, 0.04])).encode(), True)

    def end(self, qual_matches: bool = True):
        """Closes the record: the quality line is an 'I' and distance-1 matches of up to 258, or literals alone."""
        if self.seq_len() == 0:
            self.bases(1)
        n = self.seq_len()
        assert all(self.base[self.seq_start:])
        self.lit(b"\n+\nI")
        left = n - 1
        while qual_matches and left >= 3:
            k = min(left, 258)
            self.match(k, 1)
            left -= k
        self.lit(b"I" * left + b"\n")
        self.seq_start = None

    def need(self, n: int, max_line: int = 450):
        """At least n bases in the open sequence line (a fresh record where the line is long already)."""
        if self.seq_start is not None and self.seq_len() > max_line:
            self.end()
        if self.seq_start is None:
            self.begin()
        if self.seq_len() < n:
            self.bases(n - self.seq_len())

    def place(self, length: int, dist: int, via284: bool = False, max_line: int = 300):
        """The match at the first position from here on where it copies bases only, with literal bases in front of it
        until then (the source moves along with them: through a quality line and a header at the most)."""
        if self.seq_start is not None and self.seq_len() > max_line:
            self.end()
        if self.seq_start is None:
            self.begin()
        while len(self.out) < dist:
            self.bases(200)
            self.end()
            self.begin()
        for _ in range(8000):
            at = len(self.out) - dist
            if 0 not in self.base[at:at + min(length, dist)]:
                self.match(length, dist, via284)
                return
            self.bases(1)
        raise AssertionError("no place for the match")

    def finish(self):
        if self.seq_start is not None:
            self.end()
        text = bytes(self.out)
        assert dc.expand(self.tokens) == text and len(text) <= 65536
        return self.tokens, text


def exact_fastq(size: int, seed: int, tag: str) -> bytes:
    """Whole FASTQ records that fill exactly `size` bytes."""
    rng = np.random.default_rng(seed)
    recs, at = [], 0
    while at < size:
        L = int(rng.integers(80, 150))
        name = f"@{tag}{len(recs)}"
        room = size - at - (len(name) + 1 + 2 + 2)   # what is left for seq + qual of a last record
        if room < 2 * 200:
            L = room // 2
            if room % 2:
                name += "x"
                L = (room - 1) // 2
        seq = "".join(rng.choice(list("ACGT"), size=L))
        recs.append(f"{name}\n{seq}\n+\n{'I' * L}\n")
        at += len(recs[-1])
    assert at == size
    return "".join(recs).encode()


def run_tokens(data: bytes, prev: int = -1) -> list:
    """Literals, and a distance-1 match wherever a byte repeats three times or more behind itself."""
    toks, i = [], 0
    while i < len(data):
        j = i
        while j < len(data) and data[j] == prev and j - i < 258:
            j += 1
        if j - i >= 3:
            toks.append((j - i, 1))
            i = j
        else:
            toks.append(data[i])
            prev = data[i]
            i += 1
    return toks


def two_level_lens(symbols, size: int) -> list:
    """A complete code for the symbols (in this order of priority) out of two neighbouring code lengths."""
    n = len(symbols)
    k = n.bit_length() - 1
    short = (2 << k) - n
    lens = [0] * size
    for i, s in enumerate(symbols):
        lens[s] = k if i < short else k + 1
    return lens


def kraft(lens) -> float:
    return sum(2.0 ** -n for n in lens if n)


def deep_codes_member():
    """One dynamic block.  Literal/length code: one code word each of 1..9 bits, then a tail of 11- to 15-bit words —
    with a literal, length symbols and the end-of-block symbol in it; distance code: 1..8 bits, then 9..15.  Every
    code longer than the decoder's first-level tables (INFC_LBITS = 10, INFC_DBITS = 8) goes the bit-by-bit way."""
    c = Composer(101, "d")
    lengths = [3, 4, 11, 12, 64, 130, 258]
    k = 0
    for rnd in range(3):
        for s in range(16):   # distance symbols 0..15: at least and greatest extra bits, and one in between
            d = dc.DIST_BASE[s] + ((1 << dc.DIST_EXTRA[s]) - 1) * rnd // 2
            c.place(lengths[k % len(lengths)], d, via284=(k % 14 == 13))
            k += 1
        c.end(qual_matches=False)
    tokens, text = c.finish()
    lf, df = dc.count_symbols(tokens)
    used = sorted((s for s in range(286) if lf[s]), key=lambda s: (-lf[s], s))
    ll = [0] * 286
    for i, s in enumerate(used[:9]):
        ll[s] = i + 1
    tail = used[9:]
    assert 5 <= len(tail) <= 38
    spare = [s for s in range(128, 256) if not lf[s]]
    tail += spare[:38 - len(tail)]            # (code words nothing uses: legal, and they make the code complete)
    for i, s in enumerate(tail):
        ll[s] = (11, 12, 13, 14)[i] if i < 4 else 15
    dused = sorted((s for s in range(30) if df[s]), key=lambda s: (-df[s], s))
    assert len(dused) == 16
    dl = [0] * 30
    for i, s in enumerate(dused):
        dl[s] = (list(range(1, 9)) + [9, 10, 11, 12, 13, 14, 15, 15])[i]
    assert kraft(ll) == 1.0 and kraft(dl) == 1.0
    return crafted(dc.Stream().dynamic(tokens, ll, dl, final=True).bytes(), text), text


def one_dist_code_member():
    """A single distance code word of one bit (distance 1): runs of one base, length 258 spelled 285 and 284 + 31."""
    toks = []
    for i in range(6):
        toks += dc.literals(f"@o{i}\n".encode())
        for line, ch in ((0, "ACGTNA"[i]), (1, "I")):
            toks += dc.literals(ch.encode())
            for j in range(5):
                toks.append((258, 1, "via284") if (i + j + line) % 2 else (258, 1))
            toks.append((7 + i, 1))
            toks += dc.literals(b"\n" if line else b"\n+\n")
    text = dc.expand(toks)
    ll, _ = dc.auto_lens(toks)
    return crafted(dc.Stream().dynamic(toks, ll, [1], final=True).bytes(), text), text


def no_dist_code_member():
    """Literals only; HDIST says one distance length, and that is 0."""
    text = fastq_text(20, seed=12)
    toks = dc.literals(text)
    ll, _ = dc.auto_lens(toks)
    return crafted(dc.Stream().dynamic(toks, ll, [0], final=True, hdist=1).bytes(), text), text


def max_header_member():
    """HLIT 286, HDIST 30, HCLEN 19.  The code lengths' run-length spelling: a 17 of 3, a 16 directly behind it (zeros
    repeated), an 18 of 138, and a 16 that runs from the lengths of symbols 284 and 285 into those of distances 0, 1."""
    c = Composer(102, "m")
    for length, d in ((258, 300), (257, 24), (3, 1), (35, 40), (258, 2)):
        c.place(length, d)
    c.end()
    c.need(20)
    c.place(10, 700)
    tokens, text = c.finish()
    lf, df = dc.count_symbols(tokens)
    lits = sorted((s for s in range(256) if lf[s]), key=lambda s: (-lf[s], s))
    order = [285, 284, 283] + lits + [256] + list(range(257, 283))
    ll = two_level_lens(order, 286)
    dl = two_level_lens([28, 29] + list(range(28)), 30)   # (distances 0 and 1 among the 5-bit ones)
    assert ll[283] == ll[284] == ll[285] == dl[0] == dl[1] == 5 and kraft(ll) == 1.0 and kraft(dl) == 1.0
    z0 = max(lits) + 1
    zeros = 256 - z0
    assert zeros >= 144 and ll[z0 - 1] != 0
    ops = ll[:z0] + [(17, 3), (16, 3), (18, 138)] + dc.rle_greedy([0] * (zeros - 144)) + ll[256:284] + [(16, 4)] + dl[2:]
    assert dc.rle_expand(ops) == ll + dl
    body = dc.Stream().dynamic(tokens, ll, dl, final=True, hlit=286, hdist=30, hclen=19, rle=ops).bytes()
    return crafted(body, text), text


def all_symbols_members():
    """Every length symbol 257..285 and every distance symbol 0..29, each with its extra bits all zero and all one,
    behind 33 000 bytes of history in the same member; once in the fixed code, once in a dynamic one."""
    c = Composer(103, "s")
    while len(c.out) < 33000:
        c.bases(int(c.rng.integers(300, 500)))
        c.end()
    lens = []
    for t in range(29):
        lens.append((dc.LEN_BASE[t], False))
        top = dc.LEN_BASE[t] + (1 << dc.LEN_EXTRA[t]) - 1
        lens.append((258, True) if t == 27 else (top, False))
    dists = []
    for s in range(30):
        dists += [dc.DIST_BASE[s], dc.DIST_BASE[s] + (1 << dc.DIST_EXTRA[s]) - 1]
    for i, d in enumerate(dists):
        length, via = lens[i % len(lens)]
        c.place(length, d, via284=via)
    tokens, text = c.finish()
    a = crafted(dc.Stream().fixed(tokens, final=True).bytes(), text)
    b = crafted(dc.Stream().dynamic(tokens, *dc.auto_lens(tokens), final=True).bytes(), text)
    return [a, b], text + text


OVERLAP_LENGTHS = (3, 63, 64, 65, 128, 257, 258)


def overlap_distances(length: int) -> list:
    return sorted({1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, length - 1, length, length + 1})


def overlap_member():
    """The whole grid of lengths and distances round the 64-lane copy, overlapping (distance < length) and not."""
    c = Composer(104, "v")
    for length in OVERLAP_LENGTHS:
        for d in overlap_distances(length):
            c.need(d)
            c.match(length, d, via284=(length == 258 and d % 2 == 0))
    tokens, text = c.finish()
    return crafted(dc.Stream().dynamic(tokens, *dc.auto_lens(tokens), final=True).bytes(), text), text


STAGE_RUNS = (255, 256, 257, 511, 512, 513)


def stage_borders_members():
    """Literal runs of exactly 255 .. 513 between two matches (the decoder's literal stage holds 256); a member whose
    last symbol is a literal at ISIZE, and one whose last symbol is a match that ends there."""
    c = Composer(105, "g")
    for run in STAGE_RUNS:
        c.begin()
        c.bases(8)
        c.match(4, 5)
        c.bases(run)
        c.match(5, 7)
        c.end()
    tokens, text = c.finish()
    assert text.endswith(b"\n") and tokens[-1] == 10
    a = crafted(dc.Stream().dynamic(tokens, *dc.auto_lens(tokens), final=True).bytes(), text)
    rec = b"@e\n" + fastq_text(1, seed=13, length=(60, 61)).split(b"\n")[1] + b"\n+\n" + b"I" * 60 + b"\n"
    toks = dc.literals(rec) + [(len(rec), len(rec))]
    b = crafted(dc.Stream().fixed(toks, final=True).bytes(), rec + rec)
    return [a, b], text + rec + rec


MIX_STORED = (0, 1, 3, 250, 255, 256, 257, 258, 511, 512, 513, 1020, 1024, 1028, 2000)


def block_mix_member():
    """Stored, fixed and dynamic blocks in one member: stored blocks of MIX_STORED bytes, each followed by a fixed
    block of one to five symbols (so the bit phase at a stored header and the byte offset at the resume both move);
    dynamic → fixed → dynamic → fixed; a BFINAL/BTYPE field that starts in byte 256·n − 1 of the body and ends in
    byte 256·n, once in front of a fixed and once in front of a dynamic block; a dynamic header across such a byte;
    stored blocks whose data ends at byte 255, 0 and 1 (mod 256); an empty stored block as the final one."""
    text = fastq_text(60, seed=77, length=(200, 400))
    s = dc.Stream()
    p = 0

    def small(k):   # k symbols of what comes next: a match inside a run of 'I', literals elsewhere
        nonlocal p
        toks = []
        for _ in range(k):
            if p > 0 and text[p - 1:p + 3] == b"IIII":
                toks.append((3, 1))
                p += 3
            else:
                toks.append(text[p])
                p += 1
        return toks

    def stored(n):
        nonlocal p
        s.stored(text[p:p + n])
        p += n

    def land(target, then):
        """A stored block and a fixed block — one to five literals and a match of 3 — laid so that the NEXT block's
        header starts at bit 6 of body byte ≡ target (mod 256); `then` writes that block."""
        nonlocal p
        lenfield = (s.bitpos + 3 + 7) // 8
        q = p + 1
        while not (text[q:q + 4] == b"IIII" and (lenfield + q - p + 7) % 256 == target):
            q += 1
        k = 1 + (q - p) % 5 if q - p >= 5 else 1
        n = q + 1 - k - p
        stored(n)
        s.fixed(dc.literals(text[p:q + 1]) + [(3, 1)])
        p = q + 4
        assert s.bitpos % 2048 == target * 8 + 6
        then()

    def dynamic(n):
        nonlocal p
        toks = run_tokens(text[p:p + n], text[p - 1])
        s.dynamic(toks, *dc.auto_lens(toks))
        p += n

    s.fixed(small(3))
    for i, n in enumerate(MIX_STORED):          # (fixed → stored → fixed from the start on)
        stored(n)
        s.fixed(small(1 + i % 5))
    for j in range(2):                           # dynamic → fixed → dynamic → fixed
        dynamic(500 + 37 * j)
        s.fixed(small(2 + j))
    land(255, lambda: s.fixed(small(4)))         # BFINAL/BTYPE across a 256-byte border: fixed …
    land(255, lambda: dynamic(400))              # … and dynamic
    land(250, lambda: dynamic(300))              # the dynamic header's fields across the border
    for r in (255, 0, 1):                        # the resume behind a stored block next to the border
        data_at = (s.bitpos + 3 + 7) // 8 + 4
        stored((r - data_at) % 256 + 256)
        assert (s.bitpos // 8) % 256 == r
        s.fixed(small(2))
    e = text.index(b"\n@", p) + 1
    s.fixed(run_tokens(text[p:e], text[p - 1]))
    s.stored(b"", final=True)
    return crafted(s.bytes(), text[:e]), text[:e]


def isize_65536_members():
    """A member that decodes to 65536 bytes (bgzip stops at 65280), and one whose body is the longest BSIZE can state:
    65510 bytes, one stored block."""
    big = exact_fastq(65536, 18, "z")
    a = bgzf_member(big)
    text = exact_fastq(65505, 19, "y")
    b = crafted(dc.Stream().stored(text, final=True).bytes(), text)
    assert len(b) == 65536 and struct.unpack("<H", b[16:18])[0] == 65535
    return [a, b], big + text


def alignment_members():
    """The members of deep_codes and block_mix at file offsets ≡ 0, 1, 2 and 3 (mod 4), moved there by ordinary filler
    members of a suitable size.  bgzf_plan_batch states a body's place as its offset from the batch's first byte and
    the stage uploads the batch as it lies in the file, so with the whole file in one batch (the default budget) the
    file offset mod 4 is the alignment the kernel's dword loads see."""
    fill = {}
    for n in range(1, 40):
        t = fastq_text(n, seed=90)
        fill.setdefault(len(bgzf_member(t)) % 4, (bgzf_member(t), t))
    assert set(fill) == {0, 1, 2, 3}
    members, text, at = [], b"", 0
    for want in (0, 1, 2, 3):
        for m, t in (deep_codes_member(), block_mix_member()):
            f, ft = fill[(want - at) % 4]
            if (want - at) % 4:
                members.append(f)
                text += ft
                at += len(f)
            assert at % 4 == want
            members.append(m)
            text += t
            at += len(m)
    return members, text


@functools.lru_cache(maxsize=None)
def crafted_members() -> dict:
    """name → (members, text): what clean_cases() adds (each with the end-of-file marker behind it)."""
    c = {}
    for name, f in (("deep_codes", deep_codes_member), ("one_dist_code", one_dist_code_member), ("no_dist_code", no_dist_code_member),
                    ("max_header", max_header_member), ("overlap", overlap_member), ("block_mix", block_mix_member)):
        m, t = f()
        c["craft_" + name] = ([m], t)
    for name, f in (("all_symbols", all_symbols_members), ("stage_borders", stage_borders_members), ("isize_65536", isize_65536_members),
                    ("alignment", alignment_members)):
        c["craft_" + name] = f()
    return c


def zlib_refuses(body: bytes, claimed: bytes) -> bool:
    """zlib raises on the body — or reads it through, but not as exactly the body of a member that holds `claimed`:
    other bytes come out, or input is left over."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(body)
    except zlib.error:
        return True
    return not d.eof or d.unused_data != b"" or out != claimed


INFC_OK, INFC_CORRUPT, INFC_INPUT_EXHAUSTED, INFC_OUTPUT_OVER, INFC_OUTPUT_SHORT, INFC_INPUT_LEFT = range(6)


def raw_match(length: int, dist: int):
    ls, _, lx = dc.length_symbol(length)
    ds, _, dx = dc.dist_symbol(dist)
    return ("raw", ls, lx, ds, dx)


@functools.lru_cache(maxsize=None)
def rejected_members() -> dict:
    """name → (member, the status shk_inflate_core.h must give it).  Each takes the place of a member of
    damaged_cases()' 20-member file; P is the payload it claims (CRC-32 and ISIZE of the trailer)."""
    P = SMALL[:3000]
    lits = dc.literals
    good_ll, good_dl = dc.auto_lens(lits(P) + [(3, 1)])
    c = {}

    def put(name, status, body, claimed=P):
        assert zlib_refuses(body, claimed), name
        c["craft_" + name] = (raw_member(body, claimed), status)

    S = dc.Stream
    # INFC_CORRUPT
    put("dist_before_member", INFC_CORRUPT, S().fixed(lits(P[:10]) + [raw_match(3, 11)] + lits(P[13:]), True).bytes())
    far = TEXT[:33000]   # (32768 is the greatest distance DEFLATE can state: one byte in front of a member 32767 bytes in)
    put("dist_before_member_32768", INFC_CORRUPT, S().stored(far[:32767]).fixed([raw_match(3, 32768)] + lits(far[32770:]), True).bytes(), far)
    for ds in (30, 31):
        put(f"fixed_dist_symbol_{ds}", INFC_CORRUPT, S().fixed(lits(P[:50]) + [("raw", 257, 0, ds, 0)] + lits(P[53:]), True).bytes())
    for ls in (286, 287):
        put(f"fixed_length_symbol_{ls}", INFC_CORRUPT, S().fixed(lits(P[:50]) + [("raw", ls, 0, None, 0)] + lits(P[50:]), True).bytes())
    pad = [65] * 8
    put("oversubscribed_litlen", INFC_CORRUPT, S().dynamic(pad, [8] * 257, [1, 1], True, eob=False).bytes())
    put("oversubscribed_dist", INFC_CORRUPT, S().dynamic(lits(P), good_ll, [1, 1, 1], True).bytes())
    put("oversubscribed_code_lengths", INFC_CORRUPT,
        S().dynamic(lits(P), good_ll, good_dl, True, pre_lens=[1, 1, 1] + [4] * 16).bytes())
    put("incomplete_two_code_words", INFC_CORRUPT, S().dynamic(lits(P), good_ll, [2, 2], True).bytes())
    put("first_length_is_16", INFC_CORRUPT, S().dynamic(pad, [8] * 256 + [0], [0], True, rle=[(16, 3)] + [8] * 253 + [0, 0], eob=False).bytes())
    put("repeat_overruns_total", INFC_CORRUPT, S().dynamic(pad, [8] * 256 + [0], [0], True, rle=[8] * 256 + [(18, 11)], eob=False).bytes())
    put("nlen_mismatch", INFC_CORRUPT, S().stored(P, True, nlen=0x1234).bytes())
    s = S()
    s.header(True, 3)
    s.bits(0, 5)
    put("btype_3", INFC_CORRUPT, s.bytes() + P[:100])
    # INFC_INPUT_EXHAUSTED
    put("stored_len_beyond_body", INFC_INPUT_EXHAUSTED, S().stored(P[:100], True, len_field=5000).bytes())
    # no end-of-block code: the symbols run on into the trailer.  The body ends at a byte border (no padding bits that
    # could hold a symbol of their own) and ISIZE leaves room, so the first symbol read out of the trailer is the end.
    for extra in range(64):
        s = S().dynamic(lits(P) + [10, 65][:extra % 2] + [73] * (extra // 2), good_ll, good_dl, True, eob=False)
        if s.bitpos % 8 == 0:
            break
    assert s.bitpos % 8 == 0
    put("no_end_of_block", INFC_INPUT_EXHAUSTED, s.bytes(), P + SMALL[3000:3100])
    # INFC_OUTPUT_OVER: ISIZE + 1 bytes, the last by a literal, by a match, by a stored block
    put("one_byte_more_literal", INFC_OUTPUT_OVER, S().fixed(lits(P + b"A"), True).bytes())
    put("one_byte_more_match", INFC_OUTPUT_OVER, S().fixed(lits(P[:-2]) + [(3, 1)], True).bytes())
    put("one_byte_more_stored", INFC_OUTPUT_OVER, S().fixed(lits(P[:2000])).stored(P[2000:] + b"A", True).bytes())
    put("one_byte_less", INFC_OUTPUT_SHORT, S().fixed(lits(P[:-1]), True).bytes())
    put("one_spare_byte", INFC_INPUT_LEFT, S().fixed(lits(P), True).bytes() + b"\0")
    return c


@functools.lru_cache(maxsize=None)
def lenient_cases() -> dict:
    """name → (file bytes, index of the member, True where every route decodes it).  Streams zlib refuses and both of
    our decoders take by design — build_table (shk_inflate.cpp) and build() (shk_inflate_core.h) share the rule "a code
    is complete, or it has at most one code word", and the member's CRC-32 is the safeguard.  The member stands behind
    three ordinary ones; its trailer is that of what its tokens expand to."""
    front = bgzf(SMALL[:SMALL.index(b"\n@", 8000) + 1], 3000, eof=False)   # (whole records: the member behind starts one)
    assert len(front) == 3
    c = {}

    def put(name, decodes, body, payload):
        try:
            zlib.decompress(body, -15)
            raise AssertionError(f"zlib takes {name}")
        except zlib.error:
            pass
        c[name] = (b"".join(front) + raw_member(body, payload) + EOF_MEMBER, 3, decodes)

    comp = Composer(106, "l")
    for _ in range(3):
        comp.bases(150)
        comp.end()
    toks, text = comp.finish()   # (every match at distance 1: one distance symbol)
    ll, _ = dc.auto_lens(toks)
    put("one_dist_code_of_5_bits", True, dc.Stream().dynamic(toks, ll, [5], final=True).bytes(), text)
    # One code word in the code length code: every length it can spell is the same, and 258 equal lengths are no code
    # we take — except zeros (18 twice), a block without any code word: the header passes, the first symbol does not.
    body = dc.Stream().dynamic([], [0] * 257, [0], final=True, rle=[(18, 138), (18, 120)], pre_lens=[0] * 18 + [1], eob=False).bytes()
    put("one_code_length_code_word", False, body + b"\0\0\0\0", b"")
    plain = fastq_text(12, seed=14)
    ptoks = run_tokens(plain)
    pl, pd = dc.auto_lens(ptoks)
    for hlit in (287, 288):
        put(f"hlit_{hlit}", True, dc.Stream().dynamic(ptoks, pl, pd, final=True, hlit=hlit).bytes(), plain)
    for hdist in (31, 32):
        put(f"hdist_{hdist}", True, dc.Stream().dynamic(ptoks, pl, pd, final=True, hdist=hdist).bytes(), plain)
    return c
