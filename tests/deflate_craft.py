"""A DEFLATE writer for tests (RFC 1951), in plain Python: whatever stream a test asks for, bit by bit — code lengths,
header fields and run-length spellings that zlib's encoder never produces, and hooks for streams that are not DEFLATE
at all.  tests/bgzf_cases.py builds its crafted members with it; tests/test_deflate_craft_cpu.py holds it against zlib.
No GPU, no product code.

A token is a literal (an int 0..255), a match `(length, distance)`, or `(258, distance, "via284")` — length 258 spelled
as symbol 284 with extra bits 31 instead of symbol 285.  `("raw", lsym, lextra, dsym, dextra)` emits the named symbols
whatever they are (dsym None: no distance follows); `expand` refuses it."""
import heapq

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
PRE_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
EOB = 256
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def length_symbol(length: int, via284: bool = False):
    """(symbol, extra bits, their value)"""
    if via284:
        assert length == 258
        return 284, 5, 31
    if length == 258:
        return 285, 0, 0
    assert 3 <= length <= 257
    t = max(i for i in range(28) if LEN_BASE[i] <= length)
    assert length - LEN_BASE[t] < 1 << LEN_EXTRA[t]
    return 257 + t, LEN_EXTRA[t], length - LEN_BASE[t]


def dist_symbol(dist: int):
    assert 1 <= dist <= 32768
    d = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return d, DIST_EXTRA[d], dist - DIST_BASE[d]


def expand(tokens) -> bytes:
    """The reference: the tokens applied byte by byte."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            assert 0 <= t < 256
            out.append(t)
            continue
        assert t[0] != "raw" and (len(t) == 2 or t[2] == "via284")
        length, dist = t[0], t[1]
        assert 3 <= length <= 258 and 1 <= dist <= len(out), t
        for _ in range(length):
            out.append(out[-dist])
    return bytes(out)


def literals(data: bytes) -> list:
    return list(data)


def canonical_codes(lens) -> dict:
    """symbol → (code, length), the canonical way (RFC 1951 3.2.2).  Nothing is checked: an over-subscribed list gives
    code words that do not fit their length, which are written masked."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n] & ((1 << n) - 1), n)
            nxt[n] += 1
    return out


def huffman_lengths(freqs, maxbits: int) -> list:
    """Code lengths of a Huffman code for freqs (a list; 0: no code), none longer than maxbits.  One symbol in use: length
    1 (an incomplete code; the caller decides whether that is what it wants)."""
    freqs = list(freqs)
    used = [s for s, f in enumerate(freqs) if f]
    lens = [0] * len(freqs)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    while used:
        heap = [(freqs[s], s, (s,)) for s in used]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        while len(heap) > 1:
            fa, ka, a = heapq.heappop(heap)
            fb, kb, b = heapq.heappop(heap)
            for s in a + b:
                depth[s] += 1
            heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
        if max(depth.values()) <= maxbits:
            for s, d in depth.items():
                lens[s] = d
            break
        freqs = [max(1, f >> 1) if f else 0 for f in freqs]   # flatter, until it fits
    return lens


def count_symbols(tokens, eob: bool = True):
    """(literal/length frequencies[286], distance frequencies[30]) of the tokens, the end-of-block symbol included."""
    lf, df = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        else:
            lf[length_symbol(t[0], len(t) == 3)[0]] += 1
            df[dist_symbol(t[1])[0]] += 1
    lf[EOB] += eob
    return lf, df


def auto_lens(tokens):
    """Huffman code lengths for a dynamic block of these tokens (a lone distance symbol gets the one-bit code)."""
    lf, df = count_symbols(tokens)
    return huffman_lengths(lf, 15), huffman_lengths(df, 15)


def rle_greedy(lens) -> list:
    """The run-length spelling an ordinary encoder picks: 18/17 for zero runs, 16 for repeats."""
    ops, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                n = min(run, 138)
                ops.append((18, n))
                run -= n
            if run >= 3:
                ops.append((17, run))
                run = 0
            ops += [0] * run
        else:
            ops.append(v)
            run -= 1
            while run >= 3:
                n = min(run, 6)
                ops.append((16, n))
                run -= n
            ops += [v] * run
        i = j
    return ops


def rle_expand(ops) -> list:
    out = []
    for op in ops:
        if isinstance(op, int):
            out.append(op)
        else:
            out += [out[-1] if op[0] == 16 else 0] * op[1]
    return out


class Stream:
    """A DEFLATE stream under construction: blocks are appended with stored(), fixed() and dynamic(); bytes() pads the
    last byte and returns the body.  Positions (bitpos) are bits from the stream's start."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.nacc = 0
        self.marks = []   # (what, bit position) of every block header and stored resume, for tests that ask where things lie

    # ---- bits ----
    @property
    def bitpos(self) -> int:
        return len(self.buf) * 8 + self.nacc

    def bits(self, value: int, n: int):
        """n bits, least significant first (header fields, extra bits)"""
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.nacc
        self.nacc += n
        while self.nacc >= 8:
            self.buf.append(self.acc & 0xFF)
            self.acc >>= 8
            self.nacc -= 8

    def code(self, code: int, n: int):
        """a Huffman code word, most significant bit first"""
        for i in range(n - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def align(self):
        if self.nacc:
            self.bits(0, 8 - self.nacc)

    def bytes(self) -> bytes:
        self.align()
        return bytes(self.buf)

    # ---- blocks ----
    def header(self, final: bool, btype: int):
        """BFINAL and BTYPE alone (btype 3: the reserved one)"""
        self.marks.append(("header", self.bitpos))
        self.bits(int(final), 1)
        self.bits(btype, 2)

    def stored(self, data: bytes, final: bool = False, len_field=None, nlen=None):
        """len_field / nlen: what the two 16-bit fields say, where that is not the truth"""
        self.header(final, 0)
        self.align()
        n = len(data) if len_field is None else len_field
        self.bits(n, 16)
        self.bits(n ^ 0xFFFF if nlen is None else nlen, 16)
        self.buf += data
        self.marks.append(("resume", self.bitpos))
        return self

    def symbols(self, tokens, lcodes: dict, dcodes: dict, eob: bool = True):
        for t in tokens:
            if isinstance(t, int):
                self.code(*lcodes[t])
                continue
            if t[0] == "raw":
                _, ls, lx, ds, dx = t
                self.code(*lcodes[ls])
                if 257 <= ls <= 285:
                    self.bits(lx, LEN_EXTRA[ls - 257])
                if ds is not None:
                    self.code(*dcodes[ds])
                    if ds < 30:
                        self.bits(dx, DIST_EXTRA[ds])
                continue
            ls, ln, lx = length_symbol(t[0], len(t) == 3)
            ds, dn, dx = dist_symbol(t[1])
            self.code(*lcodes[ls])
            self.bits(lx, ln)
            self.code(*dcodes[ds])
            self.bits(dx, dn)
        if eob:
            self.code(*lcodes[EOB])

    def fixed(self, tokens, final: bool = False, eob: bool = True):
        self.header(final, 1)
        self.symbols(tokens, canonical_codes(FIXED_LITLEN), canonical_codes(FIXED_DIST), eob)
        return self

    def dynamic(self, tokens, litlen_lens, dist_lens, final: bool = False, hlit=None, hdist=None, hclen=None, pre_lens=None, rle="greedy",
                eob: bool = True):
        """hlit, hdist, hclen: the COUNTS the header states (257.., 1.., 4..; up to 288, 32 and 19 fit the fields), by
        default the smallest that hold the lengths.  rle: "plain" (every length on its own), "greedy", or the list of
        operations itself — an int 0..15, or (16 | 17 | 18, count) — which is written as given, whatever it expands to.
        pre_lens: the 19 lengths of the code length code, by default a Huffman code for the operations."""
        ll, dl = list(litlen_lens), list(dist_lens)
        if hlit is None:
            hlit = max([257] + [s + 1 for s, n in enumerate(ll) if n])
        if hdist is None:
            hdist = max([1] + [s + 1 for s, n in enumerate(dl) if n])
        ll += [0] * (hlit - len(ll))
        dl += [0] * (hdist - len(dl))
        seq = ll[:hlit] + dl[:hdist]
        if rle == "plain":
            ops = list(seq)
        elif rle == "greedy":
            ops = rle_greedy(seq)
        else:
            ops = list(rle)
        if pre_lens is None:
            pf = [0] * 19
            for op in ops:
                pf[op if isinstance(op, int) else op[0]] += 1
            if sum(1 for f in pf if f) == 1:   # (a complete code needs a second word)
                pf[[s for s in (0, 8) if not pf[s]][0]] = 1
            pre_lens = huffman_lengths(pf, 7)
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(PRE_ORDER) if pre_lens[s]])
        self.header(final, 2)
        self.marks.append(("dynamic", self.bitpos))
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(hclen - 4, 4)
        for s in PRE_ORDER[:hclen]:
            self.bits(pre_lens[s], 3)
        pcodes = canonical_codes(pre_lens)
        for op in ops:
            if isinstance(op, int):
                self.code(*pcodes[op])
            else:
                self.code(*pcodes[op[0]])
                base, n = {16: (3, 2), 17: (3, 3), 18: (11, 7)}[op[0]]
                self.bits(op[1] - base, n)
        self.marks.append(("dynamic_end", self.bitpos))
        self.symbols(tokens, canonical_codes(ll), canonical_codes(dl), eob)
        return self
