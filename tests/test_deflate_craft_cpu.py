"""tests/deflate_craft.py — the DEFLATE writer behind the crafted members of bgzf_cases.py — held against zlib, since a
broken writer would make every test over those members vacuous: zlib reads every valid member as what its tokens
expand to, refuses every rejected and every lenient one, and each valid member really holds the construct it is named
for — read back out of its bits by the few lines of `parse` below.  CPU only; no product code."""
import zlib

import pytest

import bgzf_cases as bc
import deflate_craft as dc


def parse(body: bytes) -> list:
    """The blocks of a valid DEFLATE stream: per block its type, where its header lies (bits), the dynamic header's
    fields, run-length operations and code lengths, every (symbol, code length, extra bits' value) it uses, the length
    of each literal run in front of a match, and for a stored block the byte at which the stream goes on."""
    val, pos, out, blocks = int.from_bytes(body, "little"), 0, 0, []

    def bits(n):
        nonlocal pos
        v = (val >> pos) & ((1 << n) - 1)
        pos += n
        return v

    def table(lens):
        return {(n, c): s for s, (c, n) in dc.canonical_codes(lens).items()}

    def sym(tab):
        code = 0
        for n in range(1, 16):
            code = code << 1 | bits(1)
            if (n, code) in tab:
                return tab[(n, code)], n
        raise AssertionError("no code word")

    while True:
        b = {"at": pos, "final": bits(1), "type": bits(2), "lsyms": [], "dsyms": [], "runs": [], "out_at": out}
        blocks.append(b)
        if b["type"] == 0:
            pos = (pos + 7) & ~7
            n, nn = bits(16), bits(16)
            assert n ^ 0xFFFF == nn
            pos += 8 * n
            out += n
            b["len"], b["resume"] = n, pos // 8
        else:
            assert b["type"] in (1, 2)
            ll, dl = dc.FIXED_LITLEN, dc.FIXED_DIST
            if b["type"] == 2:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                pre = [0] * 19
                for s in dc.PRE_ORDER[:hclen]:
                    pre[s] = bits(3)
                ptab, ops, lens = table(pre), [], []
                while len(lens) < hlit + hdist:
                    s, _ = sym(ptab)
                    if s < 16:
                        ops.append(s)
                        lens.append(s)
                    else:
                        base, n = {16: (3, 2), 17: (3, 3), 18: (11, 7)}[s]
                        ops.append((s, base + bits(n), len(lens)))   # (…, the index it starts at)
                        lens += [lens[-1] if s == 16 else 0] * ops[-1][1]
                assert len(lens) == hlit + hdist
                ll, dl = lens[:hlit], lens[hlit:]
                b.update(hlit=hlit, hdist=hdist, hclen=hclen, ops=ops, ll=ll, dl=dl, header_end=pos)
            ltab, dtab, run = table(ll), table(dl), 0
            while True:
                s, n = sym(ltab)
                if s < 256:
                    b["lsyms"].append((s, n, None))
                    run += 1
                    out += 1
                    continue
                if s == 256:
                    b["lsyms"].append((s, n, None))
                    break
                lx = bits(dc.LEN_EXTRA[s - 257])
                d, dn = sym(dtab)
                dx = bits(dc.DIST_EXTRA[d])
                b["lsyms"].append((s, n, lx))
                b["dsyms"].append((d, dn, dx))
                b["runs"].append(run)
                b.setdefault("matches", []).append((dc.LEN_BASE[s - 257] + lx, dc.DIST_BASE[d] + dx, out))
                out += dc.LEN_BASE[s - 257] + lx
                run = 0
            b["last"] = b["lsyms"][-2] if len(b["lsyms"]) > 1 else None
        if b["final"]:
            assert (pos + 7) // 8 == len(body)
            return blocks


def blocks_of(name, k=0):
    return parse(bc.crafted_members()[name][0][k][18:-8])


def test_writer_round_trips_through_zlib():
    text = bc.SMALL[:5000]
    toks = bc.run_tokens(text) + [(258, 1, "via284"), (3, 5000), (257, 4999)]
    want = dc.expand(toks)
    assert want[:5000] == text and len(want) == 5000 + 258 + 3 + 257
    ll, dl = dc.auto_lens(toks)
    for s in (dc.Stream().fixed(toks, True), dc.Stream().dynamic(toks, ll, dl, True), dc.Stream().dynamic(toks, ll, dl, True, rle="plain"),
              dc.Stream().dynamic(toks, ll, dl, True, hlit=286, hdist=30, hclen=19),
              dc.Stream().stored(text[:7]).fixed(toks[7:20]).stored(b"").dynamic(toks[20:], ll, dl, True)):
        assert zlib.decompress(s.bytes(), -15) == want
    assert dc.rle_expand(dc.rle_greedy(ll + dl)) == ll + dl


def test_every_valid_member_is_what_its_tokens_expand_to():
    """(asserted where each member is made — crafted() — and here once more over the finished files)"""
    for name, (members, text) in bc.crafted_members().items():
        assert b"".join(zlib.decompress(m[18:-8], -15) for m in members) == text, name
        assert all(len(m) <= 65536 and len(zlib.decompress(m[18:-8], -15)) <= 65536 for m in members)


def test_zlib_refuses_every_rejected_and_every_lenient_member():
    for name, (member, _status) in bc.rejected_members().items():
        d = zlib.decompressobj(-15)
        try:
            out = d.decompress(member[18:-8])
            ok = d.eof and d.unused_data == b"" and len(out) == int.from_bytes(member[-4:], "little") and zlib.crc32(out) == int.from_bytes(member[-8:-4], "little")
        except zlib.error:
            ok = False
        assert not ok, name
    for name, (member, status) in bc.rejected_members().items():
        if status == bc.INFC_CORRUPT:
            with pytest.raises(zlib.error):
                zlib.decompressobj(-15).decompress(member[18:-8] + b"\0" * 64)   # (bytes behind it: not merely short)
        elif status == bc.INFC_INPUT_EXHAUSTED:
            with pytest.raises(zlib.error):
                zlib.decompress(member[18:-8], -15)                                # (the body alone does not hold the stream)
    for name, (data, at, _decodes) in bc.lenient_cases().items():
        ms, p = [], 0
        while p < len(data):
            n = int.from_bytes(data[p + 16:p + 18], "little") + 1
            ms.append(data[p:p + n])
            p += n
        with pytest.raises(zlib.error):
            zlib.decompress(ms[at][18:-8], -15)


def test_deep_codes_holds_long_code_words():
    (b,) = blocks_of("craft_deep_codes")
    assert b["type"] == 2
    assert sorted(set(n for n in b["ll"] if n)) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15] and max(b["ll"]) == 15
    assert sorted(set(n for n in b["dl"] if n)) == list(range(1, 16))
    used_long = {s for s, n, _ in b["lsyms"] if n > 10}       # behind the 10-bit table: a literal, a length, end of block
    assert any(s < 256 for s in used_long) and any(s > 256 for s in used_long) and 256 in used_long
    assert {n for s, n, _ in b["lsyms"]} >= {1, 9, 11, 15}
    assert any(n > 8 for _d, n, _ in b["dsyms"]) and max(n for _d, n, _ in b["dsyms"]) == 15   # behind the 8-bit table


def test_sparse_distance_codes():
    (b,) = blocks_of("craft_one_dist_code")
    assert b["hdist"] == 1 and b["dl"] == [1] and {d for d, _n, _x in b["dsyms"]} == {0}
    spelled = {(s, x) for s, _n, x in b["lsyms"] if s in (284, 285)}
    assert (284, 31) in spelled and (285, 0) in spelled
    (b,) = blocks_of("craft_no_dist_code")
    assert b["hdist"] == 1 and b["dl"] == [0] and not b["dsyms"] and len(b["lsyms"]) > 1000


def test_max_header_spells_its_runs():
    (b,) = blocks_of("craft_max_header")
    assert (b["hlit"], b["hdist"], b["hclen"]) == (286, 30, 19)
    ops = b["ops"]
    runs = [op for op in ops if not isinstance(op, int)]
    assert any(op[0] == 18 and op[1] == 138 for op in runs) and any(op[0] == 17 and op[1] == 3 for op in runs)
    assert any(op[0] == 16 and op[2] < 286 < op[2] + op[1] for op in runs)            # from the literal lengths into the distance lengths
    i17 = next(i for i, op in enumerate(ops) if not isinstance(op, int) and op[0] == 17)
    assert ops[i17 + 1][0] == 16                                                      # a 16 directly behind a zero run
    assert b["ll"][285] != 0 and b["dl"][29] != 0


@pytest.mark.parametrize("k", [0, 1])
def test_all_symbols_uses_every_symbol_at_both_ends_of_its_extra_bits(k):
    (b,) = blocks_of("craft_all_symbols", k)
    assert b["type"] == 1 + k
    have_l = {(s, x) for s, _n, x in b["lsyms"] if s > 256}
    have_d = {(d, x) for d, _n, x in b["dsyms"]}
    for t in range(29):
        assert (257 + t, 0) in have_l and (257 + t, (1 << dc.LEN_EXTRA[t]) - 1) in have_l
    for d in range(30):
        assert (d, 0) in have_d and (d, (1 << dc.DIST_EXTRA[d]) - 1) in have_d
    assert min(at for _l, dist, at in b["matches"] if dist > 16384) > 32768 and max(dist for _l, dist, _at in b["matches"]) == 32768


def test_overlap_grid_is_whole():
    (b,) = blocks_of("craft_overlap")
    have = {(length, dist) for length, dist, _at in b["matches"]}
    for length in bc.OVERLAP_LENGTHS:
        for d in (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, length - 1, length, length + 1):
            assert (length, d) in have


def test_stage_borders_runs_and_last_symbols():
    (b,) = blocks_of("craft_stage_borders", 0)
    assert set(bc.STAGE_RUNS) <= set(b["runs"])
    assert b["last"][0] == 10                                        # the last symbol: a literal, at ISIZE
    (b,) = blocks_of("craft_stage_borders", 1)
    assert b["last"][0] > 256 and b["matches"][-1][0] + b["matches"][-1][2] == len(bc.crafted_members()["craft_stage_borders"][1]) - \
        len(zlib.decompress(bc.crafted_members()["craft_stage_borders"][0][0][18:-8], -15))


def test_block_mix_lays_its_blocks_where_it_says():
    bs = blocks_of("craft_block_mix")
    types = "".join("SFD"[b["type"]] for b in bs)
    stored = [b for b in bs if b["type"] == 0]
    assert [b["len"] for b in stored][:len(bc.MIX_STORED)] == list(bc.MIX_STORED)
    for i, b in enumerate(bs[:-1]):
        if b["type"] == 0 and i < 2 * len(bc.MIX_STORED):
            assert bs[i + 1]["type"] == 1 and 2 <= len(bs[i + 1]["lsyms"]) <= 6     # 1..5 symbols and the end of block
    assert "FSF" in types and "DFDF" in types
    assert bs[-1]["type"] == 0 and bs[-1]["len"] == 0 and bs[-1]["final"] == 1
    assert {b["resume"] % 4 for b in stored} == {0, 1, 2, 3}
    assert {b["resume"] % 256 for b in stored} >= {255, 0, 1}
    assert len({b["at"] % 8 for b in stored}) >= 4                                      # the bit phase at a stored header moves
    straddle = [b for b in bs if b["at"] % 2048 in (2046, 2047)]                        # BFINAL/BTYPE across body byte 256·n
    assert {b["type"] for b in straddle} >= {1, 2}
    assert any(b["type"] == 2 and (b["at"] + 3) // 2048 != b["header_end"] // 2048 and b["at"] % 2048 < 2040 for b in bs)


def test_isize_and_bsize_extremes():
    a, b = bc.crafted_members()["craft_isize_65536"][0]
    assert int.from_bytes(a[-4:], "little") == 65536
    assert len(b) == 65536 and int.from_bytes(b[16:18], "little") == 65535 and len(b[18:-8]) == 65510
