"""The gzip source's parts without a reader and without a GPU: LineWindows (the rolling output buffer) against a linear
model, and ParallelInflate (one DEFLATE stream, many threads) against one Inflater in a plain loop
(sharkmer_amd/csrc/shk_gz_source.h), in a stand-alone program (tests/native/gz_source_driver.cpp) — under AddressSanitizer
and UBSan, and under ThreadSanitizer for the decoder's workers.  The streams are written here, with zlib and
tests/deflate_craft.py, and handed over as files.  Nothing is preloaded and no sanitized code is loaded into the interpreter."""
import functools
import os
import random
import re
import subprocess
import zlib

import pytest

import deflate_craft as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sharkmer_amd", "csrc")
TRAILER = b"\x01\x02\x03\x04\x05\x06\x07\x08"   # what follows a stream (a gzip member's trailer): `after` points at it


def fastq(n_bytes: int, seed: int) -> bytes:
    rng = random.Random(seed)
    out, n = [], 0
    while n < n_bytes:
        ln = rng.randint(30, 250)
        seq = "".join(rng.choice("ACGT") for _ in range(ln))
        qual = "".join(rng.choice("FFFFF:,#") for _ in range(ln))
        rec = f"@read{len(out)} lane{rng.randint(1, 8)}\n{seq}\n+\n{qual}\n".encode()
        out.append(rec)
        n += len(rec)
    return b"".join(out)


def raw_deflate(text: bytes, level: int = 6, flush_at=(), mem_level: int = 4) -> bytes:
    """(zlib ends a block every 2^(memLevel + 6) symbols: with a small memLevel a few hundred KB are dozens of blocks,
    and most chunks of the many-thread decoder come from its workers)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level)
    out, last = b"", 0
    for at in flush_at:
        out += c.compress(text[last:at]) + c.flush(zlib.Z_FULL_FLUSH)
        last = at
    return out + c.compress(text[last:]) + c.flush()


@functools.lru_cache(maxsize=None)
def streams():
    """name → (stream, text): raw DEFLATE with TRAILER behind every stream that ends"""
    text = fastq(200_000, 1)
    s = {}
    for level, mem_level in ((1, 2), (6, 4), (9, 8)):
        s[f"level{level}"] = (raw_deflate(text, level, mem_level=mem_level) + TRAILER, text)
    # stored blocks only: the finder never finds an entry, every stretch is decoded in order
    st = dc.Stream()
    cuts = list(range(0, 100_000, 7001))
    for i, at in enumerate(cuts):
        st.stored(text[at:at + 7001][:100_000 - at], final=i == len(cuts) - 1)
    s["stored"] = (st.bytes() + TRAILER, text[:100_000])
    # fixed-Huffman blocks only
    small = text[:40_000]
    st = dc.Stream()
    for at in range(0, len(small), 5000):
        st.fixed(dc.literals(small[at:at + 5000]), final=at + 5000 >= len(small))
    s["fixed"] = (st.bytes() + TRAILER, small)
    # dynamic blocks with a 40 000-byte stored block in their middle: it lies across borders of every chunk size
    a, b = text[:40_000], text[80_000:160_000]
    mid = text[40_000:80_000]
    head = zlib.compressobj(6, zlib.DEFLATED, -15, 4)
    z = head.compress(a) + head.flush(zlib.Z_FULL_FLUSH)   # (byte-aligned behind the flush)
    assert len(z) > 512 and len(z) // 16384 != (len(z) + len(mid)) // 16384
    z += dc.Stream().stored(mid).bytes() + raw_deflate(b, 6)
    s["stored_across"] = (z + TRAILER, a + mid + b)
    s["short"] = (raw_deflate(text[:20_000], 6) + TRAILER, text[:20_000])   # less than 32 KiB: a window that is not full
    s["empty"] = (raw_deflate(b"") + TRAILER, b"")
    one_line = text[:200_000].replace(b"\n", b"N")                           # no '\n': a carry longer than the window in front
    s["no_newline"] = (raw_deflate(one_line, 6) + TRAILER, one_line)
    z6 = raw_deflate(text, 6)
    s["truncated"] = (z6[:len(z6) * 3 // 5], text)                          # ends inside a block
    # damage two thirds in: the block type of the block that begins there flipped to the reserved one, so that the text
    # in front of the damage is exactly the text's first two thirds
    at = len(text) * 2 // 3
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 4)
    head = c.compress(text[:at]) + c.flush(zlib.Z_FULL_FLUSH)
    assert head.endswith(b"\x00\x00\xff\xff")
    z, hdr = bytearray(head + c.compress(text[at:]) + c.flush()), len(head)
    btype = (z[hdr] >> 1) & 3
    assert btype in (1, 2)
    z[hdr] ^= 0x02 if btype == 2 else 0x04
    s["flipped"] = (bytes(z), text)
    return s


def run_driver(target, runtime, env_extra, tmp_path, min_checks):
    probe = subprocess.run(["g++", f"-print-file-name={runtime}"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip(f"no {runtime} in this toolchain")
    subprocess.check_call(["make", "-C", CSRC, target], stdout=subprocess.DEVNULL)
    args = []
    for name, (stream, text) in streams().items():
        zp, tp = tmp_path / f"{name}.deflate", tmp_path / f"{name}.txt"
        zp.write_bytes(stream)
        tp.write_bytes(text)
        args += [str(zp), str(tp)]
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([os.path.join(CSRC, target)] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > min_checks, r.stdout


def test_the_streams_are_what_they_are_meant_to_be():
    for name, (stream, text) in streams().items():
        d = zlib.decompressobj(-15)
        if name == "flipped":
            with pytest.raises(zlib.error):
                d.decompress(stream)
            continue
        got = d.decompress(stream)
        if name == "truncated":
            assert not d.eof and text.startswith(got) and len(got) < len(text)
        else:
            assert d.eof and got == text and d.unused_data == TRAILER, name


def test_gz_source_driver_clean_under_asan_ubsan(tmp_path):
    run_driver("gz_source_driver", "libasan.so",
               {"ASAN_OPTIONS": "halt_on_error=1:abort_on_error=0:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}, tmp_path, 20_000)


def test_gz_source_driver_clean_under_tsan(tmp_path):
    run_driver("gz_source_driver_tsan", "libtsan.so", {"TSAN_OPTIONS": "halt_on_error=1:exitcode=66"}, tmp_path, 5_000)
