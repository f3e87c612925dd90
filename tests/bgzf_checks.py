"""What tests/test_bgzf_cpu.py and tests/test_gpu_bgzf.py check of a batched BGZF route ("host" or "device") against the
existing all-members reader and the oracle, over the files of bgzf_cases.py."""
import numpy as np

import sharkmer_amd as sa

import bgzf_cases as bc


def read_all(path, **kw):
    """(reads in order, error or None, (n_reads_read, n_bases_read), member_stats)"""
    r = sa.FastqReader([path], **kw)
    reads, err = [], None
    try:
        while True:
            b, o = r.next_batch(max_seqs=777, max_bases=1 << 17)
            reads += [b[int(o[i]):int(o[i + 1])].tobytes() for i in range(len(o) - 1)]
            if r.stats()["done"]:
                break
    except sa.ShkError as e:
        err = (e.code, e.msg)
    st, ms = r.stats(), r.member_stats()
    r.close()
    return reads, err, (st["n_reads_read"], st["n_bases_read"]), ms


def oracle_counts(orc, path, k=11, chunks=2, histo_max=50):
    run = orc.Run(k, chunks, histo_max)
    try:
        run.read_fastq(path, gzip_all_members=True)
    except orc.OracleError as e:
        return ("error", e.msg)
    res = run.finish()
    return ("ok", res.histograms().tobytes(), res.stats["n_reads_read"], res.stats["n_bases_read"])


def product_counts(orc, path, reads, err, totals, k=11, chunks=2, histo_max=50):
    """the oracle's counting over the reads a reader handed out"""
    if err:
        return ("error", err[1])
    run = orc.Run(k, chunks, histo_max)
    for i in range(0, len(reads), 500):
        part = reads[i:i + 500]
        offs = np.zeros(len(part) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(x) for x in part])
        run.push_batch(np.frombuffer(b"".join(part), dtype=np.uint8), offs)
    res = run.finish()
    return ("ok", res.histograms().tobytes(), totals[0], totals[1])


CLEAN = bc.clean_cases()
DAMAGED = bc.damaged_cases()


def check_clean(orc, tmp_path, monkeypatch, name, route, stat):
    data, n_members, env, _text = CLEAN[name]
    monkeypatch.delenv("SHK_BGZF_BATCH_KB", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = str(tmp_path / f"{name}.fastq.gz")
    open(p, "wb").write(data)
    want = read_all(p, gzip_all_members=True)
    got = read_all(p, bgzf=route)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    assert want[3] == {"device": 0, "host_batch": 0, "sequential": n_members}
    # every member in a batch: the fallback cannot stand in for a decoder that does not work
    assert got[3] == {"device": 0, "host_batch": 0, "sequential": 0, stat: n_members}
    assert product_counts(orc, p, *got[:3]) == oracle_counts(orc, p)


def check_damaged(tmp_path, monkeypatch, name, route, stat):
    data, n_front = DAMAGED[name]
    monkeypatch.delenv("SHK_BGZF_BATCH_KB", raising=False)
    p = str(tmp_path / "damaged.fastq.gz")
    open(p, "wb").write(data)
    want = read_all(p, gzip_all_members=True)
    got = read_all(p, bgzf=route)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    assert got[3][stat] == n_front and got[3]["sequential"] == want[3]["sequential"] - n_front
    # … and with batches of a few members, so that the damage is met in a later batch than the first
    monkeypatch.setenv("SHK_BGZF_BATCH_KB", "7")
    got = read_all(p, bgzf=route)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3][stat] == n_front


LENIENT = bc.lenient_cases()


def check_lenient(tmp_path, monkeypatch, name, route, stat):
    """A stream zlib refuses and our decoders take by one shared rule: the batched route hands out what the
    all-members reader hands out — the same reads, or the same error — and where the stream decodes, it decodes in the
    batch, to the bytes its tokens expand to (the trailer's CRC-32 is theirs)."""
    data, at, decodes = LENIENT[name]
    monkeypatch.delenv("SHK_BGZF_BATCH_KB", raising=False)
    p = str(tmp_path / "lenient.fastq.gz")
    open(p, "wb").write(data)
    want = read_all(p, gzip_all_members=True)
    got = read_all(p, bgzf=route)
    assert got[:3] == want[:3]
    assert (want[1] is None) == decodes
    if decodes:
        assert want[3]["sequential"] == at + 2 and got[3] == {"device": 0, "host_batch": 0, "sequential": 0, stat: at + 2}
    else:
        assert got[3][stat] == at and got[3]["sequential"] == want[3]["sequential"] - at


def interleaved_file():
    """(file bytes, n_members): every crafted valid member among ordinary ones of one record each — neighbouring
    waves of a workgroup on very different streams."""
    recs = [r + b"\n" for r in bc.SMALL.split(b"\n@")]
    recs = [recs[0]] + [b"@" + r for r in recs[1:]]
    recs[-1] = recs[-1][:-1]
    assert b"".join(recs) == bc.SMALL
    plain = [bc.bgzf_member(r, level=(1, 6, 9)[i % 3]) for i, r in enumerate(recs)]
    crafted = [m for name, (ms, _t) in bc.crafted_members().items() if name != "craft_alignment" for m in ms]
    every = len(plain) // len(crafted)
    out = []
    for i, m in enumerate(plain):
        out.append(m)
        if i % every == every - 1 and crafted:
            out.append(crafted.pop(0))
    out += crafted + [bc.EOF_MEMBER]
    return b"".join(out), len(out)


def check_interleaved(orc, tmp_path, monkeypatch, route, stat, batch_kb):
    data, n_members = interleaved_file()
    assert n_members <= 300
    monkeypatch.delenv("SHK_BGZF_BATCH_KB", raising=False)
    if batch_kb:
        monkeypatch.setenv("SHK_BGZF_BATCH_KB", str(batch_kb))
    p = str(tmp_path / "mix.fastq.gz")
    open(p, "wb").write(data)
    want = read_all(p, gzip_all_members=True)
    got = read_all(p, bgzf=route)
    assert want[1] is None and got[:3] == want[:3]
    assert got[3] == {"device": 0, "host_batch": 0, "sequential": 0, stat: n_members}
    assert product_counts(orc, p, *got[:3]) == oracle_counts(orc, p)
