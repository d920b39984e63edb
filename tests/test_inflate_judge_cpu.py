"""The plain-Python inflate (tests/inflate_judge.py) before zlib: on every payload of tests/deflate_streams.py and on 10^4 seeded
mutations of them the judge and zlib.decompressobj(-15) agree on the verdict and, where the payload decodes, on the bytes.  The
verdict of zlib is the host door's (bgzf_inflate of csrc/afq_host.cpp): the stream ends (Z_STREAM_END, whatever lies behind it)
and holds exactly ISIZE bytes.  The cases are held to what they claim: every valid case decodes to the bytes its writer tracked,
every corrupt case is refused with its code at its block, every code is met, and each verdict makes up at least 5 % of the
mutations."""
import collections
import zlib

import pytest

import deflate_streams as ds
import inflate_judge as ij


def zlib_verdict(body, isize):
    """(ok, bytes) as the host door sees the payload"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(body)
    except zlib.error:
        return False, b""
    if not d.eof or len(out) != isize:
        return False, b""
    return True, out


def test_the_judges_crc_is_zlibs():
    for n in (0, 1, 7, 1000):
        data = ds.rnd(n, n)
        assert ij.crc32(data) == zlib.crc32(data) & 0xFFFFFFFF


@pytest.mark.parametrize("case", ds.VALID, ids=lambda c: c.name)
def test_valid_case(case):
    for k, p in enumerate(case.payloads):
        t = ij.inflate(p.body, p.isize, p.crc)
        assert t.code == ij.OK and t.data == p.data and t.produced == p.isize, (case.name, k, ij.CODE_NAMES[t.code])
        assert zlib_verdict(p.body, p.isize) == (True, p.data), (case.name, k)
    data, st, bad = ij.inflate_file(case.file)
    assert bad is None and data == case.data and st["n_blocks"] == len(case.payloads) and st["n_in"] == len(case.file)


def test_the_valid_cases_hold_the_edges_they_name():
    by = {c.name: c for c in ds.VALID}
    assert sorted(p.pending[0] for p in by["a stored block after pending bits"].payloads) == list(range(8))
    assert [p.isize for p in by["ISIZE 0, 1 and 65536"].payloads] == [0, 0, 1, 1, 65536, 65536]
    t = ij.inflate(by["three blocks of three types"].payloads[0].body, by["three blocks of three types"].payloads[0].isize)
    assert (t.n_stored, t.n_fixed, t.n_dynamic) == (1, 1, 1)
    t = ij.inflate(by["repeats across the alphabets"].payloads[0].body, by["repeats across the alphabets"].payloads[0].isize)
    assert t.n_dynamic == 3 and t.n_copies == 3
    for p in by["bytes behind the final block"].payloads[:2]:
        d = zlib.decompressobj(-15)
        assert d.decompress(p.body) == p.data and d.eof and d.unused_data


@pytest.mark.parametrize("case", ds.CORRUPT, ids=lambda c: c.name)
def test_corrupt_case(case):
    for k, p in enumerate(case.payloads):
        t = ij.inflate(p.body, p.isize, p.crc)
        ok, out = zlib_verdict(p.body, p.isize)
        ok = ok and zlib.crc32(out) & 0xFFFFFFFF == p.crc
        assert (t.code == ij.OK) == ok, (case.name, k)
        if k < case.bad:
            assert ok, (case.name, k, "a bad block in front of the one the case names")
        if k == case.bad:
            assert t.code == case.code, (case.name, ij.CODE_NAMES[t.code])
    _, _, bad = ij.inflate_file(case.file)
    assert bad is not None and bad[0] == case.bad and bad[1].code == case.code


def test_every_code_has_its_case():
    assert {c.code for c in ds.CORRUPT} == set(range(1, ij.CODE_COUNT))
    assert len(ij.CODE_NAMES) == ij.CODE_COUNT and set(ij.WORDS) == set(range(1, ij.CODE_COUNT)) - {ij.OUTPUT_SHORT, ij.CRC_MISMATCH}


def test_seeded_mutations():
    muts, judged = ds.mutations()
    assert len(muts) == ds.N_MUTATIONS == 10_000 and len(ds.mutation_base()) >= 40
    for k, ((body, isize), t) in enumerate(zip(muts, judged)):
        ok, out = zlib_verdict(body, isize)
        assert (t.code == ij.OK) == ok, (k, body.hex(), isize, ij.CODE_NAMES[t.code])
        if ok:
            assert t.data == out, (k, body.hex())
    tally = collections.Counter(t.code for t in judged)
    n_ok = tally[ij.OK]
    assert ds.N_MUTATIONS // 20 <= n_ok <= ds.N_MUTATIONS * 19 // 20, n_ok   # each verdict: 5 % at least
    assert set(tally) >= set(range(1, ij.CODE_COUNT)) - {ij.CRC_MISMATCH}, sorted(tally)   # (a mutation carries no CRC)
    print(f"{ds.N_MUTATIONS} mutations of {len(ds.mutation_base())} payloads: {n_ok} decode; refused by code: {sorted((c, n) for c, n in tally.items() if c)}")
