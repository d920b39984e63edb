"""The cases of tests/snappy_streams.py before the two host readers: the judge (tests/snappy_judge.py) and the library's
afq_snappy_frame_decode.  The cases must hold what they say before any device decoder is asked about them: every valid stream decodes
to the bytes it was built from, every corrupt one is refused by both."""
import ctypes as C

import pytest

import snappy_judge as sj
import snappy_streams as ss
from util import pkg


def lib_decode(stream):
    """the library's host decoder: the bytes, or None where it refuses"""
    lib = pkg.load_library()
    fn = lib["afq_snappy_frame_decode"]
    fn.argtypes, fn.restype = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t], C.c_int64
    n = fn(stream, len(stream), None, 0)
    if n < 0:
        return None
    out = C.create_string_buffer(max(int(n), 1))
    assert fn(stream, len(stream), out, n) == n
    return out.raw[:n]


def test_the_case_list_is_the_issue_s():
    names = [c.name for c in ss.VALID + ss.CORRUPT]
    assert len(names) == len(set(names))
    for n in (1, 60, 61, 256, 257, 65536):
        for f in range(5):
            assert (f"literal {n} form {f}" in names) == (n <= 60 if f == 0 else n - 1 < 256 ** f)
    assert sum(len(c.chunks) for c in ss.VALID if c.name == "300 small chunks") == 300
    offs = {sum(len(x.data) for x in c.chunks[:i]) % 16 for c in ss.VALID if c.name == "cut at 4097" for i in range(len(c.chunks))}
    assert offs == set(range(16)), "every residue of 16 is an out_off"
    assert any(len(x.body) > len(x.data) + 8192 for c in ss.VALID for x in c.chunks), "a body longer than its output by more than a window"
    assert {c.code for c in ss.CORRUPT} == {1, 2, 3, 4, 5, 6, 8} and {code for _, code in ss.CHUNKS_ONLY} == {7}


@pytest.mark.parametrize("case", ss.VALID, ids=lambda c: c.name)
def test_valid_case_decodes_to_its_bytes(case):
    s = sj.decode(case.stream, keep_chunks=True)
    assert s.data == case.data and s.n_chunks == len(case.chunks)
    assert [(c.type, c.body) for c in s.chunks] == [(0 if c.compressed else 1, c.body) for c in case.chunks]
    assert lib_decode(case.stream) == case.data


@pytest.mark.parametrize("case", ss.CORRUPT, ids=lambda c: c.name)
def test_corrupt_case_is_refused(case):
    with pytest.raises(sj.SnappyJudgeError):
        sj.decode(case.stream)
    assert lib_decode(case.stream) is None
    # ... for the chunk the case names and no earlier one: the stream up to it decodes
    upto = sj.STREAM_ID + b"".join(c.frame() for c in case.chunks[:case.bad])
    assert sj.decode(upto).n_chunks == case.bad and lib_decode(upto) is not None
    with pytest.raises(sj.SnappyJudgeError):
        sj.decode(sj.STREAM_ID + case.chunks[case.bad].frame())
