"""GPU tests of the device snappy frame encoder (csrc/afq_snappy.hip; Quantifier.snappy_frame_encode).  No compressor promises its
bytes, so every stream goes before three independent readers - tests/snappy_judge.py, the library's own afq_snappy_frame_decode,
and Google's snappy (through pyarrow) on the raw block of every compressed chunk - and its stats must equal the judge's tallies.
Shapes derive from snappy_limits()."""
import ctypes as C

import numpy as np
import pytest

import snappy_judge as sj
from test_snappy_judge_cpu import rad_like
from util import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def q():
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    qq = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    yield qq
    qq.close()


@pytest.fixture(scope="module")
def B():
    return pkg.afquant.snappy_limits()["block"]


def google():
    try:
        import pyarrow as pa
    except ImportError:
        return None
    return pa.Codec("snappy") if pa.Codec.is_available("snappy") else None


def lib_decode(stream, n):
    lib = pkg.load_library()
    lib.afq_snappy_frame_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    lib.afq_snappy_frame_decode.restype = C.c_int64
    out = C.create_string_buffer(max(n, 1))
    got = lib.afq_snappy_frame_decode(stream, len(stream), out, n)
    assert got == n, (got, n)
    return out.raw[:n]


def three_readers(stream, want, stats, B, what=""):
    """judge, library decoder, Google's snappy on every 0x00 body; the stats against the judge's tallies; the size bound.
    Returns the judge's view."""
    want = bytes(want)
    s = sj.decode(stream, keep_chunks=True)
    assert s.data == want, (what, "the judge decodes other bytes")
    assert stream[:10] == sj.STREAM_ID and s.n_identifiers == 1, what
    assert [len(c.data) for c in s.chunks] == [min(B, len(want) - i) for i in range(0, len(want), B)], (what, "one chunk per block of input, in order")
    assert lib_decode(stream, len(want)) == want, (what, "the library decodes other bytes")
    codec = google()
    for i, c in enumerate(s.chunks):
        if c.type == 0:
            assert len(c.body) < len(c.data), (what, i, "a compressed chunk that is not shorter than its bytes")
            if codec is not None:
                assert codec.decompress(c.body, decompressed_size=len(c.data), asbytes=True) == c.data, (what, i, "Google's snappy decodes other bytes")
    if stats is not None:
        assert stats == {"n_in": len(want), "n_out": len(stream), "n_blocks": s.n_chunks, "n_blocks_stored": s.n_stored, "n_literal_bytes": s.literal_bytes,
                         "n_copies": s.copies}, (what, stats)
        assert len(stream) <= 10 + len(want) + 8 * s.n_chunks, what
    return s


def encode(q, data, B, what=""):
    stream, st = q.snappy_frame_encode(data)
    return three_readers(stream, data, st, B, what), stream, st


# ------------------------------------------------------------------------------------------------------------------ lengths
def lengths(B):
    return sorted({0, 1, 3, 4, 5, 59, 60, 61, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, B - 1, B, B + 1, 2 * B + 17})


@pytest.mark.parametrize("fill", ["zeros", "random", "rad"])
def test_every_length(q, B, fill):
    rng = np.random.default_rng(11)
    for n in lengths(B):
        data = b"\0" * n if fill == "zeros" else bytes(rng.integers(0, 256, n, dtype=np.uint8)) if fill == "random" else rad_like(n, seed=n)
        s, stream, st = encode(q, data, B, f"{fill} {n}")
        if n == 0:
            assert stream == sj.STREAM_ID and st["n_blocks"] == 0
        if fill == "random":
            assert st["n_blocks_stored"] == st["n_blocks"] and len(stream) == 10 + n + 8 * st["n_blocks"], n
        if fill == "zeros" and n >= 255:
            # a chunk of zeros: the 64 positions of its first step as a literal, then copies of 3 bytes a 64; a last chunk too short
            # to gain anything is stored
            assert st["n_blocks_stored"] == (1 if 0 < n % B < 255 else 0), n
            assert len(stream) <= 10 + (8 + 3 + 66 + 3 + 3) * st["n_blocks"] + 3 * (n // 64), n
        if fill == "rad" and n >= 4096:
            assert s.chunks[0].type == 0 and st["n_copies"] > 0, n


def test_null_out_pointers_on_a_live_context(q):
    lib = pkg.load_library()
    o_b, o_n = C.POINTER(C.c_uint8)(), C.c_uint64()
    assert lib.afq_snappy_frame_encode(q._h, b"abcd", 4, 0, None, C.byref(o_n), None) == pkg._abi.AFQ_ERR_INVALID_ARG
    assert lib.afq_snappy_frame_encode(q._h, b"abcd", 4, 0, C.byref(o_b), None, None) == pkg._abi.AFQ_ERR_INVALID_ARG
    assert lib.afq_snappy_frame_encode(q._h, None, 4, 0, C.byref(o_b), C.byref(o_n), None) == pkg._abi.AFQ_ERR_INVALID_ARG
    stream, st = q.snappy_frame_encode(b"")   # (no bytes and no pointer is the empty input)
    assert stream == sj.STREAM_ID and st["n_out"] == 10


# ------------------------------------------------------------------------------------------------------------------ planted matches
def planted(rng, prefix, d, m, tail):
    x = bytearray(rng.integers(0, 256, prefix, dtype=np.uint8).tobytes())
    assert d <= len(x)
    for _ in range(m):
        x.append(x[-d])
    return bytes(x) + rng.integers(0, 256, tail, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("d", [1, 3, 4, 63, 64, 65, 2047, 2048, 2049, "B-1"])
def test_planted_matches(q, B, d):
    """a random prefix, m bytes repeated from d back, random bytes: every copy form and element split, found or (m = 3) not"""
    d = B - 1 if d == "B-1" else d
    rng = np.random.default_rng(100 + d)
    for m in (3, 4, 11, 12, 64, 65, 67, 68, 1000):
        pre = d + 5 if d < B - 1 else d   # (d = B - 1: the source is the chunk's first byte, the repeat ends at or behind its end)
        data = planted(rng, pre, d, m, 37)
        s, stream, st = encode(q, data, B, f"d {d} m {m}")
        # (a source in the step of the repeat's own start is not in the table yet: the match is then found a step - at most 64
        #  bytes - late; a slot taken by a later position can cost a few bytes more)
        if m == 1000 and d < B - 1:
            assert st["n_copies"] >= (m - 64 - 67) // 64 and s.chunks[0].type == 0, (d, m, st)
        if m >= 64 and 64 <= d < B - 1:
            assert st["n_copies"] >= 1, (d, m, st)
        if d == B - 1:   # the repeat's source is the chunk in front: nothing to find
            assert st["n_copies"] == 0 and st["n_blocks_stored"] == 2, (m, st)


def test_a_match_that_ends_with_its_chunk_and_one_that_would_cross_it(q, B):
    rng = np.random.default_rng(5)
    # the repeat fills the chunk's last 500 bytes exactly
    data = planted(rng, B - 500, 300, 500, 0)
    assert len(data) == B
    s, _, st = encode(q, data + rng.integers(0, 256, 100, dtype=np.uint8).tobytes(), B, "ends with the chunk")
    assert s.chunks[0].type == 0 and st["n_copies"] >= 7
    # a period-300 repeat of 1000 bytes that straddles the boundary: either side decodes alone
    data = planted(rng, B - 400, 300, 1000, 50)
    s, _, st = encode(q, data, B, "straddles")
    assert len(s.chunks) == 2 and s.chunks[0].type == 0 and s.chunks[1].type == 0
    for c in s.chunks:   # chunks decode independently: the judge decoded each raw block from nothing
        assert sj.raw_decode(c.body) == c.data
    # would-be matches that begin in the input's last 1..7 bytes
    for k in range(1, 8):
        head = rng.integers(0, 256, 600, dtype=np.uint8).tobytes()
        encode(q, b"\0" * 700 + head + head[:k], B, f"tail {k}")
        encode(q, head + head[:k], B, f"short tail {k}")


def test_device_slice_whose_following_bytes_continue_the_pattern(q, B):
    """a read past n_bytes would lengthen the last match and break the decode"""
    import torch

    rec = np.frombuffer(rad_like(24 * 6000, seed=2), np.uint8)
    period = np.tile(np.frombuffer(rad_like(24, seed=9), np.uint8), 9000)
    for al, n in ((0, 24 * 1000 + 5), (1, B + 24 * 50 + 7), (3, 2 * B - 2)):
        for src in (period, rec):
            t = torch.from_numpy(src.copy()).cuda()
            torch.cuda.synchronize()
            want = src[al:al + n].tobytes()
            stream, st = q.snappy_frame_encode(None, d_ptr=t.data_ptr() + al, n_bytes=n)
            three_readers(stream, want, st, B, f"slice +{al} {n}")


# ------------------------------------------------------------------------------------------------------------------ collisions, determinism, ratio
def test_two_symbol_alphabet(q, B):
    """every 4-gram recurs and the table's slots are fought over in every step"""
    data = bytes(np.random.default_rng(8).integers(0, 2, 3 * B, dtype=np.uint8))
    s, stream, st = encode(q, data, B, "two symbols")
    assert st["n_blocks_stored"] == 0 and len(stream) < len(data) // 2


def test_the_stream_is_a_function_of_the_input(q, B):
    rng = np.random.default_rng(21)
    data = rad_like(2 * B + 999, seed=4) + bytes(rng.integers(0, 2, B, dtype=np.uint8)) + bytes(rng.integers(0, 256, 3000, dtype=np.uint8))
    a, _ = q.snappy_frame_encode(data)
    q.snappy_frame_encode(bytes(rng.integers(0, 4, 3 * B + 5, dtype=np.uint8)))
    b, _ = q.snappy_frame_encode(data)
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    q2 = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    try:
        c, _ = q2.snappy_frame_encode(data)
    finally:
        q2.close()
    assert a == b and a == c
    three_readers(a, data, None, B, "determinism")


@pytest.mark.parametrize("period", [24, 64])
def test_ratio_on_periodic_records(q, B, period):
    """a greedy encoder spends 3 bytes per at most 64 on a periodic input, plus a period of literals a chunk (this one: the 64
    positions of a chunk's first step): under 1/8 of the input"""
    rec = bytes(np.random.default_rng(period).integers(0, 256, period, dtype=np.uint8))
    data = (rec * (4 * B // period + 1))[:4 * B]
    s, stream, st = encode(q, data, B, f"period {period}")
    assert st["n_blocks"] == 4 and st["n_blocks_stored"] == 0 and len(stream) < len(data) // 8, len(stream)


# ------------------------------------------------------------------------------------------------------------------ past 4 GiB
def test_offsets_past_4_gib(q, B):
    """4 GiB + 64 KiB of random bytes (stored chunks), then 1 MiB of period-24 records: the compressed chunks' source and
    destination offsets lie past 2^32.  The library's decoder reads all of it; the judge and Google's snappy the last 32 chunks."""
    import torch

    n_rand, n_rec = (1 << 32) + (64 << 10), 1 << 20
    n = n_rand + n_rec
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 30
    for a in range(0, n_rand, step):
        t[a:min(a + step, n_rand)] = torch.randint(0, 256, (min(step, n_rand - a),), dtype=torch.uint8, device="cuda", generator=g)
    rec = rad_like(n_rec, seed=6, period=24)
    t[n_rand:] = torch.from_numpy(np.frombuffer(rec, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    lib = pkg.load_library()
    o_b, o_n, st = C.POINTER(C.c_uint8)(), C.c_uint64(), pkg._abi.AfqSnappyStats()
    q._check(lib.afq_snappy_frame_encode(q._h, C.c_void_p(t.data_ptr()), n, 1, C.byref(o_b), C.byref(o_n), C.byref(st)))
    try:
        n_out, nb = int(o_n.value), -(-n // B)
        assert st.n_in == n and st.n_out == n_out and st.n_blocks == nb and n_out <= 10 + n + 8 * nb
        n_rec_blocks = n_rec // B
        assert st.n_blocks_stored == nb - n_rec_blocks, "the random chunks are stored, the records' chunks compressed"
        stream = np.ctypeslib.as_array(o_b, shape=(n_out,))
        # the library's decoder, compared in slices
        lib.afq_snappy_frame_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        lib.afq_snappy_frame_decode.restype = C.c_int64
        dec = np.empty(n, np.uint8)
        assert lib.afq_snappy_frame_decode(stream.ctypes.data, n_out, dec.ctypes.data, n) == n
        for a in range(0, n, step):
            b = min(a + step, n)
            assert np.array_equal(dec[a:b], t[a:b].cpu().numpy()), f"bytes {a}..{b}"
        del dec
        # the last 32 chunks before the judge and Google's snappy
        p, starts = 10, []
        while p < n_out:
            starts.append(p)
            p += 4 + (int(stream[p + 1]) | int(stream[p + 2]) << 8 | int(stream[p + 3]) << 16)
        assert p == n_out and len(starts) == nb
        assert starts[-n_rec_blocks] > 1 << 32, "the compressed chunks stand past 2^32 in the stream"
        tail_at = starts[-32]
        tail = sj.STREAM_ID + stream[tail_at:].tobytes()
        want = t[n - 32 * B:].cpu().numpy().tobytes()
        s = sj.decode(tail, keep_chunks=True)
        assert s.data == want and s.n_stored == 32 - n_rec_blocks
        assert s.literal_bytes == st.n_literal_bytes and s.copies == st.n_copies
        codec = google()
        if codec is not None:
            for c in s.chunks:
                if c.type == 0:
                    assert codec.decompress(c.body, decompressed_size=len(c.data), asbytes=True) == c.data
    finally:
        lib.afq_free(o_b)
