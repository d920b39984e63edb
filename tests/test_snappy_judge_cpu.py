"""CPU tests of tests/snappy_judge.py, the plain-Python reader that judges the device snappy encoder's streams, and of what the
encoder's entry points answer without a device."""
import ctypes as C

import numpy as np
import pytest

import snappy_judge as sj
from util import pkg

rad = pkg.rad


def rad_like(n, seed=0, period=24):
    """n bytes of `period`-byte records that differ in a few fields."""
    rng = np.random.default_rng(seed)
    k = n // period + 1
    rec = np.zeros((k, period), np.uint8)
    rec[:, 0] = 1
    rec[:, 4:8] = np.frombuffer(np.uint32(0x1234ABCD).tobytes(), np.uint8)
    rec[:, 8:12] = rng.integers(0, 256, (k, 4), dtype=np.uint8)
    rec[:, 12:14] = rng.integers(0, 256, (k, 2), dtype=np.uint8)
    return rec.reshape(-1)[:n].tobytes()


def test_crc32c_check_value_and_mask():
    assert sj.crc32c(b"123456789") == 0xE3069283
    assert sj.crc32c(b"") == 0
    assert sj.mask_crc(0) == 0xA282EAD8
    assert sj.mask_crc(0xE3069283) == (((0xE3069283 >> 15) | (0xE3069283 << 17)) + 0xA282EAD8) & 0xFFFFFFFF


@pytest.mark.parametrize("real", [False, True])
def test_judge_decodes_the_python_writer(real):
    rng = np.random.default_rng(3)
    data = bytes(rng.integers(0, 256, 70_000, dtype=np.uint8)) + rad_like(90_000) + b"\0" * 5000
    for chunk in (1000, 60_000, 65_536):
        s = sj.decode(rad.snappy_frame_encode(data, chunk=chunk, real=real), keep_chunks=True)
        assert s.data == data and s.n_identifiers == 1
        assert s.n_chunks == -(-len(data) // chunk) and s.n_stored == (s.n_chunks + 1) // 2
        assert [c.type for c in s.chunks] == [1 - (k & 1) for k in range(s.n_chunks)]
    assert sj.decode(rad.snappy_frame_encode(b"")).data == b""


def test_judge_decodes_googles_blocks():
    pa = pytest.importorskip("pyarrow")
    if not pa.Codec.is_available("snappy"):
        pytest.skip("pyarrow without snappy")
    codec = pa.Codec("snappy")
    rng = np.random.default_rng(4)
    for data in (rad_like(65_536), b"\0" * 65_536, bytes(rng.integers(0, 2, 40_000, dtype=np.uint8)), b"abcd" * 3 + b"x", b"a"):
        t = {}
        assert sj.raw_decode(codec.compress(data, asbytes=True), t) == data
        assert t["literal_bytes"] <= len(data) and (t["copies"] > 0 or t["literal_bytes"] == len(data))


def frame(t, body):
    return bytes([t]) + len(body).to_bytes(3, "little") + body


def data_chunk(t, payload, data):
    return frame(t, sj.mask_crc(sj.crc32c(data)).to_bytes(4, "little") + payload)


def lit(b):
    assert 0 < len(b) <= 60
    return bytes([(len(b) - 1) << 2]) + b


def copy2(off, n):
    return bytes([((n - 1) << 2) | 2]) + off.to_bytes(2, "little")


def test_judge_accepts_hand_made_streams():
    want = b"abcdabcdabcdab"
    blk = bytes([len(want)]) + lit(b"abcd") + copy2(4, 10)
    s = sj.decode(sj.STREAM_ID + data_chunk(0, blk, want) + frame(0xFE, b"\0" * 7) + frame(0x80, b"skip me") + data_chunk(1, b"xyz", b"xyz") + sj.STREAM_ID)
    assert s.data == want + b"xyz" and (s.n_chunks, s.n_stored, s.literal_bytes, s.copies, s.n_identifiers) == (2, 1, 4, 1, 2)
    one = bytes([8]) + lit(b"abcd") + bytes([1 | (0 << 2) | (0 << 5), 4])   # the 1-byte-offset form: 4 bytes from 4 back
    assert sj.raw_decode(one) == b"abcdabcd"
    assert sj.decode(sj.STREAM_ID).data == b""


REFUSED = {
    "first chunk is not the identifier": data_chunk(1, b"xyz", b"xyz"),
    "empty stream": b"",
    "reserved unskippable chunk": sj.STREAM_ID + frame(0x02, b"abcd"),
    "bad identifier": frame(0xFF, b"sNaPpX"),
    "stored chunk above 65536": sj.STREAM_ID + data_chunk(1, b"\0" * 65537, b"\0" * 65537),
    "compressed chunk above 65536": sj.STREAM_ID + data_chunk(0, bytes([0x81, 0x80, 0x04]) + lit(b"a"), b"a"),
    "offset 0": sj.STREAM_ID + data_chunk(0, bytes([8]) + lit(b"abcd") + copy2(0, 4), b"abcdabcd"),
    "offset beyond the bytes produced": sj.STREAM_ID + data_chunk(0, bytes([8]) + lit(b"abcd") + copy2(5, 4), b"abcdabcd"),
    "length mismatch (short)": sj.STREAM_ID + data_chunk(0, bytes([9]) + lit(b"abcd") + copy2(4, 4), b"abcdabcd"),
    "length mismatch (long)": sj.STREAM_ID + data_chunk(0, bytes([7]) + lit(b"abcd") + copy2(4, 4), b"abcdabcd"),
    "trailing bytes": sj.STREAM_ID + data_chunk(0, bytes([4]) + lit(b"abcd") + lit(b"e"), b"abcd"),
    "checksum": sj.STREAM_ID + data_chunk(1, b"xyz", b"xyy"),
    "truncated chunk": sj.STREAM_ID + data_chunk(1, b"xyz", b"xyz")[:-1],
    "truncated literal": sj.STREAM_ID + data_chunk(0, bytes([4, 3 << 2]) + b"abc", b"abcd"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_judge_refuses(what):
    with pytest.raises(sj.SnappyJudgeError):
        sj.decode(REFUSED[what])


def test_the_library_decoder_agrees_on_the_hand_made_streams():
    """(the second of the GPU tests' three readers, on the same streams: it reads what the judge reads)"""
    lib = pkg.load_library()
    lib.afq_snappy_frame_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    lib.afq_snappy_frame_decode.restype = C.c_int64
    want = b"abcdabcdabcdab"
    enc = sj.STREAM_ID + data_chunk(0, bytes([len(want)]) + lit(b"abcd") + copy2(4, 10), want) + data_chunk(1, b"xyz", b"xyz")
    out = C.create_string_buffer(64)
    assert lib.afq_snappy_frame_decode(enc, len(enc), out, 64) == len(want) + 3 and out.raw[:len(want) + 3] == want + b"xyz"
    for what in ("offset 0", "offset beyond the bytes produced", "checksum", "first chunk is not the identifier"):
        assert lib.afq_snappy_frame_decode(REFUSED[what], len(REFUSED[what]), out, 64) < 0, what


def test_symbols_limits_and_null_arguments_without_a_gpu():
    lib = pkg.load_library()
    for name in ("afq_snappy_frame_encode", "afq_snappy_limits", "afq_set_collate_compress", "afq_collate_sz", "afq_atac_collate_sz", "afq_collate_multi_sz"):
        assert hasattr(lib, name), name
    for name in ("afq_snappy_frame_encode", "afq_snappy_limits", "afq_set_collate_compress"):
        assert name in pkg._abi.EXPORTS
    lim = pkg.afquant.snappy_limits()
    assert 0 < lim["block"] <= 65536 and lim["hash_slots"] & (lim["hash_slots"] - 1) == 0 and lim["hash_slots"] >= 256
    assert 4 <= lim["max_copy"] <= 64 and lim["blocks_per_workgroup"] >= 1
    lib.afq_snappy_limits(None)   # (a null array is ignored)
    o_b, o_n, st = C.POINTER(C.c_uint8)(), C.c_uint64(), pkg._abi.AfqSnappyStats()
    assert lib.afq_snappy_frame_encode(None, b"abcd", 4, 0, C.byref(o_b), C.byref(o_n), C.byref(st)) == pkg._abi.AFQ_ERR_INVALID_ARG
    assert lib.afq_snappy_frame_encode(None, b"abcd", 4, 0, None, None, None) == pkg._abi.AFQ_ERR_INVALID_ARG
    assert not o_b and o_n.value == 0
    lib.afq_set_collate_compress(None, 1)   # (a null context is ignored)
    assert C.sizeof(pkg._abi.AfqSnappyStats) == 48


def test_sz_entries_check_their_options_and_ignore_compress(tmp_path):
    """The _sz doors take the opts of the plain entries: the same first refusals, and `compress` set is not one of them."""
    lib = pkg.load_library()
    lib.afq_host_last_error.restype = C.c_char_p

    def entry(name, opts):   # (function objects of this test's own: other modules declare afq_collate over struct types of theirs)
        fn = lib[name]
        fn.argtypes, fn.restype = [C.POINTER(opts)], C.c_int
        return fn, opts

    for fn, opts in (entry("afq_collate_sz", pkg._abi.AfqCollateOpts), entry("afq_atac_collate_sz", pkg._abi.AfqAtacCollateOpts),
                     entry("afq_collate_multi_sz", pkg._abi.AfqCollateMultiOpts)):
        assert fn(None) == pkg._abi.AFQ_ERR_INVALID_ARG
        o = opts()
        o.input_dir = str(tmp_path).encode()
        assert fn(C.byref(o)) == pkg._abi.AFQ_ERR_INVALID_ARG and b"-r" in lib.afq_host_last_error()
        o.rad_dir, o.compress = str(tmp_path).encode(), 1
        assert fn(C.byref(o)) == pkg._abi.AFQ_ERR_BAD_INPUT and b"generate_permit_list.json" in lib.afq_host_last_error()
    for fn, opts in (entry("afq_collate", pkg._abi.AfqCollateOpts), entry("afq_atac_collate", pkg._abi.AfqAtacCollateOpts), entry("afq_collate_multi", pkg._abi.AfqCollateMultiOpts)):
        o = opts()
        o.input_dir, o.rad_dir, o.compress = str(tmp_path).encode(), str(tmp_path).encode(), 1
        assert fn(C.byref(o)) == pkg._abi.AFQ_ERR_UNSUPPORTED and lib.afq_host_last_error() == b"compressed output is not supported"
