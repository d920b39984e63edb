"""GPU tests of the device snappy frame decoder (csrc/afq_snappy.hip, k_snappy_decode; Quantifier.snappy_frame_decode).  The cases
are tests/snappy_streams.py's - explicit element lists, held before the judge and the host decoder by test_snappy_streams_cpu.py -
plus the device encoder's own streams and the Python writer's.  Every decode is made twice; host output and device output (read
back at every shift) are the judge's bytes, the stats the judge's tallies; a corrupt stream names its lowest bad chunk and the
context serves again."""
import ctypes as C

import numpy as np
import pytest

import snappy_judge as sj
import snappy_streams as ss
from test_snappy_judge_cpu import rad_like
from util import pkg

pytestmark = pytest.mark.gpu

SENTENCE = {code: "corrupt snappy block" for code in range(1, 8)}
SENTENCE[ss.CRC_MISMATCH] = "snappy CRC mismatch"
WORDS = {ss.LITERAL_PAST_BODY: "a literal runs past the block", ss.OFFSET_ZERO: "a copy from offset 0", ss.OFFSET_PAST_START: "a copy from in front of the chunk",
         ss.OUTPUT_PAST_ULEN: "more bytes than declared", ss.TAG_CUT_OFF: "an element cut off", ss.OUTPUT_SHORT: "fewer bytes than declared"}


@pytest.fixture(scope="module")
def q():
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    qq = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    yield qq
    qq.close()


@pytest.fixture(scope="module")
def hip():
    import torch   # (the runtime the library is linked against, already in the process)

    assert torch.cuda.is_available()
    lib = C.CDLL("libamdhip64.so")
    lib.hipMemcpy.argtypes, lib.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    return lib


def read_back(hip, ptr, n):
    buf = C.create_string_buffer(max(n, 1))
    if n:
        assert hip.hipMemcpy(buf, C.c_void_p(ptr), n, 2) == 0   # hipMemcpyDeviceToHost
    return buf.raw[:n]


def decode_every_way(q, hip, stream, want, tally=None, what="", shifts=(0, 1, 2, 3)):
    """host output twice, device output at every shift twice: the same bytes; the stats against the judge's tallies"""
    want = bytes(want)
    if tally is None:
        tally = sj.decode(stream)
        assert tally.data == want, (what, "the judge decodes other bytes")
    stats = {"n_in": len(stream), "n_out": len(want), "n_blocks": tally.n_chunks, "n_blocks_stored": tally.n_stored, "n_literal_bytes": tally.literal_bytes,
             "n_copies": tally.copies}
    for _ in range(2):
        got, st = q.snappy_frame_decode(stream)
        assert got == want, (what, "host output")
        assert st == stats, (what, st, stats)
    for shift in shifts:
        for _ in range(2):
            ptr, n, st = q.snappy_frame_decode(stream, shift=shift, on_device=True)
            assert n == len(want) and st == stats and ptr % 4 == 0, (what, shift)
            assert read_back(hip, ptr + shift, n) == want, (what, "device output", shift)


def test_limits_and_arguments(q):
    lim = pkg.afquant.snappy_decode_limits()
    assert lim["threads"] % 64 == 0 and lim["window"] >= 64 and lim["piece_chunks"] >= 1
    assert 65536 + lim["window"] <= lim["lds_bytes"] <= 160 * 1024 // 2, "two workgroups share a compute unit's LDS"
    lib = pkg.load_library()
    o_b, o_n = C.POINTER(C.c_uint8)(), C.c_uint64()
    E = pkg._abi.AFQ_ERR_INVALID_ARG
    assert lib.afq_snappy_frame_decode_device(None, sj.STREAM_ID, 10, 0, 0, C.byref(o_b), C.byref(o_n), None) == E
    assert lib.afq_snappy_frame_decode_device(q._h, sj.STREAM_ID, 10, 0, 0, None, C.byref(o_n), None) == E
    assert lib.afq_snappy_frame_decode_device(q._h, sj.STREAM_ID, 10, 0, 0, C.byref(o_b), None, None) == E
    assert lib.afq_snappy_frame_decode_device(q._h, None, 10, 0, 0, C.byref(o_b), C.byref(o_n), None) == E
    assert lib.afq_snappy_frame_decode_device(q._h, sj.STREAM_ID, 10, 4, 0, C.byref(o_b), C.byref(o_n), None) == E
    lib.afq_snappy_decode_limits(None)   # (a null array is ignored)


@pytest.mark.parametrize("case", ss.VALID, ids=lambda c: c.name)
def test_valid_case(q, hip, case):
    decode_every_way(q, hip, case.stream, case.data, what=case.name)


@pytest.mark.parametrize("case", ss.CORRUPT, ids=lambda c: c.name)
def test_corrupt_case_names_its_lowest_bad_chunk_and_the_context_serves_again(q, hip, case):
    for on_device in (False, True):
        with pytest.raises(pkg.AfqError) as e:
            q.snappy_frame_decode(case.stream, on_device=on_device)
        assert e.value.code == pkg._abi.AFQ_ERR_BAD_INPUT
        msg = str(e.value)
        assert SENTENCE[case.code] in msg and f"(chunk {case.bad}" in msg, msg
        if case.code in WORDS:
            assert WORDS[case.code] in msg, msg
    good = ss.VALID[len(case.name) % len(ss.VALID)]
    decode_every_way(q, hip, good.stream, good.data, what=f"{good.name} behind {case.name}", shifts=(1,))


@pytest.mark.parametrize("what,stream,sentence", [
    ("no identifier", ss.stored(b"xyz").frame(), "snappy stream does not start with its stream identifier"),
    ("bad identifier", ss.frame(0xFF, b"sNaPpX"), "bad snappy stream identifier"),
    ("truncated chunk", sj.STREAM_ID + ss.stored(b"xyz").frame()[:-1], "truncated snappy frame chunk"),
    ("truncated header", sj.STREAM_ID + b"\x01\x07", "truncated snappy frame header"),
    ("reserved chunk", sj.STREAM_ID + ss.frame(0x02, b"abcd"), "unskippable reserved snappy chunk"),
    ("short chunk", sj.STREAM_ID + ss.frame(0x01, b"abc"), "snappy chunk too short"),
    ("above 65536", sj.STREAM_ID + ss.stored(b"\0" * 65537).frame(), "snappy chunk larger than the frame format's 65536-byte limit"),
    ("malformed length", sj.STREAM_ID + ss.frame(0x00, b"\0\0\0\0\x80"), "corrupt snappy block"),
])
def test_plan_refusals_use_the_host_decoder_s_sentences(q, what, stream, sentence):
    with pytest.raises(pkg.AfqError) as e:
        q.snappy_frame_decode(stream)
    assert e.value.code == pkg._abi.AFQ_ERR_BAD_INPUT and sentence in str(e.value), (what, str(e.value))
    assert q.snappy_frame_decode(sj.STREAM_ID + ss.stored(b"xyz").frame())[0] == b"xyz"


def test_more_chunks_than_a_launch_takes(q, hip):
    """pieces of the stream: piece_chunks + 5 and 2 piece_chunks + 1 data chunks cross in two and three launches, through both
    buffers and back into the first; a bad chunk in the last piece is named by its index in the stream"""
    pc = pkg.afquant.snappy_decode_limits()["piece_chunks"]
    kinds = ss.mixed_kinds()
    for n in (pc + 5, 2 * pc + 1):
        case = ss.Case(f"{n} chunks", [kinds[(7 * k) % len(kinds)] for k in range(n)])
        decode_every_way(q, hip, case.stream, case.data, what=case.name, shifts=(0, 3))
    bad = ss.compressed([("lit", b"abcdefgh"), ("copy", 2, 0, 4)], declared=12)
    case = ss.Case("bad in the third piece", [kinds[k % len(kinds)] for k in range(2 * pc + 3)] + [bad, kinds[0], bad], bad=2 * pc + 3, code=ss.OFFSET_ZERO)
    with pytest.raises(pkg.AfqError) as e:
        q.snappy_frame_decode(case.stream)
    assert f"corrupt snappy block (chunk {2 * pc + 3}: a copy from offset 0)" in str(e.value), str(e.value)


@pytest.mark.parametrize("name", sorted(ss.FAR_STREAMS))
def test_output_offsets_past_4_gib(hip, name):
    """ss.FarStream: 4 GiB and a little of output, mostly chunks of 65 536 zeros, in more than 16 pieces; a chunk begins `before`
    bytes in front of byte 2^32 (inside a literal, inside a copy's destination, or on it), the far chunks behind it have twins of
    other bytes 2^32 lower (tests/test_snappy_far_stream_cpu.py).  Read back: the low 2 MiB with the twins, the MiB in front of byte
    2^32 to the end, the 16 cleared bytes behind, sixteen MiB of the zeros between, then every byte of the fillers in 256 MiB pieces.
    Then a far chunk's CRC with a bit flipped.  Prints each decode's and each sweep's wall time."""
    import time

    FAR = ss.FAR
    fs = ss.FarStream(name)
    stream = fs.stream()
    pc = pkg.afquant.snappy_decode_limits()["piece_chunks"]
    si, so, sc = fs.straddler()
    far, low = fs.group("far"), fs.group("low")
    assert fs.n_chunks > 16 * pc and 150e6 < len(stream) < 300e6 and FAR < fs.total < FAR + (1 << 20)
    assert so == FAR - fs.before and so <= FAR < so + len(sc.data) and (fs.before == 0) == (name == "start on") and (fs.before % 16 != 0 or name != "in a literal")
    assert name != "in a copy" or fs.elem_at(fs.before)[0] == "copy" and fs.elem_at(fs.before)[1] < fs.before
    assert far[ss.FAR_STRADDLER] == (si, so, sc) and all(i > 1 << 16 for i, _, _ in far) and low[0][:2] == (1, len(sc.data) - fs.before)
    assert all(fo - FAR == lo and len(fc.data) == len(lc.data) and (fc.data != lc.data or not fc.data) for (_, lo, lc), (_, fo, fc) in zip(low, far[ss.FAR_STRADDLER + 1:]))
    stats = dict(fs.tallies(), n_in=len(stream), n_out=fs.total)
    windows = [(0, 1 << 21), (FAR - (1 << 20), fs.total + 16)] + [((2 * k + 1) << 27, ((2 * k + 1) << 27) + (1 << 20)) for k in range(16)]
    wants = [fs.window(a, b) for a, b in windows]
    assert wants[1][-16:] == bytes(16) and all(w == bytes(1 << 20) for w in wants[2:]) and wants[0] != fs.window(0, 1 << 21, truncated=True)
    small = ss.VALID[-1]
    q = pkg.Quantifier(pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1), np.zeros(1, np.uint32), device=0)   # its 4 GiB end with the test
    try:
        compared = 0
        for shift in (0, 3):
            t0 = time.perf_counter()
            ptr, n, st = q.snappy_frame_decode(stream, shift=shift, on_device=True)
            print("%s, shift %d: %d bytes decoded in %.2f s" % (name, shift, n, time.perf_counter() - t0))
            assert n == fs.total and st == stats and ptr % 4 == 0, (name, shift, n, st, stats)
            for (a, b), want in zip(windows, wants):
                assert read_back(hip, ptr + shift + a, b - a) == want, (name, shift, "bytes [%d, %d)" % (a, b))
                compared += 1
            # the sweep: every byte between the low 2 MiB and the MiB in front of byte 2^32 is a filler's zero
            t0, room, swept = time.perf_counter(), C.create_string_buffer(1 << 28), 0
            for a in range(0, FAR, 1 << 28):
                a, b = max(a, 1 << 21), min(a + (1 << 28), FAR - (1 << 20))
                assert hip.hipMemcpy(room, C.c_void_p(ptr + shift + a), b - a, 2) == 0
                assert not np.frombuffer(room, np.uint8, b - a).any(), (name, shift, "a byte of the fillers in [%d, %d)" % (a, b))
                swept += b - a
            assert swept == FAR - (1 << 21) - (1 << 20)
            print("%s, shift %d: %d bytes swept in %.2f s" % (name, shift, swept, time.perf_counter() - t0))
            del room
        assert compared == 2 * len(windows) == 36
        del stream
        bi = far[ss.FAR_STRADDLER + 3][0]
        bad = fs.stream(crc_flip=(bi, 9))
        t0 = time.perf_counter()
        with pytest.raises(pkg.AfqError) as e:
            q.snappy_frame_decode(bad, shift=1, on_device=True)
        print("%s, a CRC bit of chunk %d: refused in %.2f s" % (name, bi, time.perf_counter() - t0))
        assert bi > 1 << 16 and e.value.code == pkg._abi.AFQ_ERR_BAD_INPUT and f"snappy CRC mismatch (chunk {bi})" in str(e.value), str(e.value)
        decode_every_way(q, hip, small.stream, small.data, what=f"{small.name} behind the refusal", shifts=(1,))
    finally:
        q.close()


@pytest.mark.parametrize("fill", ["zeros", "random", "rad"])
def test_the_device_encoder_s_streams(q, hip, fill):
    B = pkg.afquant.snappy_limits()["block"]
    rng = np.random.default_rng(11)
    for n in (0, 1, B - 1, B, B + 1, 3 * B + 17):
        data = b"\0" * n if fill == "zeros" else bytes(rng.integers(0, 256, n, dtype=np.uint8)) if fill == "random" else rad_like(n, seed=n)
        stream, est = q.snappy_frame_encode(data)
        t = sj.decode(stream)
        assert t.data == data
        assert (est["n_blocks"], est["n_blocks_stored"], est["n_literal_bytes"], est["n_copies"]) == (t.n_chunks, t.n_stored, t.literal_bytes, t.copies)
        decode_every_way(q, hip, stream, data, tally=t, what=f"{fill} {n}", shifts=(0, 1, 2, 3) if n in (B + 1, 3 * B + 17) else (0,))


def test_the_python_writer_s_streams(q, hip):
    """rad.snappy_frame_encode: Google's blocks where pyarrow is importable (long copies, the 1-byte-offset form), the writer's own
    literal blocks otherwise"""
    try:
        import pyarrow as pa
        real = pa.Codec.is_available("snappy")
    except ImportError:
        real = False
    print("rad.snappy_frame_encode:", "Google's snappy blocks (pyarrow)" if real else "the writer's own literal blocks (no pyarrow here)")
    rng = np.random.default_rng(3)
    data = bytes(rng.integers(0, 256, 70_000, dtype=np.uint8)) + rad_like(190_000) + b"\0" * 5000 + bytes(rng.integers(0, 2, 30_000, dtype=np.uint8))
    for chunk in (1000, 60_000, 65_536):
        stream = pkg.rad.snappy_frame_encode(data, chunk=chunk, real=real)
        decode_every_way(q, hip, stream, data, what=f"python writer, chunk {chunk}", shifts=(0, 1, 2, 3) if chunk == 60_000 else (2,))


def test_a_stream_that_does_not_fit_is_refused_before_any_launch(hip, monkeypatch):
    """AFQ_TEST_SNAPPY_DEC_ROOM_BYTES: the decoder answers as a device with that many bytes free would - AFQ_ERR_OOM with the sizes -
    for what it still has to allocate; what it already holds from an earlier call is not asked for again; the context serves again"""
    big = ss.Case("two full chunks", [ss.stored(ss.rnd(65536, 1)), ss.stored(ss.rnd(65536, 2))])
    q = pkg.Quantifier(pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1), np.zeros(1, np.uint32), device=0)   # a context that holds no buffer yet
    try:
        _does_not_fit(q, hip, monkeypatch, big)
    finally:
        q.close()


def _does_not_fit(q, hip, monkeypatch, big):
    q.snappy_frame_decode(ss.VALID[0].stream)   # (small buffers are held)
    monkeypatch.setenv("AFQ_TEST_SNAPPY_DEC_ROOM_BYTES", "1000")
    with pytest.raises(pkg.AfqError) as e:
        q.snappy_frame_decode(big.stream)
    assert e.value.code == pkg._abi.AFQ_ERR_OOM and "does not fit the device" in str(e.value) and "> 1000 bytes free" in str(e.value), str(e.value)
    assert q.snappy_frame_decode(ss.VALID[0].stream)[0] == ss.VALID[0].data   # nothing to allocate: served under the same room
    monkeypatch.delenv("AFQ_TEST_SNAPPY_DEC_ROOM_BYTES")
    decode_every_way(q, hip, big.stream, big.data, what="with room again", shifts=(0,))
