"""GPU tests of the device BGZF inflater (csrc/afq_inflate.hip, k_bgzf_inflate; Quantifier.bgzf_inflate).  The cases are
tests/deflate_streams.py's - explicit deflate blocks, held before the judge and zlib by test_inflate_judge_cpu.py - plus blocks
that zlib made of BAM-like bytes at every level and strategy.  Every inflate is made twice; host output and device output (read
back at shifts 0, 1, 5 and 15) are the judge's bytes, the stats the judge's tallies; a corrupt file names its lowest bad block
with the host door's sentence and the context serves again."""
import ctypes as C
import zlib

import numpy as np
import pytest

import bam_cases as B
import deflate_streams as ds
import inflate_judge as ij
from util import pkg

pytestmark = pytest.mark.gpu

SHIFTS = (0, 1, 5, 15)


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


def inflate_every_way(q, hip, data, want, stats=None, what="", shifts=SHIFTS):
    """host output twice, device output at every shift twice: the same bytes; the stats against the judge's tallies"""
    want = bytes(want)
    if stats is None:
        got, stats, bad = ij.inflate_file(data)
        assert bad is None and got == want, (what, "the judge inflates other bytes")
    for _ in range(2):
        got, st = q.bgzf_inflate(data)
        assert got == want, (what, "host output")
        assert st == stats, (what, st, stats)
    for shift in shifts:
        for _ in range(2):
            (ptr, n), st = q.bgzf_inflate(data, shift=shift, on_device=True)
            assert n == len(want) and st == stats and ptr % 16 == 0, (what, shift)
            assert read_back(hip, ptr + shift, n) == want, (what, "device output", shift)
            if shift:
                assert read_back(hip, ptr, shift) == bytes(shift), (what, "the bytes in front", shift)
            assert read_back(hip, ptr + shift + n, 16) == bytes(16), (what, "the bytes behind", shift)


def test_limits_and_arguments(q):
    lim = pkg.inflate_limits()
    assert lim["threads"] % 64 == 0 and lim["piece_blocks"] >= 1 and lim["blocks_per_workgroup"] >= 1
    assert 65536 < lim["lds_bytes"] <= 160 * 1024
    lib = pkg.load_library()
    o_b, o_n = C.POINTER(C.c_uint8)(), C.c_uint64()
    E = pkg._abi.AFQ_ERR_INVALID_ARG
    eof = B.BGZF_EOF
    assert lib.afq_bgzf_inflate_device(None, eof, len(eof), 0, 0, C.byref(o_b), C.byref(o_n), None) == E
    assert lib.afq_bgzf_inflate_device(q._h, eof, len(eof), 0, 0, None, C.byref(o_n), None) == E
    assert lib.afq_bgzf_inflate_device(q._h, eof, len(eof), 0, 0, C.byref(o_b), None, None) == E
    assert lib.afq_bgzf_inflate_device(q._h, None, len(eof), 0, 0, C.byref(o_b), C.byref(o_n), None) == E
    assert lib.afq_bgzf_inflate_device(q._h, eof, len(eof), 16, 0, C.byref(o_b), C.byref(o_n), None) == E
    assert b"shift is 0..15" in lib.afq_last_error(q._h)
    lib.afq_inflate_limits(None)   # (a null array is ignored)


@pytest.mark.parametrize("case", ds.VALID, ids=lambda c: c.name)
def test_valid_case(q, hip, case):
    inflate_every_way(q, hip, case.file, case.data, what=case.name)


@pytest.mark.parametrize("case", ds.CORRUPT, ids=lambda c: c.name)
def test_corrupt_case_names_its_lowest_bad_block_and_the_context_serves_again(q, hip, case):
    p = case.payloads[case.bad]
    if case.code == ij.CRC_MISMATCH:
        sentence = "bad CRC32"
    elif case.code == ij.OUTPUT_SHORT:
        sentence = "ISIZE says %d bytes, the deflate stream holds %d" % (p.isize, ij.inflate(p.body, p.isize).produced)
    else:
        sentence = "the deflate stream is corrupt or longer than ISIZE (%s)" % ij.WORDS[case.code]
    for on_device in (False, True):
        with pytest.raises(pkg.AfqError) as e:
            q.bgzf_inflate(case.file, on_device=on_device)
        assert e.value.code == pkg._abi.AFQ_ERR_BAD_INPUT
        assert str(e.value).endswith("BGZF block %d: %s" % (case.bad, sentence)), str(e.value)
    good = ds.VALID[len(case.name) % len(ds.VALID)]
    inflate_every_way(q, hip, good.file, good.data, what=f"{good.name} behind {case.name}", shifts=(5,))


def test_plan_refusals_use_the_host_door_s_sentences(q):
    good = ds.GOOD[0].block()
    magic, no_bc, small, big = bytearray(good), bytearray(good), bytearray(good), bytearray(good)
    magic[1] = 0x8c
    no_bc[12] = ord("X")
    small[16:18] = (20).to_bytes(2, "little")
    big[-4:] = (65537).to_bytes(4, "little")
    for what, data, sentence in [("cut", good + good[:-5], "BGZF block 1: truncated: the block has %d bytes, the file %d more" % (len(good), len(good) - 5)),
                                 ("cut head", good + good[:7], "BGZF block 1: truncated: 7 bytes where a block header has 18"),
                                 ("magic", good + bytes(magic), "BGZF block 1: bad gzip magic (1f 8b 08 with an extra field is expected)"),
                                 ("no BC", good + bytes(no_bc), "BGZF block 1: no BC extra field: not a BGZF block"),
                                 ("small", good + bytes(small), "BGZF block 1: BSIZE is smaller than the block's own header and trailer"),
                                 ("big", good + bytes(big), "BGZF block 1: ISIZE 65537 is above the 65536 bytes of a BGZF block")]:
        with pytest.raises(pkg.AfqError) as e:
            q.bgzf_inflate(data)
        assert e.value.code == pkg._abi.AFQ_ERR_BAD_INPUT and str(e.value).endswith(sentence), (what, str(e.value))
        assert q.bgzf_inflate(good)[0] == ds.GOOD[0].data


def test_more_blocks_than_a_launch_takes(q, hip):
    """pieces of the file: piece_blocks + 5 and 2 piece_blocks + 1 tiny blocks cross in two and three launches, through both
    buffers and back into the first; a bad block in the last piece is named by its index in the file"""
    pb = pkg.inflate_limits()["piece_blocks"]
    kinds = [p for c in ds.VALID for p in c.payloads if len(p.body) < 120]
    assert len(kinds) >= 20
    tallies = [ij.inflate(p.body, p.isize, p.crc) for p in kinds]
    blocks = [p.block() for p in kinds]
    for n in (pb + 5, 2 * pb + 1):
        idx = [(7 * k) % len(kinds) for k in range(n)]
        data, want = b"".join(blocks[i] for i in idx), b"".join(kinds[i].data for i in idx)
        stats = dict(n_in=len(data), n_out=len(want), n_blocks=n, n_blocks_empty=sum(kinds[i].isize == 0 for i in idx))
        for k in ("n_stored", "n_fixed", "n_dynamic", "n_literals", "n_copies"):
            stats[k] = sum(getattr(tallies[i], k) for i in idx)
        inflate_every_way(q, hip, data, want, stats=stats, what=f"{n} blocks", shifts=(0, 15))
    bad = ds.CORRUPT_PAYLOADS[ij.DIST_PAST_START].block()
    data = b"".join(blocks[k % len(kinds)] for k in range(2 * pb + 3)) + bad + blocks[0] + bad
    with pytest.raises(pkg.AfqError) as e:
        q.bgzf_inflate(data)
    assert str(e.value).endswith("BGZF block %d: the deflate stream is corrupt or longer than ISIZE (a copy from in front of the block)" % (2 * pb + 3)), str(e.value)


def bam_like(n):
    """the inflated bytes of a BAM of tests/bam_cases.py's records, n of them"""
    recs = [B.rec("read%d" % (i // 3), ref=i % 7, flag=0x10 if i % 5 == 0 else 0, score=i % 11, cigar=[(90 << 4)], seq_len=90) for i in range(4000)]
    plain = B.plain_of(B.case("bam-like", recs))
    assert len(plain) >= n
    return plain[:n]


@pytest.mark.parametrize("strategy", ["default", "fixed", "huffman_only", "rle"])
def test_zlib_made_blocks(q, hip, strategy):
    """levels 0 / 1 / 6 / 9 at one strategy: blocks of 65280 bytes (what a BGZF writer cuts), and of 65536 where their payload fits a block"""
    st = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman_only": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE}[strategy]
    plain = bam_like(3 * 65536 + 777)
    for level in (0, 1, 6, 9):
        payloads = []
        for size in (65280, 65536):
            for a in range(0, len(plain), size):
                p = ds.zlib_payload(plain[a:a + size], level, st)
                if len(p.body) + 26 <= 65536:   # (65536 stored bytes and their headers do not fit a BGZF block)
                    payloads.append(p)
        assert len(payloads) >= 4 and (level == 0 or any(p.isize == 65536 for p in payloads))
        case = ds.Case(f"zlib level {level} {strategy}", payloads)
        inflate_every_way(q, hip, case.file, case.data, what=case.name, shifts=(0, 5) if level == 6 else (15,))
    # 65536 stored bytes and their header do not fit a BGZF block: 65400 stored bytes and a tail of copies do
    p = ds.P([("stored", plain[:65400]), ("fixed", [("copy", 136, 30000)])])
    assert p.isize == 65536 and len(p.body) + 26 <= 65536
    inflate_every_way(q, hip, p.block(), p.data, what="65536 bytes, 65400 of them stored", shifts=(1,))


def test_an_empty_file_and_an_eof_marker(q, hip):
    inflate_every_way(q, hip, b"", b"", what="empty file")
    inflate_every_way(q, hip, B.BGZF_EOF, b"", what="the EOF marker alone", shifts=(0, 15))
    inflate_every_way(q, hip, B.BGZF_EOF + ds.GOOD[0].block() + B.BGZF_EOF, ds.GOOD[0].data, what="EOF markers around a block", shifts=(5,))
