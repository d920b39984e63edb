"""GPU tests of `convert --inflate-on-device` (afq_convert_with, AFQ_CONVERT_INFLATE_ON_DEVICE): the BGZF blocks are inflated on
the device and the record kernels run on the resident stream.  Every valid case of tests/bam_cases.py - the container cases
among them: a record, a block_size field and the BAM header split across blocks, an empty block mid-file, no EOF marker, a
stored block - and headers of every length modulo 16, one of them ending on a block's edge: the RAD file and the stats are the
closed door's, byte for byte, through the Python entry and through the CLI flag.  The BGZF refusals name the block the closed
door names, with its words where they are not zlib's, and no output file is left behind."""
import os
import struct
import subprocess

import pytest

import bam_cases as B
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")


def run(*args, env=None):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, **(env or {})))


def cases():
    return [(c, fb) for c in B.all_cases(pkg.convert_limits()) for fb in c["filters"][-1:]]


N_CASES = 32


def both_doors(tmp_path, c, fb, cli=True, env=None):
    """the closed door's file and stats; the open door's through Python, and through the CLI where asked, are the same"""
    bam = str(tmp_path / "in.bam")
    with open(bam, "wb") as f:
        f.write(B.bam_bytes(c))
    closed, opened, by_cli = str(tmp_path / "closed.rad"), str(tmp_path / "open.rad"), str(tmp_path / "cli" / "open.rad")
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        st0 = pkg.convert(bam, closed, filter_best=fb, num_threads=2)
        st1 = pkg.convert(bam, opened, filter_best=fb, num_threads=2, inflate_on_device=True)
    finally:
        for k in env or {}:
            del os.environ[k]
    want = open(closed, "rb").read()
    assert st1 == st0 and open(opened, "rb").read() == want, c["name"]
    if cli:
        r = run("convert", "-b", bam, "-o", by_cli, "-t", 2, "--inflate-on-device", *(["-f"] if fb else []), env=env)
        assert r.returncode == 0, r.stderr
        assert open(by_cli, "rb").read() == want, c["name"]
        assert "parsing BAM file with the BGZF blocks inflated on the device" in r.stderr and "decompression threads" not in r.stderr
    return bam, want


@pytest.mark.parametrize("i", range(N_CASES))
def test_every_valid_case_through_both_doors(tmp_path, i):
    all_of_them = cases()
    assert len(all_of_them) == N_CASES and [c["name"] for c, _ in all_of_them[-6:]] == ["record_split", "block_size_split", "header_split", "empty_block", "no_eof", "stored_block"]
    c, fb = all_of_them[i]
    # spans of one tile, so that the host's cuts fall where the case's records stand
    both_doors(tmp_path, c, fb, env={"AFQ_TEST_CONVERT_SPAN_BYTES": str(pkg.convert_limits()["parse_tile"])})


def test_the_stderr_lines_are_the_closed_doors_but_for_the_inflate_line(tmp_path):
    c = B.container_cases()[5]
    bam = str(tmp_path / "in.bam")
    with open(bam, "wb") as f:
        f.write(B.bam_bytes(c))
    a = run("convert", "-b", bam, "-o", tmp_path / "a.rad", "-t", 3)
    b = run("convert", "-b", bam, "-o", tmp_path / "b.rad", "-t", 3, "--inflate-on-device")
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    la, lb = a.stderr.splitlines(), b.stderr.splitlines()
    assert len(la) == len(lb) and la[1] == "parsing BAM file using 2 decompression threads" and lb[1] == "parsing BAM file with the BGZF blocks inflated on the device"
    assert la[:1] + la[2:] == lb[:1] + lb[2:]
    assert open(tmp_path / "a.rad", "rb").read() == open(tmp_path / "b.rad", "rb").read()


def test_every_header_length_modulo_16_and_a_header_that_ends_on_a_block_s_edge(tmp_path):
    recs = [B.rec("q%d" % (i // 2), ref=i % 3, score=i % 3) for i in range(40)]
    seen = set()
    for k in range(16):
        c = B.case("h%d" % k, recs, ref_names=["a", "b", "c" * (1 + k)])
        h = B.header_len(c)
        seen.add(h % 16)
        both_doors(tmp_path, dict(c, cuts=[h]) if k % 4 == 0 else c, False, cli=False)
    assert seen == set(range(16))
    # a header of several blocks: the host inflates one leading block, then two, then four
    c = B.case("long header", recs, ref_names=["ref_%d_%s" % (i, "x" * (i % 50)) for i in range(4000)])
    assert B.header_len(c) > 2 * 60000
    both_doors(tmp_path, c, False, cli=False)


def test_the_bgzf_refusals_name_the_closed_door_s_block(tmp_path):
    bam = bytearray(B.bam_bytes(B.container_cases()[0]))   # three BGZF blocks: two of data, the EOF marker
    n0 = struct.unpack_from("<H", bam, 16)[0] + 1
    n1 = struct.unpack_from("<H", bam, n0 + 16)[0] + 1
    crc, isz, magic, body, first = bytearray(bam), bytearray(bam), bytearray(bam), bytearray(bam), bytearray(bam)
    crc[n0 + n1 - 8] ^= 0x40
    isz[n0 + n1 - 4] ^= 0x01
    magic[n0 + 1] = 0x8c
    body[n0 + 30] ^= 0xFF     # inside block 1's deflate stream
    first[n0 - 8] ^= 0x01     # block 0's CRC: the host inflates that block for the header
    out = str(tmp_path / "out" / "map.rad")
    for name, data, same_words in [("crc", crc, True), ("isize", isz, None), ("cut", bam[:n0 + n1 - 5], True), ("magic", magic, True), ("body", body, False), ("first", first, True)]:
        p = str(tmp_path / (name + ".bam"))
        with open(p, "wb") as f:
            f.write(bytes(data))
        said = []
        for on_device in (False, True):
            with pytest.raises(pkg.AfqError) as e:
                pkg.convert(p, out, inflate_on_device=on_device)
            assert e.value.code == pkg._abi.AFQ_ERR_BAD_INPUT and not os.path.exists(out), (name, on_device)
            said.append(str(e.value))
        block = "BGZF block %d: " % (0 if name == "first" else 1)
        assert block in said[0] and block in said[1], (name, said)
        if same_words:
            assert said[0] == said[1], (name, said)
        elif same_words is None:   # ISIZE one off: the closed door's own words where the stream is short, zlib's where it is long
            assert said[0] == said[1] or "the deflate stream is corrupt or longer than ISIZE (more bytes than ISIZE)" in said[1], (name, said)
        else:
            assert "the deflate stream is corrupt or longer than ISIZE (" in said[1], (name, said)
        r = run("convert", "-b", p, "-o", out, "--inflate-on-device")
        assert r.returncode == 1 and block in r.stderr and not os.path.exists(out), (name, r.stderr)
    # the context of a refused convert is gone with it; the next convert is served
    both_doors(tmp_path, B.container_cases()[0], False, cli=False)
