"""CPU tests of what `convert --inflate-on-device` and afq_bgzf_inflate_device decide before any device work: the flag word of
afq_convert_with, the options' size, the plan's refusals - the closed door's sentences, word for word, through the open door -
the limits, and the CLI's words."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import bam_cases as B
from util import ROOT, pkg

INVALID_ARG, BAD_INPUT, UNSUPPORTED = pkg._abi.AFQ_ERR_INVALID_ARG, pkg._abi.AFQ_ERR_BAD_INPUT, pkg._abi.AFQ_ERR_UNSUPPORTED
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")


def opts(bam, out):
    o = pkg._abi.AfqConvertOpts()
    o.bam, o.rad_out, o.num_threads = os.fsencode(bam), os.fsencode(out), 2
    return o


def test_unknown_flag_bits_are_refused_and_the_options_keep_their_size(tmp_path):
    lib = pkg.load_library()
    assert C.sizeof(pkg._abi.AfqConvertOpts) == 40 and pkg._abi.AFQ_CONVERT_INFLATE_ON_DEVICE == 1
    o = opts(str(tmp_path / "missing.bam"), str(tmp_path / "o.rad"))
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        assert lib.afq_convert_with(C.byref(o), flags) == INVALID_ARG and b"unknown flag bits" in lib.afq_host_last_error()
    for flags in (0, 1):   # the known ones reach the file
        assert lib.afq_convert_with(C.byref(o), flags) == BAD_INPUT and b"could not open" in lib.afq_host_last_error()
        assert lib.afq_convert_with(None, flags) == INVALID_ARG
    assert lib.afq_convert(C.byref(o)) == BAD_INPUT and b"could not open" in lib.afq_host_last_error()


def both_doors(tmp_path, name, data):
    """the refusal of the closed door and of the open one"""
    p, out = str(tmp_path / name), str(tmp_path / "out" / "map.rad")
    with open(p, "wb") as f:
        f.write(data)
    got = []
    for on_device in (False, True):
        with pytest.raises(pkg.AfqError) as e:
            pkg.convert(p, out, inflate_on_device=on_device)
        assert not os.path.exists(out)
        got.append((e.value.code, str(e.value)))
    return got


def test_plan_refusals_are_the_closed_doors(tmp_path):
    bam = bytearray(B.bam_bytes(B.container_cases()[0]))
    n0 = struct.unpack_from("<H", bam, 16)[0] + 1   # block 0's length
    n1 = struct.unpack_from("<H", bam, n0 + 16)[0] + 1
    magic, no_bc, small, big = bytearray(bam), bytearray(bam), bytearray(bam), bytearray(bam)
    magic[n0 + 1] = 0x8c
    no_bc[n0 + 12] = ord("X")
    struct.pack_into("<H", small, n0 + 16, 20)
    struct.pack_into("<I", big, n0 + n1 - 4, 65537)
    for name, data, words in [("cut.bam", bam[:n0 + n1 - 5], "truncated: the block has"), ("cut_head.BAM", bam[:n0 + 7], "bytes where a block header has 18"),
                              ("magic.bam", magic, "bad gzip magic"), ("no_bc.bam", no_bc, "no BC extra field: not a BGZF block"),
                              ("small.bam", small, "BSIZE is smaller than the block's own header and trailer"), ("big.bam", big, "ISIZE 65537 is above the 65536 bytes of a BGZF block")]:
        closed, opened = both_doors(tmp_path, name, bytes(data))
        assert closed == opened and closed[0] == BAD_INPUT and "BGZF block 1: " in closed[1] and words in closed[1], (name, closed, opened)
    for name in ("x.sam", "x.cram"):
        closed, opened = both_doors(tmp_path, name, bytes(bam))
        assert closed == opened and closed[0] in (UNSUPPORTED, BAD_INPUT)


def test_the_entry_points_without_a_context():
    lib = pkg.load_library()
    for name in ("afq_bgzf_inflate_device", "afq_inflate_limits"):
        assert name in pkg._abi.EXPORTS and hasattr(lib, name)
    assert hasattr(lib, "afq_convert_with") and C.sizeof(pkg._abi.AfqInflateStats) == 72
    o_b, o_n = C.POINTER(C.c_uint8)(), C.c_uint64()
    assert lib.afq_bgzf_inflate_device(None, B.BGZF_EOF, len(B.BGZF_EOF), 0, 0, C.byref(o_b), C.byref(o_n), None) == INVALID_ARG
    lim = pkg.inflate_limits()
    assert lim["threads"] % 64 == 0 and lim["piece_blocks"] >= 1 and lim["blocks_per_workgroup"] >= 1
    assert 65536 < lim["lds_bytes"] <= 160 * 1024
    lib.afq_inflate_limits(None)   # (a null array is ignored)


def test_the_cli_words(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "[--inflate-on-device]" in r.stderr and "afquant convert -b" in r.stderr
    r = subprocess.run([CLI, "convert", "--inflate-on-device", "-o", str(tmp_path / "o.rad")], capture_output=True, text=True)
    assert r.returncode == 2 and "--bam <BAM>" in r.stderr
    r = subprocess.run([CLI, "convert", "-b", str(tmp_path / "x.sam"), "-o", str(tmp_path / "o.rad"), "--inflate-on-device"], capture_output=True, text=True)
    assert r.returncode == 1 and "SAM text" in r.stderr
