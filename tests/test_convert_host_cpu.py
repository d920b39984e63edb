"""CPU tests of the host half of `convert` and of `view` (no device is touched): every refusal of afq_convert that precedes device
work, the prelude bytes against rad.py's writer, `view` on a file rad.py wrote, and the ABI entries."""
import ctypes
import os
import struct
import subprocess

import pytest

import bam_cases as B
from util import ROOT, pkg

BAD_INPUT, UNSUPPORTED = pkg._abi.AFQ_ERR_BAD_INPUT, pkg._abi.AFQ_ERR_UNSUPPORTED
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")
rad = pkg.rad


def refused(tmp_path, name, data):
    p = str(tmp_path / name)
    if data is not None:
        with open(p, "wb") as f:
            f.write(data)
    with pytest.raises(pkg.AfqError) as e:
        pkg.convert(p, str(tmp_path / "out" / "map.rad"))
    assert not os.path.exists(str(tmp_path / "out" / "map.rad"))   # nothing is written before the device call succeeded
    return e.value


@pytest.fixture(scope="module")
def good():
    return B.container_cases()[0]   # three BGZF blocks: two of data, the EOF marker


def test_the_endings(tmp_path, good):
    bam = B.bam_bytes(good)
    for name in ("x.sam", "x.SAM"):
        e = refused(tmp_path, name, bam)
        assert e.code == UNSUPPORTED and "SAM text" in str(e) and "only BAM is read" in str(e)
    for name in ("x.bam.gz", "x.cram", "bam", "x.Bam"):
        e = refused(tmp_path, name, bam)
        assert e.code == BAD_INPUT and str(e).endswith(": unsupported input file format, must end with bam/BAM or sam/SAM")
    e = refused(tmp_path, "missing.bam", None)
    assert e.code == BAD_INPUT and "could not open" in str(e)


def test_bgzf_corruption_names_the_block(tmp_path, good):
    bam = bytearray(B.bam_bytes(good))
    n0 = struct.unpack_from("<H", bam, 16)[0] + 1   # block 0's length
    n1 = struct.unpack_from("<H", bam, n0 + 16)[0] + 1
    cut = bytes(bam[:n0 + n1 - 5])
    e = refused(tmp_path, "cut.bam", cut)
    assert e.code == BAD_INPUT and "BGZF block 1:" in str(e) and "truncated" in str(e)
    e = refused(tmp_path, "cut_head.BAM", bytes(bam[:n0 + 7]))
    assert e.code == BAD_INPUT and "BGZF block 1:" in str(e) and "truncated" in str(e)
    crc = bytearray(bam)
    crc[n0 + n1 - 8] ^= 0x40
    e = refused(tmp_path, "crc.bam", bytes(crc))
    assert e.code == BAD_INPUT and "BGZF block 1:" in str(e) and "CRC32" in str(e)
    isz = bytearray(bam)
    isz[n0 + n1 - 4] ^= 0x01
    e = refused(tmp_path, "isize.bam", bytes(isz))
    assert e.code == BAD_INPUT and "BGZF block 1:" in str(e)
    magic = bytearray(bam)
    magic[n0 + 1] = 0x8c
    e = refused(tmp_path, "magic.bam", bytes(magic))
    assert e.code == BAD_INPUT and "BGZF block 1:" in str(e) and "gzip magic" in str(e)
    body = bytearray(bam)
    body[n0 + 30] ^= 0xFF   # inside block 1's deflate stream
    e = refused(tmp_path, "body.bam", bytes(body))
    assert e.code == BAD_INPUT and "BGZF block 1:" in str(e)


def test_header_corruption(tmp_path):
    def bam_of(plain):
        return B.bgzf_block(plain) + B.BGZF_EOF
    h = B.header_bytes(B.REFS)
    e = refused(tmp_path, "m.bam", bam_of(b"BAN\1" + h[4:]))
    assert e.code == BAD_INPUT and "BAM header" in str(e) and "magic" in str(e)
    e = refused(tmp_path, "t.bam", bam_of(h[:4] + struct.pack("<i", 1 << 20) + h[8:]))
    assert e.code == BAD_INPUT and "BAM header" in str(e)
    e = refused(tmp_path, "r.bam", bam_of(h[:-9]))
    assert e.code == BAD_INPUT and "BAM header: reference 6" in str(e)
    e = refused(tmp_path, "e.bam", b"")
    assert e.code == BAD_INPUT and "BAM header" in str(e)


def test_no_records_and_the_first_records_tags(tmp_path):
    def bam_of(records, tail=b""):
        c = B.case("x", records)
        return B.bgzf_block(B.plain_of(c) + tail) + B.BGZF_EOF
    e = refused(tmp_path, "none.bam", bam_of([]))
    assert e.code == BAD_INPUT and "bam file had no records!" in str(e)
    for name, first, words in (("nocr", B.rec("a", cr=None), "missing CR tag"), ("nour", B.rec("a", ur=None), "missing UR tag"),
                               ("crtype", dict(name="a", aux=[("CR", "i", 4), ("UR", "Z", "ACGT")]), "non-string (Z) tag into barcode"),
                               ("urtype", dict(name="a", aux=[("CR", "Z", "ACGT"), ("UR", "H", "AC")]), "non-string (Z) tag into umi"),
                               ("cr0", B.rec("a", cr=""), "barcode of length 0"), ("cr33", B.rec("a", cr="A" * 33), "barcode of length 33"),
                               ("ur0", B.rec("a", ur=""), "umi of length 0"), ("ur33", B.rec("a", ur="C" * 33), "umi of length 33")):
        e = refused(tmp_path, name + ".bam", bam_of([first, B.rec("b")]))
        assert e.code == BAD_INPUT and "record 0:" in str(e) and words in str(e), (name, str(e))
    e = refused(tmp_path, "past.bam", bam_of([B.rec("a"), dict(B.rec("b"), block_size=5000)]))
    assert e.code == BAD_INPUT and "record 1:" in str(e) and "past the stream" in str(e)
    e = refused(tmp_path, "tail.bam", bam_of([B.rec("a"), B.rec("b")], tail=b"\x01"))
    assert e.code == BAD_INPUT and "record 2:" in str(e)


def test_the_prelude_equals_rad_pys():
    for names in (["t0"], B.REFS, ["a" * 300, "", "chr1"]):
        for cblen, ulen in ((1, 32), (4, 17), (5, 16), (8, 9), (9, 8), (16, 12), (17, 4), (32, 1)):
            for nc in (0, 3, 1 << 40):
                got = pkg.convert_prelude(names, nc, cblen, ulen)
                assert got == rad.rad_prelude(names, nc, cblen, ulen, rad.width_for_len(cblen), rad.width_for_len(ulen)), (names, cblen, ulen)
    with pytest.raises(pkg.AfqError):
        pkg.convert_prelude(["t"], 0, 0, 4)
    with pytest.raises(pkg.AfqError):
        pkg.convert_prelude(["t"], 0, 4, 33)


def view_lines(ref_names, chunks, cblen, ulen, header):
    out = ["%d:%s" % (i, n) for i, n in enumerate(ref_names)] if header else []
    rid = 0
    for ch in chunks:
        for bc, umi, alns in ch:
            for i, (ref, fw) in enumerate(alns):
                out.append("ID:%d\tHI:%d\tNH:%d\tCB:%s\tUMI:%s\tDIR:%s\t%s" % (rid, i + 1, len(alns), rad.int_to_seq(bc, cblen), rad.int_to_seq(umi, ulen), "true" if fw else "false", ref_names[ref]))
            rid += 1
    return "".join(line + "\n" for line in out)


def test_view_on_a_file_rad_py_wrote(tmp_path):
    chunks = [[(27, 5, [(0, True), (2, False)]), (0, 0, []), (255, 63, [(1, False)])], [], [(1, 2, [(2, True)] * 3)]]
    for bw, uw, cblen, ulen in ((1, 1, 4, 3), (2, 4, 8, 16), (8, 2, 32, 5)):
        body, _ = rad.encode_chunks(chunks, bc_bytes=bw, umi_bytes=uw)
        p = str(tmp_path / f"v{bw}{uw}.rad")
        with open(p, "wb") as f:
            f.write(rad.rad_prelude(["t0", "t1", "chr2"], len(chunks), cblen, ulen, bw, uw) + bytes(body))
        for header in (False, True):
            assert pkg.view(p, header=header) == view_lines(["t0", "t1", "chr2"], chunks, cblen, ulen, header)
        r = subprocess.run([CLI, "view", "-r", p, "-H"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == view_lines(["t0", "t1", "chr2"], chunks, cblen, ulen, True), r.stderr


def test_view_refuses_what_the_reference_refuses(tmp_path):
    def tag(name, t):
        return struct.pack("<H", len(name)) + name.encode() + bytes([t])
    head = bytes([0]) + struct.pack("<Q", 1) + struct.pack("<H", 2) + b"t0" + struct.pack("<Q", 0)
    files = {"float_b": head + struct.pack("<H", 2) + tag("cblen", 2) + tag("ulen", 2) + struct.pack("<H", 2) + tag("b", 5) + tag("u", 3) + struct.pack("<H", 1) + tag("compressed_ori_refid", 3) + struct.pack("<HH", 4, 4),
             "no_u": head + struct.pack("<H", 2) + tag("cblen", 2) + tag("ulen", 2) + struct.pack("<H", 1) + tag("b", 3) + struct.pack("<H", 1) + tag("compressed_ori_refid", 3) + struct.pack("<HH", 4, 4),
             "no_ulen": head + struct.pack("<H", 1) + tag("cblen", 2) + struct.pack("<H", 2) + tag("b", 3) + tag("u", 3) + struct.pack("<H", 1) + tag("compressed_ori_refid", 3) + struct.pack("<H", 4)}
    want = {"float_b": (UNSUPPORTED, "only RAD types 1--4 are supported for 'b' and 'u' tags"), "no_u": (BAD_INPUT, "umi type tag was missing!"), "no_ulen": (BAD_INPUT, "tag map must contain ulen")}
    for name, data in files.items():
        p = str(tmp_path / (name + ".rad"))
        with open(p, "wb") as f:
            f.write(data)
        with pytest.raises(pkg.AfqError) as e:
            pkg.view(p)
        assert (e.value.code, True) == (want[name][0], want[name][1] in str(e.value)), (name, str(e.value))


def test_the_abi_entries():
    for name in ("afq_convert_bam_rad", "afq_convert_limits"):
        assert name in pkg._abi.EXPORTS
    lib = pkg.load_library()
    for name in ("afq_convert_bam_rad", "afq_convert_limits", "afq_convert", "afq_convert_prelude_bytes", "afq_view_file"):
        assert hasattr(lib, name)
    assert ctypes.sizeof(pkg._abi.AfqConvertStats) == 80 and ctypes.sizeof(pkg._abi.AfqConvertOpts) == 40
    lim = pkg.convert_limits()
    assert lim["parse_halo"] >= 36 and lim["lane_alns"] >= 1 and lim["parse_tile"] % 4 == 0 and lim["scan_block"] < B.CHUNK_RUNS
    assert pkg.Quantifier.convert_limits() == lim


def test_the_cli_words(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "afquant convert -b" in r.stderr and "afquant view -r" in r.stderr
    r = subprocess.run([CLI, "convert", "-o", str(tmp_path / "o.rad")], capture_output=True, text=True)
    assert r.returncode == 2 and "--bam <BAM>" in r.stderr
    r = subprocess.run([CLI, "convert", "-b", str(tmp_path / "x.sam"), "-o", str(tmp_path / "o.rad"), "-f", "-t", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "SAM text" in r.stderr
    r = subprocess.run([CLI, "view"], capture_output=True, text=True)
    assert r.returncode == 2 and "--rad <RAD>" in r.stderr
