"""GPU end-to-end tests of `afquant convert` and `afquant view` in fresh child processes, and of the Python `convert`: the file
written is the prelude of rad.py's writer (num_chunks patched) + the bytes of tests/convert_judge.py's `stated`; `view -H` on it
equals a Python restatement of the reference's lines; and a read set written once as a BAM and converted, once directly as a
mapper RAD, gives identical matrices through generate-permit-list -> collate -> quant."""
import ctypes as C
import os
import random
import subprocess

import pytest

import bam_cases as B
import convert_judge as J
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")


class RadInfo(C.Structure):
    _fields_ = [("ref_count", C.c_uint64), ("num_chunks", C.c_uint64), ("first_chunk_off", C.c_uint64), ("is_paired", C.c_uint32), ("cblen", C.c_uint32),
                ("ulen", C.c_uint32), ("bc_bytes", C.c_uint32), ("umi_bytes", C.c_uint32)]


def run(*args, env=None):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, **(env or {})))


def first_lengths(c):
    return len(J.tag(c["records"][0], "CR", 0)), len(J.tag(c["records"][0], "UR", 0))


def view_lines(ref_names, want, bw, uw, cblen, ulen, header):
    """convert.rs:659-706 over the judge's chunks"""
    out = ["%d:%s" % (i, n) for i, n in enumerate(ref_names)] if header else []
    rid, b = 0, want["bytes"]
    for k, n in enumerate(want["nrec"]):
        p = want["chunk_off"][k] + 8
        for _ in range(n):
            na = int.from_bytes(b[p:p + 4], "little")
            bc, umi = int.from_bytes(b[p + 4:p + 4 + bw], "little"), int.from_bytes(b[p + 4 + bw:p + 4 + bw + uw], "little")
            p += 4 + bw + uw
            for i in range(na):
                w = int.from_bytes(b[p:p + 4], "little")
                out.append("ID:%d\tHI:%d\tNH:%d\tCB:%s\tUMI:%s\tDIR:%s\t%s" % (rid, i + 1, na, rad.int_to_seq(bc, cblen), rad.int_to_seq(umi, ulen), "true" if w >> 31 else "false",
                                                                              ref_names[w & 0x7FFFFFFF]))
                p += 4
            rid += 1
    return "".join(line + "\n" for line in out)


def cases():
    lim = pkg.convert_limits()
    flags = B.flag_cases()[0]   # the first record is unmapped and sets the lengths 5 and 3
    out = [(B.tile_edge_cases(lim)[1], True), (B.run_length_cases(lim)[0], True), (B.name_cases()[0], False), (flags, False), (B.flag_cases()[1], False),
           (B.chunk_cases()[2], False)]
    # every container case: a record and a block_size field split across two BGZF blocks, the BAM header split, an empty block
    # mid-file, no EOF marker, a stored deflate block - only a reader of the file sees these, so each goes through afq_convert
    con = B.container_cases()
    assert [c["name"] for c in con] == ["record_split", "block_size_split", "header_split", "empty_block", "no_eof", "stored_block"]
    return out + [(c, k % 2 == 0) for k, c in enumerate(con)]


@pytest.mark.parametrize("i", range(12))
def test_the_cli_and_python_write_the_judges_file(tmp_path, i):
    all_of_them = cases()
    assert len(all_of_them) == 12
    c, fb = all_of_them[i]
    bam = str(tmp_path / "in.bam")
    with open(bam, "wb") as f:
        f.write(B.bam_bytes(c))
    cblen, ulen = first_lengths(c)
    bw, uw = J.width_for(cblen), J.width_for(ulen)
    want = J.stated(c["records"], fb, n_ref=len(c["ref_names"]), lane_alns=pkg.convert_limits()["lane_alns"])
    whole = rad.rad_prelude(c["ref_names"], len(want["nrec"]), cblen, ulen, bw, uw) + want["bytes"]
    out_cli, out_py = str(tmp_path / "new" / "dir" / "map.rad"), str(tmp_path / "py.rad")
    with open(out_py, "wb") as f:
        f.write(b"an existing file is replaced" * 1000)
    # the span table is the host's here: spans of one tile, so that its cuts fall where the case's records stand
    r = run("convert", "-b", bam, "-o", out_cli, "-t", 3, *(["-f"] if fb else []), env={"AFQ_TEST_CONVERT_SPAN_BYTES": str(pkg.convert_limits()["parse_tile"])})
    assert r.returncode == 0, r.stderr
    assert f"Bam file size in bytes {os.path.getsize(bam)}" in r.stderr and f"ref count: {len(c['ref_names'])}" in r.stderr and f"{len(want['nrec'])} chunks written" in r.stderr
    st = pkg.convert(bam, out_py, filter_best=fb, num_threads=1)
    assert st == want["stats"]
    got = open(out_cli, "rb").read()
    assert got == open(out_py, "rb").read()
    assert got == whole
    lib = pkg.load_library()
    lib.afq_rad_parse_prelude.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(RadInfo)]
    lib.afq_rad_parse_prelude.restype = C.c_int
    info = RadInfo()
    assert lib.afq_rad_parse_prelude(got, len(got), C.byref(info)) == 0
    assert (info.ref_count, info.num_chunks, info.cblen, info.ulen, info.bc_bytes, info.umi_bytes, info.is_paired) == (len(c["ref_names"]), len(want["nrec"]), cblen, ulen, bw, uw, 0)
    assert info.first_chunk_off == len(got) - len(want["bytes"])
    if len(want["bytes"]) < 1 << 16:
        r = run("view", "-r", out_cli, "-H")
        assert r.returncode == 0 and r.stdout == view_lines(c["ref_names"], want, bw, uw, cblen, ulen, True), r.stderr
        assert pkg.view(out_py) == view_lines(c["ref_names"], want, bw, uw, cblen, ulen, False)


def test_a_failed_convert_leaves_no_file(tmp_path):
    c = B.error_cases()[6][0]   # a base outside ACGTN
    bam, out = str(tmp_path / "in.bam"), str(tmp_path / "map.rad")
    with open(bam, "wb") as f:
        f.write(B.bam_bytes(c))
    r = run("convert", "-b", bam, "-o", out)
    assert r.returncode == 1 and "record 2:" in r.stderr and "nucleotide" in r.stderr and not os.path.exists(out), r.stderr


# ---------------------------------------------------------------------------------------------------------------- the chain
L, UL = 16, 12
REFS = ["t%d" % i for i in range(60)]
T2G = [(r, "g%d" % (i // 3)) for i, r in enumerate(REFS)]


def read_set(seed=5, n_cells=40):
    rng = random.Random(seed)
    cells = sorted({rng.randrange(1 << (2 * L)) for _ in range(n_cells)})
    reads = []
    for c in cells:
        for _ in range(rng.randrange(30, 60)):
            b = c ^ (1 << (2 * rng.randrange(L))) if rng.random() < 0.1 else c
            n = rng.choice([1, 1, 1, 2, 4, 20])
            reads.append((b, rng.randrange(1 << (2 * UL)), [(rng.randrange(len(REFS)), rng.random() < 0.85) for _ in range(n)]))
    for _ in range(150):
        reads.append((rng.randrange(1 << (2 * L)), rng.randrange(1 << (2 * UL)), [(rng.randrange(len(REFS)), True)]))
    rng.shuffle(reads)
    return reads


def pipeline(tmp_path, tag, map_rad):
    rd, out, q = str(tmp_path / (tag + "_map")), str(tmp_path / (tag + "_gpl")), str(tmp_path / (tag + "_quant"))
    os.makedirs(rd)
    os.replace(map_rad, os.path.join(rd, "map.rad"))
    with open(os.path.join(rd, "unmapped_bc_count.bin"), "wb") as f:
        f.write((5).to_bytes(8, "little") + (3).to_bytes(4, "little"))
    tg = os.path.join(rd, "t2g.tsv")
    with open(tg, "w") as f:
        f.write("".join("\t".join(row) + "\n" for row in T2G))
    for args in (("generate-permit-list", "-i", rd, "-d", "fw", "-o", out, "-k"), ("collate", "-i", out, "-r", rd), ("quant", "-i", out, "-m", tg, "-o", q, "-r", "cr-like", "-t", 2)):
        r = run(*args)
        assert r.returncode == 0, (args[0], r.stderr)
    files = [open(os.path.join(q, *p), "rb").read() for p in (("alevin", "quants_mat.mtx"), ("alevin", "quants_mat_rows.txt"), ("alevin", "quants_mat_cols.txt"), ("featureDump.txt",))]
    return files + [open(os.path.join(out, "map.collated.rad"), "rb").read()]


def test_a_bam_and_a_mapper_rad_of_one_read_set_quantify_alike(tmp_path):
    reads = read_set()
    recs = [B.rec("read%d" % i, ref=ref, flag=0 if fw else 0x10, cr=rad.int_to_seq(b, L), ur=rad.int_to_seq(u, UL)) for i, (b, u, alns) in enumerate(reads) for ref, fw in alns]
    c = B.case("chain", recs, ref_names=REFS, cuts=[70000, 70001])
    bam = str(tmp_path / "reads.bam")
    with open(bam, "wb") as f:
        f.write(B.bam_bytes(c))
    converted, direct = str(tmp_path / "converted.rad"), str(tmp_path / "direct.rad")
    r = run("convert", "-b", bam, "-o", converted)
    assert r.returncode == 0, r.stderr
    body, _ = rad.encode_chunks([reads[:700], reads[700:]], 4, 4)
    with open(direct, "wb") as f:
        f.write(rad.rad_prelude(REFS, 2, L, UL, 4, 4) + body)
    a, b = pipeline(tmp_path, "bam", converted), pipeline(tmp_path, "rad", direct)
    assert a == b
    assert len(a[1].split()) >= 25 and len(a[0]) > 1000   # cells and a matrix worth comparing
