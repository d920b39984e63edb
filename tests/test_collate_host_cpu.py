"""CPU tests of collate's host half (afq_collate, include/afquant_host.h, and `afquant collate`): every refusal with its return code
and sentence - all of them come before any device call, so they read the same with and without a GPU -, the
unmapped_bc_count_collated.bin writer, and afq_collate_limits against the GPL constants."""
import ctypes as C
import json
import os
import subprocess

import pytest

from util import ROOT, pkg

rad = pkg.rad
INVALID_ARG, BAD_INPUT, UNSUPPORTED = pkg._abi.AFQ_ERR_INVALID_ARG, pkg._abi.AFQ_ERR_BAD_INPUT, pkg._abi.AFQ_ERR_UNSUPPORTED
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")
L = 16


class CollateOpts(C.Structure):
    _fields_ = [("input_dir", C.c_char_p), ("rad_dir", C.c_char_p), ("num_threads", C.c_uint32), ("compress", C.c_uint32), ("max_records", C.c_uint32),
                ("device", C.c_uint32), ("cmdline", C.c_char_p), ("stats_out", C.POINTER(pkg._abi.AfqCollateStats))]


@pytest.fixture(scope="module")
def lib():
    l = pkg.load_library()
    l.afq_host_last_error.restype = C.c_char_p
    l.afq_collate.argtypes = [C.POINTER(CollateOpts)]
    l.afq_collate.restype = C.c_int
    return l


META = {"velo_mode": False, "expected_ori": "fw", "version_str": "0.18.0", "max-ambig-record": 3, "cmd": "x", "gpl_options": {"velo_mode": False, "expected_ori": "Forward"}}
FREQ = [(0x11, 3), (0x22, 5)]
PLAN = [(0x11, 0x11), (0x22, 0x22), (0x12, 0x11)]


def dirs(tmp_path, meta=META, freq=FREQ, freq_version=1, plan=PLAN, plan_len=L, atac=False, unmapped=None, n_chunks=1, num_chunks=None, cut=0):
    """a generate-permit-list output directory and a mapper directory; -> (input_dir, rad_dir).  map.rad holds n_chunks chunks of one
    record, less its last `cut` bytes; its prelude announces num_chunks of them (default: n_chunks)."""
    ind, rd = str(tmp_path / "gpl"), str(tmp_path / "map")
    os.makedirs(ind)
    os.makedirs(rd)
    with open(os.path.join(ind, "generate_permit_list.json"), "w") as f:
        json.dump(meta, f, indent=2)
    with open(os.path.join(ind, "permit_freq.bin"), "wb") as f:
        f.write(rad.permit_freq_bytes(L, freq, version=freq_version))
    with open(os.path.join(ind, "correction_plan.bin"), "wb") as f:
        f.write(rad.correction_plan_bytes(plan, barcode_len=plan_len))
    body, _ = rad.encode_chunks([[(0x11, 1, [(1, True)])]] * n_chunks)
    num_chunks = n_chunks if num_chunks is None else num_chunks
    prelude = rad.rad_prelude_atac(["chr1"], [1000], num_chunks) if atac else rad.rad_prelude(["t0", "t1"], num_chunks, L, 12, 4, 4)
    with open(os.path.join(rd, "map.rad"), "wb") as f:
        f.write((prelude + body)[:len(prelude) + len(body) - cut])
    if unmapped is not None:
        with open(os.path.join(rd, "unmapped_bc_count.bin"), "wb") as f:
            f.write(b"".join(int(b).to_bytes(8, "little") + int(n).to_bytes(4, "little") for b, n in unmapped))
    return ind, rd


def collate(lib, ind, rd, **kw):
    o = CollateOpts(input_dir=ind.encode() if ind else None, rad_dir=rd.encode() if rd else None, cmdline=b"afquant collate", **kw)
    rc = lib.afq_collate(C.byref(o))
    return rc, (lib.afq_host_last_error() or b"").decode()


def cli(*args):
    return subprocess.run([CLI, "collate"] + [str(a) for a in args], capture_output=True, text=True)


def refused(lib, ind, rd, code, sentence, cli_args=()):
    """the library call and the sub-command refuse alike, and no RAD is written"""
    rc, msg = collate(lib, ind, rd)
    assert rc == code and sentence in msg, (rc, msg)
    r = cli("-i", ind, "-r", rd, *cli_args)
    assert r.returncode == 1 and sentence in r.stderr and f"({code})" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(os.path.join(ind, "map.collated.rad")) and not os.path.exists(os.path.join(ind, "collate.json"))


def test_missing_rad_dir(lib, tmp_path):
    ind, rd = dirs(tmp_path)
    rc, msg = collate(lib, ind, None)
    assert rc == INVALID_ARG and "-r" in msg
    r = cli("-i", ind)
    assert r.returncode == 2 and "--rad-dir <RADDIR>" in r.stderr
    r = cli("-r", rd)
    assert r.returncode == 2 and "--input-dir <INPUTDIR>" in r.stderr
    r = cli("-i", ind, "-r", rd + "_nowhere")
    assert r.returncode == 2 and "--rad-dir <RADDIR>" in r.stderr and "does not exist" in r.stderr
    r = cli("-i", ind + "_nowhere", "-r", rd)
    assert r.returncode == 2 and "--input-dir <INPUTDIR>" in r.stderr and "does not exist" in r.stderr


def test_compress_is_refused(lib, tmp_path):
    ind, rd = dirs(tmp_path)
    rc, msg = collate(lib, ind, rd, compress=1)
    assert rc == UNSUPPORTED and "compressed output is not supported" in msg
    for flag in ("-c", "--compress"):
        r = cli("-i", ind, "-r", rd, flag, "-t", 4, "-m", 1000, "--memory-limit", "1GiB", "--collation-mode", "optimized")
        assert r.returncode == 1 and "compressed output is not supported" in r.stderr and f"({UNSUPPORTED})" in r.stderr
    assert not os.path.exists(os.path.join(ind, "map.collated.rad"))


def test_metadata_refusals(lib, tmp_path):
    refused(lib, *dirs(tmp_path / "a", meta=dict(META, multi_barcode=True)), UNSUPPORTED, "multi_barcode")
    refused(lib, *dirs(tmp_path / "b", meta=dict(META, velo_mode=True)), UNSUPPORTED, "velo_mode")
    no_version = {k: v for k, v in META.items() if k != "version_str"}
    refused(lib, *dirs(tmp_path / "c", meta=no_version), BAD_INPUT,
            "The generate_permit_list.json file does not contain a version_str field. Please re-run the generate-permit-list step with a newer version of alevin-fry")
    refused(lib, *dirs(tmp_path / "d", meta=dict(META, expected_ori="sideways")), BAD_INPUT, "could not read strand")


def test_permit_list_refusals(lib, tmp_path):
    refused(lib, *dirs(tmp_path / "a", freq_version=2), BAD_INPUT, "The permit_freq.bin file had version 2, but this version of alevin-fry requires version 1")
    refused(lib, *dirs(tmp_path / "b", freq=[]), BAD_INPUT, "single-barcode permit list contains no output cells")
    refused(lib, *dirs(tmp_path / "c", plan_len=L - 1), BAD_INPUT, "correction plan does not match this input")
    ind, rd = dirs(tmp_path / "d")
    with open(os.path.join(ind, "correction_plan.bin"), "ab") as f:
        f.write(b"\x00")   # a present but malformed plan is an error, not a reason to fall back on the legacy map
    with open(os.path.join(ind, "permit_map.bin"), "wb") as f:
        f.write(rad.permit_map_bytes(PLAN))
    refused(lib, ind, rd, BAD_INPUT, "correction plan contains trailing data")


def test_a_truncated_chunk_table(lib, tmp_path):
    """the prelude promises three chunks and the file holds two; the last chunk's nbytes runs past the file's end"""
    refused(lib, *dirs(tmp_path / "a", n_chunks=2, num_chunks=3), BAD_INPUT, "map.rad ends before chunk 2 of 3")
    refused(lib, *dirs(tmp_path / "b", n_chunks=2, cut=4), BAD_INPUT, "corrupt chunk header (chunk 1)")


def test_atac_prelude_is_refused_by_name_after_the_unmapped_counts_were_written(lib, tmp_path):
    """the unmapped counts of observed barcodes are summed onto their corrected barcodes; a barcode outside the map is dropped; a
    trailing partial pair is ignored.  The directory carries an ATAC map.rad, so the call stops at the prelude on any machine."""
    unmapped = [(0x11, 4), (0x12, 6), (0x22, 1), (0x99, 50), (0x11, 2)]
    ind, rd = dirs(tmp_path, atac=True, unmapped=unmapped)
    with open(os.path.join(rd, "unmapped_bc_count.bin"), "ab") as f:
        f.write(b"\x01\x02\x03")
    refused(lib, ind, rd, UNSUPPORTED, "scATAC")
    corr, want = dict(PLAN), {}
    for b, n in unmapped:
        if b in corr:
            want[corr[b]] = want.get(corr[b], 0) + n
    assert want == {0x11: 12, 0x22: 1}
    buf = open(os.path.join(ind, "unmapped_bc_count_collated.bin"), "rb").read()
    n = int.from_bytes(buf[:8], "little")
    assert len(buf) == 8 + 12 * n
    got = {int.from_bytes(buf[8 + 12 * i:16 + 12 * i], "little"): int.from_bytes(buf[16 + 12 * i:20 + 12 * i], "little") for i in range(n)}
    assert got == want


def test_a_missing_unmapped_file_is_an_empty_map(lib, tmp_path):
    ind, rd = dirs(tmp_path, atac=True)
    refused(lib, ind, rd, UNSUPPORTED, "scATAC")
    assert open(os.path.join(ind, "unmapped_bc_count_collated.bin"), "rb").read() == bytes(8)


def test_limits_are_the_gpl_walks_and_a_whole_number_of_waves():
    c, g = pkg.collate_limits(), pkg.gpl_limits()
    assert (c["parse_tile"], c["parse_halo"], c["lane_alns"]) == (g["parse_tile"], g["parse_halo"], g["lane_alns"])
    assert c["parse_halo"] >= 20 + 12 * c["lane_alns"]   # the widest head and lane_alns of the widest alignments
    assert c["radix_block"] > 0 and c["radix_block"] % 256 == 0
    assert pkg.Quantifier.collate_limits() == c


def test_usage_names_the_sub_command():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "afquant collate -i <input-dir> -r <rad-dir>" in r.stderr and "one device fill" in r.stderr
