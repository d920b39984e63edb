"""CPU tests of `atac collate`'s host half (afq_atac_collate, include/afquant_host.h, and `afquant atac collate`): every refusal with
its return code and sentence, through the library call and through the sub-command - all of them come before any device call, so
they read the same with and without a GPU -, and after each of them no map.collated.rad exists."""
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


class AtacCollateOpts(C.Structure):
    _fields_ = [("input_dir", C.c_char_p), ("rad_dir", C.c_char_p), ("num_threads", C.c_uint32), ("compress", C.c_uint32), ("max_records", C.c_uint32),
                ("device", C.c_uint32), ("cmdline", C.c_char_p), ("stats_out", C.POINTER(pkg._abi.AfqAtacCollateStats))]


@pytest.fixture(scope="module")
def lib():
    l = pkg.load_library()
    l.afq_host_last_error.restype = C.c_char_p
    l.afq_atac_collate.argtypes = [C.POINTER(AtacCollateOpts)]
    l.afq_atac_collate.restype = C.c_int
    return l


META = {"version_str": "0.18.0", "gpl_options": {"rc": True, "num-chunks": 7, "version_str": "x"}, "num-chunks": 1, "cmd": "x"}
FREQ = [(0x11, 3), (0x22, 5)]
PLAN = [(0x11, 0x11), (0x22, 0x22), (0x12, 0x11)]
A1 = (0, 4, 10, 50)


def dirs(tmp_path, meta=META, freq=FREQ, freq_version=1, plan=None, rna=False, chunks=None, unmapped=None, cut=0):
    """an `atac generate-permit-list` output directory and a mapper directory (map.rad less its last `cut` bytes); -> (input_dir, rad_dir)"""
    ind, rd = str(tmp_path / "gpl"), str(tmp_path / "map")
    os.makedirs(ind)
    os.makedirs(rd)
    with open(os.path.join(ind, "generate_permit_list.json"), "w") as f:
        json.dump(meta, f, indent=2)
    with open(os.path.join(ind, "permit_freq.bin"), "wb") as f:
        f.write(rad.permit_freq_bytes(L, freq, version=freq_version))
    with open(os.path.join(ind, "correction_plan.bin"), "wb") as f:
        f.write(rad.correction_plan_bytes(PLAN, barcode_len=L) if plan is None else plan)
    if rna:
        body, _ = rad.encode_chunks([[(0x11, 1, [(1, True)])]])
        prelude = rad.rad_prelude(["t0", "t1"], 1, L, 12, 4, 4)
    else:
        chunks = [[(0x11, [A1])]] if chunks is None else chunks
        body, _ = rad.encode_atac_chunks(chunks)
        prelude = rad.rad_prelude_atac(["chr1"], [1000], len(chunks), cblen=L)
    with open(os.path.join(rd, "map.rad"), "wb") as f:
        f.write((prelude + body)[:len(prelude) + len(body) - cut])
    if unmapped is not None:
        with open(os.path.join(rd, "unmapped_bc_count.bin"), "wb") as f:
            f.write(b"".join(int(b).to_bytes(8, "little") + int(n).to_bytes(4, "little") for b, n in unmapped))
    return ind, rd


def collate(lib, ind, rd, **kw):
    o = AtacCollateOpts(input_dir=ind.encode() if ind else None, rad_dir=rd.encode() if rd else None, cmdline=b"afquant atac collate", **kw)
    rc = lib.afq_atac_collate(C.byref(o))
    return rc, (lib.afq_host_last_error() or b"").decode()


def cli(*args):
    return subprocess.run([CLI, "atac", "collate"] + [str(a) for a in args], capture_output=True, text=True)


def refused(lib, ind, rd, code, sentence):
    """the library call and the sub-command refuse alike, and no RAD is written"""
    rc, msg = collate(lib, ind, rd)
    assert rc == code and sentence in msg, (rc, msg)
    r = cli("-i", ind, "-r", rd, "-m", 1000, "-t", 3)
    assert r.returncode == 1 and sentence in r.stderr and f"({code})" in r.stderr and "afquant atac collate failed" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(os.path.join(ind, "map.collated.rad")) and not os.path.exists(os.path.join(ind, "collate.json"))


def test_missing_arguments_and_directories(lib, tmp_path):
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
        r = cli("-i", ind, "-r", rd, flag)
        assert r.returncode == 1 and "compressed output is not supported" in r.stderr and f"({UNSUPPORTED})" in r.stderr
    assert not os.path.exists(os.path.join(ind, "map.collated.rad"))


def test_metadata_refusals(lib, tmp_path):
    no_version = {k: v for k, v in META.items() if k != "version_str"}   # (gpl_options' version_str does not count)
    refused(lib, *dirs(tmp_path / "a", meta=no_version), BAD_INPUT,
            "The generate_permit_list.json file does not contain a version_str field. Please re-run the generate-permit-list step with a newer version of alevin-fry")
    no_chunks = {k: v for k, v in META.items() if k != "num-chunks"}     # (nor does gpl_options' num-chunks)
    refused(lib, *dirs(tmp_path / "b", meta=no_chunks), BAD_INPUT, "num-chunks key not present")


def test_permit_list_refusals(lib, tmp_path):
    refused(lib, *dirs(tmp_path / "a", freq_version=2), BAD_INPUT, "The permit_freq.bin file had version 2, but this version of alevin-fry requires version 1")
    refused(lib, *dirs(tmp_path / "b", plan=rad.correction_plan_bytes(PLAN, barcode_len=L - 1)), BAD_INPUT, "correction plan does not match this ATAC input")
    refused(lib, *dirs(tmp_path / "c", plan=rad.correction_plan_bytes(PLAN, barcode_len=L, sample_barcode_len=8, sample_scopes=[(5, PLAN[:1])])), BAD_INPUT,
            "correction plan does not match this ATAC input")
    no_scope = b"AFCORR\0\0" + (1).to_bytes(2, "little") + b"\0" + bytes([L]) + b"\0" + bytes(8) + bytes(8)   # no sample part, no cell scope at all
    refused(lib, *dirs(tmp_path / "d", plan=no_scope), BAD_INPUT, "ATAC correction plan has no global cell scope")
    ind, rd = dirs(tmp_path / "e")
    with open(os.path.join(ind, "correction_plan.bin"), "ab") as f:
        f.write(b"\x00")   # a present but malformed plan is an error, not a reason to fall back on the legacy map
    with open(os.path.join(ind, "permit_map.bin"), "wb") as f:
        f.write(rad.permit_map_bytes(PLAN))
    refused(lib, ind, rd, BAD_INPUT, "correction plan contains trailing data")


def test_an_rna_prelude_is_refused_and_names_collate(lib, tmp_path):
    ind, rd = dirs(tmp_path, rna=True)
    refused(lib, ind, rd, UNSUPPORTED, "use `collate`")
    assert open(os.path.join(ind, "unmapped_bc_count_collated.bin"), "rb").read() == bytes(8)   # no unmapped_bc_count.bin: the empty map


def test_a_file_with_fewer_chunks_than_num_chunks_is_refused(lib, tmp_path):
    ind, rd = dirs(tmp_path, meta=dict(META, **{"num-chunks": 3}), chunks=[[(0x11, [A1])], [(0x22, [A1])]])
    refused(lib, ind, rd, BAD_INPUT, "map.rad ends before chunk 2 of 3")


def test_a_chunk_whose_nbytes_runs_past_the_file_is_refused_by_its_number(lib, tmp_path):
    ind, rd = dirs(tmp_path, meta=dict(META, **{"num-chunks": 2}), chunks=[[(0x11, [A1])], [(0x22, [A1])]], cut=4)
    refused(lib, ind, rd, BAD_INPUT, "corrupt chunk header (chunk 1)")


def test_the_unmapped_counts_are_written_before_the_prelude_is_read(lib, tmp_path):
    unmapped = [(0x11, 4), (0x12, 6), (0x22, 1), (0x99, 50), (0x11, 2)]
    ind, rd = dirs(tmp_path, rna=True, unmapped=unmapped)
    refused(lib, ind, rd, UNSUPPORTED, "use `collate`")
    buf = open(os.path.join(ind, "unmapped_bc_count_collated.bin"), "rb").read()
    n = int.from_bytes(buf[:8], "little")
    assert len(buf) == 8 + 12 * n
    got = {int.from_bytes(buf[8 + 12 * i:16 + 12 * i], "little"): int.from_bytes(buf[16 + 12 * i:20 + 12 * i], "little") for i in range(n)}
    assert got == {0x11: 12, 0x22: 1}


def test_collate_points_a_scatac_prelude_to_atac_collate(tmp_path):
    """`collate` on the same directory still refuses with AFQ_ERR_UNSUPPORTED and the word scATAC, and now names the sub-command"""
    meta = {"velo_mode": False, "expected_ori": "fw", "version_str": "0.18.0"}
    ind, rd = dirs(tmp_path, meta=meta)
    r = subprocess.run([CLI, "collate", "-i", ind, "-r", rd], capture_output=True, text=True)
    assert r.returncode == 1 and "scATAC" in r.stderr and "atac collate" in r.stderr and f"({UNSUPPORTED})" in r.stderr


def test_limits_are_the_sort_parses_and_the_radix_block(lib):
    c, s, r = pkg.atac_collate_limits(), pkg.atac_sort_limits(), pkg.collate_limits()
    assert (c["parse_tile"], c["parse_halo"]) == (s["parse_tile"], s["parse_halo"]) and c["radix_block"] == r["radix_block"] and c["aln_bytes"] == 11
    assert c["parse_halo"] >= 4 + 8 + c["aln_bytes"] + 1   # the widest head, one alignment, and the byte a 4-byte read of its last three takes
    assert pkg.Quantifier.atac_collate_limits() == c


def test_usage_names_the_sub_command():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "afquant atac collate -i <input-dir> -r <rad-dir> [-t N] [-c] [-m N] [--device N]" in r.stderr
