"""CPU tests of multi-barcode collate's host half (afq_collate_multi, include/afquant_host.h): every refusal that precedes device
work, through the library call on hand-written directories - they read the same with and without a GPU, and none leaves a
map.collated.rad, a manifest or a collate.json behind -; afq_parse_correction_plan_multi against the Python parser; the manifest
writer against rad.collation_manifest; the argument checks of afq_collate_multi_rad."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import collate_multi_judge as J
import gpl_multi_cases as MC
import gpl_multi_judge as M
from util import pkg

rad = pkg.rad
INVALID_ARG, BAD_INPUT, UNSUPPORTED = pkg._abi.AFQ_ERR_INVALID_ARG, pkg._abi.AFQ_ERR_BAD_INPUT, pkg._abi.AFQ_ERR_UNSUPPORTED
L, SL = 16, 8
u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib():
    l = pkg.load_library()
    l.afq_host_last_error.restype = C.c_char_p
    l.afq_parse_correction_plan_multi.argtypes = [C.c_char_p, C.c_size_t, u64p, u64p, C.c_size_t, u64p, u64p, u64p, C.c_size_t, u64p, u64p, u64p, C.c_size_t, u32p, u32p]
    l.afq_parse_correction_plan_multi.restype = C.c_int64
    l.afq_parse_correction_plan.argtypes = [C.c_char_p, C.c_size_t, u64p, u64p, C.c_size_t, u32p]
    l.afq_parse_correction_plan.restype = C.c_int64
    l.afq_collation_manifest_bytes.argtypes = [u64p, C.POINTER(C.c_char_p), u64p, u64p, u64p, C.c_uint64, C.c_char_p, C.c_size_t]
    l.afq_collation_manifest_bytes.restype = C.c_int64
    l.afq_collate_multi_check_args.argtypes = [C.c_uint32] * 4 + [u64p, u32p, C.c_uint64, u32p, u64p, u64p, C.c_uint64, u32p, u64p, C.c_uint64, u32p, C.c_uint64]
    l.afq_collate_multi_check_args.restype = C.c_int
    return l


META = {"velo_mode": False, "expected_ori": "fw", "version_str": "0.18.0", "cmd": "x", "multi_barcode": True, "num_barcodes": 2}
SAMPLES = [("alpha", 0xA0, {0x11: 3, 0x22: 5}), ("beta", 0xB0, {0x11: 2}), ("gamma", 0xC0, None)]
SAMPLE_MAP = {0xA0: 0xA0, 0xA1: 0xA0, 0xB0: 0xB0, 0xC0: 0xC0}
SCOPES = [(0xA0, [(0x11, 0x11), (0x22, 0x22), (0x12, 0x11)]), (0xB0, [(0x11, 0x11)]), (0xC0, [])]
UNIQUE = ("hamming-1", "unique")


def dirs(tmp_path, meta=META, samples=SAMPLES, plan="default", info=True, prelude=None, n_chunks=1, num_chunks=None, cut=0, b0_bytes=2, scopes=SCOPES, cell_len=L):
    """a multi-barcode generate-permit-list output directory and a mapper directory; -> (input_dir, rad_dir)"""
    ind, rd = str(tmp_path / "gpl"), str(tmp_path / "map")
    os.makedirs(ind)
    os.makedirs(rd)
    with open(os.path.join(ind, "generate_permit_list.json"), "w") as f:
        json.dump(meta, f, indent=2)
    if info:
        doc = {"num_samples": len(samples), "num_barcodes": 2, "sample_routing": {"exact": 1, "samples": 7},
               "samples": [{"name": n, "barcode": f"0x{bc:x}", "num_cells": len(fr or {}), "cell_correction": {"exact_reads": 0}} for n, bc, fr in samples]}
        with open(os.path.join(ind, "sample_info.json"), "w") as f:
            json.dump(doc, f, indent=2)
    for n, _, fr in samples:
        os.makedirs(os.path.join(ind, "sample_" + n))
        if fr is not None:
            with open(os.path.join(ind, "sample_" + n, "permit_freq.bin"), "wb") as f:
                f.write(rad.permit_freq_bytes(L, fr.items()))
    if plan == "default":
        plan = M.plan_bytes(SL, cell_len, None, SAMPLE_MAP, UNIQUE, scopes)
    if plan is not None:
        with open(os.path.join(ind, "correction_plan.bin"), "wb") as f:
            f.write(plan)
    body, _ = rad.encode_multi_bc_chunks([[(0xA0, 0x11, 1, [(1, True)])]] * n_chunks, b0_bytes, 4, 4)
    num_chunks = n_chunks if num_chunks is None else num_chunks
    pre = rad.rad_prelude_multi_bc(["t0", "t1"], num_chunks, SL, L, 12, b_bytes=4, umi_bytes=4, b0_bytes=b0_bytes) if prelude is None else prelude(num_chunks)
    with open(os.path.join(rd, "map.rad"), "wb") as f:
        f.write((pre + body)[:len(pre) + len(body) - cut])
    return ind, rd


def collate(lib, ind, rd, **kw):
    o = pkg._abi.AfqCollateMultiOpts(input_dir=ind.encode() if ind else None, rad_dir=rd.encode() if rd else None, cmdline=b"collate_multi", **kw)
    rc = lib.afq_collate_multi(C.byref(o))
    return rc, (lib.afq_host_last_error() or b"").decode()


def refused(lib, ind, rd, code, sentence, **kw):
    before = sorted(os.listdir(ind))
    rc, msg = collate(lib, ind, rd, **kw)
    assert rc == code and sentence in msg, (rc, msg)
    assert sorted(os.listdir(ind)) == before   # no map.collated.rad, no manifest, no collate.json, no unmapped counts
    for name in ("map.collated.rad", "collation_manifest.bin", "collate.json"):
        assert not os.path.exists(os.path.join(ind, name))


def test_null_options(lib, tmp_path):
    assert lib.afq_collate_multi(None) == INVALID_ARG
    ind, rd = dirs(tmp_path)
    assert collate(lib, ind, None)[0] == INVALID_ARG and collate(lib, None, rd)[0] == INVALID_ARG


@pytest.mark.parametrize("meta,code,sentence", [
    ({k: v for k, v in META.items() if k != "multi_barcode"}, UNSUPPORTED, "use collate"),
    (dict(META, multi_barcode=False), UNSUPPORTED, "use collate"),
    (dict(META, velo_mode=True), UNSUPPORTED, "velo_mode"),
    ({k: v for k, v in META.items() if k != "version_str"}, BAD_INPUT, "does not contain a version_str field"),
    (dict(META, expected_ori="sideways"), BAD_INPUT, "could not read strand"),
], ids=["no_multi_barcode", "multi_barcode_false", "velo_mode", "no_version_str", "bad_expected_ori"])
def test_metadata_refusals(lib, tmp_path, meta, code, sentence):
    ind, rd = dirs(tmp_path, meta=meta)
    refused(lib, ind, rd, code, sentence)


def test_a_missing_sample_info(lib, tmp_path):
    ind, rd = dirs(tmp_path, info=False)
    refused(lib, ind, rd, BAD_INPUT, "could not open sample_info.json")


def test_a_missing_plan_is_unsupported_and_says_why(lib, tmp_path):
    ind, rd = dirs(tmp_path, plan=None)
    refused(lib, ind, rd, UNSUPPORTED, "no correction_plan.bin")
    assert "on the fly" in collate(lib, ind, rd)[1]


def test_plans_that_do_not_match(lib, tmp_path):
    ind, rd = dirs(tmp_path / "global", plan=rad.correction_plan_bytes([(0x11, 0x11)], barcode_len=L))
    refused(lib, ind, rd, BAD_INPUT, "correction plan does not match this multi-barcode RAD input")
    ind, rd = dirs(tmp_path / "len", cell_len=L - 1)
    refused(lib, ind, rd, BAD_INPUT, "correction plan does not match this multi-barcode RAD input")
    ind, rd = dirs(tmp_path / "trail", plan=M.plan_bytes(SL, L, None, SAMPLE_MAP, UNIQUE, SCOPES) + b"\0")
    refused(lib, ind, rd, BAD_INPUT, "correction plan contains trailing data")
    ind, rd = dirs(tmp_path / "cut", plan=M.plan_bytes(SL, L, None, SAMPLE_MAP, UNIQUE, SCOPES)[:-3])
    refused(lib, ind, rd, BAD_INPUT, "truncated or malformed")
    ind, rd = dirs(tmp_path / "magic", plan=b"NOTAPLAN" + bytes(20))
    refused(lib, ind, rd, BAD_INPUT, "invalid magic")


def test_a_sample_with_cells_and_no_cell_scope(lib, tmp_path):
    ind, rd = dirs(tmp_path, scopes=[SCOPES[0], SCOPES[2]])
    refused(lib, ind, rd, BAD_INPUT, "correction plan has no cell scope for canonical sample 0xb0")


def test_a_correction_into_a_barcode_that_is_no_cell_of_its_sample(lib, tmp_path):
    ind, rd = dirs(tmp_path, scopes=[SCOPES[0], (0xB0, [(0x11, 0x11), (0x23, 0x22)]), SCOPES[2]])   # 0x22 is a cell of alpha, not of beta
    refused(lib, ind, rd, BAD_INPUT, "which is not a cell of that sample")


def test_an_ordinal_that_does_not_fit_b0(lib, tmp_path):
    samples = [(f"s{i}", 0x100 + i, {0x11: 1}) for i in range(257)]
    scopes = [(0x100 + i, [(0x11, 0x11)]) for i in range(257)]
    ind, rd = dirs(tmp_path, samples=samples, scopes=scopes, b0_bytes=1)
    refused(lib, ind, rd, UNSUPPORTED, "the largest sample ordinal (256) does not fit the 1-byte b0 field")


def test_prelude_refusals(lib, tmp_path):
    single = lambda n: rad.rad_prelude(["t0", "t1"], n, L, 12, 4, 4)
    atac = lambda n: rad.rad_prelude_atac(["chr1"], [1000], n)

    def with_pos(n):
        p = rad.rad_prelude_multi_bc(["t0", "t1"], n, SL, L, 12, b_bytes=4, umi_bytes=4, b0_bytes=2)
        a = (1).to_bytes(2, "little") + (20).to_bytes(2, "little") + b"compressed_ori_refid" + bytes([3])
        assert p.count(a) == 1
        return p.replace(a, (2).to_bytes(2, "little") + a[2:] + (3).to_bytes(2, "little") + b"pos" + bytes([3]))

    def three_levels(n):
        p = rad.rad_prelude_multi_bc(["t0", "t1"], n, SL, L, 12, b_bytes=4, umi_bytes=4, b0_bytes=2)
        tag = lambda name, t: len(name).to_bytes(2, "little") + name + bytes([t])
        a = (3).to_bytes(2, "little") + tag(b"b0", 2) + tag(b"b1", 3) + tag(b"u", 3)
        assert p.count(a) == 1
        p = p.replace(a, (4).to_bytes(2, "little") + tag(b"b0", 2) + tag(b"b1", 3) + tag(b"b2", 3) + tag(b"u", 3))
        v = (2).to_bytes(2, "little") + SL.to_bytes(2, "little") + L.to_bytes(2, "little")
        assert p.count(v) == 1
        return p.replace(v, (3).to_bytes(2, "little") + v[2:])

    for name, pre, sentence in (("single", single, "this is a single-barcode RAD file"), ("atac", atac, "this is a scATAC RAD file"),
                                ("pos", with_pos, "alignment tag pos"), ("three", three_levels, "only two barcode levels")):
        ind, rd = dirs(tmp_path / name, prelude=pre)
        refused(lib, ind, rd, UNSUPPORTED, sentence)


def test_compressed_output_and_a_truncated_chunk_table(lib, tmp_path):
    ind, rd = dirs(tmp_path / "c")
    refused(lib, ind, rd, UNSUPPORTED, "compressed output is not supported", compress=1)
    ind, rd = dirs(tmp_path / "short", n_chunks=2, num_chunks=3)
    refused(lib, ind, rd, BAD_INPUT, "map.rad ends before chunk 2 of 3")
    ind, rd = dirs(tmp_path / "cut", n_chunks=2, cut=5)
    refused(lib, ind, rd, BAD_INPUT, "corrupt chunk header (chunk 1)")


def test_the_single_barcode_entry_names_the_new_one(tmp_path):
    lib = pkg.load_library()
    import test_collate_host_cpu as T

    lib.afq_host_last_error.restype = C.c_char_p
    lib.afq_collate.argtypes = [C.POINTER(T.CollateOpts)]
    ind, rd = dirs(tmp_path)
    rc, msg = T.collate(lib, ind, rd)
    assert rc == UNSUPPORTED and "multi_barcode" in msg and "afq_collate_multi" in msg


# ------------------------------------------------------------------------------------------------------------------ the plan parser
def parse_multi(lib, buf):
    ns, nsc, sl, cl = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
    n = lib.afq_parse_correction_plan_multi(buf, len(buf), None, None, 0, C.byref(ns), None, None, 0, C.byref(nsc), None, None, 0, C.byref(sl), C.byref(cl))
    if n < 0:
        return int(n), (lib.afq_host_last_error() or b"").decode()
    so, sc = np.zeros(ns.value, np.uint64), np.zeros(ns.value, np.uint64)
    sb, cnt = np.zeros(nsc.value, np.uint64), np.zeros(nsc.value, np.uint64)
    co, cc = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    p = lambda a: a.ctypes.data_as(u64p)
    assert lib.afq_parse_correction_plan_multi(buf, len(buf), p(so), p(sc), len(so), None, p(sb), p(cnt), len(sb), None, p(co), p(cc), len(co), None, None) == n
    scopes, at = [], 0
    for b, k in zip(sb.tolist(), cnt.tolist()):
        scopes.append((b, list(zip(co[at:at + k].tolist(), cc[at:at + k].tolist()))))
        at += k
    return {"sample_len": sl.value, "cell_len": cl.value, "sample": list(zip(so.tolist(), sc.tolist())), "scopes": scopes}


def test_the_plan_parser_agrees_with_the_python_parser_on_the_gpl_judges_plans(lib):
    chunks, rows, kinds, cells = MC.chain_dataset()
    for name in ("knee_exact", "force_frequency", "unfiltered_unique"):
        case = next(c for c in MC.CHAIN_CASES if c["name"] == name)
        buf = MC.chain_want(case, chunks, rows, cells, list_file="x")["plan"]
        got = parse_multi(lib, buf)
        assert got == J.parse_plan(buf) and len(got["scopes"]) == 3 and got["sample_len"] == 8 and got["cell_len"] == 16
        assert sum(len(pp) for _, pp in got["scopes"]) > 50
        # the single-scope parser keeps refusing it
        assert lib.afq_parse_correction_plan(buf, len(buf), None, None, 0, None) == BAD_INPUT and b"sample-scoped" in lib.afq_host_last_error()
        assert parse_multi(lib, buf + b"\0") == (BAD_INPUT, "correction plan contains trailing data")
        assert parse_multi(lib, buf[:-1])[0] == BAD_INPUT and parse_multi(lib, b"XX" + buf[2:]) == (BAD_INPUT, "correction plan has invalid magic")
    rc, msg = parse_multi(lib, rad.correction_plan_bytes([(1, 1)]))
    assert rc == BAD_INPUT and "not sample-scoped" in msg
    assert parse_multi(lib, buf[:9])[0] == BAD_INPUT and parse_multi(lib, buf[:8] + (2).to_bytes(2, "little") + buf[10:])[0] == BAD_INPUT


def test_the_manifest_writer_agrees_with_rad_collation_manifest(lib):
    groups = [(0xA0, "alpha", 0, 2, 8), (0xB0, "a name with spaces", 2, 1, 2), (0xFFFFFFFFFFFFFFFF, "", 3, 0, 0)]
    arr = lambda k: np.asarray([g[k] for g in groups], np.uint64)
    key, start, nch, nrec = arr(0), arr(2), arr(3), arr(4)
    names = (C.c_char_p * len(groups))(*[g[1].encode() for g in groups])
    p = lambda a: a.ctypes.data_as(u64p)
    n = lib.afq_collation_manifest_bytes(p(key), names, p(start), p(nch), p(nrec), len(groups), None, 0)
    out = C.create_string_buffer(n)
    assert lib.afq_collation_manifest_bytes(p(key), names, p(start), p(nch), p(nrec), len(groups), out, n) == n
    assert out.raw == rad.collation_manifest(groups)
    assert lib.afq_collation_manifest_bytes(None, None, None, None, None, 0, None, 0) == len(rad.collation_manifest([]))


# ------------------------------------------------------------------------------------------------------------------ argument checks
def check_args(lib, b0=2, b1=4, umi=4, ori=0, so=(7, 8), si=(0, 1), cs=(0, 1), co=(5, 5), cc=(5, 6), ls=(0, 1), lb=(5, 6), b0o=(0, 1), n_samples=None, null=None):
    a = {"so": np.asarray(so, np.uint64), "si": np.asarray(si, np.uint32), "cs": np.asarray(cs, np.uint32), "co": np.asarray(co, np.uint64), "cc": np.asarray(cc, np.uint64),
         "ls": np.asarray(ls, np.uint32), "lb": np.asarray(lb, np.uint64), "b0o": np.asarray(b0o, np.uint32)}
    p = lambda k: None if k == null else a[k].ctypes.data_as(u64p if a[k].dtype == np.uint64 else u32p)
    rc = lib.afq_collate_multi_check_args(b0, b1, umi, ori, p("so"), p("si"), len(so), p("cs"), p("co"), p("cc"), len(cs), p("ls"), p("lb"), len(ls), p("b0o"),
                                          len(b0o) if n_samples is None else n_samples)
    return rc, (lib.afq_host_last_error() or b"").decode()


def test_argument_checks_of_the_device_call(lib):
    assert check_args(lib)[0] == 0
    for k in ("so", "si", "cs", "co", "cc", "ls", "lb", "b0o"):
        assert check_args(lib, null=k) == (INVALID_ARG, "null argument"), k
    for kw in (dict(b0=3), dict(b0=8), dict(b1=0), dict(b1=8), dict(umi=3), dict(ori=3)):
        assert check_args(lib, **kw)[0] == INVALID_ARG, kw
    rc, msg = check_args(lib, si=(0, 1 << 31))
    assert rc == INVALID_ARG and "2^31" in msg
    assert check_args(lib, ls=(0, 0xFFFFFFFF))[0] == INVALID_ARG and check_args(lib, cs=(0, 2))[0] == INVALID_ARG
    assert check_args(lib, n_samples=(1 << 31) + 1)[0] == INVALID_ARG
    rc, msg = check_args(lib, so=(7, 7))
    assert rc == BAD_INPUT and "occurs twice among the sample entries" in msg
    rc, msg = check_args(lib, cs=(1, 1), cc=(6, 6))
    assert rc == BAD_INPUT and "occurs twice among the corrections of sample 1" in msg
    rc, msg = check_args(lib, ls=(1, 1), lb=(6, 6), cs=(1, 1), co=(5, 7), cc=(6, 6))
    assert rc == BAD_INPUT and "cells 0 and 1 carry one barcode (6) in sample 1" in msg
    rc, msg = check_args(lib, cc=(5, 5))   # 5 is a cell of sample 0 only
    assert rc == BAD_INPUT and "correction entry 1" in msg and "not a cell of that sample" in msg
    assert check_args(lib, b0=1, so=(7, 256))[0] == BAD_INPUT and check_args(lib, b1=1, co=(5, 256))[0] == BAD_INPUT and check_args(lib, b1=2, lb=(5, 1 << 16))[0] == BAD_INPUT
    rc, msg = check_args(lib, b0=1, b0o=(0, 256))
    assert rc == UNSUPPORTED and "does not fit 1 bytes" in msg
    assert check_args(lib, so=(), si=(), cs=(), co=(), cc=(), ls=(), lb=(), b0o=())[0] == 0
