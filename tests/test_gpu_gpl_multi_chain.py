"""GPU test of the whole multi-barcode generate-permit-list step: pkg.generate_permit_list_multi on a written directory against the
files tests/gpl_multi_judge.py derives from the same records (the cases of gpl_multi_cases.CHAIN_CASES, whose reach
tests/test_gpl_multi_cases_cpu.py shows).  Maps are compared as maps, correction_plan.bin byte for byte, the JSON documents key for key
without what a run measures."""
import ctypes as C
import json
import os

import pytest

import gpl_multi_cases as MC
import gpl_multi_judge as M
from util import pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
UNSUPPORTED = pkg._abi.AFQ_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    chunks, rows, kinds, cells = MC.chain_dataset()
    d = tmp_path_factory.mktemp("flex")
    in_dir = MC.write_chain_dir(str(d / "map"), chunks)
    valid, white = MC.chain_lists(cells)
    paths = {"forward": str(d / "samples.tsv"), "reverse": str(d / "samples_rc.tsv"), "valid_bc": str(d / "valid.txt"), "unfiltered": str(d / "white.txt")}
    for name, rev in (("forward", False), ("reverse", True)):
        with open(paths[name], "w") as f:
            f.write(MC.sample_rows(rows, rev))
    for name, bcs in (("valid_bc", valid), ("unfiltered", white)):
        with open(paths[name], "w") as f:
            f.write("".join(MC.seq(b, 16) + "\n" for b in bcs))
    return {"chunks": chunks, "rows": rows, "cells": cells, "in": in_dir, "paths": paths, "root": d}


@pytest.mark.parametrize("case", MC.CHAIN_CASES, ids=lambda c: c["name"])
def test_the_whole_step_against_the_judge(dataset, case):
    out = str(dataset["root"] / ("out_" + case["name"]))
    kw = {k: v for k, v in case.items() if k != "name"}
    kw.setdefault("expected_ori", "fw")
    list_file = dataset["paths"].get(case["method"])
    cmd = "generate_permit_list_multi " + case["name"]
    got = pkg.generate_permit_list_multi(dataset["in"], out, dataset["paths"][case.get("sample_bc_ori", "forward")], list_file=list_file, cmdline=cmd, **kw)
    want = MC.chain_want(case, dataset["chunks"], dataset["rows"], dataset["cells"], list_file=list_file, cmdline=cmd)
    assert got["total_cells"] == want["total_cells"] > 0
    assert {k: got["stats"][k] for k in want["stats"]} == want["stats"]
    read = lambda *p: open(os.path.join(out, *p), "rb").read()
    assert rad.read_permit_map(read("sample_permit_map.bin")) == want["sample_permit_map"]
    for sdir, pmap, pfreq in want["samples"]:
        assert os.path.isdir(os.path.join(out, sdir))
        if pmap is None:   # the sample without a read: its directory, no permit files
            assert os.listdir(os.path.join(out, sdir)) == [] and sdir == "sample_gamma"
            continue
        assert rad.read_permit_map(read(sdir, "permit_map.bin")) == pmap
        assert rad.read_permit_freq(read(sdir, "permit_freq.bin")) == (1, 16, pfreq)
    plan = read("correction_plan.bin")
    assert plan == want["plan"]
    info = json.loads(read("sample_info.json"))
    assert info["correction_plan_bytes"] == len(plan) and all(isinstance(info[k], float) and info[k] >= 0 for k in ("cell_correction_seconds", "correction_plan_write_seconds"))
    assert isinstance(info["sample_routing"]["replay_seconds"], float)
    assert M.strip_measured(info) == want["sample_info"]
    assert json.loads(read("generate_permit_list.json")) == want["generate_permit_list"]
    assert sorted(os.listdir(out)) == sorted(["sample_permit_map.bin", "correction_plan.bin", "sample_info.json", "generate_permit_list.json"] + [s[0] for s in want["samples"]])


def test_one_fill_and_several_fills_write_the_same_files(dataset):
    case = next(c for c in MC.CHAIN_CASES if c["name"] == "force_frequency_reverse_fills")
    kw = {k: v for k, v in case.items() if k not in ("name", "fill_bytes")}
    outs = []
    for fill in (0, 20000, 3000):
        out = str(dataset["root"] / f"fills_{fill}")
        pkg.generate_permit_list_multi(dataset["in"], out, dataset["paths"]["reverse"], fill_bytes=fill, **kw)
        outs.append(out)
    for rel in ("sample_permit_map.bin", "correction_plan.bin", "generate_permit_list.json", "sample_alpha/permit_map.bin", "sample_beta/permit_freq.bin"):
        a = open(os.path.join(outs[0], rel), "rb").read()
        assert all(open(os.path.join(o, rel), "rb").read() == a for o in outs[1:]), rel


class GplOpts(C.Structure):
    _fields_ = [("input_dir", C.c_char_p), ("output_dir", C.c_char_p), ("expected_ori", C.c_uint32), ("method", C.c_uint32), ("method_count", C.c_uint64),
                ("list_file", C.c_char_p), ("min_reads", C.c_uint64), ("frequency", C.c_uint32), ("neighborhood", C.c_int32), ("conf_num", C.c_uint64),
                ("conf_den", C.c_uint64), ("num_threads", C.c_uint32), ("device", C.c_uint32), ("cmdline", C.c_char_p), ("fill_bytes", C.c_uint64),
                ("corrected_out", C.POINTER(C.c_uint64))]


def test_the_single_barcode_entry_still_refuses_the_directory(dataset):
    lib = pkg.load_library()
    lib.afq_host_last_error.restype = C.c_char_p
    lib.afq_generate_permit_list.argtypes = [C.POINTER(GplOpts)]
    o = GplOpts()
    o.input_dir, o.output_dir, o.expected_ori, o.method, o.neighborhood = dataset["in"].encode(), str(dataset["root"] / "single_out").encode(), 1, 0, -1
    assert lib.afq_generate_permit_list(C.byref(o)) == UNSUPPORTED and b"multi-barcode" in lib.afq_host_last_error()
    assert not (dataset["root"] / "single_out").exists()
