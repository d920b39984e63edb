"""GPU test of the multi-barcode chain generate_permit_list_multi -> collate_multi -> quant on gpl_multi_cases.chain_dataset():
what pkg.collate_multi writes into the directory the GPL step wrote, against tests/collate_multi_judge.py on the same directory -
map.collated.rad and collation_manifest.bin byte for byte, collate.json key for key, the empty unmapped map, exactly four new
files -, then `afquant quant` on that directory, and the single-barcode entry points, which keep refusing it."""
import ctypes as C
import json
import os
import subprocess

import pytest

import collate_multi_judge as J
import gpl_multi_cases as MC
from util import pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
UNSUPPORTED = pkg._abi.AFQ_ERR_UNSUPPORTED
CLI = os.path.join(pkg.__path__[0], "csrc", "afquant")
CASES = ("knee_exact", "force_frequency", "unfiltered_unique")   # an exact-sample, a frequency-sample and an unfiltered case
NEW_FILES = ["collate.json", "collation_manifest.bin", "map.collated.rad", "unmapped_bc_count_collated.bin"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every case of CASES: the GPL step, then collate_multi, once; the judge's outputs beside them"""
    chunks, rows, kinds, cells = MC.chain_dataset()
    d = tmp_path_factory.mktemp("flexc")
    in_dir = MC.write_chain_dir(str(d / "map"), chunks)
    valid, white = MC.chain_lists(cells)
    paths = {"forward": str(d / "samples.tsv"), "unfiltered": str(d / "white.txt")}
    with open(paths["forward"], "w") as f:
        f.write(MC.sample_rows(rows, False))
    with open(paths["unfiltered"], "w") as f:
        f.write("".join(MC.seq(b, 16) + "\n" for b in white))
    lim = pkg.collate_multi_limits()
    out = {}
    for name in CASES:
        case = next(c for c in MC.CHAIN_CASES if c["name"] == name)
        o = str(d / ("out_" + name))
        kw = {k: v for k, v in case.items() if k != "name"}
        kw.setdefault("expected_ori", "fw")
        pkg.generate_permit_list_multi(in_dir, o, paths["forward"], list_file=paths.get(case["method"]), **kw)
        before = sorted(os.listdir(o))
        want = J.from_directory(o, os.path.join(in_dir, "map.rad"), cmdline="collate_multi " + name, lane_alns=lim["lane_alns"])
        stats = pkg.collate_multi(o, in_dir, cmdline="collate_multi " + name)
        out[name] = {"dir": o, "before": before, "want": want, "stats": stats}
    return {"in": in_dir, "root": d, "runs": out}


@pytest.mark.parametrize("name", CASES)
def test_the_files_against_the_judge(runs, name):
    r = runs["runs"][name]
    want = r["want"]
    read = lambda p: open(os.path.join(r["dir"], p), "rb").read()
    assert r["stats"] == want["stats"] and want["stats"]["n_kept"] > 1000 and want["stats"]["n_unrouted"] > 0
    assert read("map.collated.rad") == want["rad"]
    assert read("collation_manifest.bin") == rad.collation_manifest(want["groups"])
    assert [g[1] for g in want["groups"]] == ["alpha", "beta"] and b"gamma" not in read("collation_manifest.bin")   # gamma has no read: no group
    assert json.loads(read("collate.json")) == want["collate_json"]
    assert read("unmapped_bc_count_collated.bin") == bytes(8) == want["unmapped"]
    assert sorted(os.listdir(r["dir"])) == sorted(r["before"] + NEW_FILES)
    info = {e["name"]: e for e in json.loads(read("sample_info.json"))["samples"]}
    for g, kept in zip(want["groups"], want["kept_per_group"]):
        assert kept == g[4] == info[g[1]]["collatable_reads"]


def test_deferred_sample_barcodes_are_routed_under_frequency(runs):
    """under sample frequency the barcodes between a0 and b0 are accepted for alpha: the plan's sample corrections hold them, and
    collate keeps their records - more than the exact case keeps"""
    assert runs["runs"]["force_frequency"]["want"]["stats"]["n_unrouted"] < runs["runs"]["knee_exact"]["want"]["stats"]["n_unrouted"]


def test_quant_runs_on_the_collated_directory(runs, tmp_path):
    name = next((n for n in CASES if min(runs["runs"][n]["want"]["nrec"]) > 0), None)   # quant refuses an empty chunk
    assert name is not None, "no case in which every cell kept a record"
    r = runs["runs"][name]
    tg = str(tmp_path / "t2g.tsv")
    with open(tg, "w") as f:
        f.write("".join(f"t{i}\tG{i % 10}\n" for i in range(100)))
    out = tmp_path / "quant"
    p = subprocess.run([CLI, "quant", "-i", r["dir"], "-m", tg, "-o", str(out), "-r", "cr-like", "-t", "2"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    names = {0: "alpha", 1: "beta"}
    ordinal = {g[2] + k: i for i, g in enumerate(r["want"]["groups"]) for k in range(g[3])}
    want_rows = [f"{names[ordinal[j]]}_{rad.int_to_seq(bc, 16)}" for j, (_, bc) in enumerate(r["want"]["cells"])]
    assert (out / "alevin/quants_mat_rows.txt").read_text().split() == want_rows


class CollateOpts(C.Structure):
    _fields_ = [("input_dir", C.c_char_p), ("rad_dir", C.c_char_p), ("num_threads", C.c_uint32), ("compress", C.c_uint32), ("max_records", C.c_uint32),
                ("device", C.c_uint32), ("cmdline", C.c_char_p), ("stats_out", C.POINTER(pkg._abi.AfqCollateStats))]


def test_the_single_barcode_entries_still_refuse_the_directory(runs):
    r = runs["runs"][CASES[0]]
    listing = sorted(os.listdir(r["dir"]))
    lib = pkg.load_library()
    lib.afq_host_last_error.restype = C.c_char_p
    lib.afq_collate.argtypes = [C.POINTER(CollateOpts)]
    o = CollateOpts(input_dir=r["dir"].encode(), rad_dir=runs["in"].encode())
    assert lib.afq_collate(C.byref(o)) == UNSUPPORTED
    msg = lib.afq_host_last_error().decode()
    assert "multi_barcode" in msg and "afq_collate_multi" in msg
    p = subprocess.run([CLI, "collate", "-i", r["dir"], "-r", runs["in"]], capture_output=True, text=True)
    assert p.returncode == 1 and "multi_barcode" in p.stderr and f"({UNSUPPORTED})" in p.stderr
    assert sorted(os.listdir(r["dir"])) == listing
