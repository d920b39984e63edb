"""GPU end-to-end tests of `afquant generate-permit-list`: the sub-command in a fresh child process over a written directory, for each
of the five filter methods and both resolutions; the five files are parsed back with rad.py's readers and must equal the maps of
tests/gpl_judge.py; the produced files load through the project's own readers and `atac sort` accepts a directory assembled from them."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import gpl_cases as G
import gpl_judge as J
from test_gpl_host_cpu import check_outputs
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")
L = 16
FREQ = ("frequency", (39, 40), 1)


@pytest.fixture(scope="module")
def data():
    chunks, cells, (heavy, sibling, midpoint) = G.cli_dataset(L=L)
    return {"chunks": chunks, "cells": cells, "sibling": sibling, "midpoint": midpoint, "heavy": heavy}


def write_input(path, chunks, pos_bytes=0, prelude=None):
    os.makedirs(path, exist_ok=True)
    body, _ = rad.encode_chunks(chunks, bc_bytes=4, umi_bytes=4, pos_bytes=pos_bytes)
    if prelude is None:
        prelude = rad.rad_prelude(["t%d" % i for i in range(100)], len(chunks), L, 12, 4, 4, pos_bytes=pos_bytes)
    with open(os.path.join(path, "map.rad"), "wb") as f:
        f.write(prelude + body)
    return path


def run(args):
    return subprocess.run([CLI, "generate-permit-list"] + [str(a) for a in args], capture_output=True, text=True)


def list_file(path, barcodes, gz=False):
    text = "".join(rad.int_to_seq(b, L) + "\n" for b in barcodes)
    if gz:
        with gzip.open(path, "wt") as f:
            f.write(text)
    else:
        with open(path, "w") as f:
            f.write(text)
    return str(path)


def method_args(method, data, tmp_path):
    """-> (command-line arguments, the judge's keyword arguments)"""
    cells = data["cells"]
    if method == "knee":
        return ["-k"], {}
    if method == "expect":
        return ["-e", 30], {"arg": 30}
    if method == "force":
        return ["-f", 35], {"arg": 35}
    if method == "valid_bc":
        listed = cells[:30] + [cells[0], 0x123456, data["sibling"]]   # a repeated line, and two barcodes that were never observed
        return ["-b", list_file(tmp_path / "valid.txt", listed)], {"listed": listed}
    listed = cells + [0x123456, 0xABCDEF01]
    return ["-u", list_file(tmp_path / "unfiltered.txt.gz", listed, gz=True), "-m", 25], {"listed": listed, "min_reads": 25}


@pytest.mark.parametrize("method", ["knee", "expect", "force", "valid_bc", "unfiltered"])
@pytest.mark.parametrize("resolution", ["unique", FREQ], ids=["unique", "frequency"])
def test_every_method_and_resolution_writes_the_judges_files(data, tmp_path, method, resolution):
    ind, out = write_input(str(tmp_path / "in"), data["chunks"]), str(tmp_path / "out")
    args, kw = method_args(method, data, tmp_path)
    r = run(["-i", ind, "-d", "fw", "-o", out, "-t", 4] + args + (["--cell-bc-correction", "frequency"] if resolution != "unique" else []))
    assert r.returncode == 0, r.stderr
    want = J.gpl_outputs(data["chunks"], "fw", method, L, resolution=resolution, **kw)
    assert want["stats"]["corrected_distinct"] > 0 and want["stats"]["not_found_distinct"] > 0 and want["max_ambig"] == 30
    j = check_outputs(out, want, L, resolution)
    assert j["expected_ori"] == "fw" and "generate-permit-list" in j["cmd"] and j["resolved_cell_bc_confidence"] == "39/40"
    assert want["neighborhood"] == (J.HAMMING if method == "unfiltered" else J.SHIFT)   # prog_opts.rs:135-144
    if method == "valid_bc":
        assert 0x123456 not in want["permit_freq"] and want["stats"]["exact_distinct"] == 32   # never observed: counted, absent from permit_freq
        mid = dict(want["plan"]).get(data["midpoint"])   # one substitution from a heavy cell and from a never-observed listed barcode
        assert mid == (None if resolution == "unique" else data["heavy"]) and want["stats"]["ambiguous_distinct"] == (1 if resolution == "unique" else 0)
    if method == "unfiltered":
        assert "not matching a known barcode exactly" in r.stderr
    assert "found 0 corrected barcodes" not in r.stderr


def test_neighbourhood_confidence_positions_and_several_fills(data, tmp_path):
    """an explicit neighbourhood and confidence; records with position bytes; the record pass cut into many device fills"""
    ind, out = write_input(str(tmp_path / "in"), data["chunks"], pos_bytes=4), str(tmp_path / "out")
    r = run(["-i", ind, "-d", "RC", "-o", out, "-f", 35, "--cell-bc-correction", "frequency", "--cell-bc-neighborhood", "hamming-1", "--cell-bc-confidence", "9/10",
             "--memory-limit", "1GiB", "--tmp-dir", str(tmp_path), "--fill-bytes", 6000])
    assert r.returncode == 0, r.stderr
    sizes = [len(rad.encode_chunks([c], pos_bytes=4)[0]) for c in data["chunks"]]
    assert sum(sizes) > 3 * 6000 and min(sizes) < 6000 < max(sizes)   # several fills; a chunk above the fill size is a fill of its own
    cells = {b for b in data["cells"]}
    assert all(any(b in cells for b, _u, _a in c) for c in data["chunks"] if len(c) > 1)   # the fills share barcodes
    res = ("frequency", (9, 10), 1)
    want = J.gpl_outputs(data["chunks"], "rc", "force", L, arg=35, neighborhood=J.HAMMING, resolution=res)
    j = check_outputs(out, want, L, res)
    assert j["expected_ori"] == "rc" and j["resolved_cell_bc_confidence"] == "9/10" and j["gpl_options"]["cell_bc_neighborhood"] == "hamming-1"


def test_both_and_either_agree_and_an_empty_result_warns(data, tmp_path):
    ind = write_input(str(tmp_path / "in"), data["chunks"])
    outs = []
    for ori in ("both", "Either"):
        out = str(tmp_path / ori)
        r = run(["-i", ind, "-d", ori, "-o", out, "-k"])
        assert r.returncode == 0, r.stderr
        outs.append({n: open(os.path.join(out, n), "rb").read() for n in ("permit_freq.bin", "all_freq.bin", "permit_map.bin", "correction_plan.bin")})
        check_outputs(out, J.gpl_outputs(data["chunks"], "both", "knee", L), L, "unique")
    assert outs[0] == outs[1]
    r = run(["-i", ind, "-d", "fw", "-o", str(tmp_path / "none"), "-f", 0])
    assert r.returncode == 0 and "found 0 corrected barcodes; please check the input." in r.stderr
    check_outputs(str(tmp_path / "none"), J.gpl_outputs(data["chunks"], "fw", "force", L, arg=0), L, "unique")


def test_refusals(data, tmp_path):
    ind = write_input(str(tmp_path / "in"), data["chunks"][:2])
    base = ["-i", ind, "-d", "fw", "-o", str(tmp_path / "o")]
    some = str(tmp_path / "some.txt")
    open(some, "w").write("ACGT\n")
    for flag, val in (("--sample-bc-list", some), ("--sample-names", some), ("--sample-bc-correction", "unique"), ("--sample-correction-mode", "exact"),
                      ("--sample-bc-neighborhood", "hamming-1"), ("--sample-bc-confidence", "0.9"), ("--sample-bc-ori", "forward")):
        r = run(base + ["-k", flag, val])
        assert r.returncode != 0 and flag in r.stderr and "multi-barcode" in r.stderr and "not supported" in r.stderr, (flag, r.stderr)
    # an ATAC prelude and a multi-barcode prelude are refused by name
    atac = str(tmp_path / "atac")
    os.makedirs(atac)
    open(os.path.join(atac, "map.rad"), "wb").write(rad.rad_prelude_atac(["chr1"], [1000], 0, cblen=16))
    r = run(["-i", atac, "-d", "fw", "-o", str(tmp_path / "o2"), "-k"])
    assert r.returncode != 0 and "atac generate-permit-list" in r.stderr and "not supported" in r.stderr
    r = subprocess.run([CLI, "atac", "generate-permit-list", "-i", atac], capture_output=True, text=True)
    assert r.returncode != 0 and "atac generate-permit-list" in r.stderr and "not supported" in r.stderr
    multi = str(tmp_path / "multi")
    os.makedirs(multi)
    open(os.path.join(multi, "map.rad"), "wb").write(rad.rad_prelude_multi_bc(["t0"], 0, 8, 16, 12))
    r = run(["-i", multi, "-d", "fw", "-o", str(tmp_path / "o3"), "-k"])
    assert r.returncode != 0 and "multi-barcode" in r.stderr and "--sample-bc-list" in r.stderr
    # flags
    for extra, msg in ((["-k", "-f", "3"], "cannot be used with one another"), ([], "required arguments"), (["-k", "--cell-bc-confidence", "1.5"], "between zero and one"),
                       (["-u", some, "-m", "0"], "min-reads < 1 is not supported"), (["-k", "--cell-bc-neighborhood", "edit-2"], "possible values")):
        r = run(base + extra)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    r = run(["-i", ind, "-o", str(tmp_path / "o"), "-d", "sideways", "-k"])
    assert r.returncode != 0 and "possible values: fw, rc, both, either" in r.stderr
    # two chunks of one barcode each cannot make a knee: the reference's sentence
    tiny = write_input(str(tmp_path / "tiny"), [[(5, 0, [(1, True)])]])
    r = run(["-i", tiny, "-d", "fw", "-o", str(tmp_path / "o4"), "-k"])
    assert r.returncode != 0 and "the list of putative cells is only of length 1" in r.stderr
    # a malformed chunk is named
    c = G.parse_case(data["chunks"][:3])
    blob = bytearray(c["data"])
    o1 = int(c["off"][1])
    blob[o1 + 4:o1 + 8] = (len(data["chunks"][1]) + 1).to_bytes(4, "little")
    bad = write_input(str(tmp_path / "bad"), [], prelude=rad.rad_prelude(["t0"], 3, L, 12, 4, 4) + bytes(blob))
    r = run(["-i", bad, "-d", "fw", "-o", str(tmp_path / "o5"), "-k"])
    assert r.returncode != 0 and "chunk 1:" in r.stderr


def test_atac_sort_accepts_a_directory_assembled_from_the_files(data, tmp_path):
    """permit_freq.bin, correction_plan.bin and permit_map.bin as generate-permit-list wrote them, in an ATAC-shaped directory (no
    multi_barcode key): `atac sort` loads them and corrects the fragments' barcodes with them"""
    ind, gpl = write_input(str(tmp_path / "in"), data["chunks"]), str(tmp_path / "gpl")
    assert run(["-i", ind, "-d", "fw", "-o", gpl, "-f", 35]).returncode == 0
    want = J.gpl_outputs(data["chunks"], "fw", "force", L, arg=35)
    corrected = [(o, t) for o, t in want["plan"] if o != t][:3]
    assert len(corrected) == 3
    dropped = next(b for recs in data["chunks"] for b, _u, _a in recs if b not in dict(want["plan"]))
    frags = [(o, [(0, 0, 100 + 10 * i, 50)]) for i, (o, _t) in enumerate(corrected)] + [(corrected[0][1], [(0, 0, 100, 50)]), (dropped, [(0, 0, 5, 50)])]
    radd = str(tmp_path / "map")
    os.makedirs(radd)
    body, _ = rad.encode_atac_chunks([frags])
    open(os.path.join(radd, "map.rad"), "wb").write(rad.rad_prelude_atac(["chr1"], [100000], 1, cblen=L) + body)
    open(os.path.join(radd, "unmapped_bc_count.bin"), "wb").write(b"")
    json.dump({"version_str": "0.18.0", "gpl_options": {"rc": False}, "num-chunks": 1}, open(os.path.join(gpl, "generate_permit_list.json"), "w"))
    for name in ("bin_recs.bin", "bin_lens.bin"):
        open(os.path.join(gpl, name), "wb").write((0).to_bytes(8, "little"))
    for use_plan in (True, False):
        if not use_plan:
            os.remove(os.path.join(gpl, "correction_plan.bin"))   # the legacy permit_map.bin then serves
        r = subprocess.run([CLI, "atac", "sort", "-i", gpl, "-r", radd, "-t", "2"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        rows = [ln.split("\t") for ln in open(os.path.join(gpl, "map.bed")).read().splitlines()]
        # the first corrected fragment and the exact one are one row of count 2; the dropped barcode's fragment is gone
        assert [(row[1], row[3], row[4]) for row in rows] == [("100", rad.int_to_seq(corrected[0][1], L), "2")] + [
            (str(100 + 10 * i), rad.int_to_seq(t, L), "1") for i, (_o, t) in enumerate(corrected) if i], rows
