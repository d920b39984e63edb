"""GPU end-to-end tests of compressed collate output, every step in a fresh child process: the permit-list step, then
collate(compress=True) / atac_collate(compress=True) / collate_multi(compress=True) into one directory and the plain command into a
sibling copy of it.  map.collated.rad.sz - two snappy frame streams back to back, the prelude's and the chunks' - must decode to
exactly the sibling's map.collated.rad, before tests/snappy_judge.py and before the library's decoder; collate.json differs in
compressed_output alone; and what reads the directory next (`quant`, `atac deduplicate`) writes the same files from either."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import snappy_judge as sj
import test_gpu_atac_collate_cli as AT
import test_gpu_collate_cli as CT
from test_gpu_snappy import lib_decode
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
TESTS = os.path.join(ROOT, "tests")
PRE = f"import importlib, os, shutil, sys\nsys.path[:0] = [{ROOT!r}, {TESTS!r}]\npkg = importlib.import_module('alevin-fry_amd')\n"


def child(code, *argv):
    """a fresh Python process with the package imported as `pkg`"""
    return subprocess.run([sys.executable, "-c", PRE + code] + [str(a) for a in argv], capture_output=True, text=True)


@pytest.fixture(scope="module")
def chunks():
    return CT.G.cli_dataset(L=CT.L)[0]


def same_but_compressed(sz_dir, plain_dir, extra_keys=()):
    """the .sz against the sibling's plain file, the JSON, the absence of a plain file; returns the plain RAD"""
    want = open(os.path.join(plain_dir, "map.collated.rad"), "rb").read()
    got = open(os.path.join(sz_dir, "map.collated.rad.sz"), "rb").read()
    assert not os.path.exists(os.path.join(sz_dir, "map.collated.rad")) and not os.path.exists(os.path.join(plain_dir, "map.collated.rad.sz"))
    s = sj.decode(got)
    assert s.data == want and s.n_identifiers == 2, "prelude stream + chunk stream"
    assert got[:10] == sj.STREAM_ID
    assert lib_decode(got, len(want)) == want
    # the first stream is the prelude's alone: the second identifier stands where the chunks' stream begins
    at = got.index(sj.STREAM_ID, 10)
    head = sj.decode(got[:at]).data
    assert want.startswith(head) and sj.decode(got[at:]).data == want[len(head):]
    jz, jp = (json.load(open(os.path.join(d, "collate.json"))) for d in (sz_dir, plain_dir))
    assert set(jz) == set(jp) >= {"cmd", "version_str", "compressed_output"} | set(extra_keys)
    assert jz["compressed_output"] is True and jp["compressed_output"] is False
    assert {k: v for k, v in jz.items() if k not in ("cmd", "compressed_output")} == {k: v for k, v in jp.items() if k not in ("cmd", "compressed_output")}
    for name in ("unmapped_bc_count_collated.bin",) + tuple(extra_keys and ("collation_manifest.bin",)):
        assert open(os.path.join(sz_dir, name), "rb").read() == open(os.path.join(plain_dir, name), "rb").read(), name
    return want


def write_t2g(path):
    with open(path, "w") as f:
        f.write("".join(f"{r}\t{g}\n" for r, g in CT.T2G))
    return str(path)


@pytest.mark.parametrize("ori,pos_bytes", [("fw", 4), ("both", 0)])
def test_permit_list_then_compressed_collate_then_quant(tmp_path, chunks, ori, pos_bytes):
    rd, out, body, off = CT.gpl_then_collate(tmp_path, chunks, ori, pos_bytes)
    plain = str(tmp_path / "gpl_plain")
    shutil.copytree(out, plain)
    r = child("print(pkg.collate(sys.argv[1], sys.argv[2], compress=True, cmdline='collate -c'))", out, rd)
    assert r.returncode == 0, r.stderr
    p = CT.run("collate", "-i", plain, "-r", rd)
    assert p.returncode == 0, p.stderr
    want = same_but_compressed(out, plain)
    head = CT.prelude(0, pos_bytes)
    tg = write_t2g(tmp_path / "t2g.tsv")
    assert CT.quant_files(out, tg, str(tmp_path / "q_sz")) == CT.quant_files(plain, tg, str(tmp_path / "q_plain"))
    # the stats the Python door returns are the uncompressed call's
    assert f"'out_bytes': {len(want) - len(head)}" in r.stdout, r.stdout


def test_a_kept_count_other_than_the_permit_lists_sum_leaves_no_sz(tmp_path, chunks):
    rd, out, _, _ = CT.gpl_then_collate(tmp_path, chunks, "fw", 0)
    p = os.path.join(out, "permit_freq.bin")
    buf = bytearray(open(p, "rb").read())
    n = int.from_bytes(buf[32:40], "little")
    buf[32:40] = (n + 1).to_bytes(8, "little")   # the first entry's count
    open(p, "wb").write(bytes(buf))
    r = child("pkg.collate(sys.argv[1], sys.argv[2], compress=True)", out, rd)
    total = sum(rad.read_permit_freq(bytes(buf))[2].values())
    assert r.returncode == 1 and f"expected to collate {total} records but retained {total - 1}" in r.stderr, r.stderr
    for name in ("map.collated.rad.sz", "map.collated.rad", "collate.json"):
        assert not os.path.exists(os.path.join(out, name)), name


def test_compressed_atac_collate_then_atac_deduplicate(tmp_path):
    chunks, freq, corr, unmapped = AT.dataset(35, idle_cells=2)
    ind, rd, head, body, off = AT.write_dirs(tmp_path, chunks, freq, corr, unmapped)
    plain = str(tmp_path / "gpl_plain")
    shutil.copytree(ind, plain)
    r = child("print(pkg.atac_collate(sys.argv[1], sys.argv[2], compress=True, cmdline='atac collate -c'))", ind, rd)
    assert r.returncode == 0, r.stderr
    p = AT.run("atac", "collate", "-i", plain, "-r", rd)
    assert p.returncode == 0, p.stderr
    same_but_compressed(ind, plain)
    logs = []
    for d in (ind, plain):
        q = AT.run("atac", "deduplicate", "-i", d, "-t", 3, "-d", "fw")
        assert q.returncode == 0, q.stderr
        logs.append([ln for ln in q.stderr.splitlines() if ln.startswith(("finished parsing", "Number of records"))])
    assert logs[0] == logs[1] and len(logs[0]) == 5
    beds = [sorted(open(os.path.join(d, "map.bed")).read().splitlines()) for d in (ind, plain)]
    assert beds[0] == beds[1] and len(beds[0]) > 200


def test_compressed_atac_collate_with_no_record_kept(tmp_path):
    """no cell keeps a record: the chunk stream is the identifier alone behind the prelude's stream"""
    chunks, freq, corr, _ = AT.dataset(34)
    ind, rd, head, body, off = AT.write_dirs(tmp_path, chunks, {}, {}, None)
    r = child("pkg.atac_collate(sys.argv[1], sys.argv[2], compress=True)", ind, rd)
    assert r.returncode == 0, r.stderr
    got = open(os.path.join(ind, "map.collated.rad.sz"), "rb").read()
    assert got.endswith(sj.STREAM_ID) and sj.decode(got).data == rad.rad_prelude_atac(AT.NAMES, AT.REF_LEN, 0, cblen=AT.L)


MULTI = """
import collate_multi_judge as J
import gpl_multi_cases as MC
d = sys.argv[1]
chunks, rows, kinds, cells = MC.chain_dataset()
in_dir = MC.write_chain_dir(os.path.join(d, "map"), chunks)
valid, white = MC.chain_lists(cells)
paths = {"forward": os.path.join(d, "samples.tsv"), "unfiltered": os.path.join(d, "white.txt")}
open(paths["forward"], "w").write(MC.sample_rows(rows, False))
open(paths["unfiltered"], "w").write("".join(MC.seq(b, 16) + "\\n" for b in white))
for name in ("knee_exact", "force_frequency", "unfiltered_unique"):
    case = next(c for c in MC.CHAIN_CASES if c["name"] == name)
    o = os.path.join(d, "out_" + name)
    kw = {k: v for k, v in case.items() if k != "name"}
    kw.setdefault("expected_ori", "fw")
    pkg.generate_permit_list_multi(in_dir, o, paths["forward"], list_file=paths.get(case["method"]), **kw)
    want = J.from_directory(o, os.path.join(in_dir, "map.rad"), cmdline="x", lane_alns=pkg.collate_multi_limits()["lane_alns"])
    if min(want["nrec"]) == 0:
        continue   # (quant refuses an empty chunk)
    shutil.copytree(o, o + "_plain")
    a = pkg.collate_multi(o, in_dir, cmdline="collate_multi -c", compress=True)
    b = pkg.collate_multi(o + "_plain", in_dir, cmdline="collate_multi")
    assert a == b == want["stats"], (a, b)
    print("CHOSEN " + o)
    break
"""


def test_compressed_multi_barcode_collate_then_quant(tmp_path):
    r = child(MULTI, tmp_path)
    assert r.returncode == 0, r.stderr
    chosen = [ln.split(" ", 1)[1] for ln in r.stdout.splitlines() if ln.startswith("CHOSEN ")]
    assert len(chosen) == 1, r.stdout
    o = chosen[0]
    same_but_compressed(o, o + "_plain", extra_keys=("multi_barcode", "num_samples"))
    tg = str(tmp_path / "t2g.tsv")
    with open(tg, "w") as f:
        f.write("".join(f"t{i}\tG{i % 10}\n" for i in range(100)))
    assert CT.quant_files(o, tg, str(tmp_path / "q_sz")) == CT.quant_files(o + "_plain", tg, str(tmp_path / "q_plain"))
