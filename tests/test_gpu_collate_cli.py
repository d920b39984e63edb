"""GPU end-to-end tests of `afquant collate` in fresh child processes: generate-permit-list -> collate -> quant from a mapper
directory with no other tool.  map.collated.rad must equal the input's prelude (num_chunks = the number of cells) + the bytes of
tests/collate_judge.py; `quant` on it must write what it writes on a directory holding the judge's bytes."""
import json
import os
import shutil
import subprocess

import pytest

import collate_cases as C
import collate_judge as J
import gpl_cases as G
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")
L = 16
REFS = ["t%d" % i for i in range(100)]
T2G = [(r, "g%d" % (i // 3)) for i, r in enumerate(REFS)]


@pytest.fixture(scope="module")
def chunks():
    return G.cli_dataset(L=L)[0]


def run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)


def prelude(n_chunks, pos_bytes):
    return rad.rad_prelude(REFS, n_chunks, L, 12, 4, 4, pos_bytes=pos_bytes)


def mapper_dir(path, chunks, pos_bytes):
    os.makedirs(path)
    body, off = C.encode(chunks, 4, 4, pos_bytes)
    with open(os.path.join(path, "map.rad"), "wb") as f:
        f.write(prelude(len(chunks), pos_bytes) + body)
    with open(os.path.join(path, "unmapped_bc_count.bin"), "wb") as f:
        f.write((chunks[1][0][0]).to_bytes(8, "little") + (3).to_bytes(4, "little"))
    return str(path), body, off


def gpl_then_collate(tmp_path, chunks, ori, pos_bytes):
    rd, body, off = mapper_dir(tmp_path / "map", chunks, pos_bytes)
    out = str(tmp_path / "gpl")
    r = run("generate-permit-list", "-i", rd, "-d", ori, "-o", out, "-k")
    assert r.returncode == 0, r.stderr
    return rd, out, body, off


def quant_files(ind, tg, out):
    r = run("quant", "-i", ind, "-m", tg, "-o", out, "-r", "cr-like", "-t", 2)
    assert r.returncode == 0, r.stderr
    return [open(os.path.join(out, *p), "rb").read() for p in (("alevin", "quants_mat.mtx"), ("alevin", "quants_mat_rows.txt"), ("featureDump.txt",))]


@pytest.mark.parametrize("ori,pos_bytes", [("fw", 4), ("both", 0)])
def test_permit_list_then_collate_then_quant(tmp_path, chunks, ori, pos_bytes):
    rd, out, body, off = gpl_then_collate(tmp_path, chunks, ori, pos_bytes)
    r = run("collate", "-i", out, "-r", rd, "-t", 4, "-m", 1000, "--collation-mode", "optimized")
    assert r.returncode == 0, r.stderr
    _, bc_len, freq = rad.read_permit_freq(open(os.path.join(out, "permit_freq.bin"), "rb").read())
    corr = dict(rad.read_correction_plan(open(os.path.join(out, "correction_plan.bin"), "rb").read())["corrections"])
    cells = J.cell_order(freq)
    assert bc_len == L and len(cells) > 10
    want = J.collate(body, off, 4, 4, pos_bytes, ori, corr, cells)
    got = open(os.path.join(out, "map.collated.rad"), "rb").read()
    head = prelude(len(cells), pos_bytes)
    assert got[:len(head)] == head
    assert got[len(head):] == want["bytes"]
    assert want["nrec"] == [freq[b] for b in cells] and want["stats"]["n_kept"] == sum(freq.values())   # collate.rs:615
    if ori == "fw":
        assert want["stats"]["n_alignments_kept"] < want["stats"]["n_alignments_in"] and want["stats"]["n_compatible"] < want["stats"]["n_records"]
    j = json.load(open(os.path.join(out, "collate.json")))
    assert j["compressed_output"] is False and j["version_str"] == "0.18.0" and "collate" in j["cmd"] and set(j) == {"cmd", "version_str", "compressed_output"}
    ub = open(os.path.join(out, "unmapped_bc_count_collated.bin"), "rb").read()
    first = chunks[1][0][0]
    assert ub == ((1).to_bytes(8, "little") + corr[first].to_bytes(8, "little") + (3).to_bytes(4, "little") if first in corr else bytes(8))
    # quant reads the directory as it stands, and a directory holding the judge's bytes, alike
    tg = rad.write_quant_input_dir(str(tmp_path / "judged"), want["bytes"], len(cells), REFS, T2G, cblen=L, prelude=head, pos_bytes=pos_bytes)
    for name in ("generate_permit_list.json", "unmapped_bc_count_collated.bin"):   # (quant reads both; they were judged above)
        shutil.copy(os.path.join(out, name), str(tmp_path / "judged" / name))
    ours = quant_files(out, tg, str(tmp_path / "q_ours"))
    theirs = quant_files(str(tmp_path / "judged"), tg, str(tmp_path / "q_judged"))
    assert ours == theirs and len(ours[1].split()) == len(cells)


def test_a_kept_count_other_than_the_permit_lists_sum_leaves_no_rad(tmp_path, chunks):
    rd, out, _, _ = gpl_then_collate(tmp_path, chunks, "fw", 0)
    p = os.path.join(out, "permit_freq.bin")
    buf = bytearray(open(p, "rb").read())
    n = int.from_bytes(buf[32:40], "little")
    buf[32:40] = (n + 1).to_bytes(8, "little")   # the first entry's count
    open(p, "wb").write(bytes(buf))
    r = run("collate", "-i", out, "-r", rd)
    total = sum(rad.read_permit_freq(bytes(buf))[2].values())
    assert r.returncode == 1 and f"expected to collate {total} records but retained {total - 1}" in r.stderr, r.stderr
    assert not os.path.exists(os.path.join(out, "map.collated.rad")) and not os.path.exists(os.path.join(out, "collate.json"))
