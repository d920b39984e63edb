"""The multi-barcode collate judge (tests/collate_multi_judge.py) on hand-made vectors of a few records each; the expected bytes are
written out literally.  Then the identity afq_collate_multi relies on: on the GPL judge's own output, every sample keeps exactly the
sum of its permit_freq.bin counts, for every filter method."""
import json
import os

import pytest

import collate_multi_judge as J
import gpl_multi_cases as MC
from util import pkg

rad = pkg.rad
FW = 0x80000000


def le(v, n):
    return int(v).to_bytes(n, "little")


def words(*ws):
    return b"".join(le(w, 4) for w in ws)


def two_chunk_input():
    """1-byte b0, 2-byte b1, 1-byte UMI.  Records (b0, b1, umi, words):
      chunk 0: (7, 0x0101, 1, [fw 5, rc 6])  (9, 0x0202, 2, [rc 7])  (7, 0x0303, 3, [])
      chunk 1: (8, 0x0101, 4, [fw 8])        (7, 0x0404, 5, [fw 9, fw 10])   (8, 0x0101, 6, [rc 11])"""
    r = lambda b0, b1, umi, *ws: le(len(ws), 4) + le(b0, 1) + le(b1, 2) + le(umi, 1) + words(*ws)
    c0 = r(7, 0x0101, 1, FW | 5, 6) + r(9, 0x0202, 2, 7) + r(7, 0x0303, 3)
    c1 = r(8, 0x0101, 4, FW | 8) + r(7, 0x0404, 5, FW | 9, FW | 10) + r(8, 0x0101, 6, 11)
    buf = le(8 + len(c0), 4) + le(3, 4) + c0 + le(8 + len(c1), 4) + le(3, 4) + c1
    return buf, [0, 8 + len(c0)]


# b0 7 -> sample 2, b0 8 -> sample 5; 9 has no sample.  Sample 2: 0x0101 -> cell 0x0111, 0x0303 -> cell 0x0303; 0x0404 has no correction.
# Sample 5: 0x0101 -> cell 0x0101 (the same observed barcode as in sample 2, another cell).
TABLES = dict(sample_table={7: 2, 8: 5}, cell_table={(2, 0x0101): 0x0111, (2, 0x0303): 0x0303, (5, 0x0101): 0x0101},
              cells=[(5, 0x0101), (2, 0x0303), (2, 0x0111), (2, 0x0999)], b0_out={2: 0, 5: 1})


def run(ori):
    buf, off = two_chunk_input()
    return J.collate_multi(buf, off, 1, 2, 1, ori, lane_alns=1, **TABLES)


def test_both_keeps_every_routed_and_corrected_record_with_all_its_alignments():
    got = run("both")
    rec = lambda na, b0, b1, umi, *ws: le(na, 4) + le(b0, 1) + le(b1, 2) + le(umi, 1) + words(*ws)
    cell0 = rec(1, 1, 0x0101, 4, FW | 8) + rec(1, 1, 0x0101, 6, 11)
    cell1 = rec(0, 0, 0x0303, 3)
    cell2 = rec(2, 0, 0x0111, 1, FW | 5, 6)
    want = le(8 + len(cell0), 4) + le(2, 4) + cell0 + le(8 + len(cell1), 4) + le(1, 4) + cell1 + le(8 + len(cell2), 4) + le(1, 4) + cell2 + le(8, 4) + le(0, 4)
    assert got["bytes"] == want
    assert got["bytes"].hex() == ("20000000" "02000000" "01000000" "01" "0101" "04" "08000080" "01000000" "01" "0101" "06" "0b000000"
                                  "10000000" "01000000" "00000000" "00" "0303" "03"
                                  "18000000" "01000000" "02000000" "00" "1101" "01" "05000080" "06000000"
                                  "08000000" "00000000")
    assert got["chunk_off"] == [0, 32, 48, 72, 80] and got["nrec"] == [2, 1, 1, 0]
    assert got["stats"] == dict(n_records=6, n_compatible=6, n_unrouted=1, n_uncorrected=1, n_kept=4, n_alignments_in=7, n_alignments_kept=4, n_long_records=2,
                                out_bytes=80)


def test_fw_cuts_the_reverse_words_and_drops_records_without_a_forward_one():
    got = run("fw")
    assert got["bytes"].hex() == ("14000000" "01000000" "01000000" "01" "0101" "04" "08000080"
                                  "08000000" "00000000"
                                  "14000000" "01000000" "01000000" "00" "1101" "01" "05000080"
                                  "08000000" "00000000")
    assert got["nrec"] == [1, 0, 1, 0] and got["chunk_off"] == [0, 20, 28, 48, 56]
    assert got["stats"] == dict(n_records=6, n_compatible=3, n_unrouted=0, n_uncorrected=1, n_kept=2, n_alignments_in=7, n_alignments_kept=2, n_long_records=2,
                                out_bytes=56)


def test_rc_keeps_the_words_with_bit_31_clear():
    got = run("rc")
    assert got["bytes"].hex() == ("14000000" "01000000" "01000000" "01" "0101" "06" "0b000000"
                                  "08000000" "00000000"
                                  "14000000" "01000000" "01000000" "00" "1101" "01" "06000000"
                                  "08000000" "00000000")
    assert got["stats"]["n_compatible"] == 3 and got["stats"]["n_unrouted"] == 1 and got["stats"]["n_kept"] == 2


def test_the_plan_parser_reads_what_the_gpl_judge_writes():
    import gpl_multi_judge as M

    spec = ("hamming-1", ("frequency", (39, 40), 1))
    buf = M.plan_bytes(8, 16, spec, {5: 4, 6: 4, 9: 9}, ("hamming-1", "unique"), [(9, [(100, 101)]), (4, [(7, 7), (8, 7)])])
    p = J.parse_plan(buf)
    assert p == {"sample_len": 8, "cell_len": 16, "sample": [(5, 4), (6, 4), (9, 9)], "scopes": [(4, [(7, 7), (8, 7)]), (9, [(100, 101)])]}
    assert J.parse_plan(M.plan_bytes(8, 16, None, {}, ("hamming-1", "unique"), []))["scopes"] == []
    with pytest.raises(AssertionError):
        J.parse_plan(buf + b"\0")
    with pytest.raises(AssertionError):
        J.parse_plan(rad.correction_plan_bytes([(1, 1)]))   # a global-scope plan


def write_gpl_dir(path, want):
    """the GPL judge's outputs as the files afq_generate_permit_list_multi writes"""
    os.makedirs(path, exist_ok=True)
    for sdir, pmap, pfreq in want["samples"]:
        os.makedirs(os.path.join(path, sdir), exist_ok=True)
        if pfreq is not None:
            with open(os.path.join(path, sdir, "permit_freq.bin"), "wb") as f:
                f.write(rad.permit_freq_bytes(16, pfreq.items()))
    with open(os.path.join(path, "correction_plan.bin"), "wb") as f:
        f.write(want["plan"])
    for name in ("sample_info", "generate_permit_list"):
        with open(os.path.join(path, name + ".json"), "w") as f:
            json.dump(want[name], f)
    return path


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    chunks, rows, kinds, cells = MC.chain_dataset()
    d = tmp_path_factory.mktemp("flexj")
    return {"chunks": chunks, "rows": rows, "cells": cells, "root": d, "rad": os.path.join(MC.write_chain_dir(str(d / "map"), chunks), "map.rad")}


@pytest.mark.parametrize("case", MC.CHAIN_CASES, ids=lambda c: c["name"])
def test_every_sample_keeps_its_collatable_reads_on_the_gpl_judges_output(chain, case):
    """the count check of afq_collate_multi is an identity on the GPL step's own output, under every filter method"""
    want = MC.chain_want(case, chain["chunks"], chain["rows"], chain["cells"], list_file="x")
    out = J.from_directory(write_gpl_dir(str(chain["root"] / case["name"]), want), chain["rad"])
    info = {e["name"]: e for e in want["sample_info"]["samples"]}
    assert [g[1] for g in out["groups"]] == ["alpha", "beta"]   # gamma, the sample without a read, has no group
    for g, kept in zip(out["groups"], out["kept_per_group"]):
        assert kept == g[4] == info[g[1]]["collatable_reads"] > 0, (g[1], kept, g[4])
        assert g[3] == info[g[1]]["num_cells"]
    st = out["stats"]
    assert st["n_kept"] == sum(out["kept_per_group"]) and st["n_compatible"] == st["n_kept"] + st["n_unrouted"] + st["n_uncorrected"]
    assert st["n_unrouted"] > 0 and len(out["cells"]) == want["total_cells"]
