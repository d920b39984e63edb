"""The oracle before the judge of tests/atac_dedup_judge.py, and the judge, its byte reader and the builders of
tests/atac_dedup_cases.py before answers written out by hand.  No device.

The barcode strings: needletail's text (bitkmer::bitmer_to_bytes, reverse_complement) is not on hand, so the hand-derived cells
below spell their barcodes out as literals and the judge's bc_string is also held against rad.int_to_seq, the encoder of this
package that the CLI tests have used so far."""
import ast
import os

import numpy as np
import pytest

import atac_dedup_cases as A
import atac_dedup_judge as J
from test_oracle_golden import _atac_reference_cells
from util import ROOT, pkg

rad = pkg.rad
NAMES = A.all_case_names()


# ------------------------------------------------------------------------------------------------------------------ the judge
def test_the_judge_imports_nothing_of_the_project():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "atac_dedup_judge.py")).read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or "").split(".")[0])
    assert mods == {"struct", "collections"}, mods


def test_the_references_own_vector(oracle):
    """16 cells x (5 good, 2 unmapped, 1 multi-mapped) (tests/atac_integration.rs:150-224, 531-607): 80 rows of count 1."""
    cells = _atac_reference_cells()
    want = J.judge_cells([r for _, r in cells])
    assert want.cell_ptr == list(range(0, 81, 5)) and all(c == 1 and fl == 120 and s < 500000 for _, s, fl, c in want.rows)
    assert want[2:] == (16 * 8, 16, 32, 0, 0)
    for ci, (_, recs) in enumerate(cells):
        assert [r[:3] for r in want.rows[5 * ci:5 * ci + 5]] == sorted((a[0][0], a[0][2], a[0][3]) for a in recs if len(a) == 1)
    b, off = rad.encode_atac_cells(cells)
    case = {"cells": cells, "data": np.frombuffer(b, np.uint8), "off": off, "bc_bytes": 4}
    A.same_as_judge(oracle.atac_dedup_rad(b, off), case, "oracle")


def test_hand_derived_cells():
    """Rows, tallies and BED lines written out by hand.  AACGTTTG = 00 00 01 10 11 11 11 10 = 0x06FE; its reverse complement:
    GTTTGCAA backwards, complemented = CAAACGTT."""
    recs = [[(1, 4, 100, 50)], [(0, 4, 7, 2000)], [(1, 4, 100, 50)], [(0, 4, 7, 1999)], [(1, 4, 99, 50)], [(1, 1, 100, 50)], [], [(0, 4, 7, 2001)],
            [(1, 4, 100, 50), (1, 4, 100, 50)], [(1, 4, 100, 49)], [(1, 4, 100, 50)]]
    c = J.judge_cell(recs)
    assert c.rows == [(0, 7, 1999, 1), (0, 7, 2000, 1), (0, 7, 2001, 1), (1, 99, 50, 1), (1, 100, 49, 1), (1, 100, 50, 3)]
    assert c[1:] == (11, 1, 2, 1, 2)
    assert J.bed_lines(c.rows, 0x06FE, ["chrA", "chrB"], 8, False) == [
        "chrA\t7\t2006\tAACGTTTG\t1", "chrB\t99\t149\tAACGTTTG\t1", "chrB\t100\t149\tAACGTTTG\t1", "chrB\t100\t150\tAACGTTTG\t3"]
    assert J.bed_lines(c.rows[3:4], 0x06FE, ["chrA", "chrB"], 8, True) == ["chrB\t99\t149\tCAAACGTT\t1"]
    # nothing kept: no alignment, one that is no proper pair, two of which one is
    c = J.judge_cell([[], [(0, 2, 1, 1)], [(0, 4, 1, 1), (0, 0, 1, 1)]])
    assert c == J.Cell([], 3, 1, 2, 0, 0) and J.bed_lines(c.rows, 5, ["x"], 4, True) == []
    # one record
    assert J.judge_cell([[(9, 4, 8, 7)]]) == J.Cell([(9, 8, 7, 1)], 1, 0, 0, 0, 0)
    # the count is cut to 16 bits, "deduplicated" is not (deduplicate.rs:222-226)
    one = [(2, 4, 5, 30)]
    for n, stored in ((65535, 65535), (65536, 0), (65537, 1), (131072, 0), (131074, 2)):
        c = J.judge_cell([one] * n + [[(2, 4, 5, 31)]])
        assert c.rows == [(2, 5, 30, stored), (2, 5, 31, 1)] and c.n_deduplicated == 1 and c.n_records == n + 1, n
    assert J.bed_lines([(0, 5, 30, 0)], 0, ["c"], 2, False) == ["c\t5\t35\tAA\t0"]
    # two cells: offsets and sums
    b = J.judge_cells([recs, [one, one]])
    assert b.cell_ptr == [0, 6, 7] and b.rows[6] == (2, 5, 30, 2) and b[2:] == (13, 1, 2, 2, 2)
    assert J.log_lines(b) == ["Number of records with greater than 1 mapping 1", "Number of records that are deduplicated 2",
                              "Number of records that are not mapped pairs 2", "Number of records that have frag length > 2000 2"]
    with pytest.raises(ValueError):   # start + frag_len beyond 2^32: not judged
        J.bed_lines([(0, (1 << 32) - 1, 1, 1)], 0, ["c"], 2, False)


def test_barcode_strings():
    assert J.bc_string(0x1B, 4, False) == "ACGT" and J.bc_string(0x1B, 4, True) == "ACGT"   # (its own reverse complement)
    assert J.bc_string(0, 3, False) == "AAA" and J.bc_string(0, 3, True) == "TTT"
    assert J.bc_string(0b000111, 3, False) == "ACT" and J.bc_string(0b000111, 3, True) == "AGT"
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for bc, n in ((A.WRAP_BC, 16), (0x06FE, 8), (0xFFFFFFFFFFFFFFFF, 32), (12345, 7)):
        s = rad.int_to_seq(bc, n)
        assert J.bc_string(bc, n, False) == s and J.bc_string(bc, n, True) == "".join(comp[ch] for ch in reversed(s))
    assert J.bc_string(A.WRAP_BC, 16, False) == "ACGTAGTCCATGCGAT"


# ------------------------------------------------------------------------------------------------------------ the byte reader
def test_read_chunk_on_bytes_written_out_by_hand():
    rec0 = bytes([2, 0, 0, 0, 0x34, 0x12]) + bytes([1, 0, 0, 0, 4, 0x10, 0x27, 0, 0, 0xD0, 0x07]) + bytes([0xFF, 0xFF, 0xFF, 0xFF, 0, 0xFE, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF])
    rec1 = bytes([0, 0, 0, 0, 0x34, 0x12])
    body = rec0 + rec1
    chunk = (8 + len(body)).to_bytes(4, "little") + (2).to_bytes(4, "little") + body
    assert J.read_chunk(b"\x00" * 3 + chunk, 3, 2) == (0x1234, [[(1, 4, 10000, 2000), (0xFFFFFFFF, 0, 0xFFFFFFFE, 0xFFFF)], []], 42)
    assert J.read_chunk((8).to_bytes(4, "little") + bytes(4), 0, 8) == (None, [], 8)
    with pytest.raises(ValueError):   # another barcode on the second record
        J.read_chunk(chunk[:-2] + b"\x35\x12", 0, 2)
    with pytest.raises(ValueError):   # the header claims a third record
        J.read_chunk(chunk[:4] + (3).to_bytes(4, "little") + body, 0, 2)
    with pytest.raises(ValueError):   # bytes left over
        J.read_chunk((9 + len(body)).to_bytes(4, "little") + chunk[4:] + b"\x00", 0, 2)


@pytest.mark.parametrize("name", NAMES)
def test_the_encoders_bytes_read_back_to_the_structures_the_judge_is_given(name):
    """rad.encode_atac_cells and the numpy encoder through the judge's reader: the chunks tile the buffer (behind the pad), and
    each reads back to its cell."""
    case = A.get_case(name)
    data = case["data"].tobytes()
    end = int(case["off"][0])
    assert end < 4 and len(case["off"]) == len(case["cells"]) >= 8
    for o, (bc, recs) in zip(case["off"].tolist(), case["cells"]):
        assert o == end
        got_bc, got, nbytes = J.read_chunk(data, o, case["bc_bytes"])
        assert got == recs and got_bc == (bc if recs else None)
        end = o + nbytes
    assert end == len(data)


# -------------------------------------------------------------------------------------------------- the oracle before the judge
@pytest.mark.parametrize("name", NAMES)
def test_oracle_from_bytes_before_the_judge(oracle, name):
    case = A.get_case(name)
    A.same_as_judge(oracle.atac_dedup_rad(case["data"], case["off"], bc_bytes=case["bc_bytes"]), case, "ora_atac_dedup_rad " + name)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_from_columns_before_the_judge(oracle, name):
    case = A.get_case(name)
    A.same_as_judge(oracle.atac_dedup(*A.kept_columns(case)), case, "ora_atac_dedup " + name, rows_only=True)


# ------------------------------------------------------------------------------------------------------------- the witnesses
@pytest.mark.parametrize("name", NAMES)
def test_cells_that_fail_the_walk_free_proof_are_the_ones_built_to(name):
    case = A.get_case(name)
    bad = [i for i, n in enumerate(A.false_starts(case)) if n]
    assert len(bad) == (0 if not name.startswith("fallback") else 2 if name == "fallback_4" else 1), (name, bad)
    empty = [i for i, (_, recs) in enumerate(case["cells"]) if not recs]   # (a chunk of zero records is walked too: no first record)
    assert len(empty) == (2 if name == "filter" else 0) and A.walked_cells(case) == sorted(bad + empty) and case["n_fallback"] == len(bad) + len(empty)
    assert case["wide"] == (max(r[0] for r in A.judged(case).rows) > 65535) == (name in ("packing_wide_first", "packing_wide_last"))


def test_wrap_case_reaches_the_count_wrap():
    case = A.get_case("wrap")
    runs = A.run_layout(case["cells"][0][1])
    assert tuple(n for _, n in runs if n > 1) == A.WRAP_RUNS == (65535, 65536, 65537, 131072, 131073)
    assert [n for _, n in runs[::2]] == [1] * 6 and len(runs) == 11   # an ordinary fragment before, between and after
    want = A.judged(case)
    assert tuple(c for _, _, _, c in want.rows[1:11:2]) == A.WRAP_COUNTS == (65535, 0, 1, 0, 1)
    first = J.judge_cell(case["cells"][0][1])
    assert first.n_deduplicated == 5 and first.n_records == sum(A.WRAP_RUNS) + 6 and want.cell_ptr[1] == 11
    second = J.judge_cell(case["cells"][1][1])
    assert second[1:] == (6, 1, 1, 1, 1) and want.cell_ptr[2] == 14 and want.n_deduplicated > 6
    assert len(case["data"]) < 10 << 20


def test_run_head_case_reaches_the_sweep_and_tile_edges():
    case = A.get_case("run_heads")
    layouts = [A.run_layout(r) for _, r in case["cells"][:7]]
    sizes = [sum(n for _, n in lay) for lay in layouts]
    assert sizes == list(A.RUN_HEAD_SIZES) == [(1 << 10) - 1, 1 << 10, (1 << 10) + 1, (1 << 14) - 1, 1 << 14, (1 << 14) + 1, (1 << 15) + 1]
    assert [len(r) for _, r in case["cells"][:7]] == sizes   # (every record is kept)
    assert layouts[1] == [(0, 1024)] and all(len(layouts[i]) == sizes[i] for i in (0, 4))   # one run; all distinct
    for i, runs in ((2, [(1023, 2)]), (3, [(1023, 3)]), (5, [(1023, 3), (2047, 3), (16382, 3)]), (6, [(16380, 10), (32767, 2)])):
        assert all(r in layouts[i] for r in runs), (i, runs)
        assert {n for _, n in layouts[i]} >= {1, 2} and len(layouts[i]) > sizes[i] // 3
    assert (1023, 2) in layouts[2] and 1023 + 2 == sizes[2]            # begins one before the boundary, ends with the cell
    assert any(p < 1 << 14 < p + n - 1 for p, n in layouts[6])          # spans a tile boundary of the sorted order
    assert any(p == 1023 and p + n > 1024 for p, n in layouts[3])


def test_packing_cases_hold_the_neighbours():
    frags, mult = A.packing_neighbours()
    assert sorted(frags) != frags and len(set(frags)) == len(frags)
    s = sorted(frags)
    top = (1 << 32) - 1
    for a, b in (((7, top, 65535), (8, 0, 0)), ((8, 0x00FFFFFF, 65535), (8, 0x01000000, 0)), ((8, 0, 65535), (8, 1, 0)), ((65534, top, 65535), (65535, 0, 0))):
        assert s.index(b) == s.index(a) + 1
    for kind in A.PACKING_KINDS:
        case = A.get_case("packing_" + kind)
        want = A.judged(case)
        for ci in (0, len(case["cells"]) - 1):
            rows = want.rows[want.cell_ptr[ci]:want.cell_ptr[ci + 1]]
            assert [r for r in rows if r[0] < 65536] == [f + (m,) for f, m in sorted(zip(frags, mult))]
            wide = [r for r in rows if r[0] > 65535]
            assert (wide == [(65536, 0, 0, 2), (65536, top, 65535, 1), (70000, 5, 50, 3)]) == (kind == ("wide_first", "wide_last")[ci > 0]) and (not wide or len(wide) == 3)
        assert max(r[0] for r in want.rows if r[0] < 65536) == 65535


def test_filter_case_holds_every_kind_of_record():
    case = A.get_case("filter")
    recs = case["cells"][0][1]
    assert sorted(a[0][1] for a in recs if len(a) == 1 and a[0][2:] == (50, 100)) == [0, 1, 2, 3, 4, 4, 5, 6, 7]
    assert any(len(a) == 2 and all(x[1] == 4 for x in a) for a in recs) and any(len(a) == 3 for a in recs) and [] in recs
    cells = [J.judge_cell(r) for _, r in case["cells"]]
    assert cells[0].rows == [(2, 49, 100, 1), (2, 50, 99, 1), (2, 50, 100, 2)] and cells[0][1:] == (14, 2, 8, 1, 0)
    assert cells[1].rows == [] and cells[1][1:] == (10, 1, 9, 0, 0)
    assert cells[2] == J.Cell([(9, 8, 7, 1)], 1, 0, 0, 0, 0) and cells[3] == J.Cell([], 1, 0, 1, 0, 0)
    assert cells[4] == cells[-1] == J.Cell([], 0, 0, 0, 0, 0)
    for i in (4, len(cells) - 1):   # the chunks of zero records are eight bytes
        o = int(case["off"][i])
        assert case["data"][o:o + 8].tobytes() == (8).to_bytes(4, "little") + bytes(4)
    assert int(case["off"][-1]) + 8 == len(case["data"])


@pytest.mark.parametrize("bc_bytes", A.WIDTHS)
def test_parse_cases_bracket_the_byte_groups_at_every_alignment(bc_bytes):
    tails, starts = set(), {}
    for pad in range(4):
        case = A.get_case("parse_%d_%d" % (bc_bytes, pad))
        off = case["off"].tolist()
        assert off[0] == pad
        for ci, o in enumerate(off):
            starts.setdefault(ci, set()).add(o % 4)
        sizes = [b - a for a, b in zip(off, off[1:])]
        assert sizes[:9] == list(A.PARSE_CHUNK_BYTES) == [n + d for n in (256, 512, 2048) for d in (-1, 0, 1)]
        for _, recs in case["cells"][:9]:
            assert {len(a) for a in recs} == {0, 1, 2} and any(a[0][1] != 4 for a in recs if len(a) == 1)
        single = case["cells"][case["single_cell"]][1]
        assert len(single) == 64 and all(len(a) == 1 and a[0][1] == 4 for a in single)
        if bc_bytes == 1:
            assert sizes[case["single_cell"]] == 8 + 64 * 16 and A.kept_in_one_bitmap_word(case, case["single_cell"]) == 16
        assert case["cells"][-1][1][-1] == [] and len(case["data"]) % 4 == 1 + pad % 3
        tails.add(len(case["data"]) % 4)
    assert tails == {1, 2, 3} and all(v == {0, 1, 2, 3} for v in starts.values())   # every chunk starts at each byte alignment


def test_compaction_case_holds_the_ref_runs():
    case = A.get_case("compaction")
    want = A.judged(case)
    runs = [A.ref_runs(want.rows[want.cell_ptr[ci]:want.cell_ptr[ci + 1]]) for ci in case["rows_cells"]]
    assert runs == [list(r) for r in A.COMPACTION_REF_RUNS] == [[700], [1] * 300, [1, 500, 1], [1], [1] * 320]
    assert sum(len(A.ref_runs(want.rows[a:b])) for a, b in zip(want.cell_ptr, want.cell_ptr[1:])) > 400 > sum(len(r) for r in runs[:4])
    assert want.n_deduplicated > 300


def test_cli_case_is_the_wrap_cell_and_the_length_boundary(oracle):
    case = A.cli_case()
    want = A.judged(case)
    assert want[2:] == (sum(A.WRAP_RUNS) + 6 + 6, 1, 2, 5, 2) and [r[2:] for r in want.rows[11:]] == [(1999, 1), (2000, 1), (2001, 1)]
    assert [J.read_chunk(case["data"].tobytes(), int(o), 4)[:2] for o in case["off"]] == [(bc, recs) for bc, recs in case["cells"]]
    A.same_as_judge(oracle.atac_dedup_rad(case["data"], case["off"]), case, "oracle")
    lines = J.bed_lines(want.rows[:11], A.WRAP_BC, ["a", "b", "c", "d"], 16, False)
    assert [ln.split("\t")[4] for ln in lines[1::2]] == ["65535", "0", "1", "0", "1"] and J.log_lines(want)[1].endswith("deduplicated 5")
