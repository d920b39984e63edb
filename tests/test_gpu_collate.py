"""GPU tests of the collate kernels: Quantifier.collate_rad against tests/collate_judge.py on the cases of tests/collate_cases.py.
Everything is exact: the output bytes, the chunk offsets, the per-cell record counts and every stat.  Shapes derive from
collate_limits()."""
import numpy as np
import pytest

import collate_cases as C
import gpl_cases as G
from util import pkg

pytestmark = pytest.mark.gpu
BAD_INPUT, INVALID_ARG = pkg._abi.AFQ_ERR_BAD_INPUT, pkg._abi.AFQ_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def q():
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    qq = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    yield qq
    qq.close()


@pytest.fixture(scope="module")
def lim():
    return pkg.collate_limits()


def run(q, c, ori):
    obs = sorted(c["corrections"])
    q.set_aln_extra_bytes(c["pos_bytes"])
    try:
        return q.collate_rad(c["data"], c["off"], obs, [c["corrections"][b] for b in obs], c["cells"], bc_bytes=c["bc_bytes"], umi_bytes=c["umi_bytes"],
                             expected_ori=ori)
    finally:
        q.set_aln_extra_bytes(0)


def same(got, want, what=""):
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert got["nrec"].tolist() == want["nrec"], (what, "nrec")
    assert got["chunk_off"].tolist() == want["chunk_off"], (what, "chunk_off")
    gb = got["bytes"].tobytes()
    if gb != want["bytes"]:
        at = next(i for i, (x, y) in enumerate(zip(gb, want["bytes"])) if x != y)
        raise AssertionError((what, "bytes differ first at", at, gb[max(0, at - 8):at + 24].hex(), want["bytes"][max(0, at - 8):at + 24].hex()))


def check(q, lim, c, oris=C.ORIS, what=""):
    out = {}
    for ori in oris:
        w = C.want(c, ori, lim["lane_alns"])
        out[ori] = (run(q, c, ori), w)
        same(out[ori][0], w, f"{what} {ori}")
    return out


# ------------------------------------------------------------------------------------------------------------------ widths
def test_every_field_width_and_every_output_alignment(q, lim):
    """every (bc_bytes, umi_bytes) with 0 and 4 position bytes, and one case at 8; over the set, records start and end at every
    residue mod 4 of the output"""
    starts, ends = set(), set()
    shapes = [(b, u_, p) for b in C.WIDTHS for u_ in C.WIDTHS for p in (0, 4)] + [(1, 2, 8), (2, 1, 1)]
    for b, u_, p in shapes:
        c = C.widths_case(b, u_, p)
        for ori, (got, w) in check(q, lim, c, what=f"bc {b} umi {u_} pos {p}").items():
            assert w["stats"]["n_kept"] > 0 and w["stats"]["n_uncorrected"] > 0
            for s, e in C.record_spans(w["bytes"], w["chunk_off"], b, u_, p):
                starts.add(s % 4)
                ends.add(e % 4)
    assert starts == {0, 1, 2, 3} and ends == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------------------------------ tile edges
@pytest.mark.parametrize("pad", [1, 2, 3])
def test_chunks_at_unaligned_addresses(q, lim, pad):
    check(q, lim, C.alignment_case(pad), what=f"pad {pad}")


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_records_at_the_tile_edge(q, lim, delta):
    check(q, lim, C.tile_edge_case(lim, delta), what=f"tile end {delta:+d}")


@pytest.mark.parametrize("extra", [0, 1])
def test_a_chunk_of_one_tile_and_of_one_tile_and_a_byte(q, lim, extra):
    c = C.one_tile_chunk_case(lim, extra)
    assert int(c["off"][1]) == 8 + lim["parse_tile"] + extra
    check(q, lim, c, what=f"one tile + {extra}")


def test_an_alignment_list_that_crosses_the_tile_and_the_halo(q, lim):
    for d in (0, 1):   # lane_alns alignments are read from the halo; one more makes the record long
        out = check(q, lim, C.halo_case(lim, lim["lane_alns"] + d), what=f"halo {d}")
        assert out["fw"][1]["stats"]["n_long_records"] == d
        assert out["fw"][1]["stats"]["n_alignments_kept"] < out["both"][1]["stats"]["n_alignments_kept"]


# ------------------------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("pos_bytes", [0, 1, 4])
def test_every_alignment_count_and_orientation_mix(q, lim, pos_bytes):
    c = C.route_case(lim, pos_bytes, bc_bytes=1 if pos_bytes == 1 else 4)
    out = check(q, lim, c, what=f"routes pos {pos_bytes}")
    assert out["fw"][1]["stats"]["n_long_records"] > 0
    # the cases reach nk = 0, 1, na - 1, na on both routes: the judge's output holds records of those sizes
    H, A = 4 + c["bc_bytes"] + c["umi_bytes"], 4 + pos_bytes
    w = out["fw"][1]
    nks = {(e - s - H) // A for s, e in C.record_spans(w["bytes"], w["chunk_off"], c["bc_bytes"], c["umi_bytes"], pos_bytes)}
    assert {1, lim["lane_alns"] - 1, lim["lane_alns"], lim["lane_alns"] + 1, 63, 64, 65, 128, 129} <= nks and 0 not in nks


# ------------------------------------------------------------------------------------------------------------------ placement
def test_a_cell_interleaved_over_three_chunks_keeps_the_input_order(q, lim):
    c = C.interleave_case()
    got, w = check(q, lim, c, oris=["both"])["both"]
    o = int(w["chunk_off"][1]) + 8   # cell 7 is the second chunk: its UMIs ascend
    umis = []
    for s, e in C.record_spans(w["bytes"], w["chunk_off"], 4, 4, 0):
        if o <= s < int(w["chunk_off"][2]):
            umis.append(int.from_bytes(w["bytes"][s + 8:s + 12], "little"))
    assert umis == [0, 2, 4, 6, 8, 9, 12]
    check(q, lim, c, oris=["fw", "rc"])


@pytest.mark.parametrize("n_cells", [1, 2, 256, 257, 65537])
def test_one_two_and_three_radix_digits(q, lim, n_cells):
    check(q, lim, C.many_cells_case(n_cells), oris=["both"], what=f"{n_cells} cells")


def test_a_cell_larger_than_a_radix_block(q, lim):
    got, w = check(q, lim, C.big_cell_case(lim))["both"]
    assert max(w["nrec"]) > lim["radix_block"]


def test_empty_cell_cross_correction_and_the_all_ones_key(q, lim):
    out = check(q, lim, C.corrected_case())
    w = out["both"][1]
    assert w["nrec"] == [0, 3, 2] and w["chunk_off"][1] == 8 and w["stats"]["n_uncorrected"] == 1


def test_no_chunks_and_no_cells(q):
    got = q.collate_rad(b"", np.zeros(0, np.uint64), [], [], [5, 6], bc_bytes=4, umi_bytes=4)
    assert got["bytes"].tobytes() == (8).to_bytes(4, "little") * 1 + bytes(4) + (8).to_bytes(4, "little") + bytes(4)
    assert got["chunk_off"].tolist() == [0, 8, 16] and got["nrec"].tolist() == [0, 0]
    c = C.interleave_case()
    got = q.collate_rad(c["data"], c["off"], [], [], [], bc_bytes=4, umi_bytes=4)
    assert len(got["bytes"]) == 0 and got["chunk_off"].tolist() == [0] and got["stats"]["n_uncorrected"] == got["stats"]["n_records"] == 13


# ------------------------------------------------------------------------------------------------------------------ errors
@pytest.mark.parametrize("kind", ["head_cut", "alns_cut", "junk", "nrec_low", "nrec_high"])
def test_malformed_chunks_are_refused_with_their_index(q, lim, kind):
    data, off = G.malformed_case(kind)
    for ori in ("both", "fw"):
        with pytest.raises(pkg.AfqError) as e:
            q.collate_rad(data, off, [1], [1], [1], bc_bytes=4, umi_bytes=4, expected_ori=ori)
        assert e.value.code == BAD_INPUT and "chunk 2:" in str(e.value), str(e.value)
    check(q, lim, C.interleave_case(), oris=["both"])   # the context serves again afterwards


def test_a_record_count_one_too_high_is_refused_by_sentence(q):
    data, off = pkg.rad.encode_chunks([[(7, 1, [(0, True)]), (8, 2, [(1, False)])], [(7, 3, [(0, True), (1, True)]), (8, 4, [(0, False), (1, True)])]])
    o1 = int(off[1])
    bad = data[:o1 + 4] + (3).to_bytes(4, "little") + data[o1 + 8:]   # chunk 1 holds two records and says three (three heads would fit it)
    with pytest.raises(pkg.AfqError) as e:
        q.collate_rad(bad, off, [7, 8], [7, 8], [7, 8], bc_bytes=4, umi_bytes=4)
    assert e.value.code == BAD_INPUT and "chunk 1:" in str(e.value) and "the records do not tile the chunk" in str(e.value), str(e.value)


def test_bad_corrections_are_refused(q, lim):
    c = C.interleave_case()
    with pytest.raises(pkg.AfqError) as e:
        q.collate_rad(c["data"], c["off"], [7, 8], [7, 99], [7, 9], bc_bytes=4, umi_bytes=4)
    assert e.value.code == BAD_INPUT and "correction entry 1" in str(e.value) and "99" in str(e.value) and "not a cell" in str(e.value)
    one, off1 = pkg.rad.encode_chunks([[(7, 1, [(0, True)])]])   # one chunk, one record; cells 1 and 2 are the same barcode
    with pytest.raises(pkg.AfqError) as e:
        q.collate_rad(one, off1, [7], [7], [9, 7, 7], bc_bytes=4, umi_bytes=4)
    assert e.value.code == BAD_INPUT and "cells 1 and 2 carry one barcode (7)" in str(e.value), str(e.value)
    with pytest.raises(pkg.AfqError) as e:
        q.collate_rad(c["data"], c["off"], [7, 8, 7], [7, 8, 8], [7, 8], bc_bytes=4, umi_bytes=4)
    assert e.value.code == BAD_INPUT and "two different corrected barcodes" in str(e.value)
    with pytest.raises(pkg.AfqError) as e:
        q.collate_rad(c["data"], c["off"], [C.ONES, C.ONES], [7, 8], [7, 8], bc_bytes=8, umi_bytes=4)
    assert e.value.code == BAD_INPUT and "two different corrected barcodes" in str(e.value)
    with pytest.raises(pkg.AfqError) as e:
        q.collate_rad(c["data"], c["off"], [7], [7], [7, 7], bc_bytes=4, umi_bytes=4)
    assert e.value.code == BAD_INPUT and "one barcode" in str(e.value)
    with pytest.raises(pkg.AfqError) as e:
        q.collate_rad(c["data"], c["off"], [7], [7], [7], bc_bytes=3, umi_bytes=4)
    assert e.value.code == INVALID_ARG
    off = c["off"].copy()
    off[1] = len(c["data"]) - 4
    with pytest.raises(pkg.AfqError) as e:
        q.collate_rad(c["data"], off, [7], [7], [7], bc_bytes=4, umi_bytes=4)
    assert e.value.code == BAD_INPUT and "chunk 1" in str(e.value)
    q.collate_rad(c["data"], c["off"], [7, 7], [7, 7], [7], bc_bytes=4, umi_bytes=4)   # the same pair twice is no conflict
    check(q, lim, c, oris=["rc"])


@pytest.mark.parametrize("al", [0, 3])
def test_device_bytes_inside_a_larger_buffer(q, lim, al):
    """the input already on the device, starting off a dword boundary, with other bytes (all ones) in front of and behind it: they
    take no part - the last record's one-byte position ends on the input's last byte, and a long record's list is read from there"""
    import torch

    c = C.route_case(lim, 1, bc_bytes=1)
    t = torch.from_numpy(np.frombuffer(b"\xFF" * al + c["data"] + b"\xFF" * 9, np.uint8).copy()).cuda()
    obs = sorted(c["corrections"])
    q.set_aln_extra_bytes(1)
    try:
        for ori in C.ORIS:
            got = q.collate_rad(None, c["off"], obs, [c["corrections"][b] for b in obs], c["cells"], bc_bytes=1, umi_bytes=c["umi_bytes"], expected_ori=ori,
                                d_ptr=t.data_ptr() + al, n_bytes=len(c["data"]))
            same(got, C.want(c, ori, lim["lane_alns"]), f"device bytes + {al} {ori}")
    finally:
        q.set_aln_extra_bytes(0)


# ------------------------------------------------------------------------------------------------------------------ determinism
def test_two_calls_return_identical_bytes(q, lim):
    c = C.big_cell_case(lim)
    a, b = run(q, c, "fw"), run(q, c, "fw")
    assert a["bytes"].tobytes() == b["bytes"].tobytes() and np.array_equal(a["chunk_off"], b["chunk_off"]) and np.array_equal(a["nrec"], b["nrec"])
