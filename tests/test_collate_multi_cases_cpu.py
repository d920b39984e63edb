"""Without a device: every case of tests/collate_multi_cases.py reaches the edge it names.  The shapes come from
collate_multi_limits(), not from constants here."""
import pytest

import collate_multi_cases as C
import collate_multi_judge as J
from util import pkg


@pytest.fixture(scope="module")
def lim():
    return pkg.collate_multi_limits()


def head(c):
    return 4 + c["b0_bytes"] + c["b1_bytes"] + c["umi_bytes"]


def starts(c, ci=0):
    """byte offsets, relative to the chunk's first record, of the records of chunk ci"""
    H, A, out, p = head(c), 4 + c["pos_bytes"], [], 0
    for r in c["chunks"][ci]:
        out.append(p)
        p += H + A * len(r[3])
    return out, p


def test_the_limits_are_collates(lim):
    assert lim == pkg.collate_limits() and lim["lane_alns"] >= 1 and lim["parse_halo"] >= 20 + 12 * lim["lane_alns"]


@pytest.mark.parametrize("b0", C.B_WIDTHS)
@pytest.mark.parametrize("b1", C.B_WIDTHS)
def test_width_cases_keep_drop_and_miss_at_every_width(lim, b0, b1):
    for uw in C.U_WIDTHS:
        c = C.widths_case(b0, b1, uw)
        assert any(r[0] == C.top(b0) and r[1] == C.top(b1) for recs in c["chunks"] for r in recs)
        assert {s for s, _ in c["cells"]} >= {1} and 0 not in {s for s, _ in c["cells"]}   # sample 1: header-only chunks; sample 0: skipped
        for ori in C.ORIS:
            st = C.want(c, ori, lim["lane_alns"])["stats"]
            assert st["n_kept"] > 0 and st["n_unrouted"] > 0, (ori, st)
            if ori == "both":
                assert st["n_uncorrected"] > 0 and st["n_compatible"] == st["n_records"], st
            else:
                assert st["n_compatible"] < st["n_records"] and st["n_alignments_kept"] < st["n_alignments_in"], (ori, st)


def test_alignment_cases_put_records_at_every_address_residue():
    tiles, outs = set(), set()
    for pad in range(4):
        c = C.alignment_case(pad)
        assert int(c["off"][0]) == pad
        tiles |= {(int(o) + 8) % 4 for o in c["off"]}
        w = C.want(c, "both")
        spans = C.record_spans(w["bytes"], w["chunk_off"], c)
        outs |= {s % 4 for s, _ in spans}
        # records that abut at an odd address and come from different input chunks (different waves wrote them)
        src = []
        for cell in range(len(c["cells"])):
            src.append([ci for ci, b0, b1, _, _ in J.records(c["data"], c["off"], 1, 1, 1) if b0 in c["sample_table"] and
                        (c["sample_table"][b0], b1) in c["cell_table"] and (c["sample_table"][b0], c["cell_table"][(c["sample_table"][b0], b1)]) == c["cells"][cell]])
        flat = [ci for s in src for ci in s]
        assert len(flat) == len(spans)
        assert any(a[1] == b[0] and a[1] % 2 == 1 and x != y for a, b, x, y in zip(spans, spans[1:], flat, flat[1:]))
    assert tiles == {0, 1, 2, 3} and outs == {0, 1, 2, 3}


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_edge_cases_start_a_record_on_the_last_byte_and_behind_it(lim, delta):
    c, at = C.tile_edge_case(lim, delta)
    st, total = starts(c)
    assert st[at] == lim["parse_tile"] + delta and total > lim["parse_tile"] + 8
    r = c["chunks"][0][at]
    s = c["sample_table"][r[0]]
    assert r[0] in c["sample_table"]
    if (s, r[1]) in c["cell_table"]:
        assert (s, c["cell_table"][(s, r[1])]) in c["cells"]


def test_the_one_tile_chunk_is_one_tile(lim):
    c = C.one_tile_chunk_case(lim)
    assert int(c["off"][1]) - int(c["off"][0]) == 8 + lim["parse_tile"] and starts(c)[1] == lim["parse_tile"]


def test_halo_cases_reach_the_halos_end_and_the_whole_wave_route(lim):
    for d in (0, 1):
        c, at = C.halo_case(lim, lim["lane_alns"] + d)
        st, _ = starts(c)
        r = c["chunks"][0][at]
        assert st[at] == lim["parse_tile"] - 4 and len(r[3]) == lim["lane_alns"] + d and head(c) == 20 and c["pos_bytes"] == 8
        assert 4 + head(c) + 12 * lim["lane_alns"] <= lim["parse_halo"] + 4
        w = C.want(c, "fw", lim["lane_alns"])
        assert w["stats"]["n_long_records"] == d
        cell = c["cells"].index((c["sample_table"][r[0]], 0xFFFFFFFF))
        assert w["nrec"][cell] >= 1


@pytest.mark.parametrize("where", ["first", "last", "absent"])
def test_long_cases_hold_a_kept_a_dropped_an_unrouted_and_an_uncorrected_long_record(lim, where):
    c = C.long_case(where)
    longs = [r for recs in c["chunks"] for r in recs if len(r[3]) > 64 * 30]
    assert len(longs) == 4 and all(len(r[3]) > lim["lane_alns"] for r in longs)
    kept, decoy, uncorr, unrouted = longs
    assert (c["sample_table"][kept[0]], kept[1]) in c["cell_table"] and (c["sample_table"][uncorr[0]], uncorr[1]) not in c["cell_table"]
    assert unrouted[0] not in c["sample_table"] and not any(fw for _, fw in decoy[3]) and (c["sample_table"][decoy[0]], decoy[1]) in c["cell_table"]
    fw = C.want(c, "fw", lim["lane_alns"])
    if where == "last":
        assert [j for j, (_, f) in enumerate(kept[3]) if f] == [len(kept[3]) - 1] and len(kept[3]) - 1 >= 64
    assert fw["nrec"][c["cells"].index((2, 2))] == (1 if where == "absent" else 2)   # (12, 0, ...) of chunk 0, and the long one unless no word fits
    assert fw["stats"]["n_long_records"] == 5


@pytest.mark.parametrize("pos_bytes", [4, 8])
def test_the_route_case_stores_position_bytes_beyond_the_first_trip_behind_earlier_fitting_words(lim, pos_bytes):
    c = C.route_case(lim, pos_bytes)
    flat = [r for recs in c["chunks"] for r in recs]
    assert [len(recs) == 1 for recs in c["chunks"]] == [False, True, False] and c["pos_bytes"] == pos_bytes
    assert {len(r[3]) for r in flat} == set(C.CC.route_nas(lim)) and [r[2] for r in flat] == list(range(len(flat)))
    first = {}   # the file-wide number of every record's first alignment: the encoder's position bytes count alignments
    n = 0
    for r in flat:
        first[r[2]] = n
        n += len(r[3])
    fate = lambda r: C.ROUTE_FATES[r[2] % 4]
    for f in C.ROUTE_FATES:   # every fate on a long record of each pattern family, and on a record without alignments or with one
        assert any(fate(r) == f and len(r[3]) > 64 for r in flat) and any(fate(r) == f and len(r[3]) <= 1 for r in flat), f
    H, A = head(c), 4 + pos_bytes
    for ori in ("fw", "rc"):
        w = C.want(c, ori, lim["lane_alns"])
        st = w["stats"]
        assert st["n_unrouted"] > 0 and st["n_uncorrected"] > 0 and all(x > 0 for i, x in enumerate(w["nrec"]) if c["cells"][i][0] == 2), (ori, st)
        assert w["nrec"][c["cells"].index((1, 10))] == 0
        cell = c["cells"].index((2, 10))
        by_umi = {int.from_bytes(w["bytes"][s + H - c["umi_bytes"]:s + H], "little"): s for s, _ in C.record_spans(w["bytes"], w["chunk_off"], c)
                  if w["chunk_off"][cell] <= s < w["chunk_off"][cell + 1]}
        reached = 0
        for r in flat:
            fit = [j for j, (_, fw) in enumerate(r[3]) if fw == (ori == "fw")]
            if fate(r) != "kept" or len(r[3]) <= 64 or not fit:
                continue
            s = by_umi[r[2]]
            assert int.from_bytes(w["bytes"][s:s + 4], "little") == len(fit)
            for rank, j in enumerate(fit):
                word = ((100 + j) | (0x80000000 if r[3][j][1] else 0)).to_bytes(4, "little")
                at = s + H + A * rank
                assert w["bytes"][at:at + A] == word + C.CC.position(first[r[2]] + j, pos_bytes), (ori, r[2], j)
                reached += j >= 64 and rank > 0 and fit[0] < 64   # base > 0 in its trip and rank > 0
        assert reached >= 2, ori
    # kept records with 0, 1, na - 1 and na fitting words beyond one trip
    for ori in ("fw", "rc"):
        counts = {(len(r[3]), sum(1 for _, fw in r[3] if fw == (ori == "fw"))) for r in flat if r[2] % 4 < 2 and len(r[3]) > 64}
        assert {k for na, k in counts if na == 129} >= {0, 1, 128, 129}, (ori, counts)


def test_records_without_alignments_are_kept_under_both_only(lim):
    c = C.no_alignment_case()
    both, fw, rc = (C.want(c, o)["stats"] for o in C.ORIS)
    n0 = sum(1 for recs in c["chunks"] for r in recs if not r[3])
    assert n0 >= 4 and both["n_compatible"] == both["n_records"] and fw["n_compatible"] + rc["n_compatible"] == both["n_records"] - n0
    assert both["n_kept"] > fw["n_kept"] + rc["n_kept"]


def test_the_lookup_case_tells_the_samples_apart():
    c = C.lookup_case()
    w = C.want(c, "both")
    assert c["b0_out"] == {0: 0, 1: 1, 2: 2, 4: 3} and all(b0 != s and b0 != c["b0_out"].get(s) for b0, s in c["sample_table"].items())
    cell = {k: w["nrec"][i] for i, k in enumerate(c["cells"])}
    assert cell == {(0, 0xFFFFFFFF): 1, (1, 0xA1): 2, (1, 0xC0FFEE): 1, (2, 5): 0, (2, 6): 0, (4, 0xB4): 2, (4, 0xC0FFEE): 2}
    assert w["stats"]["n_unrouted"] == 1 and w["stats"]["n_uncorrected"] == 3   # (1, 0x99), (3, 5), (0, 0x77)
    # a key that ignored the sample would send (501, 0x77) and (0, 0x77) to one cell
    assert c["cell_table"][(1, 0x77)] != c["cell_table"][(4, 0x77)]


def test_the_chain_case_wraps_both_tables():
    c, b0c, b0m, b1c, b1m = C.chain_case()
    scap = pkg.atac_sort_table_slot(0, len(c["sample_table"]))[1]
    ccap = pkg.atac_sort_table_slot(0, len(c["cell_table"]))[1]
    assert all(pkg.atac_sort_table_slot(b, len(c["sample_table"])) == (scap - 1, scap) for b in b0c + b0m)
    assert all(pkg.atac_sort_table_slot((3 << 32) | b, len(c["cell_table"])) == (ccap - 1, ccap) for b in b1c + b1m)
    assert all(b in c["sample_table"] for b in b0c) and not any(b in c["sample_table"] for b in b0m)
    assert all((3, b) in c["cell_table"] for b in b1c) and not any((3, b) in c["cell_table"] for b in b1m)
    seen = {(r[0], r[1]) for recs in c["chunks"] for r in recs}
    assert {(b0c[-1], b) for b in b1c + b1m} <= seen and {(b, b1c[0]) for b in b0c + b0m} <= seen
    st = C.want(c, "both")["stats"]
    assert st["n_unrouted"] == 2 * 3 and st["n_uncorrected"] == len(b0c) + 2 and st["n_kept"] > 10


@pytest.mark.parametrize("n_cells,passes", [(255, 1), (256, 2), (257, 2), (65537, 3)])
def test_many_cells_cases_take_one_two_and_three_digit_passes(n_cells, passes):
    c, hit = C.many_cells_case(n_cells)
    assert len(c["cells"]) == n_cells and {0, n_cells - 1} <= set(hit)
    n = 0
    while n_cells >> (8 * n):   # the digits of the word a dropped record carries (n_cells)
        n += 1
    assert n == passes
    w = C.want(c, "both")
    assert w["nrec"][0] > 1 and w["nrec"][-1] > 1 and w["stats"]["n_uncorrected"] == 1 and sum(w["nrec"]) < 1000


def test_placement_cases(lim):
    c = C.big_cell_case(lim)
    w = C.want(c, "both")
    assert w["nrec"] == [lim["radix_block"] + 100, 0] and len(c["chunks"][0]) < lim["radix_block"] < w["stats"]["n_records"]
    c = C.interleave_case()
    w = C.want(c, "both")
    spans = C.record_spans(w["bytes"], w["chunk_off"], c)
    umis = [int.from_bytes(w["bytes"][s + 10:s + 14], "little") for s, _ in spans if w["chunk_off"][1] <= s < w["chunk_off"][2]]
    assert umis == [0, 2, 4, 6, 8, 9, 12]


@pytest.mark.parametrize("kind", C.MALFORMED_KINDS)
def test_malformed_cases_do_not_tile(kind):
    data, off = C.malformed_case(kind)
    with pytest.raises(AssertionError):
        list(J.records(data, off, 2, 2, 4))
    list(J.records(data, [off[0], off[1], off[3]], 2, 2, 4))
