"""Without a device: every builder of tests/gpl_multi_cases.py reaches what it claims - the byte positions relative to the parse tile,
the routes, the shapes of the two tables, the kinds of sample barcode in the whole step's experiment - so that
tests/test_gpu_gpl_multi.py and tests/test_gpu_gpl_multi_chain.py run the kernels and the host where they can go wrong.  These are
conditions on the cases, checked here on the CPU; nothing is measured."""
import pytest

import gpl_judge as J
import gpl_multi_cases as MC
import gpl_multi_judge as M
from util import pkg


@pytest.fixture(scope="module")
def lim():
    L = pkg.gpl_multi_limits()
    assert L == pkg.gpl_limits()   # the walk is the single-barcode parse's
    assert L["parse_tile"] >= 256 and L["parse_halo"] >= 20 + 12 * L["lane_alns"] and L["lane_alns"] >= 2
    return L


def record_offsets(case, chunk=0):
    """byte offset of every record of a chunk relative to the chunk's first record byte, and the end of the last"""
    offs, q = [], 0
    for _b0, _b1, _umi, alns in case["chunks"][chunk]:
        offs.append(q)
        q += MC.rec_size(len(alns), case, case["pos_bytes"])
    return offs, q


def test_encoder_writes_b0_b1_umi_in_tag_order():
    one = MC.multi_case([[(0xA1B2, 0xC3, 0x11, [(5, True), (6, False)])]], [0xA1B2], 2, 1, 1, pos_bytes=2)
    assert one["data"][8:] == bytes([2, 0, 0, 0, 0xB2, 0xA1, 0xC3, 0x11, 5, 0, 0, 0x80, 0, 0, 6, 0, 0, 0, 0, 0])
    c = MC.widths_case(2, 4, 8)
    for i, recs in enumerate(c["chunks"]):
        o = int(c["off"][i])
        nb, nr = int.from_bytes(c["data"][o:o + 4], "little"), int.from_bytes(c["data"][o + 4:o + 8], "little")
        assert nr == len(recs) and nb == 8 + record_offsets(c, i)[1]
    assert [len(r) for r in c["chunks"]] == [41, 1, 44]


@pytest.mark.parametrize("b0_bytes", MC.B_WIDTHS)
@pytest.mark.parametrize("b1_bytes", MC.B_WIDTHS)
def test_width_cases_hold_the_edge_values_on_both_sides(b0_bytes, b1_bytes):
    t0, t1 = MC.top(b0_bytes), MC.top(b1_bytes)
    for ub in MC.U_WIDTHS:
        for edges in ("entries", "misses"):
            c = MC.widths_case(b0_bytes, b1_bytes, ub, edges)
            recs = [r for ch in c["chunks"] for r in ch]
            assert ({0, t0} <= set(c["entries"])) == (edges == "entries") and {0, t0} <= {r[0] for r in recs}
            assert (t0, t1) in {(r[0], r[1]) for r in recs} and (0, 0) in {(r[0], r[1]) for r in recs}   # the all-ones pair (4 + 4 included)
            assert 0 in {len(r[3]) for r in recs} and max(len(r[3]) for r in recs) == 5
            w = {o: MC.want_pairs(c, o)["stats"] for o in MC.ORIS}
            assert w["both"]["n_compatible"] == w["both"]["n_records"] > w["fw"]["n_compatible"] > 0 < w["rc"]["n_compatible"]
            assert all(s["n_routed"] > 0 and s["n_unrouted"] > 0 for s in w.values())


def test_alignment_cases_cover_every_byte_alignment():
    seen = set()
    for pad in range(4):
        c = MC.alignment_case(pad)
        assert int(c["off"][0]) == pad
        seen |= {int(o) % 4 for o in c["off"]}
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_edge_cases_end_where_they_say(lim, delta):
    c, k = MC.tile_edge_case(lim, delta)
    offs, end = record_offsets(c)
    assert offs[k] == lim["parse_tile"] + delta and end > lim["parse_tile"] + 20   # a second tile follows
    assert c["chunks"][0][k][0] in c["entries"]                                   # the record at the edge is routed
    if delta == 1:
        assert offs[k - 1] < lim["parse_tile"] < offs[k]                          # the tile's last record straddles its end


def test_halo_cases_start_on_the_tiles_last_bytes_with_the_widest_fields(lim):
    for d in (0, 1):
        c, k = MC.halo_case(lim, lim["lane_alns"] + d)
        offs, _ = record_offsets(c)
        rec = c["chunks"][0][k]
        assert (c["b0_bytes"], c["b1_bytes"], c["umi_bytes"], c["pos_bytes"]) == (4, 4, 8, 8)
        assert offs[k] == lim["parse_tile"] - 4 and len(rec[3]) == lim["lane_alns"] + d and rec[:2] == (0xFFFFFFFF, 0xFFFFFFFF) and rec[0] in c["entries"]
        assert [fw for _r, fw in rec[3]] == [False] * (lim["lane_alns"] + d - 1) + [True]   # only the LAST alignment fits fw
        if d == 0:   # the whole record is staged: it ends inside tile + halo
            assert offs[k] + MC.rec_size(len(rec[3]), c, 8) <= lim["parse_tile"] + lim["parse_halo"]
        assert sum(len(r[3]) > lim["lane_alns"] for r in c["chunks"][0]) == d


@pytest.mark.parametrize("where", ["first", "last", "absent"])
def test_long_cases(lim, where):
    c = MC.long_case(where)
    longs = [r for ch in c["chunks"] for r in ch if len(r[3]) > lim["lane_alns"]]
    assert len(longs) == 5 and sum(r[0] not in c["entries"] for r in longs) == 1
    e12 = c["entries"].index(12)
    for ori, cell in (("fw", 2), ("rc", 8)):   # the record whose only fitting word is first, last or absent, under either orientation
        w = MC.want_pairs(c, ori)
        assert ((e12, cell) in set(zip(w["entry"].tolist(), w["cell"].tolist()))) == (where != "absent"), ori
    w = MC.want_pairs(c, "fw")
    assert (e12, 4) not in set(zip(w["entry"].tolist(), w["cell"].tolist()))   # the longest record has no forward alignment


def test_malformed_bytes_have_the_two_barcode_head():
    import gpl_cases as G
    good = G.parse_case([[(0x00020001, 7, [(1, True)])]], 4, 4)
    same = MC.multi_case([[(1, 2, 7, [(1, True)])]], [1], 2, 2, 4)
    assert good["data"] == same["data"]   # a 4-byte barcode reads as b0 (low half) and b1 of 2 bytes each: one head, one walk
    for kind in ("head_cut", "alns_cut", "junk", "nrec_low", "nrec_high"):
        data, off = MC.malformed_case(kind)
        assert len(off) == 4


def test_entry_table_cases():
    for n, cap in ((0, 2), (1, 2), (64, 128), (65, 256)):
        c = MC.n_entries_case(n)
        assert len(c["entries"]) == n and pkg.atac_sort_table_slot(0, n)[1] == cap
        if n:
            hit = {r[0] for ch in c["chunks"] for r in ch} & set(c["entries"])
            assert {c["entries"][0], c["entries"][-1]} <= hit
    for wrap in (False, True):
        c, chain, misses, cap, slot = MC.entry_chain_case(wrap)
        assert len(chain) == 6 and len(c["entries"]) == 48 and cap == 128 and (slot == cap - 1) == wrap
        assert all(pkg.atac_sort_table_slot(b, 48)[0] == slot for b in chain + misses) and not set(misses) & set(c["entries"])
        seen = {r[0] for ch in c["chunks"] for r in ch}
        assert set(chain) | set(misses) <= seen   # six entries share one home slot: five of them sit behind it (past the table's end when it wraps)


def test_counting_table_cases():
    w = MC.want_pairs(MC.hot_case(), "both")
    assert w["count"].tolist() == [70, 70000, 70] and w["stats"]["n_unrouted"] == 70
    c, pairs, cap = MC.count_chain_case()
    w = MC.want_pairs(c, "both")
    assert w["stats"]["n_routed"] == 48 and cap == pkg.gpl_table_slot(0, 48, 8)[1] == 128 and len(pairs) == 4
    assert all(pkg.gpl_table_slot((e << 32) | b1, 48, 8)[0] == cap - 1 for e, b1 in pairs)
    got = dict(zip(zip(w["entry"].tolist(), w["cell"].tolist()), w["count"].tolist()))
    assert all(got[p] == 3 for p in pairs)
    a, b = MC.two_fill_cases()
    pa, pb = MC.want_pairs(a, "both"), MC.want_pairs(b, "both")
    assert set(zip(pa["entry"].tolist(), pa["cell"].tolist())) & set(zip(pb["entry"].tolist(), pb["cell"].tolist()))   # a pair present in both fills


# ------------------------------------------------------------------------------------------------------------ whole step
@pytest.fixture(scope="module")
def dataset():
    return MC.chain_dataset()


def test_the_design_holds_every_kind_of_sample_barcode():
    rows, kinds = MC.routing_design()
    info = M.load_sample_list(MC.sample_rows(rows))
    assert info["canonical"] == [rows[0][0], rows[2][0], rows[4][0]] and len(info["rotations"]) == 6 and info["L"] == 8
    r = M.build_routing(info, M.sample_spec("frequency"))
    assert set(kinds["exact"]) <= set(info["rotations"])
    assert all(b in r["permit_map"] and b not in info["rotations"] for b in kinds["unique"])
    assert set(kinds["ambig_a0_b0"] + kinds["ambig_a1_b1"]) <= set(r["deferred"]) and not set(kinds["none"]) & set(r["entries"])


@pytest.mark.parametrize("case", MC.CHAIN_CASES, ids=lambda c: c["name"])
def test_every_chain_case_reaches_every_route(dataset, case):
    chunks, rows, kinds, cells = dataset
    assert len(chunks) == 5 and 2500 < sum(len(c) for c in chunks) < 4000 and {len(c) for c in chunks} >= {1}
    ori = case.get("expected_ori", "fw")
    compat = [r for ch in chunks for r in ch if J.record_is_compatible([fw for _x, fw in r[3]], ori)]
    seen = {r[0] for r in compat}
    for k in ("exact", "unique", "ambig_a0_b0", "ambig_a1_b1", "none"):   # a compatible record of every kind: exact, unique, deferred, unrouted
        assert set(kinds[k]) <= seen, k
    w = MC.chain_want(case, chunks, rows, cells)
    t = w["sample_info"]["sample_routing"]
    assert t["exact"] > 0 and t["immediate_rejected"] > 0 and w["sample_info"]["samples"][2]["num_cells"] == 0   # gamma is never observed
    if case["sample_correction"] != "exact":
        assert t["structurally_unique"] > 0
    if case["sample_correction"] == "frequency":   # a deferred entry accepted and one rejected after replay
        assert t["deferred_accepted"] > 0 and t["deferred_rejected"] > 0 and t["deferred"] == t["deferred_accepted"] + t["deferred_rejected"]
        fin = w["sample_permit_map"]
        assert all(b in fin for b in kinds["ambig_a0_b0"]) and not any(b in fin for b in kinds["ambig_a1_b1"])
    else:
        assert t["deferred"] == 0
    assert w["sample_info"]["samples"][0]["num_cells"] > 0 and w["sample_info"]["samples"][1]["num_cells"] > 0
    if case["method"] == "unfiltered":   # cells on both sides of the list
        for i in (0, 1):
            assert w["routed"]["hist"][i] and w["routed"]["unmatched"][i]
    if case["method"] == "valid_bc":     # a listed barcode that is never observed
        valid, _ = MC.chain_lists(cells)
        assert not any(valid[-1] in h for h in w["routed"]["hist"])
    if case.get("correction") == "frequency":
        assert any(s["cell_correction"]["corrected_reads"] > 0 for s in w["sample_info"]["samples"])
