"""Without a device: every builder of tests/gpl_cases.py reaches what it claims - the byte positions relative to the parse tile,
the routes, the table shapes, the correction collisions - so that tests/test_gpu_gpl.py runs the kernels where they can go wrong."""
import numpy as np
import pytest

import gpl_cases as G
import gpl_judge as J
from util import pkg


@pytest.fixture(scope="module")
def lim():
    L = pkg.gpl_limits()
    assert L["parse_tile"] >= 256 and L["parse_halo"] >= 20 + 12 * L["lane_alns"] and L["lane_alns"] >= 2
    return L


def record_offsets(case, chunk=0):
    """byte offset of every record of a chunk relative to the chunk's first record byte, and the end of the last"""
    offs, q = [], 0
    for _bc, _umi, alns in case["chunks"][chunk]:
        offs.append(q)
        q += G.rec_size(len(alns), case["bc_bytes"], case["umi_bytes"], case["pos_bytes"])
    return offs, q


def test_encode_chunks_round_trips_through_the_header_and_sizes():
    c = G.widths_case(2, 8, 4)
    assert len(c["off"]) == 4
    for i, recs in enumerate(c["chunks"]):
        o = int(c["off"][i])
        nb, nr = int.from_bytes(c["data"][o:o + 4], "little"), int.from_bytes(c["data"][o + 4:o + 8], "little")
        assert nr == len(recs) and nb == 8 + record_offsets(c, i)[1]
    assert [len(r) for r in c["chunks"]] == [70, 1, 0, 133]   # a chunk of one record and an empty chunk
    # a record's bytes: na, barcode, umi, then (ref | fw << 31) + position bytes
    one = G.parse_case([[(0xA1B2, 0x11, [(5, True), (6, False)])]], 2, 1, 2)
    assert one["data"][8:] == bytes([2, 0, 0, 0, 0xB2, 0xA1, 0x11, 5, 0, 0, 0x80, 0, 0, 6, 0, 0, 0, 0, 0])


@pytest.mark.parametrize("bc_bytes", G.WIDTHS)
def test_width_cases_hold_the_edge_barcodes_and_every_orientation(bc_bytes):
    for ub in G.WIDTHS:
        for pb in (0, 4):
            c = G.widths_case(bc_bytes, ub, pb)
            bcs = {r[0] for recs in c["chunks"] for r in recs}
            assert 0 in bcs and (1 << (8 * bc_bytes)) - 1 in bcs
            nas = {len(r[2]) for recs in c["chunks"] for r in recs}
            assert 0 in nas and max(nas) == 5
            w = {o: G.want_hist(c, o) for o in G.ORIS}
            assert w["both"]["n_compatible"] == w["both"]["n_records"] > w["fw"]["n_compatible"] > 0 < w["rc"]["n_compatible"]


def test_alignment_cases_cover_every_byte_alignment():
    seen = set()
    for pad in range(4):
        c = G.alignment_case(pad)
        assert int(c["off"][0]) == pad
        seen |= {int(o) % 4 for o in c["off"]}
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_edge_cases_end_where_they_say(lim, delta):
    c, k = G.tile_edge_case(lim, delta)
    offs, end = record_offsets(c)
    assert offs[k] == lim["parse_tile"] + delta and end > lim["parse_tile"] + 1   # record k starts there: records 0..k-1 end there
    if delta == -1:
        assert offs[k] == lim["parse_tile"] - 1            # ... on the tile's last byte: its head lies in the halo
    if delta == 1:
        assert offs[k - 1] < lim["parse_tile"] < offs[k]   # the tile's last record straddles its end


def test_halo_cases_fill_the_halo_and_cross_the_route_threshold(lim):
    for na in (lim["lane_alns"], lim["lane_alns"] + 1):
        c, k = G.halo_case(lim, na)
        offs, _ = record_offsets(c)
        assert offs[k] == lim["parse_tile"] - 4 and len(c["chunks"][0][k][2]) == na
        assert G.rec_size(lim["lane_alns"], 8, 8, 8) <= lim["parse_halo"]
        # only the last alignment is forward: under fw the record is compatible iff the whole list is read
        w = G.want_hist(c, "fw")
        assert w["bc"].tolist() == [0xFFFFFFFFFFFFFFFF] and w["max_ambig"] == na


@pytest.mark.parametrize("where", ["first", "last", "absent"])
def test_long_cases(lim, where):
    c = G.long_case(where)
    nas = sorted(len(r[2]) for recs in c["chunks"] for r in recs)
    assert nas[-1] == 3000 and nas[-2] == nas[-3] == 2500 and nas[-1] * 4 > lim["parse_tile"] + lim["parse_halo"]
    fw, rc, both = (G.want_hist(c, o) for o in ("fw", "rc", "both"))
    assert both["max_ambig"] == 3000 and rc["max_ambig"] == 3000
    # under fw the record with the largest na is not compatible and does not set max-ambig
    assert fw["max_ambig"] == 2500
    h = dict(zip(fw["bc"].tolist(), fw["count"].tolist()))
    assert h.get(12, 0) == (1 if where == "absent" else 2) and 14 not in h and 15 not in h
    # (bc 12's second record is the mirror image: one reverse alignment at the same place, or none - then only fw takes it)
    h = dict(zip(rc["bc"].tolist(), rc["count"].tolist()))
    assert h.get(12, 0) == (1 if where == "absent" else 2) and h[14] == 1


@pytest.mark.parametrize("kind", ["head_cut", "alns_cut", "junk", "nrec_low", "nrec_high"])
def test_malformed_cases_pass_the_host_checks_and_break_the_walk(kind):
    data, off = G.malformed_case(kind)
    o = int(off[2])
    nb, nrec = int.from_bytes(data[o:o + 4], "little"), int.from_bytes(data[o + 4:o + 8], "little")
    assert o + nb <= (int(off[3]) if kind != "junk" else int(off[3])) and nrec * 12 <= nb - 8   # inside the buffer, plausible count
    # walk the chunk as the reference's reader would
    p, seen, ok = 8, 0, True
    while p < nb:
        if nb - p < 12:
            ok = False
            break
        na = int.from_bytes(data[o + p:o + p + 4], "little")
        if 12 + 4 * na > nb - p:
            ok = False
            break
        p += 12 + 4 * na
        seen += 1
    assert not (ok and seen == nrec)
    assert ok == (kind in ("nrec_low", "nrec_high"))


def test_hot_case():
    c = G.hot_case()
    w = G.want_hist(c, "fw")
    assert w["bc"].tolist() == [0, 0xABCDEF0123] and w["count"].tolist() == [70, 70000] and len(c["chunks"]) == 70
    w = G.want_hist(c, "both")
    assert w["bc"].tolist() == [0, 0xABCDEF0123, 0xFFFFFFFFFFFFFFFF] and w["count"].tolist() == [70, 70000, 70]


@pytest.mark.parametrize("wrap", [False, True])
def test_chain_cases_share_a_home_slot(wrap):
    c, bcs, cap, slot = G.chain_case(wrap)
    w = G.want_hist(c, "both")
    assert w["n_compatible"] == 48 and cap == 128 and (slot == cap - 1) == wrap
    assert len(set(bcs)) == 6 and {pkg.gpl_table_slot(b, 48)[0] for b in bcs} == {slot}
    h = dict(zip(w["bc"].tolist(), w["count"].tolist()))
    assert all(h[b] == 3 for b in bcs)


def test_capacity_step():
    assert pkg.gpl_table_slot(0, 64)[1] == 128 and pkg.gpl_table_slot(0, 65)[1] == 256 and pkg.gpl_table_slot(0, 0)[1] == 2
    assert pkg.gpl_table_slot(0, 10 ** 6, 1)[1] == 512 and pkg.gpl_table_slot(0, 10 ** 6, 2)[1] == 1 << 17   # no more keys than the width holds
    for n in (64, 65):
        w = G.want_hist(G.capacity_step_case(n), "both")
        assert len(w["bc"]) == n and set(w["count"].tolist()) == {1}


def test_two_fills_share_a_barcode():
    a, b = G.two_fill_cases()
    wa, wb = G.want_hist(a, "both"), G.want_hist(b, "both")
    assert set(wa["bc"].tolist()) & set(wb["bc"].tolist()) == {7}
    bc, cnt = G.merge_hists(wa, wb)
    assert bc.tolist() == [5, 7, 9] and cnt.tolist() == [2, 3, 1]


# ---------------------------------------------------------------------------------------------------------------- correct
@pytest.mark.parametrize("k", range(len(G.L4_RETAINED)))
def test_l4_cases_reach_every_decision(k):
    seen = set()
    for nbh in (J.HAMMING, J.SHIFT):
        for res in ("unique", G.RNA):
            c = G.l4_case(k, nbh, res)
            assert [b for b, _ in c["observed"]] == list(range(256))
            w = G.want_correct(c)
            seen |= set(w["decision"].tolist())
            assert int(w["target_count"].sum()) == w["stats"]["exact_reads"] + w["stats"]["corrected_reads"]
    assert seen == ({3} if k == 0 else {0, 1, 3} if k in (1, 2) else {0, 1, 2, 3})   # (the homopolymers lie too far apart to collide)
    if k == 4:   # the heavy priors decide some collisions that unique leaves ambiguous
        u, f = (G.want_correct(G.l4_case(k, J.SHIFT, r))["stats"]["ambiguous_distinct"] for r in ("unique", G.RNA))
        assert f < u


def test_l4_neighbour_counts_0_1_2():
    idx = J.identity_index(4, J.SHIFT, "unique", G.L4_RETAINED[3])
    n = {len(idx.candidate_sources(b)) for b in range(256) if b not in G.L4_RETAINED[3]}
    assert {0, 1, 2} <= n
    homo = J.identity_index(4, J.SHIFT, "unique", G.L4_RETAINED[2])
    x = 0x01   # AAAC: the homopolymer AAAA reaches it by a substitution and by several shifts
    assert J.inverse_shift_candidates(x, 4).count(0x00) >= 2 and homo.candidate_sources(x) == [0x00]


@pytest.mark.parametrize("L", [16, 32])
def test_random_cases(L):
    c = G.random_case(L, J.SHIFT, G.RNA, top_bit=(L == 32))
    w = G.want_correct(c)
    assert set(w["decision"].tolist()) == {0, 1, 2, 3}
    assert any(b not in dict(c["observed"]) for b in c["retained"])   # never-observed retained barcodes
    if L == 32:
        assert any(b >> 63 for b in c["retained"]) and J.U64 in dict(c["observed"])


def test_boundary_case_l32():
    c = G.boundary_case_l32()
    assert J.U64 in c["retained"] and any(b >> 63 for b, _ in c["observed"])
    w = G.want_correct(c)
    assert {0, 1} <= set(w["decision"].tolist())
    # every observed barcode that is not retained is a forward shift (or substitution) neighbour of a source: none is "not found"
    assert 3 not in set(w["decision"].tolist())


def test_frequency_cases_decide_as_named():
    cases = G.frequency_cases()
    assert "sub_and_shift_once" in cases
    for name, (c, x, dec, tgt) in cases.items():
        idx = J.identity_index(c["L"], c["neighborhood"], c["resolution"], c["retained"])
        assert idx.resolve(x) == (dec, tgt), name
    c, x, _, _ = cases["sub_and_shift_once"]
    s = max(c["retained"], key=c["retained"].get)
    assert s in J.substitutions(x, 4) and s in J.inverse_shift_candidates(x, 4)
    # counted twice, 40 of 41 would pass 39/40
    assert 40 * 40 >= 39 * 41 and not 20 * 40 >= 39 * 21


def test_never_observed_case():
    c = G.never_observed_case()
    idx = J.identity_index(c["L"], c["neighborhood"], c["resolution"], c["retained"])
    entries, st, tc = idx.compile_distinct_observed_with_target_counts(c["observed"])
    assert (0x10, 0x10) in entries and 0x10 not in tc and st["exact_distinct"] == 2
    w = G.want_correct(c)
    assert w["stats"]["exact_distinct"] == 1 and w["target_count"].tolist() == [0, 7]   # the device counts the observed ones
