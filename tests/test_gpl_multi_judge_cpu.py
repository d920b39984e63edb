"""Without a device: tests/gpl_multi_judge.py (and the index of tests/gpl_judge.py it stands on) held to known answers - the
inputs and expected values of the reference's own unit tests (src/barcode_correction.rs:853-1031, src/cellfilter.rs:2722-2754), and
small cases worked out by hand."""
import pytest

import gpl_judge as J
import gpl_multi_judge as M

RNA = ("frequency", (39, 40), 1)


def index(L, nbh, res, sources):
    return J.Index(L, nbh, res, sources)


# ---- barcode_correction.rs:853-1031: sources that differ from their targets
def test_exact_sources_win_over_neighbor_collisions():
    assert index(2, J.HAMMING, "unique", [(0, 10, 1), (1, 11, 1)]).resolve(0) == (J.EXACT, 10)


def test_unique_counts_distinct_canonical_targets():
    assert index(2, J.HAMMING, "unique", [(1, 7, 4), (2, 7, 5)]).resolve(0) == (J.CORRECTED, 7)


def test_unique_rejects_multiple_targets_independent_of_input_order():
    src = [(1, 10, 1), (2, 20, 1)]
    assert index(2, J.HAMMING, "unique", src).resolve(0) == (J.AMBIGUOUS, None) == index(2, J.HAMMING, "unique", src[::-1]).resolve(0)


def test_structural_compilation_separates_unique_and_ambiguous_routes():
    info = {"L": 1, "rotations": {0: 10, 2: 20}}
    entries, ambiguous = M.structural_table(info, J.HAMMING)
    assert sorted(entries.items()) == [(0, 10), (2, 20)] and ambiguous == [1, 3]
    # the structural table stays policy-free; Frequency accepts the high-prior target for an ambiguous barcode
    assert index(1, J.HAMMING, RNA, [(0, 10, 100), (2, 20, 1)]).resolve(1) == (J.CORRECTED, 10)


def test_frequency_sums_alias_weights_and_uses_exact_threshold():
    assert index(2, J.HAMMING, RNA, [(1, 10, 19), (2, 10, 18), (3, 20, 0)]).resolve(0) == (J.CORRECTED, 10)   # (20 + 19) / 40
    assert index(2, J.HAMMING, RNA, [(1, 10, 37), (2, 20, 1)]).resolve(0) == (J.AMBIGUOUS, None)            # 38 / 40


def test_frequency_tie_break_is_deterministic_but_still_subject_to_confidence():
    assert index(2, J.HAMMING, ("frequency", (1, 2), 1), [(1, 10, 0), (2, 20, 0)]).resolve(0) == (J.CORRECTED, 20)


# ---- cellfilter.rs:2722-2754: the sample permit map
def test_sample_one_edit_correction_drops_cross_sample_collisions():
    info = {"canonical": [0, 5], "rotations": {0: 0, 5: 5}, "names": {}, "L": 2}
    r = M.build_routing(info, M.sample_spec("1-edit"))
    assert r["permit_map"][0] == 0 and r["permit_map"][5] == 5 and 1 not in r["permit_map"] and r["deferred"] == []
    one = {"canonical": [9], "rotations": {0: 9, 5: 9}, "names": {}, "L": 2}
    assert M.build_routing(one, M.sample_spec("1-edit"))["permit_map"][1] == 9


def test_sample_corrections_are_whitelist_order_invariant():
    fwd = M.load_sample_list("AA\tAA\ta\nAC\tAA\ta\nCC\tCC\tb\n")
    rev = M.load_sample_list("CC\tCC\tb\nAC\tAA\ta\nAA\tAA\ta\n")
    spec = M.sample_spec("unique", J.HAMMING)
    assert M.build_routing(fwd, spec)["permit_map"] == M.build_routing(rev, spec)["permit_map"]
    assert fwd["canonical"] == [0, 5] and rev["canonical"] == [5, 0]   # canonical order is first appearance


# ---- the sample list
def test_sample_list_columns_comments_and_reverse():
    one = M.load_sample_list("# header\n\nACGT\nTTTT\r\n")
    assert one == {"canonical": [0x1B, 0xFF], "rotations": {0x1B: 0x1B, 0xFF: 0xFF}, "names": {0x1B: "ACGT", 0xFF: "TTTT"}, "L": 4}
    two = M.load_sample_list("ACGT\tfirst sample\n  TTTT\tsecond\t\n")
    assert two["names"] == {0x1B: "first sample", 0xFF: "second"} and two["rotations"] == {0x1B: 0x1B, 0xFF: 0xFF}
    three = M.load_sample_list("ACGT\tAAAA\ts1\textra\nAAAC\tAAAA\ts1\nTTTT\tTTTT\ts2\n")
    assert three["canonical"] == [0, 0xFF] and three["rotations"] == {0x1B: 0, 1: 0, 0xFF: 0xFF}   # (a canonical barcode need not be a source)
    rc = M.load_sample_list("ACGT\tAAAA\ts1\nAAAC\tAAAA\ts1\n", reverse=True)
    assert rc["rotations"] == {M.pack("ACGT"): M.pack("TTTT"), M.pack("GTTT"): M.pack("TTTT")} and rc["canonical"] == [0xFF]


@pytest.mark.parametrize("text, sentence", [
    ("ACGT\tACG\tx\n", "sample barcode 'ACGT' and its canonical barcode 'ACG' have different lengths"),
    ("A" * 33 + "\n", "sample barcode length 33 is unsupported; expected 1 through 32 bases"),
    ("ACGT\nACG\n", "sample barcode file mixes lengths 4 and 3"),
    ("ACNT\n", "couldn't pack sample barcode: ACNT"),
    ("ACGT\tACNT\tx\n", "couldn't pack sample barcode: ACNT"),
    ("ACGT\tAAAA\ts1\nACGT\tCCCC\ts2\n", "sample construction barcode 'ACGT' is assigned to conflicting canonical barcodes"),
    ("ACGT\tAAAA\ts1\nACGA\tAAAA\ts2\n", "canonical sample barcode 'AAAA' is assigned conflicting names 's1' and 's2'"),
    ("# nothing\n\n", "contains no barcodes"),
])
def test_sample_list_errors(text, sentence):
    with pytest.raises(ValueError) as e:
        M.load_sample_list(text)
    assert sentence in str(e.value)


# ---- the pass, by hand
def test_pair_histogram_and_routing_by_hand():
    # L = 2 sample barcodes: sources 0 (-> sample 0) and 5 (-> sample 5); hamming-1: 1 and 4 lie between them (ambiguous), 2, 3, 8, 12
    # reach only 0 and 7, 6, 9, 13 only 5
    info = M.load_sample_list("AA\ts0\nCC\ts5\n")
    uniq = M.build_routing(info, M.sample_spec("unique"))
    assert sorted(uniq["permit_map"].items()) == [(0, 0), (2, 0), (3, 0), (5, 5), (6, 5), (7, 5), (8, 0), (9, 5), (12, 0), (13, 5)] and uniq["deferred"] == []
    freq = M.build_routing(info, M.sample_spec("frequency"))
    assert freq["deferred"] == [1, 4] and freq["entries"] == sorted(list(uniq["permit_map"]) + [1, 4])
    fw = [(1, True)]
    chunks = [[(0, 100, 0, fw)] * 39 + [(5, 200, 0, fw), (1, 100, 0, fw), (1, 101, 0, fw), (2, 100, 0, fw), (10, 100, 0, fw), (0, 100, 0, [(1, False)]), (0, 7, 0, [])]]
    pairs, st = M.pair_histogram(chunks, freq["entries"], "fw")
    e = {b: i for i, b in enumerate(freq["entries"])}
    assert pairs == {(e[0], 100): 39, (e[5], 200): 1, (e[1], 100): 1, (e[1], 101): 1, (e[2], 100): 1}
    assert st == {"n_records": 46, "n_compatible": 44, "n_routed": 43, "n_unrouted": 1}
    spec = M.sample_spec("frequency")
    r = M.route_pairs(info, spec, freq, pairs, st["n_records"], st["n_unrouted"])
    # barcode 1 lies between source 0 (39 exact reads, weight 40) and source 5 (1 read, weight 2): 40 / 42 < 39 / 40 -> rejected
    assert r["tally"] == {"exact": 40, "structurally_unique": 1, "immediate_rejected": 1, "deferred": 2, "deferred_accepted": 0, "deferred_rejected": 2}
    assert r["hist"] == [{100: 40}, {200: 1}] and r["matched_reads"] == 41 and r["unmatched_reads"] == 3 and r["total_reads"] == 46
    # without the read of source 5: weight 40 against 1 is 40 / 41 >= 39 / 40 -> accepted, and the final map holds barcode 1
    chunks2 = [[rec for rec in chunks[0] if rec[0] != 5]]
    pairs2, st2 = M.pair_histogram(chunks2, freq["entries"], "fw")
    r2 = M.route_pairs(info, spec, freq, pairs2, st2["n_records"], st2["n_unrouted"])
    assert r2["tally"]["deferred_accepted"] == 2 and r2["hist"][0] == {100: 41, 101: 1} and r2["sample_permit_map"][1] == 0 and 1 not in r["sample_permit_map"]
    # a whitelist splits a sample's cells: unlisted ones only join the observed counts
    r3 = M.route_pairs(info, spec, freq, pairs2, st2["n_records"], st2["n_unrouted"], whitelist={100})
    assert r3["hist"][0] == {100: 41} and r3["unmatched"][0] == {101: 1}


def test_sample_output_by_hand():
    cspec = M.cell_spec("unique")
    empty = M.sample_output("s", 0x1B, {}, {7: 3}, cspec, "knee", 4)
    assert empty["permit_map"] is None and empty["permit_freq"] is None and empty["info"]["num_cells"] == 0 and empty["plan"] == []
    # two cells of 50 and 40 reads, a neighbour of the first with 2 reads, an unlisted barcode beside the second
    hist, unm = {0x00: 50, 0xFF: 40, 0x01: 2}, {0xFE: 3}
    o = M.sample_output("s", 0x1B, hist, unm, cspec, "unfiltered", 4, min_reads=10)
    assert o["permit_freq"] == {0x00: 52, 0xFF: 43} and o["info"]["num_reads"] == 95 == o["info"]["collatable_reads"]
    assert o["permit_map"] == {0x00: 0x00, 0x01: 0x00, 0xFF: 0xFF, 0xFE: 0xFF} == dict(o["plan"])
    f = M.sample_output("s", 0x1B, hist, {}, cspec, "force", 4, arg=2)
    assert f["permit_freq"] == {0x00: 52, 0xFF: 40} and f["info"]["num_reads"] == 90 and f["info"]["collatable_reads"] == 92
    assert len(f["permit_map"]) == 2 * (1 + 3 * 4) and dict(f["plan"]) == {0x00: 0x00, 0x01: 0x00, 0xFF: 0xFF}


def test_plan_bytes_layout():
    b = M.plan_bytes(2, 4, ("hamming-1", "unique"), {1: 0}, ("hamming-1", RNA), [(5, [(9, 8)]), (0, [])])
    want = b"AFCORR\0\0" + bytes([1, 0]) + bytes([1, 2, 4]) + bytes([1, 2, 0, 0, 0, 0, 0, 0, 0, 0]) + (1).to_bytes(8, "little") + (1).to_bytes(8, "little") + bytes(8)
    want += (2).to_bytes(8, "little")
    spec = bytes([4, 0, 0, 0, 0, 1, 0, 0, 0]) + (39).to_bytes(8, "little") + (40).to_bytes(8, "little") + (1).to_bytes(8, "little")
    want += b"\x01" + bytes(8) + spec + bytes(8)
    want += b"\x01" + (5).to_bytes(8, "little") + spec + (1).to_bytes(8, "little") + (9).to_bytes(8, "little") + (8).to_bytes(8, "little")
    assert b == want
    assert M.plan_bytes(2, 4, None, {}, ("hamming-1", "unique"), [(0, [])])[10:14] == bytes([1, 2, 4, 0])
