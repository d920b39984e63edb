"""tests/atac_gpl_judge.py on vectors derived by hand from src/atac/cellfilter.rs: the reverse-complemented list, the min_reads
threshold, unique against frequency at exactly 9/10, the f32 ceiling of initialize_rec_list, and positions that land in the next
reference's bins or past all of them.  Barcodes are 4 bases: A C G T = 0 1 2 3, first base highest, so AAAC = 1 and GTTT = 191."""
import pytest

import atac_gpl_judge as J

A1 = (0, 4, 10, 50)
AAAA, AAAC, AAAG, AAAT, GTTT = 0, 1, 2, 3, 191
RL = [1000]


def reads(*pairs):
    """one chunk: (barcode, how often) -> that many single-alignment records"""
    return [[(bc, [A1]) for bc, n in pairs for _ in range(n)]]


def test_reverse_complement_and_list_parsing():
    assert J.reverse_complement(AAAC, 4) == GTTT and J.reverse_complement(GTTT, 4) == AAAC
    assert J.reverse_complement(0b00011011, 4) == 0b00011011            # ACGT is its own reverse complement
    assert J.reverse_complement(0, 32) == (1 << 64) - 1                 # 32 A's -> 32 T's
    assert J.listed_barcodes("AAAC\nAANC\nAAAG\r\nAAAC\n", False) == ([AAAC, AAAG], 4)   # the N line adds nothing, a repeat is one key
    assert J.listed_barcodes("AAAC\n", True) == ([GTTT], 4)
    with pytest.raises(ValueError, match="found barcodes of different lengths 4 and 5"):
        J.listed_barcodes("AAAC\nAAACC\n", False)


def test_an_rc_list_against_forward_reads_matches_nothing():
    """the list says AAAC, the reads carry AAAC: under rc the listed key is GTTT, which no read has; nothing is retained, every read is
    without a candidate and the three maps are empty.  Without rc the same input is ten exact reads."""
    out = J.outputs(reads((AAAC, 10)), "AAAC\n", True, 1, RL, 4)
    assert out["listed"] == [GTTT] and out["retained"] == [] and out["permit_freq"] == {} and out["plan"] == []
    assert out["stats"]["not_found_distinct"] == 1 and out["stats"]["not_found_reads"] == 10 and out["stats"]["exact_reads"] == 0
    assert out["hist"] == {AAAC: 10} and out["n_records"] == 10
    out = J.outputs(reads((AAAC, 10)), "AAAC\n", False, 1, RL, 4)
    assert out["retained"] == [AAAC] and out["permit_freq"] == {AAAC: 10} and out["plan"] == [(AAAC, AAAC)]
    assert out["stats"]["exact_distinct"] == 1 and out["stats"]["exact_reads"] == 10 and out["stats"]["not_found_reads"] == 0


def test_a_barcode_at_min_reads_is_retained_and_one_below_is_not():
    """AAAC has 3 reads, AAAG 2, min_reads 3: AAAC is kept; AAAG - listed, but below - is one substitution from it and is corrected"""
    out = J.outputs(reads((AAAC, 3), (AAAG, 2)), "AAAC\nAAAG\n", False, 3, RL, 4)
    assert out["retained"] == [AAAC] and out["permit_freq"] == {AAAC: 5} and out["plan"] == [(AAAC, AAAC), (AAAG, AAAC)]
    s = out["stats"]
    assert (s["exact_distinct"], s["exact_reads"], s["corrected_distinct"], s["corrected_reads"]) == (1, 3, 1, 2)
    out = J.outputs(reads((AAAC, 3), (AAAG, 2)), "AAAC\nAAAG\n", False, 2, RL, 4)
    assert out["retained"] == [AAAC, AAAG] and out["permit_freq"] == {AAAC: 3, AAAG: 2} and out["stats"]["corrected_distinct"] == 0
    with pytest.raises(ValueError, match="min-reads < 1"):
        J.outputs(reads((AAAC, 3)), "AAAC\n", False, 0, RL, 4)


def test_unique_is_ambiguous_where_frequency_wins_at_exactly_nine_tenths():
    """AAAC (unlisted, 4 reads) is one substitution from the retained AAAA and AAAT.  Unique: two targets, ambiguous.  Frequency, pseudocount
    1, confidence 9/10: counts 17 and 1 weigh 18 and 2 - 18/20 is exactly 9 of 10 and is accepted; counts 88 and 10 weigh 89 and 11 - 89 of
    100 is below and stays ambiguous."""
    text = "AAAA\nAAAT\n"
    u = J.outputs(reads((AAAA, 17), (AAAT, 1), (AAAC, 4)), text, False, 1, RL, 4)
    assert u["plan"] == [(AAAA, AAAA), (AAAT, AAAT)] and u["stats"]["ambiguous_distinct"] == 1 and u["stats"]["ambiguous_reads"] == 4
    f = J.outputs(reads((AAAA, 17), (AAAT, 1), (AAAC, 4)), text, False, 1, RL, 4, resolution="frequency")
    assert f["plan"] == [(AAAA, AAAA), (AAAC, AAAA), (AAAT, AAAT)] and f["permit_freq"] == {AAAA: 21, AAAT: 1}
    assert f["stats"]["corrected_reads"] == 4 and f["stats"]["ambiguous_distinct"] == 0
    g = J.outputs(reads((AAAA, 88), (AAAT, 10), (AAAC, 4)), text, False, 1, RL, 4, resolution="frequency")
    assert g["plan"] == [(AAAA, AAAA), (AAAT, AAAT)] and g["permit_freq"] == {AAAA: 88, AAAT: 10} and g["stats"]["ambiguous_reads"] == 4


def test_bin_lens_take_the_ceiling_in_f32():
    assert J.bin_lens([100000, 100001, 99999, 0, 1]) == [0, 1, 3, 4, 4, 5]
    # 200 000 001 is not an f32: it rounds to 200 000 000, the quotient is 2000.0 and so is its ceiling (the integer ceiling is 2001)
    assert J.bin_lens([200000001]) == [0, 2000] and -(-200000001 // 100000) == 2001
    # 2^32 - 1 rounds to 2^32: 42949.67... -> 42950, three times
    assert J.bin_lens([4294967295] * 3) == [0, 42950, 85900, 128850]
    assert J.bin_lens([]) == [0] and J.bin_lens([0, 0]) == [0, 0, 0]


def test_a_position_past_its_reference_counts_in_the_next_references_bins():
    """lengths 100 000 and 250 000: bins [0, 1) and [1, 4).  Reference 0 at 150 000 is bin 0 + 1 = the first bin of reference 1 (no length
    is tested); reference 1 at 299 999 is the last bin; reference 1 at 300 000 indexes bins[4], and reference 2 indexes past blens: both
    are where the reference panics."""
    rl = [100000, 250000]
    chunks = [[(5, [(0, 4, 150000, 50)]), (5, [(1, 4, 0, 50)]), (6, [(1, 4, 299999, 50)]), (6, [(0, 4, 99999, 50)]),
               (7, []), (7, [(1, 4, 5, 50), (1, 4, 6, 50)])]]
    hist, bins, max_ambig, n = J.record_pass(chunks, J.bin_lens(rl))
    assert bins == [1, 2, 0, 1] and hist == {5: 2, 6: 2, 7: 2} and max_ambig == 2 and n == 6   # (the na == 0 and na == 2 records count their barcode)
    with pytest.raises(J.ReferencePanics, match=r"bins\[4\]"):
        J.record_pass([[(5, [(1, 4, 300000, 50)])]], J.bin_lens(rl))
    with pytest.raises(J.ReferencePanics, match=r"bins\[4\]"):
        J.record_pass([[(5, [(2, 4, 0, 50)])]], J.bin_lens(rl))      # blens[2] is the total: the index is past the bins
    with pytest.raises(J.ReferencePanics, match=r"blens\[3\]"):
        J.record_pass([[(5, [(3, 4, 0, 50)])]], J.bin_lens(rl))
    with pytest.raises(J.ReferencePanics, match="bins should not be empty"):
        J.outputs([[(5, [])]], "AAAC\n", False, 1, [0, 0], 4)


def test_max_ambig_is_over_all_records_and_max_bin_over_the_bins():
    chunks = [[(1, []), (1, [A1] * 400)], [(2, [A1]), (2, [A1]), (2, [(0, 4, 999, 9)])]]
    out = J.outputs(chunks, "AAAG\n", False, 1, RL, 4)
    assert out["max_ambig"] == 400 and out["bins"] == [3] and out["max_bin"] == 3 and out["hist"] == {1: 2, 2: 3} and out["bin_lens"] == [0, 1]
