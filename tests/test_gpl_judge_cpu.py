"""tests/gpl_judge.py held to the reference's own unit tests (src/barcode_correction.rs:853-1185, whose inputs and assertions are
data and are restated here as literals), to the forward / inverse shift relation, and to hand-worked knee and rounding vectors."""
import pytest

import gpl_judge as J

RNA = ("frequency", (39, 40), 1)


def idx(L, nbh, res, sources):
    return J.Index(L, nbh, res, sources)


def test_exact_sources_win_over_neighbor_collisions():
    assert idx(2, J.HAMMING, "unique", [(0, 10, 1), (1, 11, 1)]).resolve(0) == (J.EXACT, 10)


def test_unique_counts_distinct_canonical_targets():
    assert idx(2, J.HAMMING, "unique", [(1, 7, 4), (2, 7, 5)]).resolve(0) == (J.CORRECTED, 7)


def test_unique_rejects_multiple_targets_independent_of_input_order():
    retained = [(1, 10, 1), (2, 20, 1)]
    assert idx(2, J.HAMMING, "unique", retained).resolve(0) == (J.AMBIGUOUS, None)
    assert idx(2, J.HAMMING, "unique", retained[::-1]).resolve(0) == (J.AMBIGUOUS, None)


def test_frequency_accepts_the_high_prior_target_of_a_structurally_ambiguous_source():
    i = idx(1, J.HAMMING, RNA, [(0, 10, 100), (2, 20, 1)])
    assert i.resolve(1) == (J.CORRECTED, 10)
    # (the structural view of the same index: 1 and 3 have two possible targets)
    u = idx(1, J.HAMMING, "unique", [(0, 10, 100), (2, 20, 1)])
    assert [b for b in range(4) if u.resolve(b)[0] == J.AMBIGUOUS] == [1, 3]


def test_frequency_sums_alias_weights_and_uses_exact_threshold():
    assert idx(2, J.HAMMING, RNA, [(1, 10, 19), (2, 10, 18), (3, 20, 0)]).resolve(0) == (J.CORRECTED, 10)   # 39 of 40
    assert idx(2, J.HAMMING, RNA, [(1, 10, 37), (2, 20, 1)]).resolve(0) == (J.AMBIGUOUS, None)              # 38 of 40


def test_frequency_tie_break_is_deterministic_but_still_subject_to_confidence():
    assert idx(2, J.HAMMING, ("frequency", (1, 2), 1), [(1, 10, 0), (2, 20, 0)]).resolve(0) == (J.CORRECTED, 20)


def test_shift_candidates_are_deduplicated_before_scoring():
    assert idx(2, J.SHIFT, "unique", [(5, 9, 0)]).resolve(1) == (J.CORRECTED, 9)
    assert idx(2, J.SHIFT, RNA, [(5, 9, 0)]).candidate_sources(1) == [5]


def test_observed_compilation_is_sorted_and_aggregates_stats():
    entries, st = idx(2, J.HAMMING, "unique", [(1, 1, 4)]).compile_observed([(8, 3), (0, 2), (0, 4), (1, 4)])
    assert entries == [(0, 1), (1, 1)]
    assert (st["exact_reads"], st["corrected_reads"], st["not_found_reads"]) == (4, 6, 3)


def test_distinct_compilation_adds_unobserved_retained_identities():
    entries, st, tc = idx(2, J.HAMMING, "unique", [(1, 7, 0)]).compile_distinct_observed_with_target_counts([(8, 3)])
    assert entries == [(1, 7)]
    assert (st["exact_distinct"], st["exact_reads"], st["not_found_reads"]) == (1, 0, 3)
    assert tc == {}


def test_all_supported_lengths_validate_without_shift_overflow():
    for L in range(1, 33):
        i = idx(L, J.SHIFT, "unique", [(J.U64 >> (64 - 2 * L), 1, 0)])
        i.resolve(0)
        for b in J.inverse_shift_candidates(J.U64 >> (64 - 2 * L), L) + J.shift_neighbors(J.U64 >> (64 - 2 * L), L):
            assert 0 <= b <= J.U64 >> (64 - 2 * L)
    with pytest.raises(ValueError):
        idx(33, J.SHIFT, "unique", [])
    with pytest.raises(ValueError, match="does not fit"):
        idx(3, J.SHIFT, "unique", [(64, 64, 0)])
    with pytest.raises(ValueError, match="pseudocount"):
        idx(3, J.SHIFT, ("frequency", (1, 2), 0), [])


def test_directed_shift_lookup_preserves_historical_source_to_observation_semantics():
    assert idx(3, J.SHIFT, "unique", [(1, 1, 0)]).resolve(8) == (J.CORRECTED, 1)
    assert idx(3, J.SHIFT, "unique", [(8, 8, 0)]).resolve(1) == (J.NOT_FOUND, None)


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_inverse_shift_candidates_are_exactly_the_sources_whose_forward_neighbours_hold_x(L):
    universe = 1 << (2 * L)
    generated_by = {x: set() for x in range(universe)}
    for source in range(universe):
        for g in J.shift_neighbors(source, L):
            generated_by[g].add(source)
    for x in range(universe):
        assert {s for s in J.inverse_shift_candidates(x, L) if s != x} == generated_by[x], (L, x)


def test_substitutions_are_3L_distinct_barcodes_at_hamming_distance_one():
    for L, b in ((4, 0x1B), (16, 0x12345678), (32, 0x8000000000000001)):
        s = J.substitutions(b, L)
        assert len(s) == len(set(s)) == 3 * L and b not in s
        assert all(bin(((x ^ b) | ((x ^ b) >> 1)) & 0x5555555555555555).count("1") == 1 for x in s)


def test_full_neighborhood_counts_priors_only():
    i = J.identity_index(2, J.HAMMING, RNA, {0: 100, 2: 1})
    entries, st = i.compile_full_neighborhood()
    assert dict(entries)[0] == 0 and dict(entries)[2] == 2
    assert dict(entries)[1] == 0 and dict(entries)[3] == 0     # 101 of 103 >= 39/40: the prior decides
    assert st["exact_distinct"] == 2 and st["exact_reads"] == 0 and st["corrected_reads"] == 0


# ---- record pass
def test_record_filter_and_max_ambig():
    chunks = [[(1, 0, []), (2, 0, [(0, True)]), (3, 0, [(0, False), (1, False), (2, False)]), (2, 1, [(0, False), (1, True)])]]
    assert J.histogram(chunks, "both") == ({1: 1, 2: 2, 3: 1}, 4, 4, 3)
    assert J.histogram(chunks, "fw") == ({2: 2}, 4, 2, 2)        # the na = 3 record is not compatible: it does not set max-ambig
    assert J.histogram(chunks, "rc") == ({3: 1, 2: 1}, 4, 2, 3)


# ---- retained set
def test_rust_round_is_half_away_from_zero():
    assert [J.rust_round(x) for x in (0.5, 1.5, 2.5, -0.5, -2.5, 2.4999, 99.0 * 0.99)] == [1, 2, 3, -1, -3, 2, 98]
    assert round(0.5) == 0 and round(2.5) == 2   # what Python's own round() would have given


def test_knee_on_hand_worked_vectors():
    # cumulative 100 190 270 275 279 282 284 285 286 287 over x = i / 10: the chord runs from (0, 100/287) to (1, 1); the point
    # farthest above it is the end of the steep part, index 2 - and again on the second pass over the first min(9, 10) points
    assert J.get_knee([100, 90, 80, 5, 4, 3, 2, 1, 1, 1]) == 2
    # equal frequencies: the points (i / 4, (i + 1) / 4) rise with slope 1, the chord from (0, 1/4) to (1, 1) with slope 3/4: the
    # distance grows with i and the last index is the farthest
    assert J.max_distance_index([5, 10, 15, 20]) == 3
    # 1 3 3: chord from (0, 1/3) to (1, 1); index 1 lies 4/9 above it, index 2 only 2/9
    assert J.max_distance_index([1, 3, 3]) == 1
    # d >= max_d: 4 6 7 8 puts indices 1, 2 and 3 all 1/8 above the chord (dyadic numbers: the doubles are exact) - the later wins
    assert J.max_distance_index([4, 6, 7, 8]) == 3
    with pytest.raises(ValueError, match="only of length 1"):
        J.get_knee([7])
    with pytest.raises(ValueError, match="only of length 1"):
        J.get_knee([5, 5])   # first pass: index 1; second pass over cfreq[0:min(1, 5)] has one point


def test_select_retained_rules():
    hist = {10: 50, 11: 40, 12: 40, 13: 40, 14: 3, 15: 1}
    assert J.select_retained(hist, "force", 2) == [10, 11, 12, 13]          # ties at the threshold keep more than N
    assert J.select_retained(hist, "force", 0) == []
    assert J.select_retained(hist, "force", 99) == [10, 11, 12, 13, 14, 15]   # beyond the length: the smallest count
    assert J.select_retained(hist, "unfiltered", min_reads=40) == [10, 11, 12, 13]
    assert J.select_retained({}, "knee") == []
    # expect 150: 150 * 0.99 is the double 148.5, which rounds AWAY from zero to index 149 (Python's round() gives 148).  The count
    # at 149 is 40 -> threshold 4 and everything is kept; at 148 it is 100 -> threshold 10 would keep 149 barcodes
    assert 150 * 0.99 == 148.5 and round(150 * 0.99) == 148
    big = {i: (1000 if i < 148 else 100 if i == 148 else 40 if i == 149 else 5 + i % 5) for i in range(200)}
    assert J.select_retained(big, "expect", 150) == list(range(200))
    # expect with a threshold that rounds to 0 is lifted to 1
    assert J.select_retained({1: 4, 2: 3, 3: 1}, "expect", 3) == [1, 2, 3]
