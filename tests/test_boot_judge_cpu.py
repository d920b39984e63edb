"""The bootstrap judge (tests/boot_judge.py) against values worked out by hand, and the oracle in front of the judge.

oracle/afq_oracle.cpp::bootstrap_cell and the bootstrap kernel were written from one reading of em.rs:585-687, multinomial.rs and
quant.rs:157-210, and agree bit for bit; the judge is a second reading, from the reference's text and DESIGN's statement of the
streams alone.  Every oracle result - both summaries, B in {1, 4}, two seeds - has to be the summary of one admissible combination
of the judge's replicates: bit for bit where no label has two ids, under em_judge's bars and the derived variance bound elsewhere.
The last tests show that the judge refuses what is wrong."""
import functools
import os
import sys

import pytest

import boot_judge as bj
import boot_judge_cases as bc
import em_judge as ej
import em_judge_cases as ec
import quant_judge as qj
import quant_judge_cases as qc
from util import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as ora  # noqa: E402


@functools.lru_cache(maxsize=None)
def _oracle_run(name, res, B, summary_stat, seed):
    """The oracle's result on a quant batch; computed once per process, shared, never changed."""
    b = ec.quant_batch(name)
    return ora.quant(b.cfg(res, dump_eq=True, num_bootstraps=B, summary_stat=summary_stat, boot_seed=seed), b.t2g, b.data, b.off,
                     first_cell_index=bc.FIRST)


def _cells(name, res, B, summary_stat, seed, limit=None):
    """(name, judgement, mean row, variance row) of the cells of an oracle run that are not tiny and not undecided."""
    b = ec.quant_batch(name)
    got = _oracle_run(name, res, B, summary_stat, seed)
    tables, flags = qc.classes_of(got), got.flags.tolist()
    means, variances = bc.boot_rows(got.bootstraps, got.n_cells)
    for i, table in enumerate(tables[:limit]):
        if not flags[i] & qj.FLAG_TINY:
            j = bc.judge_table(table, b.usa, b.num_rows, B, seed, bc.FIRST + i)
            if not j.undecided:
                yield b.names[i], j, dict(means[i]), dict(variances[i])


# ---------------------------------------------------------------------------------------------------------------------- by hand

def test_philox_known_answers():
    """The three known-answer vectors of Random123 (kat_vectors: philox4x32 10)."""
    h = lambda t: " ".join(f"{x:08x}" for x in t)
    assert h(bj.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert h(bj.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert h(bj.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_the_streams_are_designs():
    """draw j is word j & 3 of block (j >> 2, b, c_lo, c_hi) under the key (seed_lo, seed_hi); the start stream sets
    bit 31 of the replicate's word."""
    seed, cell, b = 0xC0FFEE1234, (1 << 32) + 5, 2
    key = (0xFFEE1234, 0xC0)
    draws, starts = bj.stream(seed, cell, b, 6), bj.stream(seed, cell, b, 5, start=True)
    for j, w in enumerate(draws):
        assert w == bj.philox4x32_10((j >> 2, 2, 5, 1), key)[j & 3]
    for s, w in enumerate(starts):
        assert w == bj.philox4x32_10((s >> 2, 2 | 1 << 31, 5, 1), key)[s & 3]
    assert draws == [0x399429A0, 0x1A8FC6AD, 0xF9DB2DEB, 0xDD79B6BE, 0xAC91F508, 0x9C916565]
    assert bj.stream(seed, cell - (1 << 32), b, 6) != draws and bj.stream(seed, cell, b + 1, 6) != draws and bj.stream(seed + (1 << 32), cell, b, 6) != draws


def test_one_replicate_by_hand():
    """Classes {1}: 2, {4}: 1, {6}: 3, N = 6, cumulative counts 2, 3, 6.  The six words above give (word 6) >> 32 = 1, 0, 5, 5, 4,
    3: classes 0, 0, 2, 2, 2 and - 3 is not under the second cumulative count, 3 - class 2 again.  Counts 2, 0, 4."""
    seed, cell, b = 0xC0FFEE1234, (1 << 32) + 5, 2
    words = bj.stream(seed, cell, b, 6)
    assert [(w * 6) >> 32 for w in words] == [1, 0, 5, 5, 4, 3]
    assert bj.resample([2, 1, 3], words) == [2, 0, 4]
    assert bj.resample([2, 1, 3], [0x55555555, 0x55555556, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0]) == [2, 2, 2], "x = 1, 2, 2, 3, 5, 0"
    (o,), undecided = bj.replicate([((1,), 2), ((4,), 1), ((6,), 3)], seed, cell, b)
    assert not undecided and o.row == {1: 2.0, 6: 4.0} and o.rounds == (0,), "no label of two ids: the sums as they are, nothing floored"
    j = bj.judge_cell({(6,): 3, (1,): 2, (4,): 1}, False, 8, 3, seed, cell)
    assert j.exact and len(j.combos) == 1 and j.combos[0][2] == {1: 2.0, 6: 4.0}


def test_the_start_by_hand():
    """em.rs:380: a f32 from the word's top 24 bits, plus 1e-5, both f32; it replaces the unique counts (em.rs:326, 370-381)."""
    assert bj.start_value(0) == ej._f32(1e-5) and bj.start_value(0xFF) == ej._f32(1e-5)
    assert bj.start_value(0x80000000) == ej._f32(0.5 + ej._f32(1e-5)) == 0.5000100135803223
    assert bj.start_value(0xFFFFFFFF) == ej._f32((2 ** 24 - 1) * 2.0 ** -24 + ej._f32(1e-5)) > 1.0, "the largest start is above 1"
    assert bj.start_value(0x9F90690F) == 0.6233072876930237
    # {0}: 50 and {0, 1}: 2.  From the informative start entry 0 would begin at 0.0505; here both begin under 1 and the loop is
    # run_loop's from there: one outcome, the two molecules shared by weight
    seed, cell = 7, 3
    classes = [((0,), 50), ((0, 1), 2)]
    (o,), undecided = bj.replicate(classes, seed, cell, 0)
    n0, n1 = bj.resample([50, 2], bj.stream(seed, cell, 0, 52))
    a = {x: bj.start_value(w) for x, w in zip((0, 1), bj.stream(seed, cell, 0, 2, start=True))}
    want, _ = ej.run_loop([((0,), n0), ((0, 1), n1)], None, "subset", a, {0, 1})
    assert not undecided and o.row == want[0].row and abs(sum(o.row.values()) - 52) < 1e-6


def test_the_canonical_class_order_by_hand():
    """Labels that are one output column first, by column; the others lexicographic.  Four genes in USA mode: S g, U 4 + g, A 8 + g."""
    order = lambda t, usa, nr: [lab for lab, _ in bj.canonical_order(t, usa, nr)]
    t = {(2, 3): 1, (5,): 1, (0, 2): 1, (2,): 1, (0, 1, 2): 1, (0,): 1}
    assert order(t, False, 8) == [(0,), (2,), (5,), (0, 1, 2), (0, 2), (2, 3)]
    # USA: {2} is S_1 (column 1), {5} U_2 (6), {0} S_0 (0), {2, 3} A_1 (9), {0, 1, 2} is {A_0, S_1}: two columns
    assert order(t, True, 12) == [(0,), (2,), (5,), (2, 3), (0, 1, 2), (0, 2)]
    assert order({(7,): 1, (4,): 1, (6, 7): 1, (1,): 1}, True, 12) == [(4,), (1,), (7,), (6, 7)], "S_2 0 + 2, U_0 4 + 0, U_3 4 + 3, A_3 8 + 3"
    # the support is the gene ids as they are, ascending, siblings or not (quant.rs:1028-1038: usa_offsets None)
    j = bj.judge_cell({(6, 7): 3, (1, 4): 2}, True, 12, 1, 5, 0)
    assert not j.exact and set().union(*(set(r) for c in j.combos for r in c)) <= {1, 4, 6, 7}


def test_the_summaries_by_hand():
    reps = ({0: 1.0, 1: 4.0}, {0: 2.0}, {0: 6.0, 1: 2.0}, {0: 3.0, 2: 0.5})
    s = bj.summaries(reps, True)                    # em.rs:662-683: sq / B - mean^2
    assert s[0][:2] == (3.0, 50 / 4 - 9.0) and s[1][:2] == (1.5, 20 / 4 - 2.25) and s[2][:2] == (0.125, 0.0625 - 0.125 ** 2)
    r = bj.summaries(reps, False)                   # quant.rs:185-210: / (n - 1)
    assert r[0][:2] == (3.0, 14 / 3) and r[1][:2] == (1.5, (6.25 + 2.25 + 0.25 + 2.25) / 3)
    assert bj.summaries_f32(reps, True) == ({0: 3.0, 1: 1.5, 2: 0.125}, {0: 3.5, 1: 2.75, 2: 0.046875})
    # f32 where it rounds: three replicates of 1, 1, 2: the mean is f32(4 / 3), the deviations are f32's
    m, v = bj.summaries_f32(({0: 1.0}, {0: 1.0}, {0: 2.0}), False)
    f = ej._f32
    mean = f(4.0 / 3.0)
    d1, d2 = f(1.0 - mean), f(2.0 - mean)
    assert m == {0: mean} and v == {0: f(f(f(f(d1 * d1) + f(d1 * d1)) + f(d2 * d2)) / 2.0)} and mean == 1.3333333730697632
    m, v = bj.summaries_f32(({0: 1.0}, {0: 1.0}, {0: 2.0}), True)
    assert v == {0: f(f(6.0 / 3.0) - f(mean * mean))}
    # an entry whose mean is 0 has neither; a variance of 0 is not written; the --summary-stat variance can be negative
    assert bj.summaries_f32(({0: 2.0}, {0: 2.0}), False) == ({0: 2.0}, {}) and bj.summaries_f32(({}, {}), True) == ({}, {})
    m, v = bj.summaries_f32(tuple({0: f(0.7)} for _ in range(5)), True)
    assert m == {0: f(0.7)} and v == {0: -(2.0 ** -25)}, "five replicates of f32(0.7): sq / 5 rounds under mean^2"


@pytest.mark.parametrize("summary_stat", [False, True])
def test_one_replicate_has_no_variance(summary_stat):
    """B = 1: quant.rs:199-204 the one deviation is 0; em.rs:676-679 sq / 1 - mean^2 is 0 in f32 as well."""
    assert bj.summaries_f32(({0: 0.3, 4: 17.0},), summary_stat) == ({0: ej._f32(0.3), 4: 17.0}, {})
    for name in ("hand", "usa"):
        got = _oracle_run(name, "cr-like-em", 1, summary_stat, bc.SEEDS[0])
        means, variances = bc.boot_rows(got.bootstraps, got.n_cells)
        assert any(means) and not any(variances)
        for cell, j, mean, var in _cells(name, "cr-like-em", 1, summary_stat, bc.SEEDS[0], 200):
            assert bj.admits(j, mean, var, summary_stat) is True, cell
            c = min(mean)           # (the --summary-stat bound is 2.2e-5 of twice the mean's square; without, it is 0)
            assert isinstance(bj.admits(j, mean, {c: 1e-3 * mean[c] ** 2}, summary_stat), str), cell


# ------------------------------------------------------------------------------------------- the oracle in front of the judge

def _judge_oracle(name, res, B, summary_stat, seed):
    b = ec.quant_batch(name)
    what = f"{name} {res} B={B} summary_stat={summary_stat} seed {seed:#x}"
    t = bc.judge_result(b, _oracle_run(name, res, B, summary_stat, seed), B, summary_stat, seed, bc.FIRST, what)
    bc.assert_the_cap(name, t, what)
    return t


@pytest.mark.parametrize("name,res", bc.CASES)
def test_oracle_bootstraps_are_admitted(name, res):
    for seed in bc.SEEDS:
        for B in bc.BOOTS:
            for summary_stat in (False, True):
                _judge_oracle(name, res, B, summary_stat, seed)


@pytest.mark.parametrize("name", list(bc.EDGE_RUNS))
def test_oracle_bootstraps_of_the_edge_cells_are_admitted(name):
    """The cells that tests/test_gpu_boot_judge.py builds at the bootstrap kernel's edges, with the oracle: that each does what it
    was built for is asserted by boot_judge_cases.run_edge, here without a device."""
    bc.run_edge(name, lambda cfg, b, first: ora.quant(cfg, b.t2g, b.data, b.off, first_cell_index=first))


def test_the_exact_layer_judges_its_share():
    """Cells without a label of two ids are judged bit for bit, with no tolerance at all, in both modes: a third of the `base`
    cells under cr-like-em, and the hand cell "unique-only"."""
    for summary_stat in (False, True):
        t = _judge_oracle("base", "cr-like-em", 4, summary_stat, bc.SEEDS[0])
        assert t.exact >= 0.25 * t.n
        b = ec.quant_batch("hand")
        got = _oracle_run("hand", "cr-like-em", 4, summary_stat, bc.SEEDS[0])
        i = b.names.index("unique-only")
        j = bc.judge_table(qc.classes_of(got)[i], False, b.num_rows, 4, bc.SEEDS[0], bc.FIRST + i)
        assert j.exact and len(j.combos) == 1
        mean, var = bj.summaries_f32(j.combos[0], summary_stat)
        means, variances = bc.boot_rows(got.bootstraps, got.n_cells)
        assert dict(means[i]) == mean and dict(variances[i]) == var and len(var) >= 2


def test_gap_measurement():
    """The two measured figures of boot_judge.py: the largest relative gap between the judge's mean and the oracle's, in units of
    2^-24, and the largest variance error as a share of its derived bound, over every case of test_oracle_bootstraps_are_admitted.
    The gap has to stay at or under em_judge.K units - half the bar - and both at or under what boot_judge.py records."""
    gap, ratio = (0.0, ""), (0.0, "")
    for name, res in bc.CASES:
        for seed in bc.SEEDS:
            for B in bc.BOOTS:
                for summary_stat in (False, True):
                    t = _judge_oracle(name, res, B, summary_stat, seed)
                    gap, ratio = max(gap, t.gap), max(ratio, t.ratio)
    print(f"\nlargest mean gap: {gap[0]:.2f} units of 2^-24 ({gap[1]}); largest variance error: {ratio[0]:.3f} of its bound ({ratio[1]})")
    assert gap[0] <= ej.K, "the gap is above half the bar: the bootstrap bar needs a constant of its own (boot_judge.py)"
    assert gap[0] <= bj.BOOT_GAP_UNITS + 0.05, "the gap has drifted above what boot_judge.py records"
    assert ratio[0] <= bj.BOOT_VAR_RATIO + 0.005 < 0.5, "the variance error has drifted above what boot_judge.py records"
    assert bj.MEAN_BAR == ej.TIGHT_BAR == 2 * ej.K * ej.U32 < ej.HARD_BAR


# ---------------------------------------------------------------------------------------------------------- the judge has teeth

TEETH = (("base", "cr-like-em"), ("usa", "parsimony-em"))
SEED = bc.SEEDS[0]


def _refused_share(pairs, what, least):
    """pairs: (cell, judgement, mean, var, summary_stat) of rows that are NOT the judgement's own.  Returns the refused share."""
    n = refused = 0
    for cell, j, mean, var, summary_stat in pairs:
        n += 1
        refused += isinstance(bj.admits(j, mean, var, summary_stat), str)
    print(f"\n{what}: {refused} of {n} refused")
    assert n >= 200 and refused >= least * n, (what, refused, n)


def _distinct_next(name, res, summary_stat, wrong):
    """The oracle's rows of cell i before the judge of cell i's table under a wrong index or seed (wrong(judge arguments))."""
    b = ec.quant_batch(name)
    got = _oracle_run(name, res, 4, summary_stat, SEED)
    tables, flags = qc.classes_of(got), got.flags.tolist()
    means, variances = bc.boot_rows(got.bootstraps, got.n_cells)
    for i, table in enumerate(tables[:400]):
        # one class, or one molecule, draws the same under every stream
        if not flags[i] & qj.FLAG_TINY and len(table) > 1 and sum(n for _, n in table) >= 8:
            j = bc.judge_table(table, b.usa, b.num_rows, 4, *wrong(SEED, bc.FIRST + i))
            if not j.undecided:
                yield b.names[i], j, means[i], variances[i], summary_stat


@pytest.mark.parametrize("name,res", TEETH)
@pytest.mark.parametrize("summary_stat", [False, True])
def test_the_judge_refuses_the_neighbours_result(name, res, summary_stat):
    """Cell i's result is not cell i + 1's: the cell index is in the counter.  (Two streams can draw the same counts for a
    cell of two or three classes and eight molecules; 95 % of the cells must be refused.)"""
    _refused_share(_distinct_next(name, res, summary_stat, lambda seed, c: (seed, c + 1)), f"{name} {res}: cell i as cell i + 1", 0.95)


@pytest.mark.parametrize("name,res", TEETH)
@pytest.mark.parametrize("summary_stat", [False, True])
def test_the_judge_refuses_another_seeds_result(name, res, summary_stat):
    _refused_share(_distinct_next(name, res, summary_stat, lambda seed, c: (seed + 1, c)), f"{name} {res}: seed s as seed s + 1", 0.95)


def _single(name, res, summary_stat):
    """The cells with one combination that are not exact: where the bars, not bits, decide."""
    for cell, j, mean, var in _cells(name, res, 4, summary_stat, SEED, 600):
        if len(j.combos) == 1 and not j.exact:
            assert bj.admits(j, mean, var, summary_stat) is True, cell
            yield cell, j, mean, var, bj.summaries(j.combos[0], summary_stat)


@pytest.mark.parametrize("name,res", TEETH)
@pytest.mark.parametrize("summary_stat", [False, True])
def test_the_judge_refuses_a_moved_mean_and_a_dropped_variance(name, res, summary_stat):
    n = dropped = 0
    for cell, j, mean, var, judged in _single(name, res, summary_stat):
        n += 1
        c = max(mean, key=mean.get)
        assert isinstance(bj.admits(j, {**mean, c: mean[c] * (1 + 3 * bj.MEAN_BAR)}, var, summary_stat), str), f"{cell}: a mean moved by three bars"
        assert bj.admits(j, {**mean, c: mean[c] * (1 + 3 * bj.MEAN_BAR)}, var, summary_stat, tight=False) is True, cell
        assert isinstance(bj.admits(j, {**mean, c: mean[c] * (1 + 2e-4)}, var, summary_stat, tight=False), str), cell
        assert isinstance(bj.admits(j, {k: v for k, v in mean.items() if k != c}, var, summary_stat), str), f"{cell}: a mean dropped"
        for c, (_, v, bound) in judged.items():
            if abs(v) > bound:
                dropped += 1
                assert c in var, cell
                assert isinstance(bj.admits(j, mean, {k: x for k, x in var.items() if k != c}, summary_stat), str), f"{cell}: variance {v!r} of {c} dropped"
            elif c in var:
                assert bj.admits(j, mean, {k: x for k, x in var.items() if k != c}, summary_stat) is True, f"{cell}: variance {v!r} of {c} within {bound!r} of 0"
    print(f"\n{name} {res}: {n} cells, {dropped} variances above their bound dropped, all refused")
    assert n >= 200 and dropped >= 2 * n


@pytest.mark.parametrize("name,res", TEETH)
def test_the_judge_refuses_a_variance_over_n(name, res):
    """quant.rs:203 divides by n - 1: a replicate-mode variance recomputed with / B is 3 / 4 of it."""
    n = 0
    for cell, j, mean, var, judged in _single(name, res, False):
        if any(abs(v) / 4 > 2 * bound for _, v, bound in judged.values()):
            n += 1
            assert isinstance(bj.admits(j, mean, {c: ej._f32(v * 3 / 4) for c, v in var.items()}, False), str), cell
    print(f"\n{name} {res}: {n} cells with a variance recomputed over n, all refused")
    assert n >= 200


@pytest.mark.parametrize("name,res", TEETH)
def test_the_judge_refuses_one_mode_for_the_other(name, res):
    """A --summary-stat result presented as a replicate-mode one, on the cells where the two differ by more than the bounds."""
    n = 0
    summary = {cell: (mean, var) for cell, _, mean, var, _ in _single(name, res, True)}
    for cell, j, mean, var, judged in _single(name, res, False):
        other = bj.summaries(j.combos[0], True)
        if cell in summary and any(abs(judged[c][1] - other[c][1]) > 2 * (judged[c][2] + other[c][2]) for c in judged):
            n += 1
            assert isinstance(bj.admits(j, *summary[cell], False), str), cell
            assert isinstance(bj.admits(j, mean, var, True), str), cell
    print(f"\n{name} {res}: {n} cells whose two summaries differ, each refused as the other")
    assert n >= 200


def test_an_undecided_cell_admits_nothing():
    assert isinstance(bj.admits(bj.Judgement([], False, True, 4), {}, {}, False), str)
