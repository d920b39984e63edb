"""CPU: what the builders of tests/giant_cell_cases.py reach and that its expectations are right (no GPU needed).

The formulas for the pattern's rows and class table are held against tests/quant_judge.py read by read on miniatures, and against
the oracle's rows and -d class table at full size (2^22 - 1, 2^22, 2^22 + 1 and 2^23 reads).  The restated `fbits` gives 40, 39,
39 and 38 there.  On every EM cell of the module - the pattern cells and the {A, B} cells whose accumulator starts just under
2^62 - the oracle's two arithmetics agree within 1e-4 and cut the same entries at the floor (tests/test_em_arith_cpu.py's
statement, which stops at F = 40), tests/em_judge.py decides the cell and admits both, and the gap between the judge and the
reference's arithmetic is measured: the device's tight bar in tests/test_gpu_giant_cells.py is four times that gap."""
import functools
import math
import os
import sys

import numpy as np
import pytest

import em_edges as E
import em_judge as ej
import giant_cell_cases as gc
import quant_judge as qj
import quant_judge_cases as qc
from util import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as ora  # noqa: E402

SEEDS = (0, 11, 12, 13)      # the canonical class order and the suite's three shuffles
PATTERN_CELLS = [(N, usa) for N in gc.SIZES for usa in (False, True)] + [(gc.BIG, False)]
AB_CELLS = [(N, usa) for N in gc.SIZES + (gc.BIG,) for usa in (False, True)]


def _em_runs(cfg, t2g, b, off):
    """{(arith, seed): (rows, tables, rounds, flags)} of the oracle under cr-like-em: fixed point, and the reference's arithmetic
    in the canonical and three shuffled class orders."""
    out = {}
    for arith, seed in [("fixed", 0)] + [("reference", s) for s in SEEDS]:
        r, it = ora.quant(cfg, t2g, b, off, em_arith=arith, em_order_seed=seed, want_iters=True)
        out[arith, seed] = (qc.rows_of(r), qc.classes_of(r), it.tolist(), r.flags.tolist())
    return out


@functools.lru_cache(maxsize=None)
def _pattern_runs(N, usa):
    """The oracle on [50, N, 600] reads of the pattern: the cr-like and trivial rows and the cr-like-em runs; once per process
    (rows and tables only: the bytes are not kept)."""
    b, off = gc.pattern_batch(N)
    plain = {res: qc.rows_of(ora.quant(gc.cfg(res, usa), gc.t2g(usa), b, off)) for res in ("cr-like", "trivial")}
    return plain, _em_runs(gc.cfg("cr-like-em", usa, dump_eq=True), gc.t2g(usa), b, off)


@functools.lru_cache(maxsize=None)
def _ab_runs(N, usa):
    b, off = gc.ab_batch(N, usa)
    return _em_runs(gc.ab_cfg(usa, dump_eq=True), gc.ab_dims(usa)[0], b, off)


def _floats(row):
    return {c: float(v) for c, v in row.items()}


# ------------------------------------------------------------------------------------------------------- what the builders reach

def test_the_sizes_reach_each_value_of_the_scale_and_of_the_bucket_plan():
    assert [gc.fbits(N) for N in gc.SIZES + (gc.BIG,)] == [40, 39, 39, 38]
    assert [gc.fbits(n) for n in (1, 30000, 2 ** 22 - 1, 2 ** 23 - 1, 2 ** 24)] == [40, 40, 40, 39, 37]
    assert [gc.lg_nb(N) for N in gc.SIZES + (gc.BIG,)] == [14, 14, 15, 15]          # one ref a read: n_ref = N
    assert gc.G % 3 and all(n < 2 ** 22 for n in gc.NEIGHBOURS) and gc.NEIGHBOURS[0] < gc.SMALL_THRESH <= gc.NEIGHBOURS[1]
    # the accumulator of entry A starts at uA << F: just under 2^62 at 2^22 - 1 reads, about 2^61 at 2^22 and 2^23 ...
    starts = [gc.ab_counts(N)[0] << gc.fbits(N) for N in gc.SIZES + (gc.BIG,)]
    assert 0.999 * 2 ** 62 < starts[0] < 2 ** 62 and all(0.999 * 2 ** 61 < s < 2 ** 62 for s in starts[1:])
    # ... and stays under 2^62 whatever the EM gives A (every molecule of the cell on one entry); with F left at 40
    # that bound is gone from 2^22 reads on, and at 2^23 reads entry A alone would start at 2^63
    assert all((N << gc.fbits(N)) < 2 ** 62 for N in gc.SIZES + (gc.BIG,))
    assert [N << 40 >= 2 ** 62 for N in gc.SIZES + (gc.BIG,)] == [False, True, True, True]
    assert 0.999 * 2 ** 63 < gc.ab_counts(gc.BIG)[0] << 40 < 2 ** 63


def test_the_encoded_cells_hold_what_was_asked_for():
    b, off = gc.encode_pattern((50, 223, 600))
    w = np.frombuffer(b, np.uint32)
    assert [int(w[int(o) // 4 + 1]) for o in off] == [50, 223, 600]
    cells = [gc.rad.decode_chunk(bytes(b), int(o), 4, 4) for o in off]
    for n, (bc, reads) in zip((50, 223, 600), cells):
        assert [(int(u), [int(x) for x in r]) for u, r in reads] == gc.reads_as_lists(n)
    b, off = gc.ab_batch(1005 + 40, True)
    _, reads = gc.rad.decode_chunk(bytes(b), 0, 4, 4)
    assert len(reads) == 1045 and len({u for u, _ in reads}) == 1045
    labels = [tuple(int(x) for x in r) for _, r in reads]
    assert (labels.count((0,)), labels.count((0, 2)), labels.count((2,))) == (40, gc.AB_AMB, gc.AB_UB)


# --------------------------------------------------------------------------------------------- the formulas, on miniatures

@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("n", [1, 2, 50, 221, 222, 223, 224, 225, 226, 600, 667])
def test_formulas_against_the_judge_read_by_read(n, usa):
    """tests/quant_judge.py on every read of a miniature: the cr-like row and class table, the trivial row."""
    reads, t2g, num_rows = gc.reads_as_lists(n), gc.t2g(usa).tolist(), gc.dims(usa)[1]
    j = qj.judge_cell(reads, t2g, "cr-like", usa, num_rows=num_rows, small_thresh=0)
    assert qj.admits(j, row=gc.crlike_row(n, usa), classes=gc.class_table(n, usa)) is True
    j = qj.judge_cell(reads, t2g, "cr-like-em", usa, num_rows=num_rows, small_thresh=0)
    assert qj.admits(j, classes=gc.class_table(n, usa)) is True
    j = qj.judge_cell(reads, t2g, "trivial", usa, num_rows=num_rows, small_thresh=0)
    assert qj.admits(j, row=gc.trivial_row(n, usa)) is True
    assert sum(gc.class_table(n, usa).values()) == (n + 1) // 2                      # a molecule a UMI
    if n >= 6 * gc.G:                                                                # every case on every gene
        assert len(gc.class_table(n, usa)) == (3 if usa else 2) * gc.G


def test_the_shape_from_a_class_table_is_em2_shapes():
    """shape_of_table counts molecules from the table; em_edges.em2_shape from the molecules themselves."""
    for n, usa in ((600, False), (600, True), (667, True)):
        table = gc.class_table(n, usa)
        uniq, amb = {}, []
        for lab, cnt in table.items():
            lab_em = E.em_label(list(lab), gc.G, usa)
            if len(lab_em) == 1:
                uniq[lab_em[0]] = cnt
            else:
                amb += [list(lab)] * cnt
        assert gc.shape_of_table(table, usa, gc.G) == E.em2_shape(E.Cell(uniq=uniq, amb=amb), gc.G, usa)
    assert gc.shape_of_table(gc.ab_class_table(2000, True), True, 2) == E.em2_shape(E.ab_cell(gc.AB_AMB, 995, gc.AB_UB, True), 2, True)


# ------------------------------------------------------------------------------------------------ the formulas, at full size

@pytest.mark.parametrize("N,usa", PATTERN_CELLS)
def test_formulas_equal_the_oracle_at_full_size(N, usa):
    """The oracle's cr-like and trivial rows and its -d class table of [50, N, 600] reads are the formulas'."""
    plain, em = _pattern_runs(N, usa)
    for res in ("cr-like", "trivial"):
        for k, n in enumerate(gc.batch_sizes(N)):
            assert dict(plain[res][k]) == _floats(gc.plain_row(res, n, usa)), f"{res} cell of {n} reads"
    rows, tables, _, flags = em["fixed", 0]
    assert [bool(f & qj.FLAG_TINY) for f in flags] == [True, False, False]
    assert dict(rows[0]) == _floats(gc.crlike_row(gc.NEIGHBOURS[0], usa))          # the tiny neighbour: no EM
    for k in (1, 2):
        assert dict(tables[k]) == gc.class_table(gc.batch_sizes(N)[k], usa)
    assert sum(gc.class_table(N, usa).values()) == (N + 1) // 2
    # the giant cell runs the streamed instance (more classes than 16-bit ids hold), its 600-read neighbour the smallest
    assert [gc.shape_of_table(gc.class_table(n, usa), usa, gc.G).tier for n in gc.batch_sizes(N)[1:]] == [3, 0]


# ------------------------------------------------------------------------------------------------------------ the EM cells

def _judge_both_arithmetics(runs, k, table, num_rows, usa, what):
    """Cell k of the runs: the two arithmetics against each other, then both before the judge.  Returns the largest gap between
    the judge and the reference's arithmetic, in units of 2^-24."""
    fix, ref = runs["fixed", 0], runs["reference", 0]
    assert dict(fix[1][k]) == dict(ref[1][k]) == table, what
    frow, rrow = dict(fix[0][k]), dict(ref[0][k])
    assert set(frow) == set(rrow), f"{what}: the arithmetics cut different entries at the floor"
    assert max(abs(frow[c] - rrow[c]) / rrow[c] for c in rrow) <= 1e-4, what
    outcomes, undecided = gc.judge(table, num_rows, usa)
    assert not undecided and 1 <= len(outcomes) <= ej.MAX_OUTCOMES, f"{what}: {len(outcomes)} outcomes, undecided {undecided}"
    worst = 0.0
    for (arith, seed), (rows, _, iters, _) in runs.items():
        row = dict(rows[k])
        m = ej.admits(outcomes, row)
        assert m is True, f"{what} {arith} order {seed}: {m}"
        assert any(iters[k] in f.rounds for f in ej.fitting(outcomes, row)), f"{what} {arith} order {seed}: oracle {iters[k]} rounds"
        if arith == "reference":
            worst = max(worst, gc.gap_units(outcomes, row, iters[k]))
    return worst


@pytest.mark.parametrize("N,usa", PATTERN_CELLS)
def test_pattern_cells_before_the_em_judge(N, usa):
    _, em = _pattern_runs(N, usa)
    for k in (1, 2):
        n = gc.batch_sizes(N)[k]
        _judge_both_arithmetics(em, k, gc.class_table(n, usa), gc.dims(usa)[1], usa, f"pattern cell of {n} reads, usa={usa}")


@pytest.mark.parametrize("N,usa", AB_CELLS)
def test_accumulator_cells_before_the_em_judge(N, usa):
    """F = 40, 39, 39, 38: the arithmetics agree, the judge admits both, and the closed form gives the value."""
    runs = _ab_runs(N, usa)
    _judge_both_arithmetics(runs, 0, gc.ab_class_table(N, usa), gc.ab_dims(usa)[2], usa, f"{{A, B}} cell of {N} reads, usa={usa}")
    rows, _, iters, _ = runs["fixed", 0]
    want = gc.ab_row_f64(N, iters[0])
    row = dict(rows[0])
    assert set(row) == {0, 1} and all(abs(row[c] - want[c]) <= gc.GIANT_TIGHT_BAR * want[c] for c in want), (row, want)


def test_the_em_bar_of_these_cells():
    """Section 4's measurement: the largest gap between em_judge and the oracle in the REFERENCE's arithmetic over the canonical
    and the three shuffled class orders, on every pattern cell (its 600-read neighbour included) and every {A, B} cell.  The
    device's tight bar is four times what giant_cell_cases records, and has to stay under the hard bar of 1e-4."""
    worst = (0.0, "")
    for N, usa in PATTERN_CELLS:
        _, em = _pattern_runs(N, usa)
        for k in (1, 2):
            n = gc.batch_sizes(N)[k]
            gap = _judge_both_arithmetics(em, k, gc.class_table(n, usa), gc.dims(usa)[1], usa, f"pattern {n} usa={usa}")
            worst = max(worst, (gap, f"pattern cell of {n} reads, usa={usa}"))
    for N, usa in AB_CELLS:
        gap = _judge_both_arithmetics(_ab_runs(N, usa), 0, gc.ab_class_table(N, usa), gc.ab_dims(usa)[2], usa, f"ab {N} usa={usa}")
        worst = max(worst, (gap, f"{{A, B}} cell of {N} reads, usa={usa}"))
    print(f"\nlargest judge-to-reference gap on the giant cells: {worst[0]:.2f} units of 2^-24 ({worst[1]}); recorded {gc.GAP_UNITS}, "
          f"K = {gc.GIANT_K}, tight bar {gc.GIANT_TIGHT_BAR:.3g}")
    assert worst[0] <= gc.GAP_UNITS + 0.05, "the gap has drifted above what giant_cell_cases.py records"
    assert gc.GIANT_K == math.ceil(4 * gc.GAP_UNITS) and gc.GIANT_TIGHT_BAR == 2 * gc.GIANT_K * ej.U32 < ej.HARD_BAR
    assert worst[0] < gc.GIANT_K, "the measured gap is above half the bar: measure again"
