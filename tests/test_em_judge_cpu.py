"""The EM judge (tests/em_judge.py) against cells worked out by hand, and the oracle in front of the judge.

The oracle and the kernels were written from one reading of src/em.rs; the judge is a second, in float64 and plain Python, from the
reference's text alone.  Every oracle row - both arithmetics, the canonical class order and three shuffled ones, both
initialisations, `quant` and `infer` - has to be one of the judge's outcomes under the project's 1e-4 and under the tight bar of
2 K units of 2^-24, with the judge's round count where it has one.  The last tests show that the judge refuses what is wrong."""
import functools
import math
import os
import sys

import numpy as np
import pytest

import em_edges as E
import em_judge as ej
import em_judge_cases as ec
import quant_judge as qj
import quant_judge_cases as qc
from util import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as ora  # noqa: E402

SEEDS = (0, 11, 12, 13)          # the canonical class order and the suite's three shuffles (util.assert_em_within_the_reference_envelope)
INITS = {"informative": False, "uniform": True}


@functools.lru_cache(maxsize=None)
def _oracle_run(name, res, arith, init, seed):
    """(rows, class tables, rounds, flags) of the oracle on a quant batch; computed once per process, shared, never changed."""
    b = ec.quant_batch(name)
    r, iters = ora.quant(b.cfg(res, dump_eq=True, em_init_uniform=INITS[init]), b.t2g, b.data, b.off, want_iters=True, em_arith=arith,
                         em_order_seed=seed)
    return qc.rows_of(r), qc.classes_of(r), iters.tolist(), r.flags.tolist()


def _gap_units(o, row):
    return max((abs(v - o.row[c]) / o.row[c] / ej.U32 for c, v in row), default=0.0)


def _judge_rows(b, rows, tables, iters, flags, init, what):
    """Every EM row before the judge of its own class table.  Returns (judged, largest gap in units of 2^-24)."""
    judged, gap = [], 0.0
    for i, row in enumerate(rows):
        if flags[i] & qj.FLAG_TINY:          # quant.rs:794-846: no EM ran; tests/quant_judge.py judges these rows
            continue
        o, u = ec.judge_table(tables[i], b.num_rows, b.usa, "quant", init)
        judged.append((o, u))
        if u:
            continue
        m = ej.admits(o, row)
        assert m is True, f"{what}, {b.names[i]} ({len(o)} outcome(s), oracle rounds {iters[i]}): {m}"
        fit = ej.fitting(o, row)
        assert any(iters[i] in f.rounds for f in fit), f"{what}, {b.names[i]}: oracle {iters[i]} rounds, judge {[f.rounds for f in fit]}"
        if len(o) == 1 and len(o[0].rounds) == 1:
            assert iters[i] == o[0].rounds[0], f"{what}, {b.names[i]}"
        gap = max(gap, _gap_units(fit[0], row))
    return judged, gap


# ------------------------------------------------------------------------------------------------------------------ by hand

def test_constants_are_the_references():
    assert (ej.MIN_ITER, ej.MAX_ITER) == (2, 100)                                                    # em.rs:32-33
    f32 = float(np.float32(0.01))
    assert ej.MIN_OUTPUT_ALPHA == ej.ALPHA_CHECK_CUTOFF == ej.REL_DIFF_TOLERANCE == f32              # em.rs:29-30, 34
    assert ej.K == math.ceil(4 * ej.GAP_UNITS) and ej.TIGHT_BAR == 2 * ej.K * 2.0 ** -24 < ej.HARD_BAR


def test_usa_labels_by_hand():
    """utils.rs:842-926 with six genes: S g, U 6 + g, A 12 + g."""
    L = lambda *ids: ej.usa_em_label(ids, 18)
    assert L(4) == (2,) and L(5) == (8,)
    assert L(4, 5) == (14,), "{S_2, U_2} is the one entry A_2"
    assert L(2, 4, 5) == (1, 14), "U_2 follows S_2, not S_1"
    assert L(2, 3, 4) == (13, 2) and L(3, 4) == (7, 2), "an unspliced id never pairs with what follows it"
    assert L(1, 2, 5, 6, 7, 9) == (6, 1, 8, 15, 10), "not re-sorted"
    long = tuple(range(0, 24, 2)) + (23,)       # twelve genes: S_0 .. S_10, then S_11 with its U_11
    assert ej.usa_em_label(long, 36) == tuple(range(11)) + (24 + 11,), "nothing is cut at ten ids"
    assert ej.usa_em_label(long[:-1], 36) == tuple(range(12))


def test_update_by_hand():
    a = {0: 1.0, 1: 3.0, 2: 0.0}
    assert ej.update(a, [((0,), 5), ((0, 1), 8), ((2, 3), 4)], None) == {0: 7.0, 1: 6.0}, "a denominator of 0 gives nothing"
    # three genes: S_0 = 1, U_0 = 2 (index 3), A_0 = 4 (index 6), S_1 = 8
    a = {0: 1.0, 3: 2.0, 6: 4.0, 1: 8.0}
    assert [ej.abundance(x, a, 3, 6) for x in (0, 3, 6, 1, 4, 7)] == [5.0, 6.0, 7.0, 8.0, 0.0, 8.0]       # em.rs:167-187
    out = ej.update(a, [((0, 1), 13), ((6, 1), 15)], (3, 6))
    assert out == {0: 5.0, 1: 8.0 + 8.0, 6: 7.0}
    assert ej.support_of([((0, 7), 1)], (3, 6)) == {0, 6, 7, 4, 1}                                           # em.rs:97-112


def _one(judged):
    (o,), u = judged
    assert not u
    return o


def test_hand_cells_do_what_they_were_built_for():
    G = ec.HAND_G
    cells = dict(ec.hand_cells(False))
    table = lambda c, usa=False: ej.em_classes(E.gene_classes(c, G, usa), usa, 3 * G if usa else G)
    # no multi-entry class: two rounds in the dense loop, none in the subset loop, the same counts
    t = table(cells["unique-only"])
    d, s = _one(ej.judge_em(t, G, False, "dense")), _one(ej.judge_em(t, G, False, "subset"))
    assert d.row == s.row == {0: 3.0, 5: 1.0, 9: 12.0} and d.rounds == (2,) and s.rounds == (0,)
    # the two loops differ: by 3e-5 relative, between the tight bar and 1e-4
    t = table(cells["dense-and-subset-differ"])
    d, s = _one(ej.judge_em(t, G, False, "dense")), _one(ej.judge_em(t, G, False, "subset"))
    assert d.rounds == (3,) and s.rounds == (4,) and set(d.row) == set(s.row) == {0} and s.row[0] == 45.0
    assert ej.TIGHT_BAR < (s.row[0] - d.row[0]) / 45 < ej.HARD_BAR
    assert isinstance(ej.admits([d], s.row), str) and isinstance(ej.admits([s], d.row), str) and ej.admits([s], d.row, tight=False) is True
    # onto the floor: optional at the end in the dense loop, two outcomes in the subset loop
    t = table(cells["onto-the-floor"])
    d = _one(ej.judge_em(t, G, False, "dense"))
    assert d.optional == {1} and abs(d.row[1] - ej.MIN_OUTPUT_ALPHA) < ej.margin(0.01, 0.01) / 3
    assert ej.admits([d], d.row) is True and ej.admits([d], {c: v for c, v in d.row.items() if c != 1}) is True
    assert isinstance(ej.admits([d], {c: v for c, v in d.row.items() if c != 0}), str)
    outs, u = ej.judge_em(t, G, False, "subset")
    assert not u and sorted(o.row[0] for o in outs) == [pytest.approx(34.9962861, abs=1e-6), 35.0] and all(set(o.row) == {0, 2} for o in outs)
    # entries of 12 342 and 9 244: margins above the tolerance, so every round from the first converged one to the cap is a place
    # to stop; the rows stop moving and merge
    outs, u = ej.judge_em(table(cells["lost-molecule"]), G, False, "dense")
    rounds = sorted(r for o in outs for r in o.rounds)
    assert not u and 1 < len(outs) < 10 and rounds == list(range(rounds[0], 101)) and rounds[0] < 10
    # USA
    cells = dict(ec.hand_cells(True))
    assert table(cells["pair-alone"], True) == [((2 * G + 3,), 7)]
    o = _one(ej.judge_quant_em(E.gene_classes(cells["pair-alone"], G, True), 3 * G, True))
    assert o.row == {2 * G + 3: 7.0} and o.rounds == (0,)
    assert sorted(len(l) for l, _ in table(cells["more-than-ten-ids"], True) if len(l) > 1) == [11, 12]
    assert ((1, 2 * G + 2), 6) in table(cells["u-follows-its-own-s"], True) and ((G + 1, 2), 5) in table(cells["u-then-s"], True)
    # a class of count 0 whose entries are all 0 in the last round
    b = ec.infer_batch("hand")
    o = _one(ej.judge_em(b.rows[b.names.index("floored-class-denominator-0")], b.num_rows, False, "subset"))
    assert o.row == {0: 45.0} and o.rounds == (4,)


def test_round_control_by_hand():
    """The cap, and the round after a convergence at round 100."""
    o = _one(ej.judge_em([((0, 1), 300), ((1,), 3)], 4, False, "dense"))
    assert o.rounds == (100,)
    o = _one(ej.judge_em([((0, 1), 300), ((1,), 3)], 4, False, "subset"))
    assert o.rounds == (100,), "capped unconverged: no last round (em.rs:434)"
    outs, u = ej.judge_em(ec.infer_batch("rounds-usa").rows[2], 12, True, "subset")
    assert not u and (101,) in [o.rounds for o in outs]


# ------------------------------------------------------------------------------------------- the oracle in front of the judge

@pytest.mark.parametrize("name,res", ec.QUANT_CASES)
def test_oracle_quant_rows_are_admitted(name, res):
    b = ec.quant_batch(name)
    for init in INITS:
        judged = None
        for arith in ("reference", "fixed"):
            for seed in SEEDS if arith == "reference" else SEEDS[:2]:       # (the fixed-point sums are order-free)
                rows, tables, iters, flags = _oracle_run(name, res, arith, init, seed)
                what = f"{name} {res} {arith} order {seed} {init}"
                judged, _ = _judge_rows(b, rows, tables, iters, flags, init, what)
        ec.assert_the_judge_judges(judged, f"{name} {res} {init}")


@pytest.mark.parametrize("name", ["usa", "workload", "workload-usa", "hand", "hand-usa", "rounds-usa"])
def test_end_to_end_judgement_of_the_oracle(name):
    """What tests/test_gpu_em_judge.py does with the device, with the oracle in the device's arithmetic: reads to classes before
    tests/quant_judge.py, classes to row before the EM judge."""
    b = ec.quant_batch(name)
    for res in ec.EM_RES if name in ("usa", "workload", "workload-usa") else ec.EM_RES[:1]:
        got = ora.quant(b.cfg(res, dump_eq=True), b.t2g, b.data, b.off, em_arith="fixed")
        ec.judge_end_to_end(b, res, got, what=f"{name} {res}")


def _oracle_infer(ora, b, row, init, dense):
    labels, counts = [list(l) for l, _ in row], [n for _, n in row]
    uo = b.num_rows // 3
    alphas, iters = ora.em(labels, counts, b.num_rows, init_uniform=INITS[init], usa_offsets=(uo, 2 * uo) if b.usa else None, dense=dense)
    return [(int(c), float(alphas[c])) for c in np.flatnonzero(alphas > 0)], iters


@pytest.mark.parametrize("name", ec.INFER_BATCHES)
def test_oracle_infer_rows_are_admitted(oracle_module, name):
    """`infer` runs the subset loop in both modes (infer.rs:230); the reference's own dense_reference (em.rs:1049-1133) is the
    same loop over every alpha.  Without USA the oracle's em_optimize goes before the judge's dense loop on the same classes."""
    b = ec.infer_batch(name)
    for init in INITS:
        judged = []
        for cell, row in zip(b.names, b.rows):
            for loop, dense in (("subset", 0), ("subset", 2)) + ((("dense", 1),) if not b.usa and row else ()):
                o, u = ec.judge_table(row, b.num_rows, b.usa, loop, init)
                assert not u
                got, iters = _oracle_infer(oracle_module, b, row, init, dense)
                m = ej.admits(o, got)
                assert m is True, f"{name} {cell} {loop} {init}: {m}"
                assert any(iters in f.rounds for f in ej.fitting(o, got)), f"{name} {cell} {loop} {init}: oracle {iters} rounds"
                if loop == "subset" and dense == 0:
                    judged.append((o, u))
        ec.assert_the_judge_judges(judged, f"infer {name} {init}")


def test_margin_measurement():
    """K's measurement: the largest gap between the judge and the oracle IN THE REFERENCE'S ARITHMETIC, canonical and shuffled
    class orders, both initialisations, cr-like-em and parsimony-em on every quant batch, in units of 2^-24 of the value.  It has
    to stay under half the margin (2 K units), and K has to be four times what em_judge.py says was measured."""
    worst = (0.0, "")
    for name, res in ec.QUANT_CASES:
        b = ec.quant_batch(name)
        if res != "parsimony-gene-em":
            for init in INITS:
                for seed in SEEDS:
                    rows, tables, iters, flags = _oracle_run(name, res, "reference", init, seed)
                    _, gap = _judge_rows(b, rows, tables, iters, flags, init, f"{name} {res} {init} order {seed}")
                    worst = max(worst, (gap, f"{name} {res} {init} order {seed}"))
    print(f"\nlargest judge-to-reference gap: {worst[0]:.2f} units of 2^-24 ({worst[1]}); K = {ej.K}, tight bar {ej.TIGHT_BAR:.3g}, "
          f"margin of a comparison {2 * ej.K} units of the value")
    assert worst[0] < ej.K, "the measured gap is above half the margin: measure again and raise K"
    assert worst[0] <= ej.GAP_UNITS + 0.05, "the gap has drifted above what em_judge.py records"


# ---------------------------------------------------------------------------------------------------------- the judge has teeth

def _mutant(classes, num_rows, usa, loop, init="informative", no_u_sibling=False, early=0, skip_floor=False):
    """The EM once more, single-minded (no margins), with the switches of the mutations.  Returns (row, rounds).
    no_u_sibling: an ambiguous entry weighs S + A only; early: stop that many rounds before the convergence;
    skip_floor: the subset loop without its floor and last round."""
    offsets = (num_rows // 3, 2 * (num_rows // 3)) if usa else None
    unique = {}
    for lab, n in classes:
        if len(lab) == 1:
            unique[lab[0]] = unique.get(lab[0], 0.0) + n
    if loop == "subset" and all(len(lab) == 1 for lab, _ in classes):
        return {c: v for c, v in unique.items() if v > 0}, 0

    def weight(x, a):
        if offsets is None:
            return a.get(x, 0.0)
        if no_u_sibling and x >= offsets[1]:
            return a.get(x - offsets[1], 0.0) + a.get(x, 0.0)
        return ej.abundance(x, a, *offsets)

    def update(a):
        out = {}
        for lab, n in classes:
            if len(lab) == 1:
                out[lab[0]] = out.get(lab[0], 0.0) + n
                continue
            w = [weight(x, a) for x in lab]
            if sum(w) > 0:
                for x, wx in zip(lab, w):
                    out[x] = out.get(x, 0.0) + wx * n / sum(w)
        return out

    def run(stop_at):
        a = {x: 1.0 / num_rows if init == "uniform" else (unique.get(x, 0.0) + 0.5) * 1e-3 for x in ej.support_of(classes, offsets)}
        rounds, converged = 0, False
        while rounds < 2 or (rounds < 100 and not converged):
            out = update(a)
            converged = all(not (o > ej.ALPHA_CHECK_CUTOFF and abs(a.get(x, 0.0) - o) > ej.REL_DIFF_TOLERANCE) for x, o in out.items())
            a = out
            rounds += 1
            if stop_at is not None and rounds == stop_at:
                converged = True
                break
        if loop == "subset" and converged and not skip_floor:
            a = update({x: v for x, v in a.items() if v >= ej.MIN_OUTPUT_ALPHA})
            rounds += 1
        return {x: v for x, v in a.items() if v >= ej.MIN_OUTPUT_ALPHA}, rounds

    row, rounds = run(None)
    if early:
        stop = rounds - (1 if loop == "subset" and not skip_floor and rounds != 100 else 0) - early
        return run(stop) if stop >= 2 else (row, rounds)
    return row, rounds


def _changed(a, b):
    return a.keys() != b.keys() or any(abs(a[c] - b[c]) > 2 * ej.TIGHT_BAR * b[c] for c in a)


def _teeth_cells():
    """(name, EM classes, num_rows, usa, loop): the `infer` batches, and the class tables of the first 300 cells of two fuzz batches
    and of the workload cells as `quant` runs them."""
    for name in ec.INFER_BATCHES:
        b = ec.infer_batch(name)
        for cell, row in zip(b.names, b.rows):
            if row:
                yield f"infer {name} {cell}", [(tuple(l), n) for l, n in row], b.num_rows, b.usa, "subset"
    for name in ("base", "usa", "workload", "workload-usa"):
        b = ec.quant_batch(name)
        _, tables, _, flags = _oracle_run(name, "cr-like-em", "reference", "informative", 0)
        for i, t in enumerate(tables[:300]):
            if not flags[i] & qj.FLAG_TINY and t:
                yield f"quant {b.names[i]}", ej.em_classes(t, b.usa, b.num_rows), b.num_rows, b.usa, "subset" if b.usa else "dense"


MUTATIONS = {
    # mutation: (switches of _mutant, does it apply to this cell, a cell that it has to change)
    "the unspliced sibling left out of get_abundance_for": (dict(no_u_sibling=True), lambda usa, loop: usa, "infer hand-usa u-follows-its-own-s"),
    "the stop one round early": (dict(early=1), lambda usa, loop: True, "infer hand three-way"),
    "the floor round skipped": (dict(skip_floor=True), lambda usa, loop: loop == "subset", "infer hand dense-and-subset-differ"),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_the_judge_refuses_a_mutated_em(mutation):
    switches, applies, named = MUTATIONS[mutation]
    changed = []
    for what, classes, num_rows, usa, loop in _teeth_cells():
        if not applies(usa, loop):
            continue
        outcomes, u = ec.judge_table(classes, num_rows, usa, loop)
        plain, _ = _mutant(classes, num_rows, usa, loop)
        if u or len(outcomes) != 1:
            continue
        assert ej.admits(outcomes, plain) is True, f"{what}: the unmutated restatement is not the judge's row"
        row, _ = _mutant(classes, num_rows, usa, loop, **switches)
        if _changed(row, plain):
            changed.append(what)
            assert isinstance(ej.admits(outcomes, row), str), f"{mutation} passes on {what}"
    print(f"\n{mutation}: changes {len(changed)} cells, all refused")
    assert named in changed and len(changed) >= 20, (mutation, len(changed))


def test_the_judge_refuses_the_dense_loop_on_an_infer_cell():
    """What tells `infer` without USA from `quant` without USA: the floor before a last round."""
    changed = []
    for what, classes, num_rows, usa, loop in _teeth_cells():
        if usa:
            continue
        outcomes, u = ec.judge_table(classes, num_rows, False, "subset")
        dense, du = ec.judge_table(classes, num_rows, False, "dense")
        if u or du or len(outcomes) != 1 or len(dense) != 1:
            continue
        if _changed(dense[0].row, outcomes[0].row):
            changed.append(what)
            assert isinstance(ej.admits(outcomes, dense[0].row), str) and isinstance(ej.admits(dense, outcomes[0].row), str), what
    print(f"\nthe dense loop for the subset loop: changes {len(changed)} cells, all refused")
    assert "infer hand dense-and-subset-differ" in changed and len(changed) >= 20


def _lose_one(table, lab, num_rows):
    less = dict(table)
    less[lab] -= 1
    lost, u = ej.judge_quant_em({l: n for l, n in less.items() if n}, num_rows, False)
    assert not u
    return lost


def test_the_tight_bar_refuses_a_lost_molecule_that_1e4_admits():
    """One molecule removed from one multi-entry class of a cell of over 5 000 molecules.  In the 30 000-read workload cell (13 567
    molecules over 400 genes) every class has an entry small enough for 1e-4 to see the loss; in the hand cell "lost-molecule"
    (21 690 molecules, 600 of them between two entries of about 12 400 and 9 200) the loss moves both by 4e-5: 1e-4 admits the row
    and the tight bar refuses it."""
    b = ec.quant_batch("workload")
    _, tables, _, _ = _oracle_run("workload", "cr-like-em", "reference", "informative", 0)
    table = dict(tables[0])
    assert sum(table.values()) >= 5000
    outcomes, u = ec.judge_table(tables[0], b.num_rows, False)
    assert not u
    multi = sorted(lab for lab in table if len(lab) > 1)
    for lab in multi[:: max(1, len(multi) // 12)]:
        for o in _lose_one(table, lab, b.num_rows):
            assert isinstance(ej.admits(outcomes, o.row), str), f"a molecule of {lab} lost, and the row passes"
    table = E.gene_classes(dict(ec.hand_cells(False))["lost-molecule"], ec.HAND_G, False)
    assert sum(table.values()) >= 5000
    outcomes, u = ec.judge_table(table, ec.HAND_G, False)
    assert not u
    lost = _lose_one(table, (0, 1), ec.HAND_G)
    moved = max(abs(o.row[c] - outcomes[0].row[c]) / outcomes[0].row[c] for o in lost for c in (0, 1))
    print(f"\na molecule of {{0, 1}} lost from a cell of {sum(table.values())}: its entries move by {moved:.2g} relative; "
          f"1e-4: {ej.admits(outcomes, lost[0].row, tight=False)}; tight bar: {ej.admits(outcomes, lost[0].row)}")
    for o in lost:
        assert ej.admits(outcomes, o.row, tight=False) is True and isinstance(ej.admits(outcomes, o.row), str)


def test_admits_refuses_what_is_wrong():
    o = _one(ej.judge_em([((0,), 20), ((1,), 4), ((0, 1), 8), ((1, 2), 1), ((2, 3, 4), 2), ((3,), 1)], 8, False, "dense"))
    row = dict(o.row)
    assert ej.admits([o], row) is True and ej.admits([o], sorted(row.items())) is True
    c = max(row, key=row.get)
    assert isinstance(ej.admits([o], {**row, c: row[c] * (1 + 3 * ej.TIGHT_BAR)}), str) and ej.admits([o], {**row, c: row[c] * (1 + 3 * ej.TIGHT_BAR)}, tight=False) is True
    assert ej.admits([o], {**row, c: row[c] * (1 + 0.4 * ej.TIGHT_BAR)}) is True
    assert isinstance(ej.admits([o], {**row, c: row[c] * (1 + 2e-4)}, tight=False), str)
    assert isinstance(ej.admits([o], {k: v for k, v in row.items() if k != c}), str), "a column dropped"
    assert isinstance(ej.admits([o], {**row, 7: 0.5}), str), "a column too many"
    assert isinstance(ej.admits([], row), str), "an undecided cell admits nothing"
