"""The cells that tests/test_em_judge_cpu.py puts before the EM judge (tests/em_judge.py) with the oracle, and
tests/test_gpu_em_judge.py with the device.

Quant batches are reads: the four fuzz batches of tests/quant_judge_cases.py, the `_workload` cells of tests/test_gpu_em.py, the
round-control cells of tests/em_edges.py and the hand cells below, spelled out molecule by molecule as em_edges.Cell (one read a
molecule under a UMI of its own, so that cr-like-em's classes are exactly the labels written down).  `infer` batches are class
tables in EM labels: the round-control and hand cells' classes, the reference's own unit-test cells (em.rs:1175-1215) and cells
that only `infer` can be given (a class of count 0)."""
import functools

import numpy as np

import em_edges as E
import em_judge as ej
import quant_judge as qj
import quant_judge_cases as qc
from util import pkg

EM_RES = ("cr-like-em", "parsimony-em", "parsimony-gene-em")
HAND_G = 16                                  # genes of the hand cells; USA: ids 2g / 2g + 1, columns S g, U 16 + g, A 32 + g
WORKLOAD_SIZES = (30000, 9000, 4000, 1500, 700, 260, 250, 120, 99, 40, 3)
# cells above this many reads go before quant_judge.judge_cell under cr-like only: its parsimony graph is quadratic in the cell
PARSIMONY_JUDGE_MAX_READS = 1500


class QuantBatch:
    """Cells as collated chunks plus what a judge needs: reads per cell, t2g, the cell names."""

    def __init__(self, name, usa, num_genes, num_rows, t2g, data, off, reads, names=None, small_thresh=0):
        self.name, self.usa, self.num_genes, self.num_rows = name, usa, num_genes, num_rows
        self.t2g = np.asarray(t2g, np.uint32)
        self.data, self.off, self.reads, self.small_thresh = data, off, reads, small_thresh
        self.names = names or [f"{name}[{i}]" for i in range(len(reads))]

    def cfg(self, resolution, **kw):
        kw.setdefault("small_thresh", self.small_thresh)
        return pkg.WorkerConfig.for_resolution(resolution, usa_mode=self.usa, num_genes=self.num_genes, num_rows=self.num_rows, **kw)


def _of_synth(name, s, small_thresh):
    data, off = s.encode()
    return QuantBatch(name, s.usa, s.num_genes, s.num_rows, s.tid_to_gid, data, off, [r for _, r in qc.cells_of(s)], small_thresh=small_thresh)


def _reads_of_cell(c, G, usa):
    """The reads E.encode writes for a Cell: one per molecule, UMIs 0, 1, 2, ... (em_edges.encode)."""
    labels = []
    for col, cnt in sorted(c.uniq.items()):
        ids = [col] if not usa else ([2 * col] if col < G else ([2 * (col - G) + 1] if col < 2 * G else [2 * (col - 2 * G), 2 * (col - 2 * G) + 1]))
        labels += [ids] * cnt
    labels += [list(l) for l in c.amb]
    return [(i, lab) for i, lab in enumerate(labels)]


def _of_cells(name, named_cells, G, usa):
    cells = [c for _, c in named_cells]
    data, off, t2g, ng, nr = E.encode(cells, G, usa)
    return QuantBatch(name, usa, ng, nr, t2g, data, off, [_reads_of_cell(c, G, usa) for c in cells], [n for n, _ in named_cells])


# ------------------------------------------------------------------------------------------------------------------- hand cells

# Entry 1 has no molecule of its own: 13 of {0, 1} and 5 of {1, 2}, next to 22 and 18 single-label molecules of entries 0 and 2.
# It decays round by round, and the first round whose steps are all within 0.01 (the 8th) leaves it at 0.0100000127 - 1.3e-8 above
# f32's 0.01, a fifth of a unit of 2^-24 of the sums it came from.  Found by a sweep of {0}: N, {0, 1}: c, {1, 2}: d, {2}: M over
# N <= 80, c <= 120, d <= 60, M <= 20 for an entry within 1.5e-8 of the floor at the stop; this is the only one.
ONTO_THE_FLOOR = E.Cell(uniq={0: 22, 2: 18}, amb=[[0, 1]] * 13 + [[1, 2]] * 5)


def hand_cells(usa):
    """[(name, Cell)].  What each is for is asserted by tests/test_em_judge_cpu.py::test_hand_cells_do_what_they_were_built_for."""
    G = HAND_G
    if not usa:
        out = [
            # no class of several entries: the dense loop still runs two rounds, the subset loop returns at once
            ("unique-only", E.Cell(uniq={0: 3, 5: 1, 9: 12})),
            # entry 1: 0.075, 0.01 (ON the check cutoff, in a round that entry 0 keeps unconverged: no branch), 0.0013 at the stop.
            # Dense: it leaves the row and entry 0 stays at 44.9987.  Subset: it is floored and the last round hands entry 0 all 45.
            ("dense-and-subset-differ", E.Cell(uniq={0: 39}, amb=[[0, 1]] * 6)),
            ("three-way", E.Cell(uniq={0: 20, 1: 4, 3: 1}, amb=[[0, 1]] * 8 + [[1, 2]] + [[2, 3, 4]] * 2)),
        ]
        # dense: one outcome whose entry 1 may be in the row or not; subset: floored or kept before the last round, two outcomes
        out.append(("onto-the-floor", ONTO_THE_FLOOR))
        # 21 690 molecules, 600 of them between two entries of thousands: one of the 600 lost moves both by 4e-5, under 1e-4
        out.append(("lost-molecule", E.Cell(uniq={0: 12000, 1: 9000, 2: 50}, amb=[[0, 1]] * 600 + [[1, 2]] * 40)))
        return out
    S, U, A = (lambda g: g), (lambda g: G + g), (lambda g: 2 * G + g)
    return [
        # {S_3, U_3} is the one-entry label {A_3}: unique evidence; alone, the subset loop returns it at once
        ("pair-alone", E.Cell(uniq={A(3): 7})),
        # ... and next to {S_3} and labels of S_3 with S_4, A_3 weighs in for S_3 (em.rs:183-185)
        ("pair-next-to-S", E.Cell(uniq={A(3): 7, S(3): 5, S(4): 2}, amb=[[6, 8]] * 4)),
        ("unique-only", E.Cell(uniq={S(0): 3, U(5): 1, A(9): 12})),
        # twelve and thirteen ids: nothing is cut at ten (utils.rs:885-916); the second holds two S, U pairs and a lone U
        ("more-than-ten-ids", E.Cell(uniq={S(0): 6, S(5): 2, A(1): 3, U(2): 1},
                                     amb=[[2 * g for g in range(12)]] * 5 + [[0, 2, 3, 4, 5, 7, 8, 10, 12, 14, 16, 18, 20]] * 4)),
        # S_1, S_2, U_2: the unspliced id of gene 2 follows gene 2's spliced id, not gene 1's: {S_1, A_2}
        ("u-follows-its-own-s", E.Cell(uniq={S(1): 3, S(2): 2, U(2): 4, A(1): 1}, amb=[[2, 4, 5]] * 6)),
        # U_1, S_2: an unspliced id never pairs with what follows it: {U_1, S_2}
        ("u-then-s", E.Cell(uniq={U(1): 3, S(2): 1}, amb=[[3, 4]] * 5)),
    ]


@functools.lru_cache(maxsize=None)
def quant_batch(name):
    """"base" | "usa" | "wide" | "deep" (qc.BATCHES), "workload[-usa]", "rounds[-usa]", "hand[-usa]"."""
    usa = name.endswith("-usa")
    if name in qc.BATCHES:
        b = qc.batch(name)
        return QuantBatch(name, b.usa, b.num_genes, b.num_rows, b.s.tid_to_gid, b.data, b.off, [r for _, r in b.cells])
    if name.startswith("workload"):     # tests/test_gpu_em.py _workload(usa, seed=5): the default small_thresh of 100, tiny cells included
        s = pkg.synth.synth(5, list(WORKLOAD_SIZES), num_genes=400, txp_per_gene=3, usa=usa, dup=0.5, zipf=0.6, cross=0.4, umi_err=0.02,
                            max_extra_na=5)
        return _of_synth(name, s, 100)
    if name.startswith("rounds"):
        return _of_cells(name, [(f"round-cell-{i}", c) for i, c in enumerate(E.round_cells(usa, 4))], 4, usa)
    if name.startswith("hand"):
        return _of_cells(name, hand_cells(usa), HAND_G, usa)
    raise KeyError(name)


QUANT_BATCHES = qc.BATCHES + ("workload", "workload-usa", "rounds", "rounds-usa", "hand", "hand-usa")
# the round-control and hand cells are cr-like-em input (a UMI a molecule: under parsimony the UMIs 0, 1, 2, ... would be joined)
QUANT_CASES = tuple((name, res) for name in QUANT_BATCHES for res in (EM_RES if name in qc.BATCHES or name.startswith("workload") else EM_RES[:1]))


# ---------------------------------------------------------------------------------------------------------------- infer batches

class InferBatch:
    """rows: per cell [(EM label, count)], as `infer` reads them from a -d dump."""

    def __init__(self, name, usa, num_rows, rows, names):
        self.name, self.usa, self.num_rows, self.rows, self.names = name, usa, num_rows, rows, names

    def for_device(self):
        """(eq_labels, cell_classes) as Quantifier.infer takes them: global class ids, ascending in every cell."""
        ids = {}
        cells = [sorted((ids.setdefault(tuple(lab), len(ids)), n) for lab, n in row) for row in self.rows]
        return [list(l) for l, _ in sorted(ids.items(), key=lambda kv: kv[1])], cells


def _em_rows(named_cells, G, usa):
    return [ej.em_classes(E.gene_classes(c, G, usa), usa, 3 * G if usa else G) for _, c in named_cells]


@functools.lru_cache(maxsize=None)
def infer_batch(name):
    usa = name.endswith("-usa")
    if name.startswith("rounds"):
        cells = [(f"round-cell-{i}", c) for i, c in enumerate(E.round_cells(usa, 4))]
        return InferBatch(name, usa, 12 if usa else 4, _em_rows(cells, 4, usa), [n for n, _ in cells])
    if name.startswith("hand"):
        cells = hand_cells(usa)
        rows, names = _em_rows(cells, HAND_G, usa), [n for n, _ in cells]
        if not usa:
            # A class of count 0 (a bootstrap replicate's, em.rs:84-86; `quant` never holds one).  With positive counts the
            # entries of a class keep its count between them, so they cannot all be floored; here entry 1 is floored before the
            # last round and entry 2 was never given anything: the last round finds {1, 2} with a denominator of 0 (em.rs:204).
            rows.append([((0,), 39), ((0, 1), 6), ((1, 2), 0)])
            names.append("floored-class-denominator-0")
        return InferBatch(name, usa, 3 * HAND_G if usa else HAND_G, rows, names)
    if name == "reference-unit-tests":          # em.rs:1175-1184, 1204-1215
        eq = [[0], [1], [0, 1], [1, 2], [2, 3, 4]]
        rows = [[(tuple(eq[i]), n) for i, n in cd] for cd in ([], [(0, 7)], [(0, 20), (1, 4), (2, 8), (3, 1), (4, 2)])]
        rows.append([((0,), 10000), ((0, 1), 1), ((1, 2), 1), ((2, 3, 4), 1)])
        return InferBatch(name, False, 8, rows, ["empty", "singleton", "mixed", "output-threshold"])
    if name == "reference-unit-tests-usa":      # em.rs:1186-1202: three genes, S [0, 3), U [3, 6), A [6, 9)
        eq = [[0, 1], [3, 4], [6, 7], [0, 4, 8], [2]]
        rows = [[(tuple(eq[i]), n) for i, n in cd] for cd in ([(0, 5)], [(1, 5)], [(2, 5)], [(0, 3), (1, 4), (2, 5), (3, 7), (4, 2)])]
        return InferBatch(name, True, 9, rows, ["spliced", "unspliced", "ambiguous", "all-states"])
    raise KeyError(name)


INFER_BATCHES = ("rounds", "rounds-usa", "hand", "hand-usa", "reference-unit-tests", "reference-unit-tests-usa")


# ------------------------------------------------------------------------------------------------------------------ judgements

def _key(table):
    return tuple(sorted((tuple(int(g) for g in lab), int(n)) for lab, n in (table.items() if isinstance(table, dict) else table)))


@functools.lru_cache(maxsize=None)
def _judged_table(key, num_rows, usa, loop, init):
    if loop == "quant":
        return ej.judge_quant_em(key, num_rows, usa, init)
    return ej.judge_em(key, num_rows, usa, loop, init)


def judge_table(table, num_rows, usa, loop="quant", init="informative"):
    """(outcomes, undecided) of one class table; memoised per process on the table itself, shared, never changed.
    loop "quant": a gene-level -d table under `quant`; "dense" / "subset": EM labels as they are."""
    return _judged_table(_key(table), num_rows, usa, loop, init)


def shares(judged):
    """(cells, undecided, cells with exactly one outcome) of a list of judge_table results."""
    return len(judged), sum(u for _, u in judged), sum(len(o) == 1 and not u for o, u in judged)


def assert_the_judge_judges(judged, what):
    """At most 1 % undecided and at least 95 % with exactly one outcome, per batch of 2000 cells.  A batch of a dozen cells cannot
    be held to a share - one cell with an entry in the thousands (its step test never leaves the margin, em_judge.MERGE_BAR), or
    one built on an edge, is a tenth of it: there no cell may be undecided, the shares are printed, and what the cells built on an
    edge give is asserted outcome by outcome in tests/test_em_judge_cpu.py."""
    n, undecided, single = shares(judged)
    print(f"\n{what}: {n} cells, {undecided} undecided ({undecided / max(n, 1):.2%}), {single} with one outcome ({single / max(n, 1):.2%})")
    if n >= 100:
        assert undecided <= 0.01 * n and single >= 0.95 * n, what
    else:
        assert undecided == 0, what


@functools.lru_cache(maxsize=None)
def class_judgements(name, res):
    """tests/quant_judge.py's judgement of every cell of a quant batch under an -em resolution (its class tables; the row of a
    tiny cell), or None for a cell too large for the parsimony judge.  Computed once per process, shared, never changed."""
    b = quant_batch(name)
    if name in qc.BATCHES:          # the judgements tests/test_gpu_quant_judge.py shares: the plain resolution's, same classes
        return tuple(j for j, _ in qc.judgements(name, res[:-3]))
    t2g = b.t2g.tolist()
    out = []
    for reads in b.reads:
        if res != "cr-like-em" and len(reads) > PARSIMONY_JUDGE_MAX_READS:
            out.append(None)
        else:
            out.append(qj.judge_cell(reads, t2g, res, b.usa, num_rows=b.num_rows, small_thresh=b.small_thresh))
    return tuple(out)


def judge_end_to_end(b, res, got, init="informative", what=""):
    """Reads to classes to row, without the oracle: the -d class table of every cell before quant_judge.admits, its row before
    em_judge.admits on that table (a tiny cell's row before quant_judge: no EM ran, quant.rs:794-846).  Returns the EM judgements."""
    rows, tables, flags = qc.rows_of(got), qc.classes_of(got), got.flags.tolist()
    assert got.n_cells == len(b.reads) and [int(x) for x in got.nrec] == [len(r) for r in b.reads], what
    judged, n_tables = [], 0
    for i, j in enumerate(class_judgements(b.name, res)):
        tiny = bool(flags[i] & qj.FLAG_TINY)
        assert tiny == (len(b.reads[i]) < b.small_thresh), f"{what}, {b.names[i]}: flags {flags[i]:#x}"
        if j is not None and not j.undecided:
            m = qj.admits(j, rows[i] if tiny else None, classes=None if tiny else tables[i], flags=flags[i])
            assert m is True, f"{what}, {b.names[i]} ({len(j.outcomes)} class outcome(s)): {m}"
            n_tables += 1
        if tiny:
            continue
        o, u = judge_table(tables[i], b.num_rows, b.usa, "quant", init)
        judged.append((o, u))
        if not u:
            m = ej.admits(o, rows[i])
            assert m is True, f"{what}, {b.names[i]} ({len(o)} outcome(s)): {m}"
    n_judgeable = sum(j is not None for j in class_judgements(b.name, res))
    print(f"\n{what}: {n_tables} of {len(b.reads)} class tables judged (quant_judge left {n_judgeable - n_tables} undecided)")
    assert n_tables >= (0.99 if n_judgeable >= 100 else 0.5) * n_judgeable, what    # (a share means little on a dozen cells)
    assert_the_judge_judges(judged, what)
    return judged
