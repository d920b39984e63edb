"""What tests/test_boot_judge_cpu.py (the oracle) and tests/test_gpu_boot_judge.py (the device) put before the bootstrap judge
(tests/boot_judge.py): the quant batches of tests/em_judge_cases.py, and hand-built cells at the edges of the bootstrap kernel's
draw loop, scans and counters (cr-like-em input, em_edges.Cell: one read a molecule under a UMI of its own)."""
import functools

import em_edges as E
import boot_judge as bj
import em_judge_cases as ec
import quant_judge as qj
import quant_judge_cases as qc

FIRST = 1000                    # first_cell_index of the batch runs
SEEDS = (0xC0FFEE1234, 7)       # --boot-seed: one with a high word, one without
BOOTS = (1, 4)
# the batches of tests/em_judge_cases.py that go before this judge: the fuzz batches under the three -em resolutions, the others
# under cr-like-em.  (Under parsimony-em the 30 000-read workload cell has an entry above 1865 among its ambiguous ones - see
# UNDECIDABLE below: eight or nine admissible stops a replicate, more than 64 combinations of four.)
BATCHES = ("base", "usa", "wide", "hand", "hand-usa", "rounds", "rounds-usa", "workload")
CASES = tuple((name, res) for name in BATCHES for res in (ec.EM_RES if name in qc.BATCHES else ec.EM_RES[:1]))

# THE CELLS THIS JUDGE CANNOT DECIDE, by name.  em_edges.sibling_zero_cell holds 2000 molecules of gene id 0 and one molecule of
# the label {0, 2}.  An entry from 1865 up has a margin above the 0.01 tolerance itself (em_judge.MERGE_BAR): its step test never
# leaves the margin, so every round from the first converged one on is a place to stop.  Under `quant` with USA the rows stop
# moving after a few rounds and merge.  A bootstrap estimates the gene ids as they are: ids 2 and 3 share both of their classes
# ({2, 3} and {2, 3, 4}), nothing but the one molecule of {0, 2} tells them apart, and from a random start they drift for the whole
# 100 rounds - more than 64 distinct stops a replicate.  The cell is undecided whenever its {0, 2} class draws a molecule.  Its
# bootstraps stay compared with the oracle bit for bit (tests/test_gpu_em_edges.py::test_round_cap_bootstraps).
UNDECIDABLE = {"rounds-usa": ("round-cell-3",)}


def boot_rows(bs, n_cells):
    """A Bootstraps' means and variances as [(column, value)] lists, one a cell."""
    out = []
    for ptr, col, val in ((bs.mean_ptr, bs.mean_col, bs.mean_val), (bs.var_ptr, bs.var_col, bs.var_val)):
        p, c, v = ptr.tolist(), col.tolist(), val.tolist()
        assert len(p) == n_cells + 1
        out.append([list(zip(c[a:b], v[a:b])) for a, b in zip(p, p[1:])])
    return out


@functools.lru_cache(maxsize=None)
def _judged(key, usa, num_rows, B, seed, cell):
    return bj.judge_cell(key, usa, num_rows, B, seed, cell)


def judge_table(table, usa, num_rows, B, seed, cell):
    """The judgement of one cell; memoised per process on the table itself, shared, never changed."""
    return _judged(ec._key(table), usa, num_rows, B, seed, cell)


class Tally:
    """What a run before the judge adds up to: cells judged, the undecided ones by name, exact cells, cells with several
    combinations, and the two measured figures with the cells that set them."""

    def __init__(self):
        self.n, self.undecided, self.exact, self.several = 0, [], 0, 0
        self.gap, self.ratio = (0.0, ""), (0.0, "")

    def line(self, what):
        return (f"{what}: {self.n} cells, {len(self.undecided)} undecided, {self.exact} judged bit for bit, {self.several} with several "
                f"combinations; largest mean gap {self.gap[0]:.2f} units of 2^-24 ({self.gap[1]}), largest variance error "
                f"{self.ratio[0]:.3f} of its bound ({self.ratio[1]})")


def assert_the_cap(name, tally, what):
    """At most 1 % of a batch's cells undecided.  A batch of a dozen cells cannot be held to a share: there none may be undecided
    but the cells that UNDECIDABLE names, with the reason."""
    print("\n" + tally.line(what))
    if tally.n >= 100:
        assert len(tally.undecided) <= 0.01 * tally.n, what
    else:
        assert set(tally.undecided) <= set(UNDECIDABLE.get(name, ())), (what, tally.undecided)


def judge_result(b, got, B, summary_stat, seed, first, what, measure=True):
    """Every cell's bootstrap rows before the judge of the cell's own -d class table (a tiny cell has no rows, quant.rs:1028 is
    inside the branch of the cells that are not tiny).  b: names, usa, num_rows, small_thresh.  Returns a Tally."""
    tables, flags = qc.classes_of(got), got.flags.tolist()
    means, variances = boot_rows(got.bootstraps, got.n_cells)
    t = Tally()
    for i, table in enumerate(tables):
        if flags[i] & qj.FLAG_TINY:
            assert not means[i] and not variances[i], f"{what}, {b.names[i]}: a tiny cell with bootstrap rows"
            continue
        j = judge_table(table, b.usa, b.num_rows, B, seed, first + i)
        t.n += 1
        if j.undecided:
            t.undecided.append(b.names[i])
            continue
        m = bj.admits(j, means[i], variances[i], summary_stat)
        assert m is True, f"{what}, {b.names[i]} ({len(j.combos)} combination(s){', exact' if j.exact else ''}): {m}"
        t.exact += j.exact
        t.several += len(j.combos) > 1
        if measure and not j.exact:
            gap, ratio = bj.gaps(j, means[i], variances[i], summary_stat)
            t.gap, t.ratio = max(t.gap, (gap, f"{what}, {b.names[i]}")), max(t.ratio, (ratio, f"{what}, {b.names[i]}"))
    return t


# ------------------------------------------------------------------------------------------------------------------ edge cells

class CellBatch:
    """Hand-built cells as collated chunks, with what judge_result needs."""

    def __init__(self, name, named_cells, G, usa=False, small_thresh=0):
        self.name, self.usa, self.small_thresh = name, usa, small_thresh
        self.names = [n for n, _ in named_cells]
        self.cells = [c for _, c in named_cells]
        self.data, self.off, self.t2g, self.num_genes, self.num_rows = E.encode(self.cells, G, usa)

    def cfg(self, **kw):
        kw.setdefault("small_thresh", self.small_thresh)
        return E.cfg("cr-like-em", self.usa, self.num_genes, self.num_rows, dump_eq=True, **kw)


def spread(n, genes):
    """n molecules over at most `genes` single-label classes, unevenly: no label has two ids, so every replicate is integers."""
    genes = min(genes, n)
    base, rest = divmod(n, genes)
    uniq = {}
    for g in range(genes):
        uniq[3 * g + 1] = base + (rest if g == 0 else 0)
    return E.Cell(uniq=uniq)


DRAW_COUNTS = (1, 2, 3, 4, 5, 7, 8, 4095, 4096, 4097, 4100)     # a Philox block is four draws; a pass of the draw loop 1024 x 4
CLASS_COUNTS = (1023, 1024, 1025)                               # the scan of the cumulative counts takes 1024 classes a pass
SUPPORT_SIZES = (2, 3, 4, 5)                                    # the start stream's block tail; an ambiguous cell has two ids at least
AMBIGUOUS = E.Cell(uniq={0: 6, 5: 1, 9: 4}, amb=[[0, 9]] * 5 + [[3, 9]] * 4 + [[0, 3, 5]] * 2)
UNAMBIGUOUS = E.Cell(uniq={0: 6, 5: 1, 9: 4, 11: 8})
# gene 7 has one molecule of its own and one of {3, 7, 11}: in a replicate where both classes draw 0 it stays in the support, in
# the middle of it, and the start words of 9 and 11 stay where they are
ZERO_CLASS_GENE = 7
ZERO_CLASS = E.Cell(uniq={0: 6, 7: 1, 9: 4}, amb=[[0, 9]] * 5 + [[3, 9]] * 4 + [[3, 7, 11]])
TINY = E.Cell(uniq={2: 2}, amb=[[2, 4]])


def _support_cell(s):
    ids = [2 + 3 * k for k in range(s)]
    return E.Cell(uniq={ids[0]: 5, ids[-1]: 2}, amb=[ids] * 4 + [ids[:2]] * 6 + [ids[-2:]] * 3)


@functools.lru_cache(maxsize=None)
def edge_batch(name):
    if name == "draws":             # N draws: the tail of a Philox block, the second pass of the draw loop
        return CellBatch(name, [(f"N={n}", spread(n, 7)) for n in DRAW_COUNTS], 32)
    if name == "classes":           # K classes of count 1 to 3: the second pass of the scan over the cumulative counts
        return CellBatch(name, [(f"K={k}", E.Cell(uniq={g: 1 + g % 3 for g in range(k)})) for k in CLASS_COUNTS], 1032)
    if name == "support":           # S = 1 is one gene alone (a label of two ids makes S >= 2: the start stream is not read)
        return CellBatch(name, [("S=1", E.Cell(uniq={6: 9}))] + [(f"S={s}", _support_cell(s)) for s in SUPPORT_SIZES], 16)
    if name == "index-exact":       # the same cell twice: what differs is the cell index, 2^32 - 1 and 2^32
        return CellBatch(name, [("c_hi=0", UNAMBIGUOUS), ("c_hi=1", UNAMBIGUOUS)], 16)
    if name == "index-ambiguous":
        return CellBatch(name, [("c_hi=0", AMBIGUOUS), ("c_hi=1", AMBIGUOUS)], 16)
    if name == "replicates":
        return CellBatch(name, [("ambiguous", AMBIGUOUS)], 16)
    if name == "zero-class":
        return CellBatch(name, [("zero-class", ZERO_CLASS)], 16)
    if name == "tiny-between":      # 22, 3 and 22 reads under --small-thresh 10: the tiny cell has no rows and keeps its index
        return CellBatch(name, [("before", AMBIGUOUS), ("tiny", TINY), ("after", AMBIGUOUS)], 16, small_thresh=10)
    if name == "kernel-limits":     # tests/test_gpu_em_edges.py::test_bootstrap_kernel_limits
        cells = [E.boot_classes_cell(E.BOOT_LDS), E.boot_classes_cell(E.BOOT_LDS + 1), E.boot_support_cell(E.BOOT_LDS),
                 E.boot_support_cell(E.BOOT_LDS + 1), E.boot_heavy_cell(E.BOOT_HEAVY), E.boot_heavy_cell(E.BOOT_HEAVY + 1)]
        names = ["classes-at-lds", "classes-past-lds", "support-at-lds", "support-past-lds", "heavy-32", "heavy-33"]
        return CellBatch(name, list(zip(names, cells)), E.BOOT_LDS + 8)
    raise KeyError(name)


# name: (first_cell_index, seed, the replicate counts, the summary modes)
EDGE_RUNS = {
    "draws": (FIRST, SEEDS[0], (4,), (False, True)),
    "classes": (FIRST, SEEDS[0], (4,), (False, True)),
    "support": (FIRST, SEEDS[0], (4,), (False, True)),
    "index-exact": (2 ** 32 - 1, SEEDS[0], (4,), (False, True)),
    "index-ambiguous": (2 ** 32 - 1, SEEDS[0], (4,), (False, True)),
    "replicates": (FIRST, SEEDS[0], (1, 2), (False, True)),
    "zero-class": (FIRST, SEEDS[1], (4,), (False, True)),
    "tiny-between": (FIRST, SEEDS[0], (4,), (False, True)),
    # the settings of the oracle comparison; four replicates of six such cells are ten seconds of Python, once: the second mode
    # summarises the same replicates
    "kernel-limits": (0, 11, (4,), (False, True)),
}


def draws_of(cell, G, usa, B, seed, index):
    """(the canonical classes, the counts that each of B replicates draws for them), from the judge's own parts."""
    classes = bj.canonical_order(E.gene_classes(cell, G, usa), usa, 3 * G if usa else G)
    n = sum(c for _, c in classes)
    return classes, [bj.resample([c for _, c in classes], bj.stream(seed, index, b, n)) for b in range(B)]


def _refuses_under(b, got, i, B, summary_stat, seed, index):
    means, variances = boot_rows(got.bootstraps, got.n_cells)
    j = bj.judge_cell(qc.classes_of(got)[i], b.usa, b.num_rows, B, seed, index)
    return not j.undecided and isinstance(bj.admits(j, means[i], variances[i], summary_stat), str)


def run_edge(name, quant):
    """An edge batch before the judge under every setting of EDGE_RUNS; quant(cfg, batch, first_cell_index) -> QuantResult is the
    oracle's or the device's.  Asserts what the batch was built for; returns the tallies."""
    b = edge_batch(name)
    first, seed, boots, modes = EDGE_RUNS[name]
    tallies = []
    for B in boots:
        for summary_stat in modes:
            what = f"{name} B={B} summary_stat={summary_stat}"
            got = quant(b.cfg(num_bootstraps=B, summary_stat=summary_stat, boot_seed=seed), b, first)
            assert got.n_cells == len(b.cells) and got.first_cell_index == first, what
            t = judge_result(b, got, B, summary_stat, seed, first, what)
            print("\n" + t.line(what))
            assert not t.undecided, what
            tallies.append(t)
            means, _ = boot_rows(got.bootstraps, got.n_cells)
            if name in ("draws", "classes", "index-exact"):
                assert t.exact == t.n == len(b.cells), f"{what}: every cell is judged bit for bit"
            if name == "support":
                assert t.exact == 1 and t.n == len(b.cells), what
            if name.startswith("index"):
                assert means[0] != means[1], f"{what}: the two cells differ in their index alone"
                assert _refuses_under(b, got, 1, B, summary_stat, seed, (first + 1) & bj.MASK), f"{what}: the index's high word is not read"
                assert _refuses_under(b, got, 0, B, summary_stat, seed, first + (1 << 32)), what
            if name == "zero-class":
                classes, drawn = draws_of(ZERO_CLASS, 16, False, B, seed, first)
                holds = [k for k, (lab, _) in enumerate(classes) if ZERO_CLASS_GENE in lab]
                assert len(holds) == 2 and any(all(d[k] == 0 for k in holds) for d in drawn), f"{what}: no replicate draws 0 for every class of gene {ZERO_CLASS_GENE}"
            if name == "tiny-between":
                assert [bool(f & qj.FLAG_TINY) for f in got.flags.tolist()] == [False, True, False], what
                assert _refuses_under(b, got, 2, B, summary_stat, seed, first + 1), f"{what}: the tiny cell must not give its index to the next"
    return tallies
