"""A judge for the bootstrap rows: what `-b` / `--num-bootstraps` gives for ONE cell from its gene-level class table.

Written from the reference's text (COMBINE-lab/alevin-fry, src/: em.rs:306-456 and 585-757, multinomial.rs:9-49, quant.rs:157-210,
1028-1038, 1270-1277; cited `file:line` below) and from DESIGN §5's statement of the project's own streams - not from
oracle/afq_oracle.cpp, not from tests/em_edges.py, not from the kernels.  Only Python ints, floats, dicts, `struct`, `bisect`,
`itertools` and `functools`; no numpy, no ctypes.  The rounds of a replicate's EM are tests/em_judge.py's (run_loop), so the
comparisons against 0.01 are treated here as they are there: as admissible outcomes.

What the reference does (quant.rs:1028-1038): every cell that is not tiny hands its gene-level class table - the labels as gene
ids, `usa_offsets` None, USA or not - to run_bootstrap (em.rs:714-757).  A replicate redraws the class counts from a multinomial
over the observed counts, N = sum(counts) draws (em.rs:596, 612-613, 637; multinomial.rs:41-48), and estimates them with the
subset loop from a RANDOM start (em.rs:642-653, 379-381).  The support is that of the observed table, whatever a replicate draws
(em.rs:626-630).  Two summaries leave the cell: with --summary-stat em.rs:662-683, without quant.rs:185-210.

What the project defines ("The bootstrap streams"): the reference's generator is an unseeded ThreadRng, so the draws are
the project's.  With c = first_cell_index + the cell's position in the submitted range, Philox4x32-10 under the key
(seed_lo, seed_hi):
  * draw j of replicate b is word j & 3 of the block with counter (j >> 2, b, c_lo, c_hi), and selects the first class, in the
    canonical class order, whose cumulative count exceeds (word * N) >> 32;
  * the start of support entry s (the distinct gene ids of all labels, ascending) is word s & 3 of the block with counter
    (s >> 2, b | 2^31, c_lo, c_hi): f32(f32((word >> 8) 2^-24) + f32(1e-5)) (rand's f32 from the top 24 bits, em.rs:380);
  * the canonical class order: labels that are one output column first, by column (USA: S_g at g, U_g at G + g, and {S_g, U_g}
    at 2 G + g), then the others, lexicographic in their gene ids.

    judge_cell(table, usa, num_rows, B, seed, cell) -> Judgement
    admits(judgement, mean_row, var_row, summary_stat) -> True, or a message naming the first difference
"""
import functools
import itertools
import struct
from bisect import bisect_right
from collections import namedtuple

import em_judge as ej

_f32 = ej._f32
MASK = 0xFFFFFFFF

# THE BARS.  None is taken from the code under test.
# Means: the replicates are EM rows, so the bar of a replicate is em_judge's; a mean of values each within a relative bar of the
# judge's is within that bar of the judge's mean (they are all >= 0), to which the B + 1 f32 roundings of the summary add at most
# B + 1 units.  MEASURED (tests/test_boot_judge_cpu.py::test_gap_measurement, on boot_judge_cases.CASES, both summary modes, B in
# {1, 4}, seeds 0xC0FFEE1234 and 7, first cell index 1000: 144 000 cell-runs of the fuzz batches and some 200 of the others): the
# largest relative gap between this judge's mean and the oracle's, taken against the combination that the oracle's rows fit most
# closely, was BOOT_GAP_UNITS units of 2^-24, on BOOT_GAP_CELL.  That test asserts that the gap stays
# at or under the recorded value and at or under em_judge.K units, which leaves the bar (2 K units) at least twice the gap; so the
# bar on a mean is em_judge.TIGHT_BAR, and HARD_BAR (1e-4) applies always.
BOOT_GAP_UNITS = 12.3
BOOT_GAP_CELL = "cell 1742 of the `usa` fuzz batch under cr-like-em, B = 4, seed 0xC0FFEE1234"
MEAN_BAR = min(ej.HARD_BAR, ej.TIGHT_BAR)
# Variances: DERIVED, not measured.  The mean bar is carried to first order through the formula in use (every replicate r and the
# mean m move by at most bar |r|, bar |m|) and one f32 rounding is added per operation of the formula (B + 3 at the most on any
# path to the result):
#   --summary-stat, sq / B - m^2:          (2 bar + (B + 3) 2^-24) (sum r^2 / B + m^2)
#   replicates, sum (r - m)^2 / max(B-1,1): 2 bar sum |r - m| (|r| + |m|) / max(B - 1, 1) + (B + 3) 2^-24 var
# A variance whose judged value lies within its bound of 0 may be absent from the row (the reference writes none that is 0).
# MEASURED next to the gap: the largest error-to-bound ratio of an oracle variance was BOOT_VAR_RATIO (a ratio near 1 would mean
# the derivation is wrong).
BOOT_VAR_RATIO = 0.09
BOOT_VAR_CELL = "the same cell, without --summary-stat"
MAX_COMBINATIONS = 64       # of the replicates' admissible outcomes, an optional column a two-way choice; beyond: undecided

# combos: tuples of B replicate rows {gene id: value > 0}, one tuple per admissible combination; exact: no label of the cell has
# more than one id, so every replicate is a vector of integers and the summaries are judged bit for bit
Judgement = namedtuple("Judgement", "combos exact undecided B")


# ------------------------------------------------------------------------------------------------------------------ Philox4x32-10

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85      # the golden ratio and sqrt(3) - 1, as the key's per-round bumps


def philox4x32_10(counter, key):
    """Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3" (SC'11), Philox4x32 with ten rounds."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + PHILOX_W0) & MASK, (k1 + PHILOX_W1) & MASK
    return c0, c1, c2, c3


def stream(seed, cell, b, n, start=False):
    """The first n words of replicate b's draw stream, or with `start` of its start stream, for the cell of index `cell`."""
    key = (seed & MASK, (seed >> 32) & MASK)
    c1 = b | (1 << 31) if start else b
    out = []
    for block in range((n + 3) >> 2):
        out.extend(philox4x32_10((block, c1, cell & MASK, (cell >> 32) & MASK), key))
    return out[:n]


# ------------------------------------------------------------------------------------------------------------------- the cell

def column_of(label, usa, num_rows):
    """The output column of a label that is one column, else None."""
    if not usa:
        return label[0] if len(label) == 1 else None
    em = ej.usa_em_label(label, num_rows)
    return em[0] if len(em) == 1 else None


def canonical_order(table, usa, num_rows):
    """[(label, count)] of a -d table ({label: count} or [(label, count)]) in the order the draws count the classes in."""
    items = table.items() if isinstance(table, dict) else table
    items = [(tuple(int(g) for g in lab), int(n)) for lab, n in items]
    single = sorted((column_of(lab, usa, num_rows), lab, n) for lab, n in items if column_of(lab, usa, num_rows) is not None)
    multi = sorted((lab, n) for lab, n in items if column_of(lab, usa, num_rows) is None)
    return [(lab, n) for _, lab, n in single] + multi


def resample(counts, words):
    """multinomial.rs:41-48 with one word a draw: N draws, each to the first class whose cumulative count exceeds (word N) >> 32."""
    cum, total = [], 0
    for n in counts:
        total += n
        cum.append(total)
    out = [0] * len(counts)
    for w in words:
        out[bisect_right(cum, (w * total) >> 32)] += 1
    return out


def start_value(word):
    return _f32(_f32((word >> 8) * 2.0 ** -24) + _f32(1e-5))


def replicate(classes, seed, cell, b):
    """Replicate b of a cell whose classes are in canonical order: (outcomes, undecided), as em_judge.run_loop returns them.
    Memoised per process (the replicates of a cell are the same under every B and both summaries), shared, never changed."""
    return _replicate(tuple(classes), seed, cell, b)


@functools.lru_cache(maxsize=None)
def _replicate(classes, seed, cell, b):
    n_total = sum(n for _, n in classes)
    drawn = resample([n for _, n in classes], stream(seed, cell, b, n_total))
    redrawn = [(lab, n) for (lab, _), n in zip(classes, drawn)]
    if all(len(lab) == 1 for lab, _ in classes):                      # em.rs:339-341: the single-label sums as they are
        row = {}
        for lab, n in redrawn:
            row[lab[0]] = row.get(lab[0], 0.0) + n
        return [ej.Outcome({x: v for x, v in row.items() if v > 0}, frozenset(), (0,))], False
    support = sorted(set(g for lab, _ in classes for g in lab))     # em.rs:626-630: of the observed table, classes that draw 0 included
    words = stream(seed, cell, b, len(support), start=True)
    alphas = {x: start_value(w) for x, w in zip(support, words)}    # em.rs:370-381: REPLACES the unique counts of :326
    return ej.run_loop(redrawn, None, "subset", alphas, set(support))


def judge_cell(table, usa, num_rows, B, seed, cell):
    """table: the cell's -d class table; cell: first_cell_index + the cell's position in the range (tiny cells count)."""
    classes = canonical_order(table, usa, num_rows)
    exact = all(len(lab) == 1 for lab, _ in classes)
    if not classes:
        return Judgement([()], exact, False, B)
    per, total = [], 1
    for b in range(B):
        outs, undecided = replicate(classes, seed, cell, b)
        if undecided:
            return Judgement([], exact, True, B)
        choices = []
        for o in outs:
            opt = sorted(o.optional)
            for pick in range(1 << len(opt)):
                choices.append({c: v for c, v in o.row.items() if not (c in o.optional and pick >> opt.index(c) & 1)})
        per.append(choices)
        total *= len(choices)
        if total > MAX_COMBINATIONS:
            return Judgement([], exact, True, B)
    return Judgement(list(itertools.product(*per)), exact, False, B)


# -------------------------------------------------------------------------------------------------------------- the summaries

def _columns(reps):
    return sorted(set(c for r in reps for c in r))


def summaries(reps, summary_stat):
    """{column: (mean, variance, variance bound)} in float64 for every column whose mean is not 0."""
    B = len(reps)
    out = {}
    for c in _columns(reps):
        r = [rep.get(c, 0.0) for rep in reps]
        m = sum(r) / B
        if m == 0.0:
            continue
        if summary_stat:                                                        # em.rs:662-683
            sq = sum(x * x for x in r) / B
            var = sq - m * m
            bound = (2 * MEAN_BAR + (B + 3) * ej.U32) * (sq + m * m)
        else:                                                                   # quant.rs:185-210
            den = max(B - 1, 1)
            var = sum((x - m) * (x - m) for x in r) / den
            bound = 2 * MEAN_BAR * sum(abs(x - m) * (abs(x) + abs(m)) for x in r) / den + (B + 3) * ej.U32 * var
        out[c] = (m, var, bound)
    return out


def summaries_f32(reps, summary_stat):
    """({column: mean}, {column: variance}) as the reference's f32 operations give them from f32 replicates: every f32 operation
    on f32 operands is the double operation rounded to f32 (53 >= 2 24 + 2: the double rounding is innocuous).  Only entries
    that are not 0 are there (quant.rs:172-181, 194, 204)."""
    B = len(reps)
    n = float(B)
    mean, var = {}, {}
    for c in _columns(reps):
        r = [_f32(rep.get(c, 0.0)) for rep in reps]
        s = 0.0
        for x in r:
            s = _f32(s + x)
        m = _f32(s / n)
        if summary_stat:
            q = 0.0
            for x in r:
                q = _f32(q + _f32(x * x))                                       # em.rs:663-664
            v = _f32(_f32(q / n) - _f32(m * m))                                 # em.rs:676-679
        else:
            if m == 0.0:
                continue                                                        # quant.rs:194
            q = 0.0
            for x in r:
                d = _f32(x - m)
                q = _f32(q + _f32(d * d))
            v = _f32(q / _f32(max(n - 1.0, 1.0)))                               # quant.rs:203
        if m != 0.0:
            mean[c] = m
        if v != 0.0:
            var[c] = v
    return mean, var


# -------------------------------------------------------------------------------------------------------------------- admitting

def _as_row(row):
    return {int(c): float(v) for c, v in (row.items() if isinstance(row, dict) else row)}


def _bits(x):
    return struct.pack("f", x)


def _fits_exactly(reps, mean_row, var_row, summary_stat):
    mean, var = summaries_f32(reps, summary_stat)
    for what, want, got in (("mean", mean, mean_row), ("variance", var, var_row)):
        for c in sorted(set(want) | set(got)):
            if c not in got:
                return f"{what} of column {c}: judge {want[c]!r} exactly, row lacks it"
            if c not in want:
                return f"{what} of column {c}: judge has none, got {got[c]!r}"
            if _bits(want[c]) != _bits(got[c]):
                return f"{what} of column {c}: judge {want[c]!r} exactly, got {got[c]!r}"
    return None


def _fits(reps, mean_row, var_row, summary_stat, bar):
    judged = summaries(reps, summary_stat)
    for c in sorted(set(judged) | set(mean_row)):
        if c not in mean_row:
            return f"mean of column {c}: judge {judged[c][0]!r}, row lacks it"
        if c not in judged:
            return f"mean of column {c}: judge has none, got {mean_row[c]!r}"
        m = judged[c][0]
        if abs(mean_row[c] - m) > bar * abs(m):
            return f"mean of column {c}: judge {m!r}, got {mean_row[c]!r} ({abs(mean_row[c] - m) / abs(m) / ej.U32:.1f} units of 2^-24)"
    for c in sorted(set(judged) | set(var_row)):
        if c not in judged:
            return f"variance of column {c}: judge has no mean there, got {var_row[c]!r}"
        _, v, bound = judged[c]
        if c not in var_row:
            if abs(v) > bound:
                return f"variance of column {c}: judge {v!r} (bound {bound:.3g}), row lacks it"
        elif abs(var_row[c] - v) > bound:
            return f"variance of column {c}: judge {v!r}, got {var_row[c]!r} ({abs(var_row[c] - v) / bound if bound else float('inf'):.2f} of the bound {bound:.3g})"
    return None


def admits(j, mean_row, var_row, summary_stat, tight=True):
    """Are the two rows the summaries of one admissible combination of replicates?  Exact cells: bit for bit.  Others: every
    mean within HARD_BAR of the judge's and, with tight, within em_judge.TIGHT_BAR; every variance within its derived bound."""
    if j.undecided:
        return "the judge left this cell undecided"
    mean_row, var_row = _as_row(mean_row), _as_row(var_row)
    bar = MEAN_BAR if tight else ej.HARD_BAR
    first = None
    for reps in j.combos:
        if j.exact:
            msg = _fits_exactly(reps, mean_row, var_row, summary_stat)
        else:
            msg = _fits(reps, mean_row, var_row, summary_stat, bar)
        if msg is None:
            return True
        first = first or msg
    return f"{first} (against the first of {len(j.combos)} combinations; none fits)" if len(j.combos) > 1 else first


def gaps(j, mean_row, var_row, summary_stat):
    """(largest relative gap of a mean in units of 2^-24, largest variance error over its bound) against the combination that
    the rows fit most closely (two combinations within the bar of each other both fit); for measuring, after admits said True."""
    mean_row, var_row = _as_row(mean_row), _as_row(var_row)
    best = None
    for reps in j.combos:
        if _fits(reps, mean_row, var_row, summary_stat, MEAN_BAR) is None:
            judged = summaries(reps, summary_stat)
            gap = max((abs(mean_row[c] - m) / abs(m) / ej.U32 for c, (m, _, _) in judged.items()), default=0.0)
            ratio = max((abs(var_row.get(c, 0.0) - v) / bound for c, (_, v, bound) in judged.items() if bound > 0), default=0.0)
            best = (gap, ratio) if best is None else min(best, (gap, ratio))
    assert best is not None, "no combination fits"
    return best
