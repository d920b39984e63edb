"""Cells at the top of a cell's read count - 2^22 reads, where three things in csrc/ change with `nrec` alone - shared by
tests/test_giant_cell_cases_cpu.py (builders and expectations, no device) and tests/test_gpu_giant_cells.py (the device).

  * the order-free EM's fixed-point scale, F = min(40, 62 - bitlen(nrec)) (afq_em2.hip em2_fbits, afq_oracle.cpp em_fbits):
    40 up to 2^22 - 1 reads, 39 from 2^22, 38 from 2^23 (`fbits` restates it);
  * parsimony's ceiling: a cell of 2^22 reads or more goes to the one-workgroup kernel, which refuses it (afq_api.cpp run_range);
  * the bucket plan of cr-like and trivial cells: the smallest lg with 256 << lg >= n_ref (`lg_nb`): 14 for 2^22 single-ref
    reads, 15 for one read more.

No judge of tests/ can take 4 M reads in plain Python, so the giant cr-like / trivial / cr-like-em cells follow ONE PATTERN whose
row and class table are formulas in N, and everything is encoded with numpy (rad.encode_cells_np).

The pattern (`pattern_reads`).  Read i has UMI i >> 1 and one ref.  Gene g has the refs 2g and 2g + 1; without USA both map to gene
g, with USA the ref id is the gene id (2g spliced, 2g + 1 unspliced) - the SAME bytes serve both modes.  UMI u belongs to gene
g = u % G, G = 37 (coprime to 3, so that (u % 3, u % G) runs through all 3 G combinations evenly).  Its first read names ref 2g;
its second read depends on u % 3:
    0: ref 2g again - a single-label molecule of gene g (USA: of S_g);
    1: ref 2((g + 1) % G) - a tie of two genes: cr-like drops it (USA: two spliced ids of different genes, utils.rs:688-753),
       cr-like-em gets the ambiguous class {g, g + 1};
    2: ref 2g + 1 - without USA the same gene through its other ref, a single-label molecule; with USA the spliced and the
       unspliced id of one gene, the column A_g (and, for the EM, single-label evidence of the entry A_g - a passive sibling of S_g).
An odd N leaves the last UMI with its first read alone: one more single-label molecule of its gene.
The molecules of case c and gene g among U = N >> 1 whole UMIs are the u < U with u = r mod 3 G, r the one residue with r % 3 = c
and r % G = g: ceil((U - r) / 3 G) of them (`molecules`).  The rows and the class table are sums of those (`crlike_row`,
`trivial_row`, `class_table`); tests/test_giant_cell_cases_cpu.py holds them against tests/quant_judge.py read by read on
miniatures and against the oracle at full size.

Each giant cell sits between a 50-read cell (under the tiny-cell threshold: cr-like whatever -r says, quant.rs:794-846) and a
600-read cell of the same pattern.

The accumulator at its top (`ab_batch`): uA = N - 1005 single-label molecules of A, 1000 molecules of {A, B}, 5 of B (the shape of
em_edges.ab_cell), a read and a UMI each.  Entry A starts at uA << F: just under 2^62 at 2^22 - 1 reads (F = 40), about 2^61 at 2^22
(F = 39) and at 2^23 (F = 38); with F left at 40 it would start within a thousandth of 2^62, and at 2^23 reads of 2^63.

Parsimony at its ceiling (`parsimony_ceiling_cell`): one cell of exactly 2^22 - 1 reads from the native generator, with the
parameters of tests/test_gpu_pug.py::test_parsimony_cell_of_more_than_2_pow_20_reads but for the gene popularity.  MEASURED on
the CPU these tests were written on (one thread): with those parameters as they are the oracle takes 20 s for 2^20 reads and had not
finished 2^22 - 1 after six and a half minutes.  It compares every two UMIs of a class and of every two classes that share a ref,
as the reference does (pugutils.rs:65-267): its time is the sum of the classes' squared sizes, which the popular genes of
zipf = 1.1 dominate.  Neither dup nor umi_err changes that (2^20 reads: 21 s at dup = 0.1, 18 s at dup = 0.8, 21 s at
umi_err = 0); zipf = 0.5 does: 3.8 s for 2^20 reads and PARS_ORACLE_SECONDS[resolution] for 2^22 - 1 (3.5 M molecules, 42 000
components with a tie).  The read count is what the test is about and stays.

The EM bar for these cells.  em_judge.TIGHT_BAR is measured on that module's batches only.  Here the oracle merges equal labels
as the reference does (a class table of at most 3 G classes, whatever N), so an entry of the reference's f32 sum still adds a few
dozen shares; the device adds up to N / 3 of them, in integers.  MEASURED (tests/test_giant_cell_cases_cpu.py::
test_the_em_bar_of_these_cells): the largest relative gap between em_judge's float64 values and the oracle IN THE REFERENCE'S
ARITHMETIC, over the canonical class order and the shuffled orders 11, 12, 13, on every pattern cell and every {A, B} cell, is
1.69 units of 2^-24 (GAP_UNITS = 1.7; the 2^22 - 1-read USA pattern cell).  The device's tight bar is four times that, rounded up
(em_judge's convention for K): GIANT_K = 7 units, GIANT_TIGHT_BAR = 14 x 2^-24 = 8.3e-7 relative - below em_judge.HARD_BAR (1e-4),
so both bars are asserted.  It is derived from the reference-arithmetic oracle, never from the device."""
import functools
import importlib
import math

import numpy as np

import em_edges as E
import em_judge as ej
from util import pkg

rad = pkg.rad

G = 37
SIZES = (2 ** 22 - 1, 2 ** 22, 2 ** 22 + 1)
BIG = 2 ** 23                                   # F = 38; non-USA only
NEIGHBOURS = (50, 600)                          # the cells before and after the giant one
SMALL_THRESH = 100                              # the default tiny-cell threshold (quant.rs:449)
BUCKET_TARGET, MAX_LG_NB = 256, 20              # afq_api.cpp kBucketTarget, afq_common.h kMaxLgNb
PARS_CEILING = 1 << 22                          # afq_api.cpp run_range: `m.nrec >= (1u << 22)` goes to the one-workgroup kernel

GAP_UNITS = 1.7                                 # (measured: 1.69, on the 2^22 - 1-read USA pattern cell; see the docstring)
GIANT_K = math.ceil(4 * GAP_UNITS)
GIANT_TIGHT_BAR = 2 * GIANT_K * ej.U32
PARS_ORACLE_SECONDS = {"parsimony": 17, "parsimony-em": 19}      # (measured; see the docstring)


def fbits(nrec):
    """em2_fbits (afq_em2.hip:108), em_fbits (afq_oracle.cpp:629): acc = count << F stays under 2^62 whatever the cell."""
    return min(40, 62 - (int(nrec) | 1).bit_length())


def lg_nb(n_ref):
    """afq_api.cpp:720: the bucket plan of a cr-like / trivial cell."""
    lg = 0
    while (BUCKET_TARGET << lg) < n_ref and lg < MAX_LG_NB:
        lg += 1
    return lg


# ------------------------------------------------------------------------------------------------------------------ the pattern

def pattern_reads(n):
    """(umi u32[n], ref u32[n]) of an n-read cell of the pattern; one ref a read."""
    i = np.arange(n, dtype=np.int64)
    u = i >> 1
    g = u % G
    c = u % 3
    second = np.where(c == 0, 2 * g, np.where(c == 1, 2 * ((g + 1) % G), 2 * g + 1))
    return u.astype(np.uint32), np.where(i & 1 == 0, 2 * g, second).astype(np.uint32)


def reads_as_lists(n):
    """The same reads as the judges take them: [(umi, [ref])]."""
    umi, ref = pattern_reads(n)
    return [(int(u), [int(r)]) for u, r in zip(umi, ref)]


def t2g(usa):
    return np.arange(2 * G, dtype=np.uint32) if usa else np.arange(2 * G, dtype=np.uint32) >> 1


def dims(usa):
    """(num_genes, num_rows)"""
    return (2 * G, 3 * G) if usa else (G, G)


def cfg(res, usa, **kw):
    ng, nr = dims(usa)
    return pkg.WorkerConfig.for_resolution(res, usa_mode=usa, num_genes=ng, num_rows=nr, **kw)


def encode_pattern(sizes, bc0=7000):
    """Cells of the pattern, one per size, as collated chunks: (bytes, chunk_off)."""
    parts = [pattern_reads(n) for n in sizes]
    umi = np.concatenate([p[0] for p in parts])
    ref = np.concatenate([p[1] for p in parts])
    return rad.encode_cells_np(list(sizes), [bc0 + k for k in range(len(sizes))], umi, np.ones(len(umi), np.int64), ref)


def batch_sizes(N):
    return (NEIGHBOURS[0], N, NEIGHBOURS[1])


@functools.lru_cache(maxsize=1)
def pattern_batch(N):
    """(bytes, chunk_off) of [50 reads, N reads, 600 reads]; the last one built is kept (a 2^23-read cell is 128 MiB)."""
    return encode_pattern(batch_sizes(N))


def molecules(N):
    """(m, lone): m[c][g] = whole UMIs of case c and gene g among the first N reads; lone = the gene of the last UMI's only
    read when N is odd, else None."""
    U = N >> 1
    m = [[0] * G for _ in range(3)]
    for r in range(3 * G):
        m[r % 3][r % G] = max(0, -(-(U - r) // (3 * G)))
    return m, (U % G if N & 1 else None)


def class_table(N, usa):
    """The cell's gene-level classes as -d dumps them under cr-like-em: {label: molecules}."""
    m, lone = molecules(N)
    out = {}

    def add(label, n):
        if n:
            out[label] = out.get(label, 0) + n

    for g in range(G):
        one = m[0][g] + (lone == g)
        if usa:
            add((2 * g,), one)
            add(tuple(sorted((2 * g, 2 * ((g + 1) % G)))), m[1][g])
            add((2 * g, 2 * g + 1), m[2][g])
        else:
            add((g,), one + m[2][g])
            add(tuple(sorted((g, (g + 1) % G))), m[1][g])
    return out


def crlike_row(N, usa):
    """{column: molecules}: the single-label molecules; USA: S_g for cases 0 and the lone read, A_g = 2 G + g for case 2."""
    m, lone = molecules(N)
    out = {}
    for g in range(G):
        one = m[0][g] + (lone == g)
        for col, n in ((g, one), (2 * G + g, m[2][g])) if usa else ((g, one + m[2][g]),):
            if n:
                out[col] = n
    return out


def trivial_row(N, usa):
    """{column: distinct UMIs among the reads of that gene id} (pugutils.rs:852-911): every read names one ref, so a UMI counts
    for every gene id it touches; with USA the gene ids 2g and 2g + 1 are counted apart."""
    m, lone = molecules(N)
    out = {}
    for g in range(G):
        first = m[0][g] + m[1][g] + m[2][g] + (lone == g) + m[1][(g - 1) % G]      # UMIs with a read on ref 2g
        for col, n in ((2 * g, first), (2 * g + 1, m[2][g])) if usa else ((g, first),):
            if n:
                out[col] = n
    return out


def plain_row(res, n, usa):
    """The expected row of an n-read cell under `cr-like` or `trivial`; a tiny cell's under any resolution."""
    return crlike_row(n, usa) if n < SMALL_THRESH or res == "cr-like" else trivial_row(n, usa)


# ------------------------------------------------------------------------------------------------------------- the EM's shape

def shape_of_table(table, usa, G_, min_tier=0):
    """em_edges.em2_shape from a class table {gene label: molecules} (the device keeps a class per molecule: K and Wc count
    molecules, L and P distinct entries), without a Python loop over the molecules."""
    labels = {lab: E.em_label(list(lab), G_, usa) for lab in table}
    amb = {lab: n for lab, n in table.items() if len(labels[lab]) > 1}
    K = sum(amb.values())
    Wc = sum(len(labels[lab]) * n for lab, n in amb.items())
    live = set(x for lab in amb for x in labels[lab])
    uniq = set(labels[lab][0] for lab in table if len(labels[lab]) == 1)
    P = 0
    if usa:
        uo, ao = G_, 2 * G_
        for col in uniq - live:
            sib = (col - ao, col - uo) if col >= ao else ((col + uo,) if col >= uo else (col + ao,))
            P += any(x in live for x in sib)
    return E.shape_of_counts(len(live), P, K, Wc, usa, min_tier)


# -------------------------------------------------------------------------------------------- the accumulator at its top: {A, B}

AB_AMB, AB_UB = 1000, 5


def ab_counts(N):
    """(uA, molecules of {A, B}, uB) of the N-read cell."""
    return N - AB_AMB - AB_UB, AB_AMB, AB_UB


def ab_dims(usa):
    """(tid_to_gid, num_genes, num_rows): genes A = 0 and B = 1; USA: their spliced ids 0 and 2."""
    return (np.arange(4, dtype=np.uint32), 4, 6) if usa else (np.arange(2, dtype=np.uint32), 2, 2)


def ab_cfg(usa, **kw):
    _, ng, nr = ab_dims(usa)
    return pkg.WorkerConfig.for_resolution("cr-like-em", usa_mode=usa, num_genes=ng, num_rows=nr, **kw)


def ab_batch(N, usa):
    """One cell: uA reads of A, 1000 reads of A and B, 5 reads of B, a UMI each.  (bytes, chunk_off)."""
    uA, n, uB = ab_counts(N)
    a, b = (0, 2) if usa else (0, 1)
    na = np.concatenate((np.ones(uA, np.int64), np.full(n, 2, np.int64), np.ones(uB, np.int64)))
    refs = np.concatenate((np.full(uA, a, np.uint32), np.tile(np.asarray([a, b], np.uint32), n), np.full(uB, b, np.uint32)))
    return rad.encode_cells_np([N], [4242], np.arange(N, dtype=np.uint32), na, refs)


def ab_class_table(N, usa):
    uA, n, uB = ab_counts(N)
    a, b = (0, 2) if usa else (0, 1)
    return {(a,): uA, (a, b): n, (b,): uB}


def ab_row_f64(N, rounds):
    """The {A, B} cell's row after `rounds` rounds, in float64 (em_edges.two_entry_em_row_f64): {column: value}."""
    uA, n, uB = ab_counts(N)
    return dict(zip((0, 1), E.two_entry_em_row_f64(n, uA, uB, rounds)))


# ----------------------------------------------------------------------------------------------------------------- the judge

@functools.lru_cache(maxsize=None)
def _judged(key, num_rows, usa):
    return ej.judge_quant_em(key, num_rows, usa)


def judge(table, num_rows, usa):
    """(outcomes, undecided) of em_judge on a class table; memoised, shared, never changed."""
    return _judged(tuple(sorted(table.items())), num_rows, usa)


def as_row(g, v):
    return {int(c): float(x) for c, x in zip(g, v)}


def gap_units(outcomes, row, rounds=None):
    """The relative gap between a row and the judge's outcome for it, in units of 2^-24: the outcome of the given round count
    where there is one, else the nearest.  None if no outcome has the row's columns."""
    best = None
    for o in outcomes:
        if set(o.row) - set(o.optional) <= set(row) <= set(o.row):
            gap = max(abs(v - o.row[c]) / o.row[c] / ej.U32 for c, v in row.items())
            if rounds is not None and rounds in o.rounds:
                return gap
            best = gap if best is None else min(best, gap)
    return best


def admits_within(outcomes, row, bar):
    """em_judge.admits at a bar of this module's: True, or the first difference from the first outcome."""
    first = None
    for o in outcomes:
        msg = ej._fits(o, row, bar)
        if msg is None:
            return True
        first = first or msg
    return first or "the judge left this cell undecided"


# ----------------------------------------------------------------------------------------------------- parsimony at its ceiling

PARS_GEN = dict(seed=12, median_reads=1.15e6, sigma=0.0, num_genes=36601, ref_count=199138, umi_err=0.01, zipf=0.5)
PARS_CASES = (("parsimony", False), ("parsimony-em", True))


def _native():
    return importlib.import_module("alevin-fry_amd.synth_native")


def parsimony_cells(sizes, usa):
    """Cells of the given sizes from the native generator (host side)."""
    return _native().generate(sizes=np.asarray(sizes, np.uint32), n_cells=len(sizes), usa=usa, **PARS_GEN)


def parsimony_ceiling_cell(usa):
    """The last cell the phase kernels accept: 2^22 - 1 reads."""
    return parsimony_cells([PARS_CEILING - 1], usa)


def parsimony_refused_batch():
    """[300 reads, exactly 2^22 reads, 300 reads]: cell 1 is the first one refused."""
    return parsimony_cells([300, PARS_CEILING, 300], False)


def parsimony_cfg(res, d):
    return pkg.WorkerConfig.for_resolution(res, usa_mode=d.usa, num_genes=d.num_genes, num_rows=d.num_rows, umi_len=12)
