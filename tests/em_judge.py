"""A judge for the EM rows: what alevin-fry's EM computes for ONE cell from its class table, in plain float64.

Written from the reference's text (COMBINE-lab/alevin-fry, src/; cited `file:line` below) and from nothing else: not from
oracle/afq_oracle.cpp, not from tests/em_edges.py, not from the kernels.  Only Python floats, dicts, tuples and sets; no numpy, no
ctypes.  tests/quant_judge.py judges reads -> classes; this file judges classes -> row, for the three -em resolutions and `infer`.

Two loops.  `quant` without USA runs em_optimize (em.rs:487-582, "dense"): rounds until converged or capped, then the output floor.
`quant` with USA (quant.rs:892-911) and `infer` in either mode (infer.rs:230) run em_optimize_subset_impl (em.rs:306-456, "subset"):
the unique counts are returned as they are when no class has more than one entry; otherwise, after a converged round, entries under
0.01 are floored and ONE more round runs on what is left, so a floored entry's mass goes to its class mates.

The float64 trajectory is not the reference's: the reference sums f32 shares in a HashMap's order (em.rs:464), the device in fixed
point.  Both stay within a few units of 2^-24 of this file's values (measured, see K), EXCEPT where a comparison against 0.01
decides: the step test and check cutoff of a round (em.rs:407-415, 546-557), the floor before the subset loop's last round
(em.rs:434-441) and the output floor (em.rs:446-451, 568-572).  Within the margin of such a comparison the judge does not pick a
side; it returns every admissible outcome, as the parsimony judge does for cover ties:
  * a round that otherwise converged, with a step test or check cutoff within the margin: stopping there is one outcome, and the
    main line goes on as unconverged;
  * an entry within the margin of the floor before the last round: floored and kept are both outcomes; with more than three such
    entries in one cell the cell is undecided;
  * an entry within the margin of the output floor: the row may hold it or not.

    judge_em(classes, num_rows, usa, loop, init="informative") -> (outcomes, undecided)
    run_loop(classes, offsets, loop, alphas, support) -> (outcomes, undecided): the rounds alone, from an explicit start vector
    admits(outcomes, row, tight=True) -> True, or a message naming the first difference

Random initialisation (em.rs:379-381) is not judge_em's: its draws are not the reference's.  It occurs in bootstrap replicates
only, whose draws are the project's own streams; tests/boot_judge.py judges those, and runs this file's rounds from the random
start through run_loop.
"""
import struct
from collections import namedtuple


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


# em.rs:28-34 (f32 constants, as f32 holds them)
MIN_OUTPUT_ALPHA = _f32(0.01)
ALPHA_CHECK_CUTOFF = _f32(1e-2)
MIN_ITER = 2
MAX_ITER = 100
REL_DIFF_TOLERANCE = _f32(1e-2)

U32 = 2.0 ** -24        # f32's unit roundoff

# K: the margin of every comparison against 0.01 is K 2^-24 (|in| + |out|), and the tight bar on values 2 K 2^-24 relative.
# MEASURED (tests/test_em_judge_cpu.py::test_margin_measurement, on the batches of tests/em_judge_cases.py): the largest relative
# gap between this judge and the oracle in the REFERENCE's arithmetic, over the canonical class order and the shuffled orders 11,
# 12, 13, both initialisations, was 11.16 units of 2^-24 of the value - on the {A, B} cell of 300 molecules that runs into the cap
# of 100 rounds (em_edges.ROUND_CELLS); 8.3 on the fuzz batches, 6.4 on the 30 000-read cell.  K is four times the gap, rounded up:
# the shuffles sample the order space, they are not its worst case.  That test asserts that the gap stays under half the margin (K
# units) and at or under GAP_UNITS, so drift is seen.
GAP_UNITS = 11.2
K = 45
HARD_BAR = 1e-4         # north_star: EM resolutions within 1e-4 relative
# THE TIGHT BAR HOLDS FOR THESE BATCHES ONLY.  f32's error in an entry grows with the classes summed into it; cells with entries in
# thousands of classes (full-size workloads, tests/test_gpu_fullsize.py) need their own measurement and are not judged here.
TIGHT_BAR = 2 * K * U32
MAX_NEAR_FLOOR = 3      # entries within the margin of the floor before the last round: more leave the cell undecided
MAX_OUTCOMES = 64
# Outcomes that no bar of this file can tell apart are ONE outcome with several round counts.  An entry in the thousands has a
# margin above the 0.01 tolerance itself (K 2^-24 2 v > 0.01 from v = 1865): its step test never leaves the margin, every round from
# the first converged one on is a place to stop, and all of them give the same row.
MERGE_BAR = TIGHT_BAR / 1000

# row: {column: value > 0}; optional: the columns within the margin of the output floor (the row holds their value; a judged row
# may lack them); rounds: the EM rounds run, the subset loop's last round included (0: the subset loop's early return) - a tuple,
# of one count unless stops at several rounds give this row
Outcome = namedtuple("Outcome", "row optional rounds")


def margin(a, b):
    return K * U32 * (abs(a) + abs(b))


# ---------------------------------------------------------------------------------------------------------------- USA EM labels

def is_spliced(g):
    return g & 1 == 0                       # utils.rs:419-422


def usa_em_label(label, num_rows):
    """The EM label of a gene-level label in USA mode (utils.rs:842-926).  u_off = num_rows / 3, a_off = 2 u_off (:861-862)."""
    u_off = num_rows // 3
    a_off = 2 * u_off
    if len(label) == 1:                                                 # :871-882
        g = label[0]
        return (g >> 1,) if is_spliced(g) else (u_off + (g >> 1),)
    out = []
    i = 0
    while i < len(label):                                               # :885-916, in label order, every id, nothing cut
        g = label[i]
        idx = g >> 1
        if is_spliced(g):
            if i + 1 < len(label) and label[i + 1] >> 1 == g >> 1:     # the NEXT id is the same gene's: the pair is ambiguous
                idx += a_off
                i += 1
        else:
            idx += u_off
        out.append(idx)
        i += 1
    return tuple(out)                                                   # :917-921 not re-sorted; {S_g, U_g} is the ONE entry {A_g}


def em_classes(table, usa, num_rows):
    """A cell's gene-level class table (what -d dumps: {label: molecules} or [(label, molecules)]) as the EM's classes."""
    items = table.items() if isinstance(table, dict) else table
    return [(usa_em_label(tuple(int(g) for g in lab), num_rows) if usa else tuple(int(g) for g in lab), int(n)) for lab, n in items]


# ----------------------------------------------------------------------------------------------------------------- the update

def abundance(idx, alphas, u_off, a_off):
    """get_abundance_for, em.rs:167-187: an entry weighs what its gene's entries that could explain the same molecule hold."""
    if idx >= a_off:
        return alphas.get(idx - u_off, 0.0) + alphas.get(idx - a_off, 0.0) + alphas.get(idx, 0.0)      # U + S + A
    if idx >= u_off:
        return alphas.get(idx + u_off, 0.0) + alphas.get(idx, 0.0)                                      # A + U
    return alphas.get(idx + a_off, 0.0) + alphas.get(idx, 0.0)                                          # A + S


def update(alphas, classes, offsets):
    """One round: em.rs:189-217 and 458-485 (offsets None), em.rs:219-248 (USA).  A class of one entry gives its count to it; a
    class of several shares its count by weight; a class whose denominator is 0 gives nothing."""
    out = {}
    for label, count in classes:
        if len(label) > 1:
            w = [alphas.get(x, 0.0) for x in label] if offsets is None else [abundance(x, alphas, *offsets) for x in label]
            den = sum(w)
            if den > 0.0:
                inv = count / den
                for x, wx in zip(label, w):
                    out[x] = out.get(x, 0.0) + wx * inv
        else:
            out[label[0]] = out.get(label[0], 0.0) + count
    return out


def support_of(classes, offsets):
    """em.rs:87-113: every entry of a label and, in USA mode, both siblings of it."""
    s = set()
    for label, _ in classes:
        for x in label:
            s.add(x)
            if offsets is not None:
                u_off, a_off = offsets
                if x >= a_off:
                    s.update((x - u_off, x - a_off))
                elif x >= u_off:
                    s.add(x + u_off)                    # (:105-106: an unspliced entry marks its ambiguous sibling)
                else:
                    s.add(x + a_off)
    return s


# --------------------------------------------------------------------------------------------------------------------- the loops

class _Undecided(Exception):
    pass


def _round_verdict(alphas, out, support):
    """em.rs:405-416, 545-558.  'moved': some entry surely above the cutoff surely moved by more than the tolerance;
    'near': none surely did, but a comparison that would say so lies within the margin; 'still' otherwise."""
    near = False
    for x in support:
        o, a = out.get(x, 0.0), alphas.get(x, 0.0)
        m = margin(a, o)
        if o <= ALPHA_CHECK_CUTOFF - m:
            continue
        step = abs(a - o)
        if step <= REL_DIFF_TOLERANCE - m:
            continue
        if o > ALPHA_CHECK_CUTOFF + m and step > REL_DIFF_TOLERANCE + m:
            return "moved"
        near = True
    return "near" if near else "still"


def _add(outcomes, o):
    for i, have in enumerate(outcomes):
        if have.optional == o.optional and have.row.keys() == o.row.keys() and \
                all(abs(v - have.row[c]) <= MERGE_BAR * have.row[c] for c, v in o.row.items()):
            outcomes[i] = have._replace(rounds=tuple(sorted(set(have.rounds + o.rounds))))
            return
    outcomes.append(o)
    if len(outcomes) > MAX_OUTCOMES:
        raise _Undecided


def _output(alphas, rounds):
    """em.rs:446-451, 568-572: entries under 0.01 leave; one within the margin of 0.01 may be in the row or not."""
    row, optional = {}, set()
    for x, v in alphas.items():
        m = margin(v, v)
        if v < MIN_OUTPUT_ALPHA - m or v <= 0.0:
            continue
        row[x] = v
        if v < MIN_OUTPUT_ALPHA + m:
            optional.add(x)
    return Outcome(row, frozenset(optional), (rounds,))


def _floor_choices(alphas):
    """em.rs:434-441: the vectors that flooring at 0.01 can leave, one per choice for the entries within the margin."""
    sure = {x: v for x, v in alphas.items() if v >= MIN_OUTPUT_ALPHA + margin(v, v)}
    near = sorted(x for x, v in alphas.items() if x not in sure and v >= MIN_OUTPUT_ALPHA - margin(v, v))
    if len(near) > MAX_NEAR_FLOOR:
        raise _Undecided
    for pick in range(1 << len(near)):
        a = dict(sure)
        a.update((x, alphas[x]) for i, x in enumerate(near) if pick >> i & 1)
        yield a


def _stop(alphas, rounds, classes, offsets, loop, outcomes):
    """What follows a converged round: the output floor (dense), or the floor, one last round and the output floor (subset)."""
    if loop == "dense":
        _add(outcomes, _output(alphas, rounds))
        return
    for a in _floor_choices(alphas):
        _add(outcomes, _output(update(a, classes, offsets), rounds + 1))       # em.rs:391 `|| last_round`, :426-428


def judge_em(classes, num_rows, usa, loop, init="informative"):
    """classes: [(EM label, molecules)] (em_classes of a -d table, or `infer`'s classes as they are); num_rows: the number of
    alphas (USA: 3 G); loop: "dense" or "subset"; init: "informative" or "uniform".  Returns (outcomes, undecided)."""
    assert loop in ("dense", "subset") and init in ("informative", "uniform")
    assert not (usa and loop == "dense"), "the reference has no dense USA loop (quant.rs:887-925)"
    classes = [(tuple(label), int(n)) for label, n in classes]
    offsets = (num_rows // 3, 2 * (num_rows // 3)) if usa else None
    unique = {}
    needs_em = False
    for label, n in classes:                                        # em.rs:322-334, 499-510
        if len(label) == 1:
            unique[label[0]] = unique.get(label[0], 0.0) + n
        else:
            needs_em = True
    if loop == "subset" and not needs_em:                           # em.rs:339-341: as they are - no floor, no round
        return [Outcome({x: v for x, v in unique.items() if v > 0}, frozenset(), (0,))], False
    # em.rs:370-383 over the support; em.rs:519-531 over every alpha, of which only those of some label are ever read or written
    support = support_of(classes, offsets)
    prior = _f32(1.0 / _f32(num_rows))
    return run_loop(classes, offsets, loop, {x: prior if init == "uniform" else (unique.get(x, 0.0) + 0.5) * 1e-3 for x in support}, support)


def run_loop(classes, offsets, loop, alphas, support):
    """The rounds of either loop (em.rs:391-451, 538-572) from an explicit start vector over the support, whatever filled it: an
    initialisation of judge_em, or a bootstrap replicate's random start (tests/boot_judge.py).  Returns (outcomes, undecided)."""
    outcomes = []
    rounds = 0
    try:
        while True:                                                 # em.rs:391, 538
            out = update(alphas, classes, offsets)
            verdict = _round_verdict(alphas, out, support)
            alphas = out
            rounds += 1
            if rounds < MIN_ITER:
                continue
            if rounds >= MAX_ITER:                                  # the cap: the dense loop ends the same way whatever the verdict
                if loop == "dense" or verdict == "moved":
                    _add(outcomes, _output(alphas, rounds))         # em.rs:434: no last round for a cell capped unconverged
                elif verdict == "still":
                    _stop(alphas, rounds, classes, offsets, loop, outcomes)    # round 101 after a convergence at round 100
                else:
                    _stop(alphas, rounds, classes, offsets, loop, outcomes)
                    _add(outcomes, _output(alphas, rounds))
                break
            if verdict == "still":
                _stop(alphas, rounds, classes, offsets, loop, outcomes)
                break
            if verdict == "near":
                _stop(alphas, rounds, classes, offsets, loop, outcomes)        # ... and the main line goes on
    except _Undecided:
        return [], True
    return outcomes, False


def judge_quant_em(table, num_rows, usa, init="informative"):
    """`quant -r *-em` on a cell's gene-level class table: the dense loop without USA, the subset loop on the USA labels with."""
    return judge_em(em_classes(table, usa, num_rows), num_rows, usa, "subset" if usa else "dense", init)


# -------------------------------------------------------------------------------------------------------------------- admitting

def _as_row(row):
    return {int(c): float(v) for c, v in (row.items() if isinstance(row, dict) else row)}


def _fits(o, row, bar):
    for c in sorted(set(o.row) | set(row)):
        if c not in row:
            if c not in o.optional:
                return f"column {c}: judge {o.row[c]!r}, row lacks it"
        elif c not in o.row:
            return f"column {c}: judge has none, got {row[c]!r}"
        elif abs(row[c] - o.row[c]) > bar * abs(o.row[c]):
            return f"column {c}: judge {o.row[c]!r}, got {row[c]!r} ({abs(row[c] - o.row[c]) / abs(o.row[c]) / U32:.1f} units of 2^-24)"
    return None


def fitting(outcomes, row, tight=True):
    """The outcomes that the row fits (at most one, wherever two outcomes differ by more than the bar)."""
    row = _as_row(row)
    bar = min(HARD_BAR, TIGHT_BAR) if tight else HARD_BAR
    return [o for o in outcomes if _fits(o, row, bar) is None]


def admits(outcomes, row, tight=True):
    """Is the row one of the outcomes?  Every value within HARD_BAR of the judge's and, with tight, within TIGHT_BAR as well.
    True, or a message naming the first difference from the first outcome."""
    if not outcomes:
        return "the judge left this cell undecided"
    row = _as_row(row)
    bar = min(HARD_BAR, TIGHT_BAR) if tight else HARD_BAR
    first = None
    for o in outcomes:
        msg = _fits(o, row, bar)
        if msg is None:
            return True
        first = first or msg
    return f"{first} (against the first of {len(outcomes)} outcomes; none fits)" if len(outcomes) > 1 else first


def rounds_of(outcomes):
    """The admissible round counts where the judge has one outcome (a tuple, of one count as a rule), else None."""
    return outcomes[0].rounds if len(outcomes) == 1 else None
