"""The judge (tests/quant_judge.py) against the hand cases, and the oracle in front of the judge on small fuzzed cells.

The oracle follows the reference's control flow and the kernels were matched to the oracle; the judge states the same results as
definitions, from the reference's text alone.  Where the parsimony cover's scan order decides (the reference walks a HashSet,
pugutils.rs:1110), the judge holds every outcome some order can give, and the oracle's two scans both have to land among them."""
import pytest

import quant_judge as qj
import quant_judge_cases as qc
from util import load_golden, pkg


def test_flag_bits_are_the_packages():
    assert (qj.FLAG_TINY, qj.FLAG_ALT, qj.FLAG_EMPTY) == (pkg._abi.CELL_TINY_PATH, pkg._abi.CELL_ALT_RES, pkg._abi.CELL_EMPTY)


def _exact(j, expected, what):
    assert not j.undecided and len(j.outcomes) == 1, what
    assert qj.admits(j, [tuple(e) for e in expected]) is True, (what, j.outcomes[0][0], expected)


# ------------------------------------------------------------------------------------------------------------------- hand cases

@pytest.mark.parametrize("small_thresh", [0, 100])
def test_crlike_hand_cases(small_thresh):
    for case in load_golden("crlike_hand_cases.json")["cases"]:
        for c in case["cells"]:
            j = qj.judge_cell(c["reads"], case["t2g"], "cr-like", case["usa"], num_rows=case["num_rows"], small_thresh=small_thresh)
            _exact(j, c["expected"], (case["name"], c["bc"], c["why"]))
            assert j.flags == (qj.FLAG_TINY if len(c["reads"]) < small_thresh else 0)


def test_prefer_ambig_hand_cases():
    for case in load_golden("prefer_ambig_hand_cases.json")["cases"]:
        for c in case["cells"]:
            kw = dict(num_rows=case["num_rows"])
            j = qj.judge_cell(c["reads"], case["t2g"], "cr-like", case["usa"], sa_model="prefer-ambig", **kw)
            _exact(j, c["expected"], (case["name"], c["bc"], c["why"]))
            assert j.flags == 0, "prefer-ambig keeps every cell off the tiny path (quant.rs:794)"
            _exact(qj.judge_cell(c["reads"], case["t2g"], "cr-like", case["usa"], small_thresh=0, **kw), c["expected_wta"], "winner-take-all")
    case = load_golden("crlike_hand_cases.json")["cases"][0]     # outside USA mode the switch is ignored (quant.rs:1456-1469)
    for c in case["cells"]:
        j = qj.judge_cell(c["reads"], case["t2g"], "cr-like", False, sa_model="prefer-ambig")
        _exact(j, c["expected"], c["why"])
        assert j.flags == qj.FLAG_TINY


def test_pug_hand_cases():
    d = load_golden("pug_hand_cases.json")
    for c in d["cells"]:
        _exact(qj.judge_cell(c["reads"], d["t2g"], "parsimony", False, small_thresh=0), c["expected"], (c["bc"], c["why"]))
        if "crlike" in c:
            _exact(qj.judge_cell(c["reads"], d["t2g"], "cr-like", False, small_thresh=0), c["crlike"], (c["bc"], "cr-like"))


@pytest.mark.parametrize("m", [63, 64, 126, 127, 128])
def test_direction_rule(m):
    """x -> y only, one base apart, iff reads(x) >= 2 reads(y) (pugutils.rs:88-97): a path with reads (2 m, m, 2 m) is two
    molecules, its middle reaching neither end, and (2 m - 1, m, 2 m - 1) is one."""
    for big, molecules in ((2 * m, 2), (2 * m - 1, 1)):
        for res in ("parsimony", "parsimony-gene"):
            j = qj.judge_cell(qc.path(m, big), qc.S_T2G, res, False, small_thresh=0)
            _exact(j, [(0, molecules)], (m, big, res))


def test_structured_cells_have_the_outcome_written_next_to_them():
    """The CPU twin of test_gpu_quant_judge.py's structured cells: one outcome each, the one worked out by hand."""
    for thresh in (None, 3):
        s = qc.structured(thresh)
        for i, (name, _, classes, _) in enumerate(s.items):
            for res in ("parsimony", "parsimony-em"):
                j = s.judge(i, res)
                assert not j.undecided and len(j.outcomes) == 1, name
                assert j.outcomes[0][1] == classes, (name, j.outcomes[0][1])
                assert j.flags == (qj.FLAG_ALT if thresh else 0)
            assert s.judge(i, "parsimony").outcomes[0][0] == {lab[0]: n for lab, n in classes.items() if len(lab) == 1}, name


# ------------------------------------------------------------------------------------------- the oracle in front of the judge

def _all_admitted(b, js, res, what, classes=False):
    rows, tables, flags = (None, qc.classes_of(res), None) if classes else (qc.rows_of(res), None, res.flags.tolist())
    for i, (j, _) in enumerate(js):
        if j.undecided:
            continue
        got = qj.admits(j, None if classes else rows[i], classes=tables[i] if classes else None, flags=None if classes else flags[i])
        assert got is True, f"{what}, cell {i}: {got}; reads {b.cells[i][1]}"


@pytest.mark.parametrize("case", list(qc.INTEGER_EXACT))
@pytest.mark.parametrize("name", qc.BATCHES + qc.MULTI_BATCHES)
def test_fuzz_integer_exact(oracle, name, case):
    """cr-like, prefer-ambig, trivial: one outcome, and the oracle's row and flags are that outcome on every cell."""
    b = qc.batch(name)
    res, ckw, _ = qc.INTEGER_EXACT[case]
    js = qc.judgements(name, case)
    assert all(not j.undecided and len(j.outcomes) == 1 for j, _ in js)
    got = oracle.quant(b.cfg(res, **ckw), b.s.tid_to_gid, b.data, b.off)
    _all_admitted(b, js, got, f"{name} {case}")
    if case == "cr-like-tiny-below-30":
        tiny = sum(j.flags == qj.FLAG_TINY for j, _ in js)
        assert 0 < tiny < len(js)
    if res == "cr-like":
        em = oracle.quant(b.cfg("cr-like-em", dump_eq=True, **ckw), b.s.tid_to_gid, b.data, b.off)
        _all_admitted(b, js, em, f"{name} {case} -d", classes=True)


def fuzz_counts(js, asc=None, desc=None):
    n = len(js)
    one = [big for j, big in js if not j.undecided and len(j.outcomes) == 1]
    out = dict(cells=n, undecided=sum(j.undecided for j, _ in js), one_outcome=len(one), of_those_with_a_component_of_3=sum(x >= 3 for x in one))
    if asc is not None:
        out["scans_differ"] = sum(a != d for a, d in zip(qc.rows_of(asc), qc.rows_of(desc)))
    return out


@pytest.mark.parametrize("case", list(qc.PARSIMONY))
@pytest.mark.parametrize("name", qc.BATCHES)
def test_fuzz_parsimony(oracle, name, case):
    """The oracle's row under both scan orders, and its class table under the -em sibling, are admitted on every cell; where the
    judge has one outcome the two scans agree.  And the judge judges: at most 1 % undecided, at least 40 % of the cells with
    one outcome, at least 25 % of those with a component of three or more vertices."""
    b = qc.batch(name)
    res, ckw, _ = qc.PARSIMONY[case]
    js = qc.judgements(name, case)
    t2g = b.s.tid_to_gid
    asc = oracle.quant(b.cfg(res, **ckw), t2g, b.data, b.off)
    desc = oracle.quant(b.cfg(res, **ckw), t2g, b.data, b.off, tie_break_descending=True)
    em_cfg = b.cfg(qc.EM_OF[res], dump_eq=True, **ckw)
    for scan, r, e in (("ascending", asc, oracle.quant(em_cfg, t2g, b.data, b.off)),
                       ("descending", desc, oracle.quant(em_cfg, t2g, b.data, b.off, tie_break_descending=True))):
        _all_admitted(b, js, r, f"{name} {case} {scan}")
        _all_admitted(b, js, e, f"{name} {case} {scan} -d", classes=True)
    for i, (a, d) in enumerate(zip(qc.rows_of(asc), qc.rows_of(desc))):
        if not js[i][0].undecided and len(js[i][0].outcomes) == 1:
            assert a == d, f"{name} {case}, cell {i}: one outcome, two rows"
    n = fuzz_counts(js, asc, desc)
    print(f"\n{name} {case}: {n}")
    assert n["undecided"] <= 0.01 * n["cells"], n
    assert n["one_outcome"] >= 0.40 * n["cells"], n
    assert n["of_those_with_a_component_of_3"] >= 0.25 * n["one_outcome"], n
    if case == "large-graph-thresh-3":
        assert any(j.flags == qj.FLAG_ALT for j, _ in js)


# ------------------------------------------------------------------------------------------------------------ the checker bites

def _a_cell(n_outcomes, fits):
    for i, (j, _) in enumerate(qc.judgements("base", "parsimony")):
        if len(j.outcomes) == n_outcomes and fits(j.outcomes):
            return i, j
    raise AssertionError("no such cell in the batch")


def _differing(a, b):
    return [k for k in sorted(set(a) | set(b)) if a.get(k, 0) != b.get(k, 0)]


def test_admits_refuses_what_is_wrong():
    i, j = _a_cell(1, lambda o: len(o[0][0]) >= 3)
    row, classes = j.outcomes[0]
    assert qj.admits(j, row, classes, flags=0) is True and qj.admits(j, sorted(row.items()), sorted(classes.items())) is True
    cols = sorted(row)
    for c in cols:
        for d in (1, -1):
            assert isinstance(qj.admits(j, {**row, c: row[c] + d}), str), "one count off by one"
    moved = dict(row)
    moved[cols[0]] -= 1
    moved[cols[1]] += 1
    assert isinstance(qj.admits(j, {c: v for c, v in moved.items() if v}), str), "a molecule moved to another gene"
    lab = next(l for l in classes if len(l) == 1)
    other = next(l for l in classes if l != lab)
    assert isinstance(qj.admits(j, classes={**classes, lab: classes[lab] - 1, other: classes[other] + 1}), str), "a molecule moved to another label"
    assert isinstance(qj.admits(j, classes={l: n for l, n in classes.items() if l != lab}), str), "a single-gene class dropped"
    assert isinstance(qj.admits(j, {c: v for c, v in row.items() if c != cols[0]}), str), "a column dropped"
    assert isinstance(qj.admits(j, {**row, max(cols) + 1: 1}), str), "a column too many"
    for wrong in (qj.FLAG_TINY, qj.FLAG_ALT, qj.FLAG_EMPTY):
        assert isinstance(qj.admits(j, row, flags=wrong), str), f"flag {wrong:#x}"
    assert isinstance(qj.admits(qj.Judgement([], True, 0), row), str), "an undecided cell admits nothing"


def test_admits_refuses_the_mix_of_two_outcomes():
    i, j = _a_cell(2, lambda o: len(_differing(o[0][0], o[1][0])) >= 2)
    (row_a, cl_a), (row_b, cl_b) = j.outcomes
    assert qj.admits(j, row_a) is True and qj.admits(j, row_b) is True
    differ = _differing(row_a, row_b)
    mix = dict(row_a)
    mix[differ[0]] = row_b.get(differ[0], 0)      # this column from the second outcome, all others from the first
    assert isinstance(qj.admits(j, {c: v for c, v in mix.items() if v}), str)
    labs = _differing(cl_a, cl_b)
    assert len(labs) >= 2
    mixc = dict(cl_a)
    mixc[labs[0]] = cl_b.get(labs[0], 0)
    assert isinstance(qj.admits(j, classes={l: n for l, n in mixc.items() if n}), str)
    assert isinstance(qj.admits(j, row_a, cl_b), str), "the row of one outcome with the classes of the other"


def _chain(k):
    """One UMI under the labels {r}, {r, r+1}, {r+1, r+2}, {r+2} (r = 5 k; every ref its own gene): a path of four vertices, all
    edges at distance 0.  The largest candidates are the three neighbouring pairs.  Either end pair first leaves the other end
    pair: molecules of genes r and r+2.  The middle pair first is a molecule of their common ref r+1 and leaves both ends alone:
    genes r, r+1, r+2.  Two outcomes, whatever the rest of the cell holds."""
    r, umi = 5 * k, 0x111 * (k + 1)
    return [(umi, [r]), (umi, [r, r + 1]), (umi, [r + 1, r + 2]), (umi, [r + 2])]


def test_two_outcomes_by_hand_and_the_bound(oracle):
    t2g = list(range(5 * 13))
    j = qj.judge_cell(_chain(0), t2g, "parsimony", False, small_thresh=0)
    assert sorted(sorted(row.items()) for row, _ in j.outcomes) == [[(0, 1), (1, 1), (2, 1)], [(0, 1), (2, 1)]]
    three = [r for k in range(3) for r in _chain(k)]
    j3 = qj.judge_cell(three, t2g, "parsimony", False, small_thresh=0)
    assert len(j3.outcomes) == 8 and not j3.undecided
    b, off = pkg.rad.encode_cells([(1, three)], 4, 4)
    cfg = pkg.WorkerConfig.for_resolution("parsimony", num_genes=len(t2g), num_rows=len(t2g), small_thresh=0)
    for desc in (False, True):
        assert qj.admits(j3, qc.rows_of(oracle.quant(cfg, t2g, b, off, tie_break_descending=desc))[0]) is True
    assert isinstance(qj.admits(j3, {0: 1, 2: 1, 5: 1, 7: 1, 10: 1, 11: 1}), str), "gene 11 without gene 12: no scan leaves that"
    twelve = qj.judge_cell([r for k in range(12) for r in _chain(k)], t2g, "parsimony", False, small_thresh=0)
    assert len(twelve.outcomes) == qj.BOUND and not twelve.undecided
    thirteen = qj.judge_cell([r for k in range(13) for r in _chain(k)], t2g, "parsimony", False, small_thresh=0)
    assert thirteen.undecided and thirteen.outcomes == []
    assert isinstance(qj.admits(thirteen, {0: 1}), str)
