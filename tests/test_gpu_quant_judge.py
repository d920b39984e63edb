"""The device in front of the judge (tests/quant_judge.py): the rows, flags and class tables that pkg.Quantifier returns, against
a statement of the reference's rules that shares nothing with the oracle or the kernels.  These tests ADD a judge; every comparison
with the oracle stays where it is.  The integer-exact resolutions have to equal the judge's one outcome; a parsimony row has to be
one of the outcomes that some scan order of the cover can give (the reference's own order is a HashSet's, pugutils.rs:1110), and
equal where there is only one.  tests/test_quant_judge_cpu.py puts the oracle before the same judge, on the same cells."""
import numpy as np
import pytest

import quant_judge as qj
import quant_judge_cases as qc
from pug_routes import PUG_ROUTES, set_pug_route
from util import pkg

pytestmark = pytest.mark.gpu

DECODE_ROUTES = {
    "as-planned": {},
    "decode-recs": {"AFQ_TEST_DECODE": "recs"},
    "decode-keys": {"AFQ_TEST_DECODE": "keys"},
}
# what only a cell of several buckets can reach (csrc/afq_api.cpp plans more than one bucket above 256 alignment words): slabs that
# every bucket outgrows, so that the placement fix-up runs, and the sort resolve in place of the UMI table
BUCKET_ROUTES = {
    **DECODE_ROUTES,
    "slab-cap-8": {"AFQ_TEST_SLAB_CAP": "8"},
    "divert-all": {"AFQ_TEST_RESOLVE_DIVERT": "all"},
}
ALL_CASES = {**qc.INTEGER_EXACT, **qc.PARSIMONY}


@pytest.fixture(scope="module")
def judged():
    """{(batch, case): the judgement of every cell}, computed here once for the module, shared by its tests, never changed."""
    out = {(name, case): [j for j, _ in qc.judgements(name, case)] for name in qc.BATCHES for case in ALL_CASES}
    out.update({(name, case): [j for j, _ in qc.judgements(name, case)] for name in qc.MULTI_BATCHES for case in qc.INTEGER_EXACT})
    return out


def _device(cfg, t2g, data, off, stats=None):
    q = pkg.Quantifier(cfg, np.asarray(t2g, np.uint32))
    try:
        got = q.quant_chunks(data, off)
        if stats is not None:
            stats.update(q.batch_stats(), n_divert=q.resolve_divert_count())
        return got
    finally:
        q.close()


def _judge_device(got, cells, js, what, classes=False):
    assert got.n_cells == len(cells)
    assert [int(x) for x in got.bc] == [bc for bc, _ in cells] and [int(x) for x in got.nrec] == [len(r) for _, r in cells], what
    rows, tables, flags = (None, qc.classes_of(got), got.flags.tolist()) if classes else (qc.rows_of(got), None, got.flags.tolist())
    judged_cells = 0
    for i, j in enumerate(js):
        if j.undecided:
            continue
        m = qj.admits(j, None if classes else rows[i], classes=tables[i] if classes else None, flags=flags[i])
        assert m is True, f"{what}, cell {i} ({len(j.outcomes)} outcome(s)): {m}; reads {cells[i][1]}"
        judged_cells += 1
    assert judged_cells >= 0.99 * len(cells), what


@pytest.mark.parametrize("route", list(DECODE_ROUTES))
@pytest.mark.parametrize("case", list(qc.INTEGER_EXACT))
@pytest.mark.parametrize("name", qc.BATCHES)
def test_integer_exact_rows_are_the_judges(judged, monkeypatch, name, case, route):
    """cr-like (with and without tiny cells), prefer-ambig, trivial; USA and not; as planned and through each walk-free decoder:
    rows and flags equal the judge's single outcome.  These cells are one bucket each, which the cr-like resolve sorts: the slab
    and resolve routes are test_multi_bucket_cells'."""
    for k, v in DECODE_ROUTES[route].items():
        monkeypatch.setenv(k, v)
    b = qc.batch(name)
    res, ckw, _ = qc.INTEGER_EXACT[case]
    js = judged[name, case]
    assert all(len(j.outcomes) == 1 for j in js)
    _judge_device(_device(b.cfg(res, **ckw), b.t2g, b.data, b.off), b.cells, js, f"{name} {case} {route}")


@pytest.mark.parametrize("route", list(BUCKET_ROUTES))
@pytest.mark.parametrize("case", list(qc.INTEGER_EXACT))
@pytest.mark.parametrize("name", qc.MULTI_BATCHES)
def test_multi_bucket_cells(judged, monkeypatch, name, case, route):
    """Cells of 280 to 2500 reads - several buckets each, 100 to 250 keys a bucket - next to a few small ones, USA and not: rows
    and flags equal the judge's single outcome through both decoders, with slabs of 8 keys and with every bucket sent to the sort
    resolve.  The batch's own counters say that the route was taken: the cells hold more buckets than there are cells; as
    planned, the UMI table resolves more than half of the buckets (the divert list holds the single-bucket cells and the buckets
    above 256 keys); under divert-all the list holds nearly all of them; with slabs of 8 keys the mean bucket holds more than 8,
    so slabs overflow.  `trivial` and USA prefer-ambig are the sort path's whatever the route, so the table is not asked for there."""
    for k, v in BUCKET_ROUTES[route].items():
        monkeypatch.setenv(k, v)
    b = qc.batch(name)
    res, ckw, _ = qc.INTEGER_EXACT[case]
    js = judged[name, case]
    assert all(len(j.outcomes) == 1 for j in js)
    st = {}
    _judge_device(_device(b.cfg(res, **ckw), b.t2g, b.data, b.off, stats=st), b.cells, js, f"{name} {case} {route}")
    print(f"\n{name} {case} {route}: {st}")
    live = st["n_buckets"] - st["n_overflow_buckets"]     # buckets over 512 keys are neither the table's nor the divert list's
    assert st["n_buckets"] >= 3 * len(b.cells), st
    if route == "slab-cap-8":
        assert st["n_keys"] > 8 * st["n_buckets"], st
    # prefer-ambig in USA mode and trivial send every bucket straight to the sort path (csrc/afq_kernels.hip, launch_resolve)
    if res == "cr-like" and not (b.usa and ckw.get("sa_model") == "prefer-ambig"):
        if route == "divert-all":
            assert 0.9 * live <= st["n_divert"] <= live, st
        else:   # diverted: the single-bucket cells and buckets above 256 keys, the planned mean being at most 256 - under half
            assert live - st["n_divert"] >= 0.5 * live, st


@pytest.mark.parametrize("route", list(PUG_ROUTES))
@pytest.mark.parametrize("case", ["parsimony", "parsimony-gene"])
@pytest.mark.parametrize("name", qc.BATCHES)
def test_parsimony_rows_are_admitted_on_every_route(judged, monkeypatch, name, case, route):
    """The row is one of the judge's outcomes, and the one where there is only one.  No cell of these batches has 300 reads, so
    the two routes that give cells of 300 reads the 1024-thread instances (cover-1024, graph-per-cell-1024) repeat their siblings
    here; the structured cells below hold paths of 315 to 640 reads, which do reach those instances."""
    set_pug_route(monkeypatch, route)
    b = qc.batch(name)
    res, ckw, _ = qc.PARSIMONY[case]
    _judge_device(_device(b.cfg(res, **ckw), b.t2g, b.data, b.off), b.cells, judged[name, case], f"{name} {case} {route}")


@pytest.mark.parametrize("case", ["umi-edit-dist-0", "large-graph-thresh-3"])
@pytest.mark.parametrize("name", qc.BATCHES)
def test_parsimony_switches(judged, name, case):
    """--umi-edit-dist 0, and components above --large-graph-thresh 3 resolved cr-like with the cell flagged."""
    b = qc.batch(name)
    res, ckw, _ = qc.PARSIMONY[case]
    js = judged[name, case]
    got = _device(b.cfg(res, **ckw), b.t2g, b.data, b.off)
    _judge_device(got, b.cells, js, f"{name} {case}")
    if case == "large-graph-thresh-3":
        assert (got.flags & pkg._abi.CELL_ALT_RES).any()


@pytest.mark.parametrize("case", ["cr-like", "prefer-ambig", "parsimony", "parsimony-gene"])
@pytest.mark.parametrize("name", qc.BATCHES)
def test_class_tables_of_the_em_resolutions_are_admitted(judged, name, case):
    """cr-like-em, parsimony-em, parsimony-gene-em with dump_eq: the gene-level classes the EM is given (what -d dumps).  The EM's
    values are judged from these tables on in tests/test_gpu_em_judge.py."""
    b = qc.batch(name)
    res, ckw, _ = ALL_CASES[case]
    got = _device(b.cfg(qc.EM_OF[res], dump_eq=True, **ckw), b.t2g, b.data, b.off)
    _judge_device(got, b.cells, judged[name, case], f"{name} {qc.EM_OF[res]} -d", classes=True)


@pytest.mark.parametrize("route", list(PUG_ROUTES))
@pytest.mark.parametrize("thresh", [None, 3])
@pytest.mark.parametrize("res", ["parsimony", "parsimony-em"])
def test_structured_cells(monkeypatch, res, thresh, route):
    """Paths on both sides of the direction rule's threshold; stars of 1, 3, 7, 8, 63 and 64 leaves round a hub (the
    lane-per-component, eight-lane, wave and above-64 covers; 65 vertices hand the cell to the per-cell kernel), alone and six in one
    cell; stars whose labels share one ref, or two refs of two genes; one UMI under twelve labels; near-misses without a shared ref;
    a component above large_graph_thresh 3.  Each has one outcome, written down by hand in quant_judge_cases.structured_cells and
    checked against the judge by tests/test_quant_judge_cpu.py; the device has to give exactly it."""
    set_pug_route(monkeypatch, route)
    s = qc.structured(thresh)
    em = res.endswith("-em")
    js = [s.judge(i, res) for i in range(len(s.items))]
    assert all(not j.undecided and len(j.outcomes) == 1 and j.outcomes[0][1] == c[2] for j, c in zip(js, s.items))
    got = _device(s.cfg(res, dump_eq=em), s.t2g, s.data, s.off)
    for i, (name, _, _, _) in enumerate(s.items):
        m = qj.admits(js[i], None if em else qc.rows_of(got)[i], classes=qc.classes_of(got)[i] if em else None, flags=int(got.flags[i]))
        assert m is True, f"{name} {res} {route}: {m}"
    assert [int(x) for x in got.nrec] == [len(c[1]) for c in s.items]
