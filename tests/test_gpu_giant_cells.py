"""The device at the top of a cell's read count: 2^22 reads (tests/giant_cell_cases.py has the cells and what is expected of them,
tests/test_giant_cell_cases_cpu.py shows that those expectations are right).

Three things in csrc/ are decided by a cell's `nrec` alone and met by no other module: the order-free EM's fixed-point scale F
below its default of 40 (2^22 reads: 39, 2^23: 38), parsimony's ceiling of 2^22 reads a cell, and bucket plans of 2^14 and 2^15
buckets.  The giant cr-like / trivial / cr-like-em cells follow a pattern whose row and class table are formulas in N, so the
device is held against the formula, against the oracle bit for bit, and - the EM rows - against tests/em_judge.py, a float64
statement that shares no fixed-point scale with either."""
import time

import numpy as np
import pytest

import em_edges as E
import em_judge as ej
import giant_cell_cases as gc
import quant_judge_cases as qc
from util import assert_same_result, pkg

pytestmark = pytest.mark.gpu

PATTERN_CELLS = [(N, usa) for N in gc.SIZES for usa in (False, True)] + [(gc.BIG, False)]
AB_CELLS = [(N, usa) for N in gc.SIZES + (gc.BIG,) for usa in (False, True)]
_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _device(cfg, t2g, b, off):
    q = pkg.Quantifier(cfg, t2g)
    try:
        got = q.quant_chunks(b, off)
        return got, q.batch_stats(), q.em_instance_counts()
    finally:
        q.close()


def _pattern_oracle(ora, res, N, usa, **kw):
    """The oracle on [50, N, 600] reads; once per module (the EM resolution in the device's fixed-point arithmetic)."""
    b, off = gc.pattern_batch(N)
    return _once((res, N, usa), lambda: ora.quant(gc.cfg(res, usa, **kw), gc.t2g(usa), b, off, em_arith="fixed"))


def _floats(row):
    return {c: float(v) for c, v in row.items()}


# ----------------------------------------------------------------------------------------- 1. closed-form cells: cr-like, trivial

@pytest.mark.parametrize("N,usa", PATTERN_CELLS)
@pytest.mark.parametrize("res", ["cr-like", "trivial"])
def test_rows_are_the_formulas_and_the_oracles(oracle_module, res, N, usa):
    """2^22 - 1 and 2^22 single-ref reads plan 2^14 buckets, one read more 2^15 (n_buckets is the witness, as in
    tests/test_gpu_crlike.py::test_giant_cell_beyond_the_lds_histogram); the neighbours' rows are asserted too."""
    b, off = gc.pattern_batch(N)
    got, st, _ = _device(gc.cfg(res, usa), gc.t2g(usa), b, off)
    assert gc.lg_nb(N) == (14 if N <= 2 ** 22 else 15) and st["n_buckets"] >= 1 << gc.lg_nb(N)
    assert [int(x) for x in got.nrec] == list(gc.batch_sizes(N))
    for k, (n, row) in enumerate(zip(gc.batch_sizes(N), qc.rows_of(got))):
        assert dict(row) == _floats(gc.plain_row(res, n, usa)), f"{res} usa={usa}: cell {k} of {n} reads"
    assert_same_result(got, _pattern_oracle(oracle_module, res, N, usa), what=f"{res} N={N} usa={usa}")


ROUTES = {   # name: (environment, chunk shift)
    "recs": ({"AFQ_TEST_DECODE": "recs"}, 0),
    "keys": ({"AFQ_TEST_DECODE": "keys"}, 0),
    "walk": ({}, 1),                              # chunks at offsets 1 mod 4: the walking decoder
    "slab-cap-8": ({"AFQ_TEST_SLAB_CAP": "8"}, 0),   # every slab of the 32 768-bucket cell overflows: k_fix_slabs places the cell
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_crlike_through_each_route_at_32768_buckets(oracle_module, monkeypatch, route):
    """cr-like at 2^22 + 1 reads through the three decode routes and with slabs that every bucket outgrows: bit-identical rows."""
    N = gc.SIZES[2]
    env, shift = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b, off = gc.pattern_batch(N)
    if shift:
        b, off = np.concatenate((np.zeros(shift, np.uint8), np.frombuffer(b, np.uint8))), off + np.uint64(shift)
    got, st, _ = _device(gc.cfg("cr-like", False), gc.t2g(False), b, off)
    assert st["n_buckets"] >= 32768 and st["n_keys"] == sum(gc.batch_sizes(N))
    assert dict(qc.rows_of(got)[1]) == _floats(gc.crlike_row(N, False)), route
    assert_same_result(got, _pattern_oracle(oracle_module, "cr-like", N, False), what=route)


# ------------------------------------------------------------------------------------------------ 1. closed-form cells: the EM

def _admitted(table, num_rows, usa, row, what):
    """The row before em_judge on the FORMULA's class table: at 1e-4, and at this module's measured tight bar."""
    outcomes, undecided = gc.judge(table, num_rows, usa)
    assert not undecided, what
    m = ej.admits(outcomes, row, tight=False)
    assert m is True, f"{what}: {m}"
    m = gc.admits_within(outcomes, row, gc.GIANT_TIGHT_BAR)
    assert m is True, f"{what}, at {gc.GIANT_K} units of 2^-24: {m}"


@pytest.mark.parametrize("N,usa", PATTERN_CELLS)
def test_crlike_em_rows_at_every_scale(oracle_module, N, usa):
    """F = 40, 39, 39, 38.  The -d class table is the formula's, the row is the fixed-point oracle's bit for bit, and it stands
    before the float64 judge; the giant cell takes the streamed instance of the rounds kernel, its 600-read neighbour the
    smallest (em_edges' mirror of k_em2_setup, against the device's counter)."""
    b, off = gc.pattern_batch(N)
    got, _, counts = _device(gc.cfg("cr-like-em", usa, dump_eq=True), gc.t2g(usa), b, off)
    sizes = gc.batch_sizes(N)
    rows, tables = qc.rows_of(got), qc.classes_of(got)
    assert dict(rows[0]) == _floats(gc.crlike_row(sizes[0], usa)), "the tiny neighbour"
    shapes = [gc.shape_of_table(gc.class_table(n, usa), usa, gc.G) for n in sizes[1:]]
    assert [s.tier for s in shapes] == [3, 0], "the cells no longer cover the streamed instance"
    assert counts == E.instance_counts(shapes), f"device {counts}, mirror {shapes}"
    for k in (1, 2):
        assert dict(tables[k]) == gc.class_table(sizes[k], usa), f"cell of {sizes[k]} reads"
    assert_same_result(got, _pattern_oracle(oracle_module, "cr-like-em", N, usa, dump_eq=True), what=f"N={N} usa={usa}")
    for k in (1, 2):
        _admitted(gc.class_table(sizes[k], usa), gc.dims(usa)[1], usa, dict(rows[k]), f"cell of {sizes[k]} reads, usa={usa}, F={gc.fbits(sizes[k])}")


# ------------------------------------------------------------------------------------------------ 2. the accumulator at its top

@pytest.mark.parametrize("N,usa", AB_CELLS)
def test_accumulator_just_under_2_pow_62(oracle_module, N, usa):
    """uA = N - 1005 single-label molecules on A: entry A's accumulator starts at uA << F, just under 2^62 at 2^22 - 1 reads and
    about 2^61 at 2^22 and 2^23 - with F left at 40 it would pass 2^62 and, at 2^23 reads, start at 2^63."""
    b, off = gc.ab_batch(N, usa)
    t2g, _, num_rows = gc.ab_dims(usa)
    cfg = gc.ab_cfg(usa, dump_eq=True)
    got, _, counts = _device(cfg, t2g, b, off)
    assert counts == E.instance_counts([gc.shape_of_table(gc.ab_class_table(N, usa), usa, 2)]) == [1, 0, 0, 0, 0, 0]
    want, iters = oracle_module.quant(cfg, t2g, b, off, em_arith="fixed", want_iters=True)
    assert_same_result(got, want, what=f"N={N} usa={usa}")
    assert dict(qc.classes_of(got)[0]) == gc.ab_class_table(N, usa)
    row = dict(qc.rows_of(got)[0])
    _admitted(gc.ab_class_table(N, usa), num_rows, usa, row, f"{{A, B}} cell of {N} reads, usa={usa}, F={gc.fbits(N)}")
    closed = gc.ab_row_f64(N, int(iters[0]))
    assert set(row) == {0, 1} and all(abs(row[c] - closed[c]) <= gc.GIANT_TIGHT_BAR * closed[c] for c in closed), (row, closed)


# ------------------------------------------------------------------------------------------------- 3. parsimony at its ceiling

@pytest.fixture(scope="module")
def ceiling(oracle_module):
    """resolution -> (the 2^22 - 1-read cell, its config, the oracle's result): one oracle run per resolution and module."""
    made = {}

    def get(res):
        if res not in made:
            d = gc.parsimony_ceiling_cell(dict(gc.PARS_CASES)[res])
            assert [int(x) for x in d.cell_nrec] == [gc.PARS_CEILING - 1]
            cfg = gc.parsimony_cfg(res, d)
            t0 = time.perf_counter()
            want = oracle_module.quant(cfg, d.tid_to_gid, d.data, d.chunk_off, em_arith="fixed")
            print(f"\noracle, {res} on {gc.PARS_CEILING - 1} reads: {time.perf_counter() - t0:.1f} s")
            made[res] = (d, cfg, want)
        return made[res]

    yield get
    made.clear()


@pytest.mark.parametrize("graph", ["default", "per-cell"])
@pytest.mark.parametrize("res", [r for r, _ in gc.PARS_CASES])
def test_parsimony_takes_the_last_cell_under_the_ceiling(ceiling, monkeypatch, res, graph):
    """2^22 - 1 reads, the last cell the phase kernels take (afq_pug2.hip's "cannot happen ... R < 2^22" rests on this bound):
    `parsimony` without USA and `parsimony-em` with, rows bit-exact against the oracle, by the range-wide graph build and by
    the per-cell graph kernel; no cell is handed to the one-workgroup kernel, which would refuse it."""
    d, cfg, want = ceiling(res)
    if graph == "per-cell":
        monkeypatch.setenv("AFQ_TEST_P2_GRAPH", "cell")
    q = pkg.Quantifier(cfg, d.tid_to_gid)
    try:
        got = q.quant_chunks(d.data, d.chunk_off)
        assert q.mono_cell_count() == 0
    finally:
        q.close()
    assert_same_result(got, want, what=f"{res} {graph}")
    assert got.val.sum() > 0


def test_parsimony_refuses_the_first_cell_at_the_ceiling_and_goes_on(ceiling):
    """[300, exactly 2^22, 300 reads] under parsimony: AFQ_ERR_UNSUPPORTED naming cell 1, no rows for the neighbours, and the
    same context then quantifies the 2^22 - 1-read cell to the rows it had before (include/afquant.h documents the limit).
    The same 2^22 reads a cell under cr-like are accepted: test_rows_are_the_formulas_and_the_oracles."""
    d, cfg, want = ceiling("parsimony")
    bad = gc.parsimony_refused_batch()
    assert [int(x) for x in bad.cell_nrec] == [300, gc.PARS_CEILING, 300] and np.array_equal(bad.tid_to_gid, d.tid_to_gid)
    q = pkg.Quantifier(cfg, d.tid_to_gid)
    try:
        with pytest.raises(pkg.AfqError) as e:
            q.quant_chunks(bad.data, bad.chunk_off)
        assert e.value.code == pkg._abi.AFQ_ERR_UNSUPPORTED and "cell 1:" in str(e.value) and "2^22 reads" in str(e.value), e.value
        got = q.quant_chunks(d.data, d.chunk_off)
    finally:
        q.close()
    assert_same_result(got, want, what="after the refusal")
