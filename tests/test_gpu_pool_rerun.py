"""GPU parity tests for the parsimony pool's re-runs on a device WITHOUT room for a larger pool.

The parsimony path keeps a range's graph data in one bump-allocated pool (csrc/afq_api.cpp run_range, 24 words per read).  A
range that outgrows it is run again (finish_range): with four times the pool when the device has room for that, otherwise in
halves - a half that fails again regrows or is halved in turn, down to one cell, which takes four times a pool of its own.  A
test box always has room, so AFQ_TEST_POOL_ROOM_WORDS=n stands in for a full device (afq_hooks.h) and AFQ_TEST_POOL_WORDS=12
for dense ranges.  Every test compares the device with the oracle bit for bit (EM resolutions: in the device's arithmetic, as
every `-m gpu` test) and with a plain run of the same batch without the pool hooks.  The routes are named per test (the autouse
fixture of test_gpu_pug.py would run each one seven times)."""
import numpy as np
import pytest

from fuzz_workloads import cell_nrec, first_pool_words, room_budget
from util import assert_same_result, cfg_for, pkg

pytestmark = pytest.mark.gpu
synth = pkg.synth

# about ten cells of 15-40 k reads over 7-nt UMIs (16 384 of them): every vertex has many same-UMI and one-base neighbours, and a
# range of them outgrows a pool of 12 words per read (the regrow test of test_gpu_pug.py, ten times over)
DENSE = [15000, 40000, 22000, 31000, 18000, 36000, 26000, 17000, 33000, 24000]
SMALL = [1, 300]


def stitch(*parts):
    """One batch out of several synth.synth() batches over the same genes (tid_to_gid depends on num_genes, txp_per_gene and usa
    only), cells in the order given; barcodes made distinct."""
    a = parts[0]
    for p in parts[1:]:
        assert np.array_equal(p.tid_to_gid, a.tid_to_gid) and p.usa == a.usa
    bc = np.concatenate([p.cell_bc ^ np.uint64(k << 28) for k, p in enumerate(parts)])
    return synth.SynthRad(np.concatenate([p.cell_nrec for p in parts]), bc, np.concatenate([p.umi for p in parts]),
                          np.concatenate([p.na for p in parts]), np.concatenate([p.refs for p in parts]), a.tid_to_gid,
                          a.num_genes, a.num_rows, a.usa, max(p.umi_len for p in parts))


def dense_batch(usa, where="first"):
    """The dense cells and a 1-read and a 300-read cell in front of them, among them or behind them."""
    kw = dict(num_genes=17, txp_per_gene=3, usa=usa, dup=0.5, cross=0.9, umi_err=0.02, max_extra_na=6, umi_len=7)
    d = synth.synth(7101, DENSE, **kw)
    sm = synth.synth(7102, SMALL, **kw)
    if where == "first":
        return stitch(sm, d)
    if where == "last":
        return stitch(d, sm)
    lo = synth.synth(7101, DENSE[:5], **kw)
    hi = synth.synth(7103, DENSE[5:], **kw)
    return stitch(lo, sm, hi)


def run(cfg, t2g, b, off, env, monkeypatch, first_cell_index=0):
    """One context, one batch under the hooks in env (and none of the pool hooks else): (rows, re-runs, batch statistics)."""
    for k in ("AFQ_TEST_POOL_WORDS", "AFQ_TEST_POOL_ROOM_WORDS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    q = pkg.Quantifier(cfg, t2g)
    try:
        got = q.quant_chunks(b, off, first_cell_index=first_cell_index)
        return got, q.pool_regrow_count(), q.batch_stats()
    finally:
        q.close()
        for k in env:
            monkeypatch.delenv(k, raising=False)


def full_device(nrec, cfg):
    """Pool hooks for a dense range on a full device: 12 words per read, room for twice the range's first pool (no whole-range
    regrow fits) and at least four times the largest cell's own pool (every single cell does)."""
    room = room_budget(nrec, cfg)
    first = first_pool_words(nrec, cfg, 12)
    assert first <= room < 4 * first, (first, room)
    assert all(4 * first_pool_words([n], cfg, 12) <= room for n in nrec)
    return {"AFQ_TEST_POOL_WORDS": "12", "AFQ_TEST_POOL_ROOM_WORDS": str(room)}


_want = {}


def oracle_rows(oracle, key, cfg, t2g, b, off, **kw):
    if key not in _want:
        _want[key] = oracle.quant(cfg, t2g, b, off, n_threads=16, **kw)
    return _want[key]


@pytest.mark.parametrize("graph", ["flat", "per-cell"])
@pytest.mark.parametrize("res,usa", [("parsimony", False), ("parsimony", True), ("parsimony-em", False), ("parsimony-em", True)])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_dense_range_on_a_full_device(oracle, monkeypatch, where, res, usa, graph):
    """Ten dense cells and two small ones in ONE range, a pool of 12 words per read, and a device with room for twice the range's
    pool: the whole range cannot regrow.  A range-wide failure names no cell (the flat graph build fails for the whole range, and
    a bump-pool request fails for whichever cell asked last), so the range is halved until its parts fit or a single cell
    regrows - not cut around cell 0, which with the small cells in front is a one-read cell, and which after three such cuts
    left the rest to a four times larger pool the device did not have (AFQ_ERR_OOM).  Both graph builds: the range-wide flat
    kernels and the per-cell graph kernel (AFQ_TEST_P2_GRAPH=cell) reach different allocation sites."""
    s = dense_batch(usa, where)
    b, off = s.encode()
    cfg = cfg_for(s, res, small_thresh=0)
    route = {"AFQ_TEST_P2_GRAPH": "cell"} if graph == "per-cell" else {}
    want = oracle_rows(oracle, ("dense", where, res, usa), cfg, s.tid_to_gid, b, off)
    got, regrows, st = run(cfg, s.tid_to_gid, b, off, {**route, **full_device(cell_nrec(b, off), cfg)}, monkeypatch)
    assert 1 <= regrows <= 2 * len(off), regrows
    assert_same_result(got, want, what=f"{res} usa={usa} small cells {where}, {graph} graph build")
    plain, plain_regrows, plain_st = run(cfg, s.tid_to_gid, b, off, route, monkeypatch)
    assert_same_result(got, plain, what="the same rows as a run without the pool hooks")
    assert st == plain_st
    assert st["n_records"] == int(s.cell_nrec.sum())


def _assert_same_extras(got, want, what):
    n = got.n_cells
    for i in range(n):
        assert got.eqclasses.cell(i) == want.eqclasses.cell(i), (what, i)
    gb, wb = got.bootstraps, want.bootstraps
    for name in ("mean_ptr", "mean_col", "var_ptr", "var_col"):
        assert np.array_equal(getattr(gb, name), getattr(wb, name)), (what, name)
    assert np.array_equal(gb.mean_val.view(np.uint32), wb.mean_val.view(np.uint32)), what
    assert np.array_equal(gb.var_val.view(np.uint32), wb.var_val.view(np.uint32)), what


@pytest.mark.parametrize("summary_stat", [False, True])
@pytest.mark.parametrize("branch", ["regrow", "halve"])
def test_what_rides_on_a_rerun(oracle, monkeypatch, branch, summary_stat):
    """A range run again must leave everything a plain run leaves: the rows, the -d classes, the -b replicates (drawn per cell
    from first_cell_index + the cell's place in the batch, so a part of a range must draw what the whole range would), the
    flags of cells past --large-graph-thresh, nrec, barcodes and the batch statistics (each failed attempt taken back).  Both
    re-runs: four times the pool (the test box's room) and halves (a full device)."""
    s = dense_batch(True, "middle")
    b, off = s.encode()
    cfg = cfg_for(s, "parsimony-em", small_thresh=0, dump_eq=True, num_bootstraps=5, summary_stat=summary_stat, boot_seed=0x5EED, large_graph_thresh=3000)
    first = 7000
    want = oracle_rows(oracle, ("rides", summary_stat), cfg, s.tid_to_gid, b, off, first_cell_index=first)
    flagged = np.asarray(want.flags) & pkg._abi.CELL_ALT_RES   # (winner-take-all over a component past --large-graph-thresh)
    assert 0 < np.count_nonzero(flagged) < len(off), want.flags
    env = {"AFQ_TEST_POOL_WORDS": "12"}
    if branch == "halve":
        env = full_device(cell_nrec(b, off), cfg)
    got, regrows, st = run(cfg, s.tid_to_gid, b, off, env, monkeypatch, first_cell_index=first)
    assert regrows >= 1
    if branch == "regrow":
        assert regrows <= 3, "the test box has room: the whole range runs again with four times the pool"
    assert got.first_cell_index == first
    assert_same_result(got, want, what=branch)
    _assert_same_extras(got, want, branch)
    plain, _, plain_st = run(cfg, s.tid_to_gid, b, off, {}, monkeypatch, first_cell_index=first)
    assert_same_result(got, plain, what="plain run")
    _assert_same_extras(got, plain, "plain run")
    assert st == plain_st


@pytest.mark.parametrize("source", ["pageable", "pinned", "device"])
def test_rerun_in_the_middle_of_a_pipelined_batch(oracle, monkeypatch, source):
    """A batch cut into many ranges runs them on two buffer sets in turn: a range is re-run (halved, on a full device) while the
    next one is in flight on the other set, and its input arrives piped over PCIe behind the ranges before it (pageable or
    pinned host memory) or is on the device already.  Sparse cells (12-nt UMIs) fill the ranges before and after the dense
    ones.  The same context then takes a second, ordinary batch: its rows equal a fresh context's - the enlarged pool was that
    re-run's alone."""
    import torch

    kw = dict(num_genes=17, txp_per_gene=3, usa=True, dup=0.5, cross=0.9, umi_err=0.02, max_extra_na=6)
    sparse = [9000, 7000, 8000, 6000, 9500, 5000]
    s = stitch(synth.synth(7201, sparse, umi_len=12, **kw), dense_batch(True, "last"), synth.synth(7202, sparse[::-1], umi_len=12, **kw))
    b, off = s.encode()
    nrec = cell_nrec(b, off)
    cfg = cfg_for(s, "parsimony-em", small_thresh=0)
    # (ranges of two or three dense cells: a range's planned bytes are some 40 x its chunk bytes; every range the pool hooks let
    #  start - its first pool is under the room - and none with two dense cells or more regrows whole)
    nbytes = np.diff(np.append(np.asarray(off, np.int64), len(b)))
    monkeypatch.setenv("AFQ_TEST_RANGE_BYTES", str(int(40 * 2.5 * nbytes[len(sparse):len(sparse) + len(DENSE)].max())))
    room = 4 * first_pool_words([int(nrec.max())], cfg, 12)
    hooks = {"AFQ_TEST_POOL_WORDS": "12", "AFQ_TEST_POOL_ROOM_WORDS": str(room)}
    want = oracle_rows(oracle, ("pipelined",), cfg, s.tid_to_gid, b, off)
    s2 = synth.synth(7301, [12000, 3000, 700, 90, 4], umi_len=10, **kw)
    b2, off2 = s2.encode()
    want2 = oracle_rows(oracle, ("second",), cfg, s2.tid_to_gid, b2, off2)

    for k, v in hooks.items():
        monkeypatch.setenv(k, v)
    q = pkg.Quantifier(cfg, s.tid_to_gid)
    try:
        if source == "pageable":
            q.submit(b, off)
        elif source == "pinned":
            h = torch.from_numpy(np.asarray(b).copy()).pin_memory()
            q.submit_ptr(h.data_ptr(), h.numel(), off)
        else:
            d = torch.from_numpy(np.asarray(b).copy()).to("cuda:0")
            q.submit_device(d.data_ptr(), d.numel(), off)
        got = q.collect()
        regrows = q.pool_regrow_count()
        st = q.batch_stats()
        for k in hooks:
            monkeypatch.delenv(k)
        again = q.quant_chunks(b2, off2)
        assert q.pool_regrow_count() == regrows, "the second batch fits the product's pool"
    finally:
        q.close()
    assert regrows >= 1
    assert_same_result(got, want, what=source)
    plain, _, plain_st = run(cfg, s.tid_to_gid, b, off, {}, monkeypatch)
    assert_same_result(got, plain, what="plain run")
    assert st == plain_st
    fresh, _, _ = run(cfg, s2.tid_to_gid, b2, off2, {}, monkeypatch)
    assert_same_result(again, fresh, what="a reused context after a re-run")
    assert_same_result(again, want2, what="second batch")
