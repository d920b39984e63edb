"""GPU parity tests for the range pipeline's copy stream (csrc/afq_api.cpp: run_batch / run_range / finish_range).

A range whose rows were compacted behind its kernels hands them to a copy stream and the host goes on to enqueue the range
after next without waiting for them (afq_collect does); everything else - a range run again, rows beyond the slot's row
buffers, an error - first lets the copy stream drain.  The hazards are the slot's row buffers (range i+2 compacts into what
range i's rows are still read from) and the result arrays (they grow while rows cross into them).  Every test reads
Quantifier.range_pipeline_counts() - [ranges, non-waiting, fallen back, growths that waited] - so that it cannot pass on one
range or on the waiting path alone, and compares rows, cell order, bc, nrec and flags with the oracle.  The batches are those
of test_many_ranges_pipeline: cells of 5000 ... 1 reads, the small ones last, where a range's rows outlast the next range's
kernels."""
import numpy as np
import pytest

from util import assert_same_result, cfg_for, pkg

pytestmark = pytest.mark.gpu
synth = pkg.synth

SIZES = [5000, 3000, 2500, 2000, 1500, 1200, 900, 600, 300, 120, 60, 20, 5, 1]
# AFQ_TEST_RANGE_BYTES that cuts SIZES into exactly that many ranges (the planner's need per cell: 16 B per alignment word, 48 B
# in cells of more than one bucket, 116 B per read more under parsimony; plan_ranges) - each test asserts the count it got
BUDGET = {"cr-like": {1: "2000000", 2: "600000", 3: "500000", 4: "300000", 9: "40000"},
          "trivial": {1: "2000000", 2: "600000", 3: "500000", 4: "300000", 9: "40000"},
          "parsimony": {1: "1000000000", 2: "2000000", 3: "1000000", 4: "800000", 9: "100000"}}

_cache = {}


def batch(res="cr-like", num_genes=200):
    """(synth, bytes, offsets, config) of the SIZES batch, made once."""
    key = ("batch", num_genes)
    if key not in _cache:
        s = synth.synth(41, SIZES, num_genes=num_genes, txp_per_gene=3, dup=0.5, cross=0.4, umi_err=0.02)
        _cache[key] = (s,) + tuple(s.encode())
    s, b, off = _cache[key]
    return s, b, off, cfg_for(s, res)


def want_of(oracle, key, cfg, t2g, b, off):
    if key not in _cache:
        _cache[key] = oracle.quant(cfg, t2g, b, off, n_threads=16)
    return _cache[key]


def sub_batch(b, off, a, e):
    n = len(off)
    lo, hi = int(off[a]), (int(off[e]) if e < n else len(b))
    return b[lo:hi], np.asarray(off[a:e], np.uint64) - np.uint64(lo)


def stitch(*parts):
    """One batch out of several synth.synth() batches over the same genes, cells in the order given; barcodes made distinct."""
    a = parts[0]
    for p in parts[1:]:
        assert np.array_equal(p.tid_to_gid, a.tid_to_gid) and p.usa == a.usa
    bc = np.concatenate([p.cell_bc ^ np.uint64(k << 28) for k, p in enumerate(parts)])
    return synth.SynthRad(np.concatenate([p.cell_nrec for p in parts]), bc, np.concatenate([p.umi for p in parts]),
                          np.concatenate([p.na for p in parts]), np.concatenate([p.refs for p in parts]), a.tid_to_gid,
                          a.num_genes, a.num_rows, a.usa, max(p.umi_len for p in parts))


@pytest.mark.parametrize("n_ranges", [1, 2, 3, 4, 9])
@pytest.mark.parametrize("res", ["cr-like", "trivial", "parsimony"])
def test_range_counts(oracle, monkeypatch, res, n_ranges):
    """Batches of exactly 1, 2, 3, 4 and 9 ranges: the pipeline's prologue (two ranges enqueued), its steady state and its end
    (the last range is finished in afq_collect).  A context's first batch finds no row buffers and falls back; its second,
    identical one sends every range down the non-waiting path, and nothing has to grow."""
    s, b, off, cfg = batch(res)
    want = want_of(oracle, ("want", res), cfg, s.tid_to_gid, b, off)
    monkeypatch.setenv("AFQ_TEST_RANGE_BYTES", BUDGET[res][n_ranges])
    q = pkg.Quantifier(cfg, s.tid_to_gid)
    try:
        first = q.quant_chunks(b, off)
        c1 = q.range_pipeline_counts()
        assert c1[0] == n_ranges and c1[1] + c1[2] == n_ranges and c1[2] >= 1, c1
        second = q.quant_chunks(b, off)
        c2 = q.range_pipeline_counts()
        assert c2 == [n_ranges, n_ranges, 0, 0], c2
    finally:
        q.close()
    assert_same_result(first, want, what=f"{res}, {n_ranges} ranges, first batch")
    assert_same_result(second, want, what=f"{res}, {n_ranges} ranges, second batch")


def test_slot_buffers_are_not_recycled_under_a_copy(oracle, monkeypatch):
    """Range i+2 compacts into the row buffers range i's rows are copied out of: the same nine-range batch five times on one
    context, every result kept (so every batch's rows land in a block of their own), all compared at the end.  Rows of a few
    kilobytes cross in microseconds, so the link is made slow: AFQ_TEST_ROWS_DELAY_US holds every range's rows back by 0.5 ms,
    several times what the kernels of the following ranges take - without the wait for rows_done in front of the compaction
    the rows that arrive are those of the range after next."""
    s, b, off, cfg = batch()
    want = want_of(oracle, ("want", "cr-like"), cfg, s.tid_to_gid, b, off)
    monkeypatch.setenv("AFQ_TEST_RANGE_BYTES", BUDGET["cr-like"][9])
    monkeypatch.setenv("AFQ_TEST_ROWS_DELAY_US", "500")
    q = pkg.Quantifier(cfg, s.tid_to_gid)
    kept, counts = [], []
    try:
        for _ in range(5):
            kept.append(q.quant_chunks(b, off))
            counts.append(q.range_pipeline_counts())
        for k, c in enumerate(counts):
            assert c[0] == 9 and c[1] + c[2] == 9, (k, c)
            assert k == 0 or c[1] == 9, (k, c)
        for k, got in enumerate(kept):
            assert_same_result(got, want, what=f"batch {k} of five")
    finally:
        q.close()


@pytest.mark.parametrize("order", ["small first", "large first"])
def test_growth_while_rows_are_crossing(oracle, monkeypatch, order):
    """A two-cell batch and the nine-range batch on one context, in both orders, results kept.  After the two-cell batch the slots'
    row buffers and the result arrays (sized from the last batch) are too small for the large one: its ranges fall back, and the
    result arrays grow - moving rows that have landed, never under a copy."""
    s, b, off, cfg = batch(num_genes=3000)   # (rows of up to 3000 entries: the result arrays start at 4096 and have to grow)
    want = want_of(oracle, ("want", "cr-like", 3000), cfg, s.tid_to_gid, b, off)
    b2, off2 = sub_batch(b, off, 7, 9)
    want2 = want_of(oracle, ("want2", "cr-like", 3000), cfg, s.tid_to_gid, b2, off2)
    # (a result block sized from the two cells holds 4096 entries: the large batch's first range fits, the whole batch does not)
    assert int(want.cell_ptr[-1]) > 4096 > int(want.cell_ptr[1]) > int(want2.cell_ptr[-1]) > 0
    monkeypatch.setenv("AFQ_TEST_RANGE_BYTES", BUDGET["cr-like"][9])
    monkeypatch.setenv("AFQ_TEST_ROWS_DELAY_US", "300")   # (the rows are still on their way when the arrays have to grow)
    q = pkg.Quantifier(cfg, s.tid_to_gid)
    kept = []
    try:
        if order == "small first":
            kept.append((q.quant_chunks(b2, off2), want2))
            kept.append((q.quant_chunks(b, off), want))
            c = q.range_pipeline_counts()
            assert c[0] == 9 and c[1] + c[2] == 9 and c[2] >= 1, c   # (the first ranges of either slot find row buffers of two small cells)
        else:
            kept.append((q.quant_chunks(b, off), want))
            kept.append((q.quant_chunks(b2, off2), want2))
            c = q.range_pipeline_counts()
            assert c[0] == 2 and c[1] == 2, c
            # and the large one again, into a fresh result block sized from the two cells: every range's rows cross unwaited-for
            # (the slots have seen them), and the block is outgrown while they do
            kept.append((q.quant_chunks(b, off), want))
            c = q.range_pipeline_counts()
            assert c[0] == 9 and c[1] == 9 and c[3] >= 1, c
        for k, (got, w) in enumerate(kept):
            assert_same_result(got, w, what=f"{order}, batch {k}")
    finally:
        q.close()


def test_a_late_range_beyond_the_slots_row_buffers(oracle, monkeypatch):
    """Small ranges, then one cell with more rows than either slot's row buffers hold, on a context that has seen only the small
    ranges: the large cell's range falls back - its row buffers are freed and grown - while the small ranges' rows are crossing."""
    kw = dict(num_genes=3000, txp_per_gene=3, dup=0.5, cross=0.4, umi_err=0.02)
    small = synth.synth(43, [900, 600, 300, 120, 60, 20, 5, 1], **kw)
    s = stitch(small, synth.synth(44, [9000], **kw))
    cfg = cfg_for(s)
    bs, offs = small.encode()
    b, off = s.encode()
    monkeypatch.setenv("AFQ_TEST_RANGE_BYTES", "1")   # every cell a range of its own
    q = pkg.Quantifier(cfg, s.tid_to_gid)
    try:
        warm = q.quant_chunks(bs, offs)
        got = q.quant_chunks(b, off)
        c = q.range_pipeline_counts()
        assert c[0] == 9 and c[1] == 8 and c[2] == 1, c
    finally:
        q.close()
    assert_same_result(warm, oracle.quant(cfg, s.tid_to_gid, bs, offs), what="the small ranges")
    assert_same_result(got, oracle.quant(cfg, s.tid_to_gid, b, off), what="small ranges, then one large cell")


def test_retry_in_the_middle(oracle, monkeypatch):
    """parsimony with a pool of 12 words per read: the dense 120 000-read cell in the middle of eleven one-cell ranges outgrows
    it and its range is run again with four times the pool (tests/test_gpu_pug.py), while the rows of the ranges in front of it
    are crossing - on the context's second batch, when those ranges no longer wait for their rows."""
    kw = dict(num_genes=17, txp_per_gene=3, usa=True, dup=0.5, cross=0.9, umi_err=0.02, max_extra_na=6, umi_len=7)
    s = stitch(synth.synth(5013, [700, 400, 200], **kw), synth.synth(5012, [900, 120000, 300], **kw), synth.synth(5014, [500, 200, 60, 5, 1], **kw))
    b, off = s.encode()
    cfg = cfg_for(s, "parsimony", small_thresh=0)
    want = oracle.quant(cfg, s.tid_to_gid, b, off, n_threads=16)
    monkeypatch.setenv("AFQ_TEST_POOL_WORDS", "12")
    monkeypatch.setenv("AFQ_TEST_RANGE_BYTES", "1")   # every cell a range of its own
    q = pkg.Quantifier(cfg, s.tid_to_gid)
    try:
        first = q.quant_chunks(b, off)
        r1 = q.pool_regrow_count()
        assert r1 >= 1, "the small first pool was meant to run out"
        second = q.quant_chunks(b, off)
        c = q.range_pipeline_counts()
        assert q.pool_regrow_count() >= r1 + 1
        assert c[0] == 11 and c[1] + c[2] == 11 and c[2] >= 1 and c[1] >= 4, c   # (the four ranges in front of the dense cell at least)
    finally:
        q.close()
    assert_same_result(first, want, what="first batch")
    assert_same_result(second, want, what="second batch")


def test_error_in_the_middle(oracle, monkeypatch):
    """A record's `na` overwritten in the cell that is the fourth of nine ranges (test_bad_input_is_reported_not_crashed), on a
    context whose earlier ranges do not wait for their rows: AFQ_ERR_BAD_INPUT names the cell, and the context then quantifies
    the clean batch."""
    s, b, off, cfg = batch()
    want = want_of(oracle, ("want", "cr-like"), cfg, s.tid_to_gid, b, off)
    monkeypatch.setenv("AFQ_TEST_RANGE_BYTES", BUDGET["cr-like"][9])
    q = pkg.Quantifier(cfg, s.tid_to_gid)
    try:
        assert_same_result(q.quant_chunks(b, off), want, what="clean batch, first")
        assert q.range_pipeline_counts()[0] == 9
        bad = np.asarray(b).copy()
        bad[8 + int(off[3])] = 77   # first record's na in cell 3 (a range of its own, the fourth) no longer tiles the chunk
        with pytest.raises(pkg.AfqError) as e:
            q.quant_chunks(bad, off)
        assert e.value.code == pkg._abi.AFQ_ERR_BAD_INPUT and "cell 3:" in str(e.value), str(e.value)
        c = q.range_pipeline_counts()
        assert c[0] == 9 and c[1] == 3 and c[2] == 1, c   # three ranges' rows were on their way when the fourth reported
        got = q.quant_chunks(b, off)
        assert q.range_pipeline_counts() == [9, 9, 0, 0]
        assert_same_result(got, want, what="clean batch after the error")
    finally:
        q.close()


@pytest.mark.parametrize("pinned", [False, True])
def test_submit_from_host_memory(oracle, monkeypatch, pinned):
    """afq_submit brings the input over range by range (an upload thread for pageable memory, the DMA engine alone for pinned):
    range i+2 is enqueued - and its bytes waited for - right behind range i's early finish."""
    import torch

    s, b, off, cfg = batch()
    want = want_of(oracle, ("want", "cr-like"), cfg, s.tid_to_gid, b, off)
    monkeypatch.setenv("AFQ_TEST_RANGE_BYTES", BUDGET["cr-like"][9])
    q = pkg.Quantifier(cfg, s.tid_to_gid, device=0)
    try:
        for k in range(2):
            if pinned:
                t = torch.empty(len(b), dtype=torch.uint8, pin_memory=True)
                t.numpy()[:] = np.asarray(b)
                q.submit_ptr(t.data_ptr(), len(b), off)
                got = q.collect()
            else:
                got = q.quant_chunks(b, off)
            c = q.range_pipeline_counts()
            assert c[0] == 9 and c[1] + c[2] == 9 and (k == 0 or c[1] == 9), (k, c)
            assert_same_result(got, want, what=f"pinned={pinned}, batch {k}")
    finally:
        q.close()


@pytest.mark.parametrize("delay", ["0", "500"])
def test_submit_device(oracle, monkeypatch, delay):
    """afq_submit_device (input resident on the device: no upload events, what the benchmark's steps call) through the same
    nine ranges, three batches on one context, with the rows on time and held back."""
    import torch

    s, b, off, cfg = batch()
    want = want_of(oracle, ("want", "cr-like"), cfg, s.tid_to_gid, b, off)
    monkeypatch.setenv("AFQ_TEST_RANGE_BYTES", BUDGET["cr-like"][9])
    monkeypatch.setenv("AFQ_TEST_ROWS_DELAY_US", delay)
    d = torch.from_numpy(np.asarray(b).copy()).to("cuda:0")
    torch.cuda.synchronize()
    q = pkg.Quantifier(cfg, s.tid_to_gid, device=0)
    kept = []
    try:
        for k in range(3):
            q.submit_device(d.data_ptr(), d.numel(), off)
            kept.append(q.collect())
            c = q.range_pipeline_counts()
            assert c[0] == 9 and c[1] + c[2] == 9 and (k == 0 or c == [9, 9, 0, 0]), (k, c)
        for k, got in enumerate(kept):
            assert_same_result(got, want, what=f"submit_device, delay {delay} us, batch {k}")
    finally:
        q.close()
