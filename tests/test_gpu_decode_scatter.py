"""GPU parity tests (bit-exact) of the scattering record decoder: lane-per-record decode of a batch without parsimony cells places
the keys of multi-bucket cells straight into their bucket slabs (no k_scatter).  Its fallbacks - cells whose walk-free proof
fails, cells whose slabs overflow - are decoded again into keys0 and placed exactly; every case against the CPU oracle."""
import numpy as np
import pytest

from util import assert_same_result, cfg_for, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
synth = pkg.synth


@pytest.fixture(autouse=True)
def records_decoder(monkeypatch):
    """The lane-per-record decoder whatever the batch's record lengths (the route under test)."""
    monkeypatch.setenv("AFQ_TEST_DECODE", "recs")


def run_both(oracle, cfg, t2g, b, off):
    q = pkg.Quantifier(cfg, t2g)
    try:
        got = q.quant_chunks(b, off)
        st = q.batch_stats()
    finally:
        q.close()
    want = oracle.quant(cfg, t2g, b, off)
    return got, want, st


def encode(s, width):
    return rad.encode_cells_np(s.cell_nrec, s.cell_bc, s.umi, s.na, s.refs, bc_bytes=width, umi_bytes=width)


@pytest.mark.parametrize("cap", ["8", "200"])
@pytest.mark.parametrize("res,usa", [("cr-like", False), ("cr-like-em", True), ("trivial", False)])
def test_slab_overflow(oracle, monkeypatch, cap, res, usa):
    """Slabs so small that every multi-bucket cell overflows (8), and slabs only a heavy-UMI cell outgrows (200): the overflowed
    cells are decoded again into keys0 and placed exactly, next to cells that did not overflow."""
    monkeypatch.setenv("AFQ_TEST_SLAB_CAP", cap)
    s = synth.synth(81, [40000, 12000, 3000, 900, 300, 60, 4], num_genes=500, txp_per_gene=3, usa=usa, dup=0.5, zipf=0.7, cross=0.3,
                    umi_err=0.02)
    r0 = int(s.cell_nrec[0])
    s.umi[r0:r0 + 900] = s.umi[r0]   # one UMI with 900 reads in the second cell: a bucket far above its slab
    b, off = s.encode()
    got, want, st = run_both(oracle, cfg_for(s, res), s.tid_to_gid, b, off)
    assert_same_result(got, want, what=f"{res} cap {cap}")
    assert st["n_fallback_cells"] == 0   # (an overflow is not a failed proof)
    assert got.val.sum() > 0


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("res", ["cr-like", "cr-like-em", "trivial"])
def test_proof_failures_next_to_clean_cells(oracle, res, width):
    """Cells whose UMI words equal their barcode give the walk-free decoder false record starts, so their proof fails: one
    multi-bucket cell and one single-bucket cell of that kind, in one range with clean cells of both kinds."""
    s = synth.synth(82, [9000, 5000, 2500, 150, 90, 7], num_genes=300, dup=0.4, cross=0.3, umi_err=0.02)
    starts = np.concatenate([[0], np.cumsum(s.cell_nrec)]).astype(np.int64)
    for c in (1, 4):   # a multi-bucket cell and a single-bucket one: every seventh read's UMI is the barcode
        s.umi[starts[c]:starts[c + 1]:7] = s.cell_bc[c]
    b, off = encode(s, width)
    cfg = cfg_for(s, res, bc_bytes=width, umi_bytes=width)
    got, want, st = run_both(oracle, cfg, s.tid_to_gid, b, off)
    assert_same_result(got, want, what=f"{res} width {width}")
    assert st["n_fallback_cells"] == 2


@pytest.mark.parametrize("usa", [False, True])
def test_instances_and_single_bucket_cells(oracle, usa):
    """One range with a cell of 1024 buckets (the kLdsBins instance), one of 4096 (beyond kLdsBins: a cursor atomic per key),
    cells of 2-512 buckets and single-bucket cells."""
    s = synth.synth(83, [600000, 200000, 30000, 3000, 600, 200, 40, 1], num_genes=3000, usa=usa, dup=0.4, zipf=0.8)
    b, off = s.encode()
    got, want, st = run_both(oracle, cfg_for(s), s.tid_to_gid, b, off)
    assert st["n_buckets"] >= 4096 + 1024
    assert_same_result(got, want)
    assert st["n_fallback_cells"] == 0


@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("res", ["cr-like", "cr-like-em", "trivial"])
def test_modes_and_field_widths(oracle, res, usa):
    """trivial, USA and cr-like-em over 4- and 8-byte barcode / UMI fields."""
    s = synth.synth(84, [20000, 7000, 1500, 400, 120, 30, 2], num_genes=400, txp_per_gene=3, usa=usa, dup=0.5, cross=0.3, umi_err=0.02)
    for width in (4, 8):
        b, off = encode(s, width)
        got, want, st = run_both(oracle, cfg_for(s, res, bc_bytes=width, umi_bytes=width), s.tid_to_gid, b, off)
        assert_same_result(got, want, what=f"{res} usa={usa} width {width}")
        assert st["n_fallback_cells"] == 0


TILE_SLABS, STAGE_KEYS = 16, 1536   # the decoder's tile (AFQ_DTILE_SLABS x 4 waves) and its LDS stage (AFQ_DTILE_KEYS)


def max_tile_keys(s, width=4):
    """Most keys any decoder tile of a multi-bucket cell holds: records counted where they start (1 KiB slabs from the chunk start),
    a record's keys = its distinct genes (cr-like)."""
    hw = 1 + 2 * (width // 4)
    starts = np.concatenate([[0], np.cumsum(s.na)]).astype(np.int64)
    genes = s.tid_to_gid[np.asarray(s.refs, np.int64)]
    rec = 0
    most = 0
    for n in s.cell_nrec.astype(np.int64):
        na = s.na[rec:rec + n].astype(np.int64)
        pos = 2 + np.concatenate([[0], np.cumsum(hw + na)[:-1]])   # dword of every record start
        keys = np.array([len(set(genes[starts[r]:starts[r + 1]].tolist())) for r in range(rec, rec + n)], np.int64)
        if na.sum() > 256:   # (a multi-bucket cell)
            most = max(most, int(np.bincount(pos // (256 * TILE_SLABS), weights=keys).max()))
        rec += n
    return most


@pytest.mark.parametrize("cap", [None, "200", "8"])
@pytest.mark.parametrize("res", ["cr-like", "cr-like-em"])
def test_tiles_beyond_the_stage(oracle, monkeypatch, cap, res):
    """USA reads that all carry a gene's spliced and unspliced form: two keys per 20-byte record, more keys per tile than the LDS
    stage holds, so the keys after the stage's prefix go to their buckets one cursor atomic each; with small slabs those direct
    keys overflow too (and go through the spill into keys0)."""
    if cap:
        monkeypatch.setenv("AFQ_TEST_SLAB_CAP", cap)
    s = synth.synth(86, [30000, 9000, 2500, 600, 150, 5], num_genes=400, usa=True, p_unspliced=0.0, p_both=1.0, cross=0.0, dup=0.4,
                    umi_err=0.02)
    assert max_tile_keys(s) > STAGE_KEYS   # (the input does reach the path under test)
    b, off = s.encode()
    got, want, st = run_both(oracle, cfg_for(s, res), s.tid_to_gid, b, off)
    assert_same_result(got, want, what=f"{res} cap {cap}")
    assert st["n_fallback_cells"] == 0


@pytest.mark.parametrize("ranges", ["one", "many"])
def test_context_reused_across_batches(oracle, monkeypatch, ranges):
    """One context, batch after batch, in one range and in many: the tile table and the slabs of one batch must not leak into the
    next, in both orders of sizes."""
    if ranges == "many":
        monkeypatch.setenv("AFQ_TEST_RANGE_BYTES", "150000")
    s = synth.synth(85, [15000, 6000, 3000, 800, 300, 90, 20, 3], num_genes=400, dup=0.4, cross=0.3, umi_err=0.02)
    b, off = s.encode()
    n = len(off)
    cfg = cfg_for(s, "cr-like")

    def batch(a, e):
        lo, hi = int(off[a]), (int(off[e]) if e < n else len(b))
        return b[lo:hi], np.asarray(off[a:e], np.uint64) - np.uint64(lo)

    cuts = [(n - 3, n), (0, n), (0, n), (2, n), (1, n - 2)]
    for order in (cuts, cuts[::-1]):
        q = pkg.Quantifier(cfg, s.tid_to_gid)
        try:
            for a, e in order:
                bb, oo = batch(a, e)
                assert_same_result(q.quant_chunks(bb, oo), oracle.quant(cfg, s.tid_to_gid, bb, oo), what=f"cells [{a}, {e})")
        finally:
            q.close()
