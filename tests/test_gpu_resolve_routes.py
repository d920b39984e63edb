"""The routes of the cr-like resolve, each against the oracle (bit-exact).  k_resolve_hash resolves the buckets its UMI table
serves and hands every other one to k_resolve_sort through a divert list (afq_resolve_divert_count): single-bucket cells,
buckets of 257..512 keys, a UMI that does not fit 32 bits, a UMI with more genes than the in-register merge holds (kHtMerge),
a bucket with more parked keys than the table keeps (kHtOvf).  Buckets over 512 keys go on to k_resolve_mid.  Every case runs
twice: as the library routes it, and with AFQ_TEST_RESOLVE_DIVERT=all, which sends every bucket down the divert list."""
import hashlib
import importlib

import numpy as np
import pytest

from util import assert_same_result, cfg_for, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
synth = pkg.synth

ROUTES = ["table", "divert-all"]


def _route(monkeypatch, route):
    if route == "divert-all":
        monkeypatch.setenv("AFQ_TEST_RESOLVE_DIVERT", "all")
    else:
        monkeypatch.delenv("AFQ_TEST_RESOLVE_DIVERT", raising=False)


def run_both(oracle, cfg, t2g, b, off):
    q = pkg.Quantifier(cfg, t2g)
    try:
        got = q.quant_chunks(b, off)
        st = q.batch_stats()
        st["n_divert"] = q.resolve_divert_count()
    finally:
        q.close()
    want = oracle.quant(cfg, t2g, b, off)
    assert_same_result(got, want)
    return got, st


def _check_diverted(st, route, at_least=1):
    if route == "divert-all":   # every bucket that is neither empty nor over 512 keys
        assert st["n_divert"] >= at_least and st["n_divert"] <= st["n_buckets"] - st["n_overflow_buckets"]
    else:
        assert st["n_divert"] >= at_least, st


def _multi_bucket_pad(rng, n, n_txp):
    """n single-read UMIs that push a cell over one bucket"""
    return [(int(rng.integers(1 << 20, 1 << 24)), [int(rng.integers(0, n_txp))]) for _ in range(n)]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("usa", [False, True])
def test_wide_umis(oracle, monkeypatch, route, usa):
    """UMIs of an 8-byte field that do not fit the table's 32-bit slot word (0xFFFFFFFF itself included), inside a
    multi-bucket cell: their buckets are diverted before anything is written."""
    _route(monkeypatch, route)
    rng = np.random.default_rng(31)
    n_txp, num_genes = 64, 32
    reads = _multi_bucket_pad(rng, 3000, n_txp)
    for wide in (0xFFFFFFFF, 0xFFFFFFFE, 0x100000005, 0xABC12345678):
        reads += [(wide, [3]), (wide, [3]), (wide, [9]), (wide, [40])]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    b, off = rad.encode_cells([(5, reads), (6, reads[:900])], 4, 8)
    cfg = pkg.WorkerConfig.for_resolution("cr-like", usa_mode=usa, num_genes=num_genes, num_rows=(num_genes // 2) * 3 if usa else num_genes,
                                          bc_bytes=4, umi_bytes=8, small_thresh=0)
    got, st = run_both(oracle, cfg, (np.arange(n_txp, dtype=np.uint32) % 32), b, off)
    _check_diverted(st, route)
    assert got.val.sum() > 0


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n_genes", [8, 9, 14])
def test_umi_with_many_genes(oracle, monkeypatch, route, n_genes):
    """One UMI seen with n_genes genes (ties and a unique winner): three sit in its slot, the rest are parked; the merge holds
    kHtMerge = 8 genes, so 9 and 14 send the bucket to the sort path and 8 is resolved by the table."""
    _route(monkeypatch, route)
    rng = np.random.default_rng(40 + n_genes)
    n_txp = 200
    reads = _multi_bucket_pad(rng, 2500, n_txp)
    for k, umi in enumerate((77, 78, 79)):
        genes = rng.choice(n_txp, size=n_genes, replace=False)
        for j, g in enumerate(genes):
            reads += [(umi, [int(g)])] * (1 + (j == k))   # UMI 77 / 78 / 79: the first / second / third gene wins
    reads += [(80, [int(g)]) for g in rng.choice(n_txp, size=n_genes, replace=False)]   # all tied
    reads = [reads[i] for i in rng.permutation(len(reads))]
    b, off = rad.encode_cells([(1, reads)], 4, 4)
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=n_txp, num_rows=n_txp, small_thresh=0)
    _, st = run_both(oracle, cfg, np.arange(n_txp, dtype=np.uint32), b, off)
    _check_diverted(st, route, at_least=1 if (n_genes > 8 or route == "divert-all") else 0)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("usa", [False, True])
def test_parked_keys_beyond_the_list(oracle, monkeypatch, route, usa):
    """Half of the UMIs seen with four to six genes, one read each, the other half with one: one to three keys of such a UMI
    are parked, about 60 per bucket - more than the kHtOvf = 64 the table keeps in some buckets, fewer in others (those resolve
    through the merge)."""
    _route(monkeypatch, route)
    rng = np.random.default_rng(50 + usa)
    n_txp = 400
    reads = []
    for umi in range(1000, 1000 + 1000):
        k = (1, 1, 1, 4, 5, 6)[int(rng.integers(0, 6))]
        reads += [(umi * 7919, [int(g)]) for g in rng.choice(n_txp, size=k, replace=False)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    b, off = rad.encode_cells([(2, reads), (3, reads[: len(reads) // 2])], 4, 4)
    num_genes = n_txp // 2 if usa else n_txp
    cfg = pkg.WorkerConfig.for_resolution("cr-like", usa_mode=usa, num_genes=num_genes, num_rows=(num_genes // 2) * 3 if usa else num_genes,
                                          small_thresh=0)
    t2g = (np.arange(n_txp, dtype=np.uint32) // 2) if usa else np.arange(n_txp, dtype=np.uint32)
    _, st = run_both(oracle, cfg, t2g, b, off)
    _check_diverted(st, route)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("slab_cap", [None, "512", "8"])
@pytest.mark.parametrize("n_same", [400, 1500])
def test_large_buckets(oracle, monkeypatch, route, slab_cap, n_same):
    """One UMI carried by n_same reads: a bucket of 257..512 keys (the sort path of k_resolve_sort) or over 512 (k_resolve_mid),
    placed in slabs that hold it (512), that it outgrows (default 384), or that every bucket outgrows (8)."""
    _route(monkeypatch, route)
    if slab_cap:
        monkeypatch.setenv("AFQ_TEST_SLAB_CAP", slab_cap)
    s = synth.synth(60, [n_same + 3000, 700], num_genes=400, dup=0.3, cross=0.6)
    umi = s.umi.copy()
    umi[:n_same] = 0x0A0B0C
    s.umi = umi
    b, off = s.encode()
    _, st = run_both(oracle, cfg_for(s), s.tid_to_gid, b, off)
    if n_same > 512:
        assert st["n_overflow_buckets"] >= 1
    else:
        _check_diverted(st, route)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("usa", [False, True])
def test_single_bucket_cells(oracle, monkeypatch, route, usa):
    """Cells of at most 256 keys are one bucket: the sort path sorts and counts their columns in place.  small_thresh = 0, so
    that they are not all on the tiny-cell path; next to multi-bucket cells of the same batch."""
    _route(monkeypatch, route)
    sizes = [1, 2, 3, 17, 64, 99, 100, 180, 250, 256, 257, 900, 5000]
    s = synth.synth(61 + usa, sizes, num_genes=300, usa=usa, dup=0.5, zipf=0.5, cross=0.6, max_extra_na=4)
    b, off = s.encode()
    _, st = run_both(oracle, cfg_for(s, small_thresh=0), s.tid_to_gid, b, off)
    _check_diverted(st, route, at_least=5)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("usa", [False, True])
def test_crlike_em(oracle, monkeypatch, route, usa):
    """cr-like-em: the hash kernel stages the labels of tied molecules and the sort path writes them straight to the label
    area; the EM on the device follows the oracle's operation order, so the rows are bit-identical."""
    _route(monkeypatch, route)
    sizes = [20000, 6000, 1500, 700, 260, 250, 120, 99, 40, 3]
    s = synth.synth(62 + usa, sizes, num_genes=300, usa=usa, dup=0.5, zipf=0.5, cross=0.7, max_extra_na=6)
    umi = s.umi.copy()
    umi[:600] = umi[0]   # and a bucket over 512 keys in the first cell
    s.umi = umi
    b, off = s.encode()
    got, st = run_both(oracle, cfg_for(s, "cr-like-em"), s.tid_to_gid, b, off)
    _check_diverted(st, route)
    assert (got.val != np.round(got.val)).any()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("usa", [False, True])
def test_many_gene_batch(oracle, monkeypatch, route, usa):
    """A batch whose reads average two or more alignments (the label-length tail): cr-like buckets through the two-table
    hash (the MULTI instance), the rest sorted; cr-like-em of such a batch is sorted without a hash pass."""
    _route(monkeypatch, route)
    sn = importlib.import_module("alevin-fry_amd.synth_native")
    d = sn.generate(seed=63 + usa, n_cells=70, median_reads=2500.0, sigma=1.4, num_genes=300, txp_per_gene=4, usa=usa, umi_err=0.02,
                    tail=0.75, tail_max=64, family=8)
    for resolution in ("cr-like", "cr-like-em"):
        cfg = pkg.WorkerConfig.for_resolution(resolution, usa_mode=usa, num_genes=d.num_genes, num_rows=d.num_rows, umi_len=12)
        _, st = run_both(oracle, cfg, d.tid_to_gid, d.data, d.chunk_off)
        if resolution == "cr-like":
            _check_diverted(st, route)


def _digest(r):
    h = hashlib.sha256()
    for a in (r.cell_ptr, r.gene, r.val.view(np.uint32), r.bc, r.nrec, r.flags):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_bench_sized_sample_through_the_divert_list(monkeypatch):
    """The configs[1]-sized sample (11 000 cells, ~4e8 reads): the table diverts under 1 % of the buckets, and the same batch
    with every bucket sent down the divert list to the sort path gives the same rows bit for bit."""
    sn = importlib.import_module("alevin-fry_amd.synth_native")
    d = sn.generate(seed=2, n_cells=11000, median_reads=30000.0, sigma=0.6, num_genes=36601, txp_per_gene=5)
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=d.num_genes, num_rows=d.num_rows)
    q = pkg.Quantifier(cfg, d.tid_to_gid)
    try:
        monkeypatch.delenv("AFQ_TEST_RESOLVE_DIVERT", raising=False)
        r = q.quant_chunks(d.data, d.chunk_off)
        st, n_div = q.batch_stats(), q.resolve_divert_count()
        print(f"\nbench-sized sample: {st['n_buckets']} buckets, {n_div} diverted ({100.0 * n_div / st['n_buckets']:.3f} %), "
              f"{st['n_overflow_buckets']} over 512 keys")
        assert n_div < 0.01 * st["n_buckets"]
        monkeypatch.setenv("AFQ_TEST_RESOLVE_DIVERT", "all")
        r_all = q.quant_chunks(d.data, d.chunk_off)
        st_all, n_all = q.batch_stats(), q.resolve_divert_count()
        print(f"divert-all: {n_all} diverted of {st_all['n_buckets']}")
        assert n_all > 0.9 * st_all["n_buckets"] and n_all <= st_all["n_buckets"] - st_all["n_overflow_buckets"]
        assert _digest(r_all) == _digest(r)
    finally:
        q.close()
