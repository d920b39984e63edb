"""GPU parity tests (bit-exact against the oracle) of the scattering decoder's per-bucket LDS words and of the hash resolve's table
at its limits.  The decoder's tail keeps a tile's bucket counts, offsets and slab positions in 16 bits each; its six-workgroup
instance takes cells of up to kDecodeSplitBins buckets (csrc/afq_kernels.h), the other one cells of up to 2048, larger cells one
cursor atomic per key.  k_resolve_hash serves buckets of up to kHtKeys keys from a table of n + n / 8 slots (csrc/afq_kernels.hip)."""
import os
import re

import numpy as np
import pytest

from util import ROOT, assert_same_result, cfg_for, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
synth = pkg.synth


def _const(path, pattern):
    text = open(os.path.join(ROOT, "alevin-fry_amd", "csrc", path)).read()
    return int(re.search(pattern, text).group(1))


SPLIT_BINS = _const("afq_kernels.h", r"#define\s+AFQ_DECODE_SPLIT_BINS\s+(\d+)")
HT_KEYS = _const("afq_kernels.hip", r"constexpr uint32_t kHtKeys = (\d+);")
assert SPLIT_BINS == 1024 and HT_KEYS == 256
# a cell of n_ref alignment words has 2^lg buckets, 256 << lg >= n_ref: both sides of the decoder's instance boundaries
# (1024 | 2048, 2048 | 4096), the old boundary (512 | 1024), small cells and single-bucket cells
BUCKETS = [4096, 2048, 2048, 1024, 1024, 512, 8, 2, 1, 1]


@pytest.fixture(autouse=True)
def records_decoder(monkeypatch):
    """The lane-per-record (scattering) decoder whatever the batch's record lengths."""
    monkeypatch.setenv("AFQ_TEST_DECODE", "recs")


def bucket_of(umi, lg):
    """csrc/afq_common.h bucket_of, restated"""
    umi = np.asarray(umi, np.uint64)
    lo, hi = umi & np.uint64(0xFFFFFFFF), umi >> np.uint64(32)
    x = (lo ^ ((hi << np.uint64(19)) & np.uint64(0xFFFFFFFF)) ^ hi) & np.uint64(0xFFFFFFFF)
    h = (x * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return (h >> np.uint64(32 - lg)).astype(np.int64) if lg else np.zeros(len(umi), np.int64)


def refs_for(k, j):
    """Alignment words of the j-th test cell of k buckets: inside (128 k, 256 k], at either end or in between"""
    if k == 1:
        return (256, 131)[j % 2]
    lo, hi = 128 * k + 1, 256 * k
    return (lo, hi, (lo + hi) // 2)[j % 3]


def cells_with_refs(seed, n_refs, usa):
    """A synthetic batch whose cell i carries exactly n_refs[i] alignment words: whole reads of a larger draw, then single-alignment
    reads of the same cell up to the count."""
    s = synth.synth(seed, [int(n) for n in n_refs], num_genes=700, txp_per_gene=3, usa=usa, dup=0.45, zipf=0.6, cross=0.4, umi_err=0.02)
    r0 = np.concatenate(([0], np.cumsum(s.cell_nrec))).astype(np.int64)
    a0 = np.concatenate(([0], np.cumsum(s.na))).astype(np.int64)
    nrec, umi, na, refs = [], [], [], []
    for i, want in enumerate(n_refs):
        lo, hi = r0[i], r0[i + 1]
        cum = np.cumsum(s.na[lo:hi])
        keep = int(np.searchsorted(cum, want, side="right"))   # reads whose words fit
        have = int(cum[keep - 1]) if keep else 0
        ones = lo + np.flatnonzero(s.na[lo:hi] == 1)[: want - have]
        assert len(ones) == want - have
        idx = np.concatenate((np.arange(lo, lo + keep), ones))
        nrec.append(len(idx)); umi.append(s.umi[idx]); na.append(s.na[idx])
        refs.append(np.concatenate((s.refs[a0[lo]:a0[lo + keep]], s.refs[a0[ones]])))   # the kept prefix's words, then the added reads'
        assert int(na[-1].sum()) == want == len(refs[-1])
    s.cell_nrec = np.asarray(nrec, np.int64); s.umi = np.concatenate(umi); s.na = np.concatenate(na); s.refs = np.concatenate(refs)
    return s


_BATCH = {}


def batch(usa):
    if usa not in _BATCH:
        s = cells_with_refs(90 + usa, [refs_for(k, j) for j, k in enumerate(BUCKETS)], usa)
        _BATCH[usa] = (s,) + s.encode()
    return _BATCH[usa]


_WANT = {}


def run(oracle, cfg, t2g, b, off, key=None):
    q = pkg.Quantifier(cfg, t2g)
    try:
        got = q.quant_chunks(b, off)
        st = q.batch_stats()
        st["n_divert"] = q.resolve_divert_count()
    finally:
        q.close()
    if key is None or key not in _WANT:   # (the oracle does not see the library's test hooks: one run per batch and resolution)
        want = oracle.quant(cfg, t2g, b, off)
        if key is not None:
            _WANT[key] = want
    else:
        want = _WANT[key]
    return got, want, st


# slabs every bucket outgrows (the spill and k_fix_slabs), and slabs beyond the 16-bit slab positions (the per-key path)
@pytest.mark.parametrize("env", [{}, {"AFQ_TEST_SLAB_CAP": "8"}, {"AFQ_TEST_SLAB_CAP": "70000"}], ids=["default", "slab-cap-8", "slab-cap-70000"])
@pytest.mark.parametrize("res,usa", [("cr-like", False), ("cr-like", True), ("cr-like-em", False), ("trivial", False)])
def test_cells_on_both_sides_of_the_instance_boundaries(oracle, monkeypatch, env, res, usa):
    """One range with cells of 512, 1024 (the six-workgroup instance's last), 2048 (the other instance) and 4096 buckets (a cursor
    atomic per key), small cells and single-bucket cells: rows equal to the oracle's."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, b, off = batch(usa)
    got, want, st = run(oracle, cfg_for(s, res, small_thresh=0), s.tid_to_gid, b, off, key=(res, usa))
    assert st["n_buckets"] == sum(BUCKETS)
    assert_same_result(got, want, what=f"{res} usa={usa} {env}")
    assert st["n_fallback_cells"] == 0
    assert got.val.sum() > 0


@pytest.mark.parametrize("cap", [None, "512", "4000"])
def test_bucket_positions_beyond_16_bits(oracle, monkeypatch, cap):
    """Three UMIs with 70 000, 40 000 and 30 000 reads in a cell of 1024 buckets: their buckets' cursors pass 65 535 (and 2^16 -
    the tile's keys, where the 16-bit position saturates), so tile after tile finds the slab full at a position that 16 bits no
    longer hold; every such key must still be seen to be past its slab (spilled, the cell placed exactly), whatever the capacity."""
    if cap:
        monkeypatch.setenv("AFQ_TEST_SLAB_CAP", cap)
    s = synth.synth(93, [190000, 3000, 100], num_genes=500, txp_per_gene=2, dup=0.4, zipf=0.5, cross=0.3, p_na=(0.8, 0.15, 0.05))
    umi = s.umi.copy()
    umi[:70000] = 0x123456; umi[70000:110000] = 0x0FEDCB; umi[110000:140000] = 0x00ABCD
    perm = np.random.default_rng(5).permutation(190000)   # the heavy UMIs' reads spread over the cell's tiles
    starts = np.concatenate(([0], np.cumsum(s.na))).astype(np.int64)
    order = np.concatenate((perm, np.arange(190000, len(s.na))))
    s.refs = np.concatenate([s.refs[starts[r]:starts[r + 1]] for r in order])
    s.umi, s.na = umi[order], s.na[order]
    assert 131072 < int(s.na[:190000].sum()) <= 262144
    b, off = s.encode()
    got, want, st = run(oracle, cfg_for(s), s.tid_to_gid, b, off)
    assert st["n_buckets"] == 1024 + 16 + 1
    assert st["n_overflow_buckets"] >= 3
    assert_same_result(got, want, what=f"cap {cap}")


def _one_bucket_cell(n_in_bucket, n_ref=1000, n_multi=0):
    """A cell of four buckets (n_ref single-alignment reads) whose bucket 0 holds exactly n_in_bucket keys - distinct UMIs, but
    n_multi UMIs seen with five genes (two of their keys are parked) - and whose other buckets share the rest evenly.  The UMIs
    are picked by their bucket on the host."""
    cand = np.unique(np.arange(1000, 1000 + 64 * n_ref, dtype=np.uint64) * np.uint64(7919) % np.uint64(1 << 24))
    bk = bucket_of(cand, 2)
    rest = n_ref - n_in_bucket
    share = [rest // 3 + (1 if j < rest % 3 else 0) for j in range(3)]
    assert max(share) < HT_KEYS
    own = cand[bk == 0][:n_in_bucket - 4 * n_multi]
    reads = [(int(u), [int(u) % 50]) for u in own] + [(int(u), [(int(u) + 7 * g) % 50]) for u in own[:n_multi] for g in range(1, 5)]
    reads += [(int(u), [int(u) % 50]) for j in range(3) for u in cand[bk == j + 1][:share[j]]]
    assert len(reads) == n_ref
    rng = np.random.default_rng(n_in_bucket)
    return [reads[i] for i in rng.permutation(n_ref)]


@pytest.mark.parametrize("n_multi", [0, 12])
@pytest.mark.parametrize("usa", [False, True])
def test_bucket_at_the_table_limit(oracle, monkeypatch, usa, n_multi):
    """A bucket one key under, at, and one key over kHtKeys: the first two are the table's - all keys distinct UMIs, the table at
    its highest load (256 UMIs in 288 slots), with and without parked keys - the third is diverted to the sort path: n_divert moves
    by exactly that one bucket, and each resolves to the oracle's rows."""
    monkeypatch.delenv("AFQ_TEST_RESOLVE_DIVERT", raising=False)
    n_txp = 100
    num_genes = n_txp // 2 if usa else n_txp
    t2g = (np.arange(n_txp, dtype=np.uint32) // 2) if usa else np.arange(n_txp, dtype=np.uint32)
    cfg = pkg.WorkerConfig.for_resolution("cr-like", usa_mode=usa, num_genes=num_genes, num_rows=(num_genes // 2) * 3 if usa else num_genes,
                                          small_thresh=0)
    for n, over in ((HT_KEYS - 1, 0), (HT_KEYS, 0), (HT_KEYS + 1, 1), (HT_KEYS + 40, 1)):
        b, off = rad.encode_cells([(7, _one_bucket_cell(n, n_multi=n_multi))], 4, 4)
        got, want, st = run(oracle, cfg, t2g, b, off)
        assert_same_result(got, want, what=f"bucket of {n} keys")
        assert st["n_buckets"] == 4
        assert st["n_divert"] == over, (n, st)
    # three cells, one bucket over the limit in two of them: two diverted buckets
    cells = [(7, _one_bucket_cell(HT_KEYS + 1, n_multi=n_multi)), (8, _one_bucket_cell(HT_KEYS + 2, n_multi=n_multi)), (9, _one_bucket_cell(HT_KEYS, n_multi=n_multi))]
    b, off = rad.encode_cells(cells, 4, 4)
    got, want, st = run(oracle, cfg, t2g, b, off)
    assert_same_result(got, want)
    assert st["n_divert"] == 2, st
