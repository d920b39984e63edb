"""GPU parity tests (bit-exact against the oracle) of the scattering record decoder's wave-uniform state and of the buckets its
tail gives the staged keys.  A workgroup takes a tile of 16 one-KiB slabs of one cell, four per wave, and keeps the tile's state (slab
range, cell, cell metadata) in scalar registers and the cell's output addresses in vector registers: the cases give waves nothing, one
and all of their slabs, next to workgroups of other cells.  The tail ranks and places every staged key by bucket_of() of its UMI; the
UMI cases hold the bit patterns at which a shortcut for that - a bucket number carried in a key's unused top bits was built and measured
in round 14, and not kept - would go wrong: a stray top bit reads as a UMI beyond 32 bits, which the rows or the divert counters
show."""
import numpy as np
import pytest

from test_gpu_decode_bins import cells_with_refs, refs_for
from test_gpu_decode_scatter import STAGE_KEYS, TILE_SLABS, max_tile_keys
from util import assert_same_result, cfg_for, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
synth = pkg.synth

SLAB = 1024
assert TILE_SLABS == 16
# (KiB, single-bucket): multi-bucket cells whose last tile gives its waves 4+1+0+0, 4+4+4+3 and 4+4+4+4 slabs, a one-slab tile behind
# one and behind two whole tiles, four whole tiles; between them single-bucket cells of one and of three slabs, so that neighbouring
# workgroups belong to different cells
SHAPE = [(5, False), (1, True), (15, False), (3, True), (16, False), (1, True), (17, False), (3, True), (33, False), (1, True),
         (64, False), (3, True)]


@pytest.fixture(autouse=True)
def records_decoder(monkeypatch):
    """The lane-per-record (scattering) decoder whatever the batch's record lengths."""
    monkeypatch.setenv("AFQ_TEST_DECODE", "recs")


def cut_to_slabs(s, shape, hw):
    """Cell i of the pool cut to shape[i] = (KiB, single): the longest prefix of its reads (of its single-alignment reads, for a
    single-bucket cell) whose chunk - 8 header bytes and 4 * (hw + na) per record - ends inside the KiB-th slab."""
    r0 = np.concatenate(([0], np.cumsum(s.cell_nrec))).astype(np.int64)
    a0 = np.concatenate(([0], np.cumsum(s.na))).astype(np.int64)
    nrec, umi, na, refs = [], [], [], []
    for i, (kib, single) in enumerate(shape):
        idx = np.arange(r0[i], r0[i + 1])
        if single:
            idx = idx[s.na[idx] == 1]
        size = 8 + np.cumsum(4 * (hw + s.na[idx]))
        keep = int(np.searchsorted(size, kib * SLAB, side="right"))
        assert (kib - 1) * SLAB < size[keep - 1] <= kib * SLAB, (i, kib, len(idx))
        idx = idx[:keep]
        n_ref = int(s.na[idx].sum())
        assert (n_ref <= 256) if single else (n_ref > 256), (i, kib, n_ref)   # (one bucket per 256 alignment words)
        nrec.append(keep); umi.append(s.umi[idx]); na.append(s.na[idx])
        refs.append(np.concatenate([s.refs[a0[r]:a0[r + 1]] for r in idx]))
    s.cell_nrec = np.asarray(nrec, np.int64); s.umi = np.concatenate(umi); s.na = np.concatenate(na); s.refs = np.concatenate(refs)
    return s


_SLAB_BATCH = {}


def slab_batch(usa, bw, uw, wide_umis=False):
    """The SHAPE batch for one field layout; barcodes of 8 bytes use their high word, UMIs of 8 bytes stay below 2^32 unless
    wide_umis (then every molecule's UMI has bits 32..43 set from its low word)."""
    key = (usa, bw, uw, wide_umis)
    if key not in _SLAB_BATCH:
        hw = 1 + bw // 4 + uw // 4
        pool = [(kib * SLAB) // (4 * (hw + 1)) * (3 if single else 1) + 60 for kib, single in SHAPE]
        s = synth.synth(140 + usa, pool, num_genes=400, txp_per_gene=3, usa=usa, dup=0.45, p_na=(0.5, 0.3, 0.2), cross=0.4, umi_err=0.02)
        s = cut_to_slabs(s, SHAPE, hw)
        if bw == 8:
            s.cell_bc = s.cell_bc | ((s.cell_bc * np.uint64(40503) & np.uint64(0xFFFFFFFF)) << np.uint64(32))
        if wide_umis:
            assert uw == 8
            s.umi = s.umi | (((s.umi * np.uint64(2654435761)) >> np.uint64(9)) & np.uint64(0xFFF)) << np.uint64(32)
            assert int(s.umi.max()) >> 32 and int(s.umi.max()) < 1 << 44
        b, off = rad.encode_cells_np(s.cell_nrec, s.cell_bc, s.umi, s.na, s.refs, bc_bytes=bw, umi_bytes=uw)
        sizes = np.diff(np.concatenate((off, [len(b)])).astype(np.int64))
        assert [int(-(-n // SLAB)) for n in sizes] == [kib for kib, _ in SHAPE]
        _SLAB_BATCH[key] = (s, b, off)
    return _SLAB_BATCH[key]


_WANT = {}


def run(oracle, cfg, t2g, b, off, key):
    """Device rows, the oracle's (one oracle run per batch and resolution: it does not see the library's test hooks), the counters."""
    q = pkg.Quantifier(cfg, t2g)
    try:
        got = q.quant_chunks(b, off)
        st = q.batch_stats()
        st["n_divert"] = q.resolve_divert_count()
    finally:
        q.close()
    if key not in _WANT:
        _WANT[key] = oracle.quant(cfg, t2g, b, off)
    return got, _WANT[key], st


@pytest.mark.parametrize("bw,uw", [(4, 4), (4, 8), (8, 4)])
@pytest.mark.parametrize("res,usa", [("cr-like", False), ("cr-like", True), ("trivial", False)])
def test_waves_with_nothing_one_and_all_of_their_slabs(oracle, res, usa, bw, uw):
    """Tiles whose last wave has 0, 1 or 3 slabs, whole tiles and one-slab last tiles, between workgroups of single-bucket cells."""
    s, b, off = slab_batch(usa, bw, uw)
    got, want, st = run(oracle, cfg_for(s, res, bc_bytes=bw, umi_bytes=uw), s.tid_to_gid, b, off, key=("slabs", res, usa, bw, uw))
    assert_same_result(got, want, what=f"{res} usa={usa} {bw}/{uw}")
    assert st["n_fallback_cells"] == 0, st
    assert got.val.sum() > 0


@pytest.mark.parametrize("res,usa", [("cr-like", False), ("cr-like", True), ("trivial", False)])
def test_eight_byte_umis_above_32_bits(oracle, res, usa):
    """The same tiles with 8-byte UMIs that use bits 32..43: their keys' top bits are the UMI's."""
    s, b, off = slab_batch(usa, 4, 8, wide_umis=True)
    got, want, st = run(oracle, cfg_for(s, res, bc_bytes=4, umi_bytes=8), s.tid_to_gid, b, off, key=("wide", res, usa))
    assert_same_result(got, want, what=f"{res} usa={usa} wide UMIs")
    assert st["n_fallback_cells"] == 0, st


# cells of 2, 4 and 256 buckets, of 2048 (the other instance) and a giant one beyond it (a cursor atomic per key)
UMI_BUCKETS = [4096, 2048, 256, 4, 2]
# what the same batch counts with the library of the parent commit (AFQ_LIB_PATH, the run recorded in profiles/r14_bench.txt): a key
# that reaches keys1 with bits above its UMI can only add to them
PARENT_DIVERT, PARENT_OVERFLOW = 270, 0
_UMI_BATCH = []


def umi_batch():
    """Every cell's UMIs spread over all 32 bits (an odd multiple: one to one, so reads of one molecule keep one UMI), and in every
    cell reads with the UMIs 0, 0xFFFFFFFF and 0x80000000, pairs that differ only in bits 20..31, and a run of consecutive values
    across 2^31."""
    if not _UMI_BATCH:
        s = cells_with_refs(141, [refs_for(k, j) for j, k in enumerate(UMI_BUCKETS)], False)
        s.umi = (s.umi * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
        r0 = np.concatenate(([0], np.cumsum(s.cell_nrec))).astype(np.int64)
        low = 0x5A5A5
        special = [0, 0xFFFFFFFF, 0x80000000, 0, 0xFFFFFFFF, 0x80000000]
        special += [low | (k << 20) for k in (0, 1, 2, 0x800, 0xFFF, 0x7FF, 0x555, 1)]
        special += [0x7FFFFFF0 + k for k in range(32)]
        for c in range(len(s.cell_nrec)):
            n = min(len(special), int(s.cell_nrec[c]))
            at = r0[c] + np.linspace(0, int(s.cell_nrec[c]) - 1, n).astype(np.int64)   # spread over the cell's tiles
            s.umi[at] = np.asarray(special[:n], np.uint64)
        _UMI_BATCH.append((s,) + s.encode())
    return _UMI_BATCH[0]


def test_umi_bit_patterns_in_every_bucket_count(oracle):
    s, b, off = umi_batch()
    got, want, st = run(oracle, cfg_for(s, "cr-like", small_thresh=0), s.tid_to_gid, b, off, key="umis")
    print("counters:", st)
    assert st["n_buckets"] == sum(UMI_BUCKETS)
    assert_same_result(got, want)
    assert st["n_fallback_cells"] == 0
    assert st["n_divert"] <= PARENT_DIVERT and st["n_overflow_buckets"] <= PARENT_OVERFLOW, st


_EXIT_BATCH = []


def exit_batch():
    if not _EXIT_BATCH:
        s = synth.synth(142, [30000, 9000, 2500, 600, 150, 5], num_genes=600, txp_per_gene=2, p_na=(0.0, 0.0, 1.0), cross=1.0, dup=0.4,
                        umi_err=0.02)
        s.umi = (s.umi * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
        assert max_tile_keys(s) > STAGE_KEYS   # (a tile holds more keys than the stage: the direct exit is taken)
        _EXIT_BATCH.append((s,) + s.encode())
    return _EXIT_BATCH[0]


@pytest.mark.parametrize("cap", [None, "200", "8"])
def test_staged_and_direct_keys_on_every_exit(oracle, monkeypatch, cap):
    """Records of three genes each: a 16-slab tile makes about 2048 keys, more than the 1536 the stage holds, so the first go out
    bucket-major from the stage, the rest directly; with small slabs both kinds spill into keys0, and the
    cells are placed exactly by k_fix_slabs or decoded again."""
    if cap:
        monkeypatch.setenv("AFQ_TEST_SLAB_CAP", cap)
    s, b, off = exit_batch()
    got, want, st = run(oracle, cfg_for(s, "cr-like"), s.tid_to_gid, b, off, key="exit")
    assert_same_result(got, want, what=f"cap {cap}")
    assert st["n_fallback_cells"] == 0
