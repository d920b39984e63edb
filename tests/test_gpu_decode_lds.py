"""GPU parity tests (bit-exact against the oracle) of the scattering decoder's LDS layout (csrc/afq_decode.hip, k_decode_recs): a
slab's candidate list keeps a record's staged position (0 .. 255) in one byte, a slab that follows one of its own cell takes its
first row from the halo the slab before left staged, and the tail's per-bucket words lie on the waves' slab stages - 2 * 1024 +
2 * 1024 bytes of them for the instance of up to 1024 buckets, 2 * 2048 for the one of up to 2048."""
import numpy as np
import pytest

from test_gpu_decode_bins import bucket_of, cells_with_refs, run
from util import assert_same_result, cfg_for, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad

SLAB = 256   # dwords of a slab (kSlabWords); a record's staged position is its first dword's index in its slab
POSITIONS = (2, 127, 128, 254, 255)   # the first record of a chunk, both sides of a signed byte's limit, the slab's last two words
# dwords (from the chunk start) records are made to start at: every position above in at least one slab, gaps of 125 and more
STARTS = (2, 127, 254, SLAB + 128, SLAB + 255, 2 * SLAB + 127, 2 * SLAB + 255, 3 * SLAB + 128, 4 * SLAB + 2, 4 * SLAB + 254,
          5 * SLAB + 255, 7 * SLAB + 128, 8 * SLAB + 127, 9 * SLAB + 254)


@pytest.fixture(autouse=True)
def records_decoder(monkeypatch):
    """The lane-per-record (scattering) decoder whatever the batch's record lengths."""
    monkeypatch.setenv("AFQ_TEST_DECODE", "recs")


def reads_starting_at(starts, hw, n_after, n_txp, rng):
    """Reads of one or two alignments (hw + 1 or hw + 2 dwords) sized so that a record starts at every dword of `starts` (the first
    at dword 2, behind the chunk header), then n_after more of one to three alignments."""
    na = []
    at = 2
    for s in starts[1:]:
        gap = s - at
        two = gap % (hw + 1)   # records of hw + 2 dwords: (hw + 2) two = two mod (hw + 1)
        one = (gap - (hw + 2) * two) // (hw + 1)
        assert one >= 0 and one * (hw + 1) + two * (hw + 2) == gap
        lens = np.array([1] * one + [2] * two)
        na += rng.permutation(lens).tolist()
        at = s
    na += rng.integers(1, 4, n_after).tolist()
    umis = rng.integers(1, max(4, len(na) // 2), len(na)) * 7919 % (1 << 24)   # (about two reads a UMI)
    return [(int(u), rng.integers(0, n_txp, n).tolist()) for u, n in zip(umis, na)]


@pytest.mark.parametrize("res", ["cr-like", "trivial"])
@pytest.mark.parametrize("width", [4, 8])
def test_record_starts_at_slab_boundaries(oracle, res, width):
    """One cell whose records start at staged positions 2, 127, 128, 254 and 255 of a slab (a list entry that is signed, or cut
    below eight bits, reads the last three from a wrong place: the cell's proof fails), beside a short cell that ends with the last
    of those records.  Rows equal to the oracle's, and no cell taken by the fall-back decode."""
    hw = 1 + 2 * (width // 4)
    n_txp = 120
    t2g = (np.arange(n_txp, dtype=np.uint32) // 2).astype(np.uint32)
    rng = np.random.default_rng(7 + width)
    cells = [(0x1234567 + 11 * j, reads_starting_at(STARTS, hw, n_after, n_txp, rng)) for j, n_after in enumerate((6000, 1))]
    for _, reads in cells:   # (the input does have its records where the test wants them)
        first = 2 + np.concatenate(([0], np.cumsum([hw + len(r[1]) for r in reads])[:-1]))
        assert set(STARTS) <= set(first.tolist())
    assert {s % SLAB for s in STARTS} == set(POSITIONS)
    b, off = rad.encode_cells(cells, width, width)
    cfg = pkg.WorkerConfig.for_resolution(res, usa_mode=False, num_genes=n_txp // 2, num_rows=n_txp // 2, small_thresh=0,
                                          bc_bytes=width, umi_bytes=width)
    got, want, st = run(oracle, cfg, t2g, b, off)
    assert_same_result(got, want, what=f"{res} width {width}")
    assert st["n_fallback_cells"] == 0, st
    assert st["n_buckets"] > 2   # (multi-bucket cells: the scattering tail runs)
    assert got.val.sum() > 0


BUCKETS = [1, 1024, 4096, 2048]   # the largest cell of either instance, beside a single-bucket cell and a cell beyond both
_BATCH = {}


def batch(usa):
    if usa not in _BATCH:
        # 256 k alignment words make k buckets at the most; the 4096-bucket cell has the fewest that make 4096
        s = cells_with_refs(95 + usa, [200 if k == 1 else 128 * k + 1 if k == 4096 else 256 * k for k in BUCKETS], usa)
        _BATCH[usa] = (s,) + s.encode()
    return _BATCH[usa]


@pytest.mark.parametrize("env", [{}, {"AFQ_TEST_SLAB_CAP": "8"}], ids=["default", "slab-cap-8"])
@pytest.mark.parametrize("res,usa", [("cr-like", False), ("cr-like", True), ("trivial", False)])
def test_every_bucket_word_in_use(oracle, monkeypatch, env, res, usa):
    """A cell of exactly 1024 buckets and one of exactly 2048, each with keys in every bucket - the first and the last among them
    - so that every per-bucket word laid over the slab stages is counted in, scanned and read back; in one range with a
    single-bucket cell (which leaves the tail before it touches them) and a cell of 4096 buckets (a cursor atomic per key)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, b, off = batch(usa)
    r0 = np.concatenate(([0], np.cumsum(s.cell_nrec))).astype(np.int64)
    for j, k in enumerate(BUCKETS):
        if k in (1024, 2048):
            used = np.unique(bucket_of(s.umi[r0[j]:r0[j + 1]], k.bit_length() - 1))
            assert len(used) == k and used[0] == 0 and used[-1] == k - 1
    got, want, st = run(oracle, cfg_for(s, res, small_thresh=0), s.tid_to_gid, b, off, key=("lds", res, usa))
    assert st["n_buckets"] == sum(BUCKETS)
    assert_same_result(got, want, what=f"{res} usa={usa} {env}")
    assert st["n_fallback_cells"] == 0
    assert got.val.sum() > 0
