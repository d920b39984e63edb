"""GPU parity tests (bit-exact against the oracle) of the scattering decoder's span load (csrc/afq_decode.hip, k_decode_recs with
BINS != 0; csrc/afq_decode_span.h): a wave requests every row of its four slabs and their halo - 17 rows of 64 dwords - in front
of its slab loop, all waves but the one that holds the chunk's end without a guard.  The shapes are the smallest at which that can
go wrong: chunks that end on either side of a row, a slab, a halo and a span, the same at the end of the device buffer, records
that lie across two waves' spans and two tiles, and a cell that is decoded twice."""
import numpy as np
import pytest

from test_gpu_decode_bins import cells_with_refs, run
from util import assert_same_result, cfg_for, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad

SPAN = 1024    # dwords of a wave's four slabs
TILE = 4096    # dwords of a workgroup's four spans
N_TXP = 120
T2G = (np.arange(N_TXP, dtype=np.uint32) // 2).astype(np.uint32)
KS = (0, 1, 3, 4, 5, 16, 17)
QS = (63, 64, 65, 255, 256, 257, 319, 320, 321, 1023, 0, 1)   # both sides of a row, a slab, the halo and the span
BUCKET_TARGET = 256   # alignment words a bucket is planned for: a cell of n_ref words has 2^lg buckets, 256 << lg >= n_ref


@pytest.fixture(autouse=True)
def records_decoder(monkeypatch):
    """The lane-per-record (scattering) decoder whatever the batch's record lengths."""
    monkeypatch.setenv("AFQ_TEST_DECODE", "recs")


def hw_of(width):
    return 1 + 2 * (width // 4)


def fill(n, hw):
    """Alignment counts (ones and twos) of records that take exactly n dwords, as few twos as do it."""
    for two in range(hw + 2):
        rest = n - (hw + 2) * two
        if rest >= 0 and rest % (hw + 1) == 0:
            return [1] * (rest // (hw + 1)) + [2] * two
    raise AssertionError(f"no records of one and two alignments take {n} dwords")


def na_for_length(length, hw, rng):
    """Records of a chunk of exactly `length` dwords (two of them the chunk's header)."""
    return rng.permutation(np.array(fill(length - 2, hw), np.int64))


def na_for_starts(starts, hw, rng, long_at=None, long_na=70, n_after=40):
    """Records such that one starts at every dword of `starts` (ascending, from the chunk's start); the one at long_at has long_na
    alignments.  n_after records of one to three alignments follow."""
    na, at = [], 2
    for s in starts:
        na += rng.permutation(np.array(fill(s - at, hw), np.int64)).tolist()
        at = s
        if s == long_at:
            na.append(long_na)
            at += hw + long_na
    na += rng.integers(1, 4, n_after).tolist()
    return np.array(na, np.int64)


class Batch:
    """Cells as the arrays rad.encode_cells_np takes."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.cell_nrec, self.cell_bc, self.umi, self.na, self.refs = [], [], [], [], []

    def add(self, bc, na, umi_lo=1000):
        na = np.asarray(na, np.int64)
        n = len(na)
        umi = umi_lo + (self.rng.integers(1, max(4, n // 2), n) * 7919) % ((1 << 24) - umi_lo)   # (about two reads a UMI; never a barcode)
        first = np.concatenate(([0], np.cumsum(na)[:-1]))
        refs = np.zeros(int(na.sum()), np.int64)
        for r in np.flatnonzero(na > 2):   # (few)
            refs[first[r]:first[r] + na[r]] = np.sort(self.rng.choice(N_TXP, int(na[r]), replace=False))
        short = np.flatnonzero(na <= 2)
        a = self.rng.integers(0, N_TXP - 1, len(short))
        refs[first[short]] = a
        two = na[short] == 2
        refs[first[short][two] + 1] = a[two] + 1 + self.rng.integers(0, N_TXP - 1 - a[two])   # (ascending, distinct)
        self.cell_nrec.append(n); self.cell_bc.append(bc); self.umi.append(umi); self.na.append(na); self.refs.append(refs)
        return self

    def words(self, hw):
        """dwords of every cell's chunk"""
        return [2 + int((hw + na).sum()) for na in self.na]

    def n_ref(self):
        return [int(na.sum()) for na in self.na]

    def encode(self, width):
        b, off = rad.encode_cells_np(np.array(self.cell_nrec), np.array(self.cell_bc, np.uint64), np.concatenate(self.umi), np.concatenate(self.na),
                                     np.concatenate(self.refs), bc_bytes=width, umi_bytes=width)
        ends = np.concatenate((off[1:], [len(b)])).astype(np.int64)
        assert ((ends - off.astype(np.int64)) // 4).tolist() == self.words(hw_of(width))   # (the chunks are as long as the test wants them)
        return b, off


def lg_buckets(n_ref):
    lg = 0
    while (BUCKET_TARGET << lg) < n_ref:
        lg += 1
    return lg


def cfg(res, width, small_thresh=None):
    kw = {} if small_thresh is None else {"small_thresh": small_thresh}
    return pkg.WorkerConfig.for_resolution(res, usa_mode=False, num_genes=N_TXP // 2, num_rows=N_TXP // 2, bc_bytes=width, umi_bytes=width, **kw)


def check(oracle, batch, res, width, small_thresh=None, what="", key=None, fallback=0):
    b, off = batch if isinstance(batch, tuple) else batch.encode(width)
    got, want, st = run(oracle, cfg(res, width, small_thresh), T2G, b, off, key=key)
    assert_same_result(got, want, what=f"{what} {res} width {width} small_thresh {small_thresh}")
    assert st["n_fallback_cells"] == fallback, st
    assert got.val.sum() > 0
    return st


# ------------------------------------------------------------------------------------------------------------------ chunk ends
LENGTHS = [(k, q) for k in KS for q in QS if k * SPAN + q >= 6]   # (a chunk below one record is none)
_ENDS = {}


def chunk_ends(width):
    """One cell per (k, q): a chunk of k * 1024 + q dwords.  Last waves of four, three, two, one and no slabs, last tiles of one to
    four waves, a cell of exactly one tile (k = 4, q = 0) and of exactly four (k = 16, q = 0)."""
    if width not in _ENDS:
        hw = hw_of(width)
        bt = Batch(17 + width)
        for j, (k, q) in enumerate(LENGTHS):
            bt.add(0x1234567 + 11 * j, na_for_length(k * SPAN + q, hw, bt.rng))
        assert bt.words(hw) == [k * SPAN + q for k, q in LENGTHS]
        _ENDS[width] = (bt, bt.encode(width))
    return _ENDS[width]


@pytest.mark.parametrize("res,width,small_thresh", [("cr-like", 4, None), ("cr-like", 8, None), ("trivial", 4, None), ("trivial", 8, None),
                                                    ("cr-like", 8, 0), ("trivial", 4, 0)])
def test_chunks_ending_at_every_phase_of_a_span(oracle, res, width, small_thresh):
    """Cells whose chunks are k * 1024 + q dwords long, k in KS and q in QS, in one batch: rows equal to the oracle's, no cell taken
    by the fall-back decode.  The cells from k = 3 on are multi-bucket (their keys go through the staged tail), the cells of k = 0
    single-bucket (keys0): both paths share the loader."""
    bt, enc = chunk_ends(width)
    lgs = [lg_buckets(n) for n in bt.n_ref()]
    for (k, q), lg in zip(LENGTHS, lgs):
        assert (lg > 0) if k >= 3 else (lg == 0) if k == 0 else True, (k, q, lg)
    st = check(oracle, enc, res, width, small_thresh, what="chunk ends", key=("span-ends", res, width, small_thresh))
    assert st["n_buckets"] == sum(1 << lg for lg in lgs)


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("q", QS)
def test_last_chunk_of_the_buffer(oracle, q, width):
    """The chunk that ends the device buffer ends at every phase q of a span: a short cell, a cell of two tiles and, last, a cell of
    k * 1024 + q dwords with k going through 1, 3, 4 and 5 (last waves of every slab count)."""
    hw = hw_of(width)
    k = (1, 3, 4, 5)[QS.index(q) % 4]
    bt = Batch(300 + q + width)
    for j, length in enumerate((200, 5 * SPAN + 77, k * SPAN + q)):
        bt.add(0x2345671 + 13 * j, na_for_length(length, hw, bt.rng))
    assert bt.words(hw)[-1] == k * SPAN + q
    check(oracle, bt, "cr-like", width, 0, what=f"last chunk q {q}")


# ----------------------------------------------------------------------------------------------------------------------- seams
SEAM_STARTS = (SPAN - 4, 2 * SPAN - 3, 3 * SPAN - 2, TILE - 4, 5 * SPAN - 1, 6 * SPAN - 10, 2 * TILE - 3, 3 * TILE - 2, 4 * TILE - 1)
LONG_AT = 6 * SPAN - 10


@pytest.mark.parametrize("res", ["cr-like", "trivial"])
@pytest.mark.parametrize("width", [4, 8])
def test_records_across_span_and_tile_seams(oracle, res, width):
    """Records that start at span positions 1020 ... 1023 and tile positions 4092 ... 4095 - header, UMI and alignments in the next
    wave's span, the next workgroup's tile - and one record of 70 alignments that starts 10 dwords before a span's end: it reaches
    past the staged halo, so its successor (and at 8-byte fields its last alignments) is read from the chunk itself."""
    hw = hw_of(width)
    bt = Batch(41 + width)
    na = na_for_starts(SEAM_STARTS, hw, bt.rng, long_at=LONG_AT)
    bt.add(0x1234567, na).add(0x1234599, na_for_length(300, hw, bt.rng))
    first = 2 + np.concatenate(([0], np.cumsum(hw + na)[:-1]))
    assert set(SEAM_STARTS) <= set(first.tolist()) and na[first.tolist().index(LONG_AT)] == 70
    assert {s % SPAN for s in SEAM_STARTS} >= {1020, 1021, 1022, 1023} and {s % TILE for s in SEAM_STARTS} >= {4092, 4093, 4094, 4095}
    st = check(oracle, bt, res, width, 0, what="seams")
    assert st["n_buckets"] > 2


# --------------------------------------------------------------------------------------------------------------- a failed proof
@pytest.mark.parametrize("width", [4, 8])
def test_cell_decoded_twice(oracle, width):
    """A cell whose second record's alignment count is falsified: it claims the whole third record as alignments of its own (every
    word of that record is a valid reference id, so the sequential parse stands and finds one record fewer), while the walk-free
    decoder still sees the third record's barcode.  The cell's proof fails and it is decoded again; it is the only one, and the rows
    are the oracle's."""
    hw = hw_of(width)
    s = cells_with_refs(77, [3000, 200], False)
    bc = 37   # (a reference id: the swallowed barcode word is an alignment like any other; UMIs start at 1000, reference words carry bit 31)
    assert bc not in s.cell_bc.tolist()
    bt = Batch(5 + width)
    na = np.sort(na_for_length(2 * SPAN + 300, hw, bt.rng))   # (the records of one alignment first)
    bt.add(bc, na)
    bt.umi[0][2] = 50   # the third record's UMI: a reference id as well, and not the barcode
    cell_nrec = np.concatenate((s.cell_nrec, [len(na)]))
    b, off = rad.encode_cells_np(cell_nrec, np.concatenate((s.cell_bc, [bc])).astype(np.uint64), np.concatenate((s.umi, bt.umi[0])),
                                 np.concatenate((s.na, na)), np.concatenate((s.refs, bt.refs[0])), bc_bytes=width, umi_bytes=width)
    w = np.frombuffer(bytes(b), np.uint32).copy()
    c0 = int(off[-1]) // 4
    assert w[c0 + 1] == len(na) and w[c0 + 2] == 1 and w[c0 + 2 + hw + 1] == 1 and w[c0 + 3] == bc
    w[c0 + 2 + hw + 1] = 1 + hw + 1   # the second record's count: its own alignment and the third record's hw + 1 dwords
    w[c0 + 1] = len(na) - 1           # (what the sequential parse finds)
    cfg_ = cfg_for(s, "cr-like", small_thresh=0, bc_bytes=width, umi_bytes=width)
    got, want, st = run(oracle, cfg_, s.tid_to_gid, w.view(np.uint8), off)
    assert_same_result(got, want, what=f"falsified count, width {width}")
    assert st["n_fallback_cells"] == 1, st
    assert got.val.sum() > 0
