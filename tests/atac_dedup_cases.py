"""Hand-built inputs at the limits of `atac deduplicate` (k_atac_parse, k_atac_dedup64, k_atac_dedup, k_atac_compact and the two host
routes of afq_atac_dedup_rad), shared by tests/test_atac_dedup_judge_cpu.py (the oracle before the judge, builders and witnesses, no
device) and tests/test_gpu_atac_dedup_judge.py (the device before the judge).

A case is a dict: "cells" - [(barcode, records)], a record the list of its (ref, map_type, start, frag_len) alignments, what the
judge is given -, "data" / "off" (the chunk bytes and offsets the device and the oracle are given), "bc_bytes", "wide" (a reference
id of 65536 and more is present: the batch is redone by k_atac_dedup) and "n_fallback" (cells built so that the walk-free proof
fails, and chunks of zero records, which it does not cover).  The JUDGE of a result is tests/atac_dedup_judge.py on "cells"; tests/test_atac_dedup_judge_cpu.py reads "data" back with
the judge's own byte reader and finds "cells", so the bytes say what the structures say.  Everything below that restates a kernel -
`false_starts` and `walked_cells` (the candidate rule of k_atac_parse), `kept_in_one_bitmap_word` (how it files the candidates), `run_layout` (where
runs lie in the sorted order the dedup kernels sweep), `ref_runs` (the compaction's run list) - is a WITNESS: it shows that a
builder's input reaches the edge it names, and never decides whether a result is right.

Sizes are the 2^k - 1, 2^k, 2^k + 1 the issue of this suite names (a sweep of 2^10 positions, a sort tile of 2^14 keys, a count of
2^16, byte groups of 2^8, 2^9, 2^11); no kernel constant is imported.  Every batch has at least eight cells, so that
AFQ_TEST_ATAC_PIPE_BYTES=1 sends it through the eight-range pipeline."""
import numpy as np

import atac_dedup_judge as J
from util import pkg

rad = pkg.rad


# ---------------------------------------------------------------------------------------------------------------- encoders
def _py_cell(bc, records):
    return {"bc": int(bc), "records": records}


def _run_cell(bc, frags, mult, seed, ty=4):
    """A cell of single-alignment records: fragment frags[i] mult[i] times, in a shuffled order.  Carries its numpy columns (the
    large shapes are encoded with a structured dtype); the records of one fragment are one shared list object."""
    idx = np.repeat(np.arange(len(frags)), mult)
    idx = idx[np.random.default_rng(seed).permutation(len(idx))]
    table = np.asarray(frags, np.uint64).reshape(-1, 3)
    recs = [[(int(r), ty, int(s), int(f))] for r, s, f in frags]
    cols = (table[idx, 0].astype(np.uint32), np.full(len(idx), ty, np.uint8), table[idx, 1].astype(np.uint32), table[idx, 2].astype(np.uint16))
    return {"bc": int(bc), "records": [recs[i] for i in idx.tolist()], "cols": cols}


def encode_na1(bc, ref, ty, start, fl, bc_bytes):
    """one chunk of single-alignment records, encoded with numpy"""
    dt = np.dtype([("na", "<u4"), ("bc", "<u%d" % bc_bytes), ("ref", "<u4"), ("ty", "u1"), ("start", "<u4"), ("fl", "<u2")])
    assert dt.itemsize == 15 + bc_bytes
    r = np.zeros(len(ref), dt)
    r["na"], r["bc"], r["ref"], r["ty"], r["start"], r["fl"] = 1, bc, ref, ty, start, fl
    body = r.tobytes()
    return (len(body) + 8).to_bytes(4, "little") + len(r).to_bytes(4, "little") + body


def _case(cells, bc_bytes, wide=False, n_fallback=0, pad=0, min_cells=8, **more):
    out, offs = bytearray(pad), []
    for c in cells:
        offs.append(len(out))
        if "cols" in c:
            out += encode_na1(c["bc"], *c["cols"], bc_bytes)
        else:
            out += rad.encode_atac_cells([(c["bc"], c["records"])], bc_bytes=bc_bytes)[0]
    assert len(cells) >= min_cells
    case = {"cells": [(c["bc"], c["records"]) for c in cells], "data": np.frombuffer(bytes(out), np.uint8).copy(), "off": np.asarray(offs, np.uint64),
            "bc_bytes": bc_bytes, "wide": wide, "n_fallback": n_fallback}
    case.update(more)
    return case


def _bc(i, bc_bytes):
    """barcodes whose bytes are all non-zero and unlike the small field values of the cases (no accidental record start)"""
    return (0xA7C3E5F1B2D4E6 * 256 + 0x81 + i) & ((1 << (8 * bc_bytes)) - 1)


def _fillers(k, bc_bytes, first=100):
    """k small ordinary cells: a duplicate, a long fragment, a record without alignments, one with two"""
    out = []
    for i in range(k):
        recs = [[(i % 3, 4, 10 + i, 100)], [(i % 3, 4, 10 + i, 100)], [(2, 4, 77, 2000 + i)], [], [(0, 4, 1, 30), (1, 4, 2, 30)]][: 1 + (i + 2) % 5]
        out.append(_py_cell(_bc(first + i, bc_bytes), recs))
    return out


# --------------------------------------------------------------------------------------------------------------- comparison
_judged = {}


def judged(case):
    """the judge's answer for a case, computed once"""
    k = id(case)
    if k not in _judged:
        _judged[k] = (case, J.judge_cells([recs for _, recs in case["cells"]]))
    return _judged[k][1]


TALLIES = ("n_records", "n_multimapped", "n_not_mapped_pair", "n_deduplicated", "n_long_fragments")


def same_as_judge(got, case, what="", rows_only=False):
    """(cell_ptr, bc, ref, start, frag_len, count, stats) of the device or the oracle against the judge, cell by cell; every cell
    is judged.  rows_only: (cell_ptr, ref, start, frag_len, count) of the column-level entry points."""
    want = judged(case)
    if rows_only:
        ptr, ref, start, fl, cnt = got
        bc = st = None
    else:
        ptr, bc, ref, start, fl, cnt, st = got
    assert (ref.dtype, start.dtype, fl.dtype, cnt.dtype) == (np.uint32, np.uint32, np.uint16, np.uint16), what
    ptr = [int(x) for x in ptr]
    assert len(ptr) == len(case["cells"]) + 1 and len(ref) == len(start) == len(fl) == len(cnt) == ptr[-1], (what, ptr[-1], len(ref))
    rows = list(zip(ref.tolist(), start.tolist(), fl.tolist(), cnt.tolist()))
    n_judged = 0
    for i, (cell_bc, recs) in enumerate(case["cells"]):
        w = want.rows[want.cell_ptr[i]:want.cell_ptr[i + 1]]
        g = rows[ptr[i]:ptr[i + 1]]
        if g != w:
            k = next((j for j, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            raise AssertionError("%s cell %d: %d rows for %d; row %d is %r, the judge says %r" % (what, i, len(g), len(w), k, g[k:k + 1], w[k:k + 1]))
        if bc is not None and recs:   # (the barcode of a cell without records is not defined)
            assert int(bc[i]) == cell_bc, (what, i, hex(int(bc[i])), hex(cell_bc))
        n_judged += 1
    assert n_judged == len(case["off"]) == len(case["cells"]), what
    assert ptr == want.cell_ptr, what
    if st is not None:
        seen = {k: int(st[k]) for k in TALLIES}
        assert seen == {k: getattr(want, k) for k in TALLIES}, (what, seen, {k: getattr(want, k) for k in TALLIES})
        if "n_distinct" in st:
            assert st["n_distinct"] == len(want.rows), what


def kept_columns(case):
    """the kept fragments of a case as the column-level entry points take them: ref, start, frag_len, cell_ptr"""
    ref, start, fl, ptr = [], [], [], [0]
    for _, recs in case["cells"]:
        for a in recs:
            f = J.kept_fragment(a)
            if f is not None:
                ref.append(f[0]); start.append(f[1]); fl.append(f[2])
        ptr.append(len(ref))
    return np.asarray(ref, np.uint32), np.asarray(start, np.uint32), np.asarray(fl, np.uint16), np.asarray(ptr, np.uint64)


# --------------------------------------------------------------------------------------------------------------- witnesses
def _le(b, first, n, width):
    """the little-endian integers of `width` bytes at positions first .. first + n - 1 of the byte array b"""
    v = np.zeros(n, np.uint64)
    for k in range(width):
        v |= b[first + k:first + k + n].astype(np.uint64) << np.uint64(8 * k)
    return v


def false_starts(case):
    """WITNESS.  Per cell, the byte positions that k_atac_parse takes for a record start and that are none: position p (8 <= p,
    p + 4 + bc_bytes <= nbytes) is a candidate iff the barcode field at p + 4 equals that of the chunk's first record and the na
    at p fits the rest of the chunk; every true start is one, so the false ones are the candidates beyond nrec.  A cell with a
    false start fails the proof and is walked."""
    H = 4 + case["bc_bytes"]
    out = []
    for o in case["off"].tolist():
        nb, nrec = (int.from_bytes(case["data"][o + k:o + k + 4].tobytes(), "little") for k in (0, 4))
        n = nb - H - 8 + 1
        if n <= 0:
            assert nrec == 0
            out.append(0)
            continue
        b = np.concatenate((case["data"][o:o + nb], np.zeros(16, np.uint8)))
        na, bcv = _le(b, 8, n, 4), _le(b, 12, n, case["bc_bytes"])
        room = (nb - H - np.arange(8, 8 + n)) // 11
        out.append(int(((bcv == bcv[0]) & (na <= room.astype(np.uint64))).sum()) - nrec)
    assert min(out) >= 0
    return out


def walked_cells(case):
    """WITNESS.  The cells k_atac_parse cannot prove and hands to the record-by-record walk: those with a false start, and the
    chunks of zero records - the proof starts from the first record's barcode, and a chunk without one has nothing to start from
    (its walk reads no record)."""
    return [i for i, (n, (_, recs)) in enumerate(zip(false_starts(case), case["cells"])) if n or not recs]


def kept_in_one_bitmap_word(case, cell):
    """WITNESS.  The most kept records of a cell that k_atac_parse finds in one bitmap word: the word of position q (counted from
    the dword boundary at or below the chunk's first byte) is that of its group of 256 positions and of q mod 4."""
    o = int(case["off"][cell])
    H, p, words = 4 + case["bc_bytes"], 8, {}
    for a in case["cells"][cell][1]:
        if J.kept_fragment(a) is not None:
            q = p + o % 4
            words[(q >> 8, q & 3)] = words.get((q >> 8, q & 3), 0) + 1
        p += H + 11 * len(a)
    return max(words.values())


def run_layout(records):
    """WITNESS.  [(first position, length)] of the runs of a cell's kept fragments in sorted order."""
    from collections import Counter

    kept = Counter(f for f in map(J.kept_fragment, records) if f is not None)
    out, at = [], 0
    for f in sorted(kept):
        out.append((at, kept[f]))
        at += kept[f]
    return out


def ref_runs(rows):
    """WITNESS.  The lengths of the runs of the ref column of a cell's rows (what k_atac_compact lists)."""
    out = []
    for i, r in enumerate(rows):
        if i and rows[i - 1][0] == r[0]:
            out[-1] += 1
        else:
            out.append(1)
    return out


# --------------------------------------------------------------------------------------------------------------- count wrap
WRAP_RUNS = (65535, 65536, 65537, 131072, 131073)
WRAP_COUNTS = (65535, 0, 1, 0, 1)
WRAP_BC = 0x1B2D4E63   # (ACGTAGTCCATGCGAT)


def wrap_cell(bc=WRAP_BC):
    """One cell: the five runs of WRAP_RUNS identical fragments, an ordinary (single) fragment before, between and after them."""
    frags, mult = [], []
    for k, n in enumerate(WRAP_RUNS):
        frags += [(3, 1000 * k, 150), (3, 1000 * k + 500, 150)]
        mult += [1, n]
    frags.append((3, 1000 * len(WRAP_RUNS), 150))
    mult.append(1)
    return _run_cell(bc, frags, mult, seed=65536)


def wrap_case():
    """The wrap cell, then a small cell with a duplicate, a long fragment, a multi-mapped and an unmapped record (row offsets and
    tallies carry over), then fillers."""
    second = _py_cell(0x2222, [[(1, 4, 5, 60)], [(1, 4, 5, 60)], [(0, 4, 9, 2500)], [(0, 4, 1, 30), (1, 4, 1, 30)], [], [(1, 4, 4, 60)]])
    return _case([wrap_cell(), second] + _fillers(6, 4), 4)


def cli_case():
    """What the command-line test writes into a directory: the wrap cell and a cell on the 2000-base boundary of write_bed
    (1999 is written; 2000 and 2001 are counted) without a duplicate, so that the five wrapped runs are all that is deduplicated."""
    edge = _py_cell(0x0E4D2B1B, [[(0, 4, 10, 2000)], [(0, 4, 10, 1999)], [(1, 4, 10, 2001)], [], [(0, 4, 1, 30), (1, 4, 1, 30)], [(2, 1, 10, 50)]])
    return _case([wrap_cell(), edge], 4, min_cells=2)


# ------------------------------------------------------------------------------------------------- run heads and sort tiles
RUN_HEAD_SIZES = (1023, 1024, 1025, 16383, 16384, 16385, 32769)


def _distinct_frags(rng, n):
    """n distinct (ref, start, frag_len), ascending"""
    key = np.unique((rng.integers(0, 6, size=2 * n + 64, dtype=np.uint64) << np.uint64(48)) | (rng.integers(0, 1 << 27, size=2 * n + 64, dtype=np.uint64) << np.uint64(16))
                    | rng.integers(30, 2500, size=2 * n + 64, dtype=np.uint64))
    key = np.sort(rng.permutation(key)[:n])
    assert len(key) == n
    return [(k >> 48, (k >> 16) & 0xFFFFFFFF, k & 0xFFFF) for k in key.tolist()]


def _fill_runs(n, forced, rng):
    """run lengths that sum to n: the forced runs [(first position, length)] where they are asked for, runs of 1 .. 3 between"""
    out, at = [], 0
    for pos, ln in sorted(forced) + [(n, 0)]:
        assert pos >= at
        while at < pos:
            ln1 = min(int(rng.integers(1, 4)), pos - at)
            out.append(ln1)
            at += ln1
        if ln:
            out.append(ln)
            at += ln
    assert at == n and sum(out) == n
    return out


def run_head_plan():
    """{kept fragments of the cell: run lengths or the forced runs}: all distinct | one run | a run on the last two positions,
    which begins one before the first 2^10 boundary | a mix with a run over 1023 .. 1025 | all distinct | a mix with runs over
    1023 .. 1025, 2047 .. 2049 and 16382 .. 16384 | a mix with a run of ten across position 2^14 and a run on the last two
    positions, 2^15 - 1 and 2^15."""
    return {1023: "distinct", 1024: "one run", 1025: [(1023, 2)], 16383: [(1023, 3)], 16384: "distinct", 16385: [(1023, 3), (2047, 3), (16382, 3)],
            32769: [(16380, 10), (32767, 2)]}


def run_head_case():
    rng = np.random.default_rng(1024)
    cells = []
    for ci, (n, plan) in enumerate(run_head_plan().items()):
        if plan == "distinct":
            mult = [1] * n
        elif plan == "one run":
            mult = [n]
        else:
            mult = _fill_runs(n, plan, rng)
        cells.append(_run_cell(_bc(ci, 4), _distinct_frags(rng, len(mult)), mult, seed=n))
    return _case(cells + _fillers(2, 4), 4)


# --------------------------------------------------------------------------------------------------------------- key packing
def packing_neighbours(r=7):
    """Fragments that are neighbours in (ref, start, frag_len) order and differ only across a field boundary of a packed
    ref:16 | start:32 | frag_len:16 key, with their multiplicities: the top of start and frag_len next to the bottom of the next
    ref; frag_len 65535 next to the next start with frag_len 0; the same at the top of the 16-bit refs."""
    top = (1 << 32) - 1
    frags = [(r, top - 1, 65535), (r, top, 0), (r, top, 65534), (r, top, 65535), (r + 1, 0, 0), (r + 1, 0, 1),
             (r + 1, 0x00FFFFFF, 65535), (r + 1, 0x01000000, 0), (r + 1, 0x0000FFFF, 0), (r + 1, 0, 65535), (r + 1, 1, 0),
             (65534, top, 65535), (65535, 0, 0), (65535, top, 65535), (0, 0, 0), (0, 0, 65535), (0, 1, 0)]
    return frags, [1 + i % 3 for i in range(len(frags))]


PACKING_KINDS = ("fast", "wide_first", "wide_last")


def packing_case(kind):
    """Ten cells; the first and the last hold the neighbours.  fast: no reference id above 65535 (65535 itself is there).
    wide_first / wide_last: the first / the last cell also holds (65536, 0, 0) twice and (65536, 2^32 - 1, 65535) - next to
    (65535, 2^32 - 1, 65535), with which a key cut to 16 ref bits would not merge it but (0, ...) would."""
    frags, mult = packing_neighbours()
    wide_f, wide_m = [(65536, 0, 0), (65536, (1 << 32) - 1, 65535), (70000, 5, 50)], [2, 1, 3]
    cells = []
    for pos in ("first", "last"):
        w = kind == "wide_" + pos
        cells.append(_run_cell(_bc(10 + len(cells), 4), frags + (wide_f if w else []), mult + (wide_m if w else []), seed=len(kind)))
    return _case([cells[0]] + _fillers(8, 4) + [cells[1]], 4, wide=kind != "fast")


# -------------------------------------------------------------------------------------------------------------------- filter
def filter_case():
    """cell 0: one alignment of each type 0 .. 7 on one fragment (type 4 twice), two alignments both of type 4, three of mixed
    types, none; cell 1: nothing is kept; cell 2: one kept record; cell 3: one record without alignments; cell 4 and the last
    cell: chunks of zero records; the rest fillers."""
    c0 = [[(2, t, 50, 100)] for t in range(8)] + [[(2, 4, 50, 100)], [(2, 4, 50, 100), (2, 4, 50, 100)], [(1, 4, 3, 30), (1, 0, 3, 30), (1, 7, 3, 30)], [],
                                                  [(2, 4, 49, 100)], [(2, 4, 50, 99)]]
    c1 = [[(2, t, 50, 100)] for t in (0, 1, 2, 3, 5, 6, 7)] + [[], [(2, 4, 50, 100), (2, 4, 50, 100)], []]
    cells = [_py_cell(_bc(0, 4), c0), _py_cell(_bc(1, 4), c1), _py_cell(_bc(2, 4), [[(9, 4, 8, 7)]]), _py_cell(_bc(3, 4), [[]]), _py_cell(_bc(4, 4), [])]
    return _case(cells + _fillers(4, 4) + [_py_cell(_bc(5, 4), [])], 4, n_fallback=2)   # (the two chunks without a first record)


# --------------------------------------------------------------------------------------------------------------------- parse
PARSE_CHUNK_BYTES = (255, 256, 257, 511, 512, 513, 2047, 2048, 2049)
WIDTHS = (1, 2, 4, 8)


def _tiling(total, H):
    """(n0, n1, n2): records without, with one and with two alignments - some of each - whose sizes sum to `total` bytes"""
    for n0 in range(1, 40):
        for n2 in range(1, 6):
            rest = total - n0 * H - n2 * (H + 22)
            if rest >= H + 11 and rest % (H + 11) == 0:
                return n0, rest // (H + 11), n2
    raise AssertionError((total, H))


def parse_case(bc_bytes, pad):
    """Chunks of exactly PARSE_CHUNK_BYTES bytes (records of no, one and two alignments, mixed); a cell of 64 single-alignment
    records and nothing else (with a 1-byte barcode they are 16 bytes each: sixteen kept records in one bitmap word); and a last
    cell that ends with a record without alignments, sized so that the buffer - `pad` bytes in front shift every chunk to another
    byte alignment - ends in a partial dword."""
    H = 4 + bc_bytes
    rng = np.random.default_rng(10 * bc_bytes + pad)

    def rec(na, ty=4):
        return [(int(rng.integers(0, 25)), ty, int(rng.integers(0, 1 << 27)), int(rng.integers(30, 2500))) for _ in range(na)]

    cells = []
    for ci, nbytes in enumerate(PARSE_CHUNK_BYTES):
        n0, n1, n2 = _tiling(nbytes - 8, H)
        recs = [rec(0) for _ in range(n0)] + [rec(1, 4 if i % 7 else 1) for i in range(n1)] + [rec(2) for _ in range(n2)]
        cells.append(_py_cell(_bc(ci, bc_bytes), [recs[i] for i in rng.permutation(len(recs))]))
    cells.append(_py_cell(_bc(20, bc_bytes), [rec(1) for _ in range(64)]))
    size = pad + sum(8 + sum(H + 11 * len(a) for a in c["records"]) for c in cells)
    n1, n0 = next((a, b) for a in range(4) for b in range(1, 5) if (size + 8 + a * (H + 11) + b * H) % 4 == 1 + pad % 3)
    cells.append(_py_cell(_bc(21, bc_bytes), [rec(1) for _ in range(n1)] + [[] for _ in range(n0)]))
    return _case(cells, bc_bytes, pad=pad, single_cell=len(PARSE_CHUNK_BYTES))


# ------------------------------------------------------------------------------------------------------------------ fallback
def fallback_case(bc_bytes):
    """Cells in which a field spells the barcode where a record could start, so that the walk-free proof fails and the cell is
    walked (n_fallback_cells counts them), between cells that are proven.
    4 bytes: a type-0 record whose start_pos is the barcode (the bytes in front of it read as na == 0); and a cell with barcode 2
    whose kept record has ref == 2 (the barcode field in front of it reads as na == 2).
    2 bytes: a KEPT record whose frag_len is the barcode and whose start_pos is 0 (read as na == 0).
    1 byte: a type-0 record with ref < 256 whose start_pos ends in the barcode byte."""
    if bc_bytes == 4:
        bc = 0x00ABCDEF
        a = [[(1, 4, 1000 + i, 100)] for i in range(50)]
        a[17] = [(1, 0, bc, 100)]
        b = [[(2, 4, 5, 50)], [(1, 4, 6, 50)], [(1, 4, 6, 50)], [(0, 4, 1, 1), (0, 4, 1, 1)], [(3, 4, 9, 2000)]]
        special = [_py_cell(bc, a), _py_cell(2, b)]
    elif bc_bytes == 2:
        bc = 0x0C11
        a = [[(3, 4, 70 + i % 5, 100)] for i in range(30)]
        a[11] = [(3, 4, 0, bc)]
        special = [_py_cell(bc, a)]
    else:
        bc = 0xA7
        a = [[(3, 4, 0x100 * i, 100 + i)] for i in range(40)]
        a[23] = [(200, 0, 0x5500A7, 100)]
        special = [_py_cell(bc, a)]
    fill = _fillers(8, bc_bytes)
    return _case(fill[:3] + special[:1] + fill[3:6] + special[1:] + fill[6:], bc_bytes, n_fallback=len(special))


# ---------------------------------------------------------------------------------------------------------------- compaction
COMPACTION_REF_RUNS = ([700], [1] * 300, [1, 500, 1], [1], [1] * 320)


def compaction_case():
    """cell 0: 700 rows of one reference; cell 1: 300 rows, each a new reference; cell 2: one row, 500 rows, one row - the first
    run ends after the cell's first row, the last begins on its last row; cell 3: one row; cell 4 (behind fillers, in a late
    range): 320 rows of 320 references - with the others more than 400 runs."""
    rng = np.random.default_rng(5)
    cells = []
    for ci, runs in enumerate(COMPACTION_REF_RUNS):
        frags, ref = [], 3 * ci
        for n in runs:
            starts = np.sort(rng.permutation(100000)[:n])
            frags += [(ref, int(s), 40 + ci) for s in starts]
            ref += 2
        cells.append(_run_cell(_bc(30 + ci, 4), frags, [1 + (i % 5 == 0) for i in range(len(frags))], seed=ci))
    return _case(cells[:4] + _fillers(5, 4) + cells[4:], 4, rows_cells=(0, 1, 2, 3, 9))


# ------------------------------------------------------------------------------------------------------------------ the list
_memo = {}


def all_case_names():
    names = ["wrap", "run_heads"] + ["packing_" + k for k in PACKING_KINDS] + ["filter"]
    names += ["parse_%d_%d" % (w, p) for w in WIDTHS for p in range(4)] + ["fallback_%d" % w for w in (4, 2, 1)] + ["compaction"]
    return names


def get_case(name):
    if name not in _memo:
        kind, _, arg = name.partition("_")
        if name == "wrap":
            c = wrap_case()
        elif name == "run_heads":
            c = run_head_case()
        elif kind == "packing":
            c = packing_case(arg)
        elif name == "filter":
            c = filter_case()
        elif kind == "parse":
            c = parse_case(*(int(x) for x in arg.split("_")))
        elif kind == "fallback":
            c = fallback_case(int(arg))
        else:
            assert name == "compaction"
            c = compaction_case()
        c["name"] = name
        _memo[name] = c
    return _memo[name]
