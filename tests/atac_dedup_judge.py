"""A judge for `atac deduplicate`: what alevin-fry computes for ONE cell of a barcode-collated scATAC RAD, in plain Python.

Written from the reference's text (COMBINE-lab/alevin-fry; cited `file:line` below) and from nothing else:
src/atac/deduplicate.rs:37-66 and 199-237, src/atac/sort.rs:37-59 and the record layout of tests/atac_integration.rs:110-121.  Not
from oracle/afq_oracle.cpp, not from the kernels, not from alevin-fry_amd/rad.py.  The oracle follows the reference's control flow
(push, sort, count runs, cut the count); this file says what the result IS - a multiset of kept fragments and what is read off it -
so that a rule misread there is not repeated here.  Only ints, tuples, lists, dicts and Counters; no numpy, no ctypes.

A cell is its records, a record the list of its alignments:  [[(ref, map_type, start, frag_len), ...], ...]

    judge_cell(records)                       -> Cell(rows, n_records, n_multimapped, n_not_mapped_pair, n_deduplicated, n_long_fragments)
    judge_cells([records, ...])               -> Batch(cell_ptr, rows, and the five tallies summed)
    bed_lines(rows, barcode, ref_names, bc_len, rev) -> the lines write_bed adds for the cell
    log_lines(batch)                          -> the four "Number of records ..." lines
    read_chunk(data, off, bc_bytes)           -> (barcode or None, records, bytes of the chunk): the byte reader, on `struct` alone

What the judge does NOT define, and what its cases stay clear of:
  * a chunk whose records carry different barcodes.  The barcode is the last key of HitInfo's order and a field of its equality
    (sort.rs:37, 55-56), so such a chunk has an answer - but it is not collated input, and read_chunk refuses it;
  * a BED line whose start + frag_len passes 2^32: `start + frag_len as u32` (deduplicate.rs:51) panics in a debug build and wraps
    in a release build.  bed_lines refuses such a row;
  * the barcode of a cell without records: nothing in the reference reads it (HitInfo.barcode comes from a record,
    deduplicate.rs:209).  read_chunk answers None and the comparisons skip it.
Everything else has exactly one outcome.

The barcode string is needletail's (src/atac/utils.rs:9-18: bitkmer::reverse_complement when asked, then bitmer_to_bytes).  needletail's
text is not part of the reference tree; what is used here is its published encoding - two bits a base, A C G T = 0 1 2 3, the first
base in the highest of the 2 * bc_len bits - which tests/test_atac_dedup_judge_cpu.py pins with strings written out by hand.
"""
import struct
from collections import Counter, namedtuple

PROPER_PAIR = 4          # deduplicate.rs:204: `r.map_type[0] == 4`
LONG_FRAGMENT = 2000     # deduplicate.rs:47: `frag_len < 2000` is written, the rest is counted
COUNT_MODULUS = 1 << 16  # deduplicate.rs:222: `hv.count = count as u16`

# rows: [(ref, start, frag_len, count)] ascending; the tallies are the cell's share of what deduplicate.rs:265-284 logs
Cell = namedtuple("Cell", "rows n_records n_multimapped n_not_mapped_pair n_deduplicated n_long_fragments")
Batch = namedtuple("Batch", "cell_ptr rows n_records n_multimapped n_not_mapped_pair n_deduplicated n_long_fragments")


def kept_fragment(alignments):
    """(ref, start, frag_len) of a record that is kept, else None: exactly one alignment, and that one a properly mapped pair
    (deduplicate.rs:202-211)."""
    if len(alignments) == 1 and alignments[0][1] == PROPER_PAIR:
        ref, _, start, frag_len = alignments[0]
        return (ref, start, frag_len)
    return None


def judge_cell(records):
    """One chunk (deduplicate.rs:197-237).
    kept: the multiset of kept fragments.  Within a cell the barcode is one value, so HitInfo's order (sort.rs:47-58: chr, start,
    frag_len, barcode) is the order of the triples and HitInfo's equality (sort.rs:37, derived: every field, the count still 0) is
    equality of the triples: `sort_unstable` + `dedup_with_count` (deduplicate.rs:219-221) yield every distinct triple once,
    ascending, with its multiplicity.
    rows: the stored count is the multiplicity cut to 16 bits (deduplicate.rs:222).
    n_deduplicated: `if count > 1` is asked of the usize (deduplicate.rs:224) - the multiplicity, not the stored count.
    n_multimapped: more than one alignment, whatever their types (deduplicate.rs:212-214; the `na == 1 && type == 4` arm comes
    first and cannot take a record with two alignments).  n_not_mapped_pair: every record left - none, or one that is no proper
    pair (deduplicate.rs:215-217).  n_long_fragments: rows write_bed counts instead of writing (deduplicate.rs:47, 58-60).
    n_records: all of the chunk's (deduplicate.rs:198, 200)."""
    kept = Counter()
    multi = non = 0
    for alignments in records:
        f = kept_fragment(alignments)
        if f is not None:
            kept[f] += 1
        elif len(alignments) > 1:
            multi += 1
        else:
            non += 1
    rows = [(ref, start, fl, kept[(ref, start, fl)] % COUNT_MODULUS) for ref, start, fl in sorted(kept)]
    return Cell(rows=rows, n_records=len(records), n_multimapped=multi, n_not_mapped_pair=non,
                n_deduplicated=sum(1 for m in kept.values() if m > 1),
                n_long_fragments=sum(1 for _, _, fl in kept if fl >= LONG_FRAGMENT))


def judge_cells(cells):
    """Cells are independent (a chunk per iteration, deduplicate.rs:197) and the counters are sums over them (atomics,
    deduplicate.rs:124-127): the rows cell after cell, cell i's at rows[cell_ptr[i]:cell_ptr[i + 1]]."""
    judged = [judge_cell(r) for r in cells]
    ptr, rows = [0], []
    for j in judged:
        rows += j.rows
        ptr.append(len(rows))
    return Batch(ptr, rows, *(sum(getattr(j, k) for j in judged) for k in Cell._fields[1:]))


def bc_string(barcode, bc_len, rev):
    """get_bc_string (src/atac/utils.rs:9-18).  rev: the reverse complement - the bases in reverse order, each one's complement
    (A <-> T, C <-> G: 3 - code)."""
    codes = [(barcode >> (2 * (bc_len - 1 - i))) & 3 for i in range(bc_len)]
    if rev:
        codes = [3 - c for c in reversed(codes)]
    return "".join("ACGT"[c] for c in codes)


def bed_lines(rows, barcode, ref_names, bc_len, rev):
    """write_bed (deduplicate.rs:46-57) for one cell's rows: name, start, start + frag_len, barcode string, the STORED count."""
    s = bc_string(barcode, bc_len, rev)
    out = []
    for ref, start, fl, count in rows:
        if fl < LONG_FRAGMENT:
            if start + fl >= 1 << 32:
                raise ValueError("start + frag_len passes 2^32: the reference panics or wraps (deduplicate.rs:51); not judged")
            out.append("\t".join([ref_names[ref], str(start), str(start + fl), s, str(count)]))
    return out


def log_lines(batch):
    """deduplicate.rs:265-284, the text after the logger's prefix."""
    return ["Number of records with greater than 1 mapping %d" % batch.n_multimapped,
            "Number of records that are deduplicated %d" % batch.n_deduplicated,
            "Number of records that are not mapped pairs %d" % batch.n_not_mapped_pair,
            "Number of records that have frag length > 2000 %d" % batch.n_long_fragments]


# ------------------------------------------------------------------------------------------------------------- the byte reader
_BC = {1: "<B", 2: "<H", 4: "<I", 8: "<Q"}
_ALN = struct.Struct("<IBIH")   # ref:u32, type:u8, start_pos:u32, frag_len:u16 in that order (tests/atac_integration.rs:111-116)


def read_chunk(data, off, bc_bytes):
    """The chunk at data[off:]: nbytes:u32 (the header's eight bytes included), nrec:u32, then nrec records of na:u32, the read
    tag b (the barcode, tests/atac_integration.rs:104-108: here 1, 2, 4 or 8 bytes), na alignments.  Little-endian, unpadded.
    Returns (barcode of the records - None when there are none -, the records, nbytes).  Raises ValueError when the records do not
    tile the chunk or do not share one barcode."""
    assert _ALN.size == 11
    nbytes, nrec = struct.unpack_from("<II", data, off)
    p, end = off + 8, off + nbytes
    bcs, records = set(), []
    for _ in range(nrec):
        if p + 4 + bc_bytes > end:
            raise ValueError("records run past the chunk")
        na, = struct.unpack_from("<I", data, p)
        bcs.add(struct.unpack_from(_BC[bc_bytes], data, p + 4)[0])
        p += 4 + bc_bytes
        if p + 11 * na > end:
            raise ValueError("alignments run past the chunk")
        records.append([_ALN.unpack_from(data, p + 11 * k) for k in range(na)])
        p += 11 * na
    if p != end:
        raise ValueError("records do not tile the chunk")
    if len(bcs) > 1:
        raise ValueError("records of one chunk carry different barcodes: not collated input, not judged")
    return (bcs.pop() if bcs else None), records, nbytes
