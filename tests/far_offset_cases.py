"""Chunk tables whose 64-bit offsets lie at and across byte 2^32 of one buffer, for the eight record passes (gpl, gpl multi, atac gpl,
atac sort, collate, collate multi, atac collate, atac deduplicate).  Pure Python / numpy: nothing here touches a device.

`place` moves the chunks of an existing case to new offsets of an otherwise zeroed buffer of N_BYTES = 2^32 + 2^21 bytes and returns
the few pieces to write; the chunks' contents do not change, so what a pass owes is what the family's existing judge says of the
ORIGINAL case.  Beside every byte placed at an offset o >= 2^32, `place` writes at o - 2^32 the same byte of the chunk's DECOY: the
same chunk (nbytes, nrec and every na unchanged) with the low bit of every barcode and UMI flipped and, so that a truncated read of an
alignment LIST shows as well, one bit of every alignment (an RNA word's orientation bit, an ATAC start position's low bit).  A kernel
that drops the high half of an offset therefore walks a well-formed chunk and returns a wrong answer, not a refusal: `decoy_view` is
the input such a kernel would see, and tests/test_far_offset_cases_cpu.py shows that the family's judge tells it from the original.

A record layout is (fields, A): fields = [(name, width), ...] behind the 4-byte na, A = the bytes of one alignment.  A FAMILY (below)
binds a layout to the family's existing case builders and judge; it adds no judge of its own - `from_bytes` only decodes bytes back
into the structures the family's judge takes.

Below the families: `chunk_table_placement` (a collated stream for afq_collated_chunk_table) and `bam_placement` (a BAM record stream for
afq_convert_bam_rad), built on the same buffer size with their own decoys; each section says how."""
import numpy as np

import atac_collate_cases as AC
import atac_dedup_cases as AD
import atac_dedup_judge as ADJ
import atac_gpl_cases as AG
import atac_sort_cases as AS
import collate_cases as CC
import collate_judge as CJ
import collate_multi_cases as CM
import gpl_cases as G
import gpl_multi_cases as MC
from util import pkg

FAR = 1 << 32
N_BYTES = FAR + (1 << 21)
GAP = 4096                 # low-high: the far chunks begin at FAR + gap + pad (a caller whose chunk 0 is larger hands in a larger gap)
LAYOUTS = ("low-high", "start-on", "straddle-head", "straddle-list", "descending", "tile-first", "tile-last")
LONG_NA = 64               # straddle-list: a record of more alignments than one 64-lane trip takes


# ------------------------------------------------------------------------------------------------------------------ bytes
def u(buf, at, width):
    return int.from_bytes(buf[at:at + width], "little")


def head_bytes(fields):
    return 4 + sum(w for _, w in fields)


def walk(data, off, fields, A):
    """per chunk: (nbytes, [(q, na), ...]) - q the record's byte offset from the chunk's first byte (the 8 header bytes included)"""
    H, out = head_bytes(fields), []
    for o in off:
        o = int(o)
        nbytes, nrec = u(data, o, 4), u(data, o + 4, 4)
        q, recs = 8, []
        for _ in range(nrec):
            na = u(data, o + q, 4)
            recs.append((q, na))
            q += H + A * na
        assert q == nbytes, "the records do not tile the chunk"
        out.append((nbytes, recs))
    return out


def tile_starts(recs, tile):
    """where the record passes begin their tiles in a chunk: a tile begins at a record start (the first at byte 8), takes the records
    that start less than `tile` bytes behind it, and the next begins where the last of them ends"""
    out, i = [], 0
    while i < len(recs):
        p = recs[i][0]
        out.append(p)
        while i < len(recs) and recs[i][0] - p < tile:
            i += 1
    return out


def decoy(chunk, fields, A, aln_flip=None):
    """the chunk with the low bit of every field of every record's head flipped; nbytes, nrec and every na unchanged.  aln_flip =
    (byte, mask): that byte of every alignment is XORed with mask too, so that a read of an alignment LIST through a truncated offset
    shows as well (the orientation bit of an RNA word, the low bit of an ATAC start position)"""
    b = bytearray(chunk)
    (_, recs), = walk(chunk, [0], fields, A)
    H = head_bytes(fields)
    for q, na in recs:
        at = q + 4
        for _, w in fields:
            b[at] ^= 1
            at += w
        for j in range(na if aln_flip is not None else 0):
            b[q + H + A * j + aln_flip[0]] ^= aln_flip[1]
    return bytes(b)


def chunk_bytes(data, off, walked):
    return [bytes(data[int(o):int(o) + nb]) for o, (nb, _) in zip(off, walked)]


def _around(sizes, c, at):
    """offsets of chunks packed back to back such that chunk c begins at `at`"""
    out = [0] * len(sizes)
    out[c] = at
    for i in range(c - 1, -1, -1):
        out[i] = out[i + 1] - sizes[i]
    for i in range(c + 1, len(sizes)):
        out[i] = out[i - 1] + sizes[i - 1]
    return out


def _from(sizes, first, skip=()):
    out, at = [0] * len(sizes), first
    for i, s in enumerate(sizes):
        if i not in skip:
            out[i] = at
            at += s
    return out


def anchor(walked, layout, fields, A, pad=0, tile=None, gap=GAP):
    """the new offset of every chunk under `layout`, or None where the case has not what the layout needs (a second chunk, a record
    in the middle of a chunk, a first chunk of at most `gap` bytes, a record of more than LONG_NA alignments, a chunk of three tiles)"""
    H = head_bytes(fields)
    sizes = [nb for nb, _ in walked]
    n = len(sizes)
    if layout == "low-high":
        if n < 2 or pad + sizes[0] > gap:   # (chunk 0 would lie on the far chunks' decoys)
            return None
        out = _from(sizes, FAR + gap + pad, skip=(0,))
        out[0] = pad
        return out
    if layout == "descending":
        if n < 2:
            return None
        out = _from(sizes, FAR + (1 << 20) + pad, skip=(1,))   # chunk 0 far, chunk 1 low, the others behind chunk 0
        out[1] = pad
        return out
    if layout == "start-on":
        c = next((i for i in range(1, n) if walked[i][1]), None)
        return None if c is None else _around(sizes, c, FAR)
    if layout == "straddle-head":
        c = max(range(n), key=lambda i: len(walked[i][1]))
        recs = walked[c][1]
        if len(recs) < 3:
            return None
        return _around(sizes, c, FAR - 2 - recs[len(recs) // 2][0])
    if layout == "straddle-list":
        na, c, q = max((na, c, q) for c, (_, recs) in enumerate(walked) for q, na in recs) if any(r for _, r in walked) else (0, 0, 0)
        return _around(sizes, c, FAR - (q + H + A * max(na // 2, LONG_NA) + 1)) if na > LONG_NA else None   # (inside a word behind the first trip)
    if layout in ("tile-first", "tile-last"):
        assert tile, "the tile layouts take the family's parse_tile"
        for c, (nb, recs) in enumerate(walked):
            ts = tile_starts(recs, tile)
            if len(ts) >= 3 and ts[1] + tile <= nb:   # (the middle tile is a whole one)
                return _around(sizes, c, FAR - ts[1] - (tile - 1 if layout == "tile-last" else 0))
        return None
    raise ValueError(layout)


def place(data, off, layout, fields, A, pad=0, tile=None, aln_flip=None, gap=GAP):
    """-> (pieces, new_off, n_bytes): pieces = [(byte offset, bytes)] to write into a zeroed buffer of n_bytes; new_off the chunk table.
    None where the layout does not apply to the case (see `anchor`)."""
    walked = walk(data, off, fields, A)
    new_off = anchor(walked, layout, fields, A, pad, tile, gap)
    if new_off is None:
        return None
    chunks = chunk_bytes(data, off, walked)
    real, decoys = [], []
    for o, ch in zip(new_off, chunks):
        assert 0 <= o and o + len(ch) + 16 <= N_BYTES - 3, (layout, o, len(ch))
        real.append((o, ch))
        if o + len(ch) > FAR:
            skip = max(0, FAR - o)
            decoys.append((o + skip - FAR, decoy(ch, fields, A, aln_flip)[skip:]))
    for kind in (real, real + decoys):   # no chunk overlaps another, no decoy overlaps a real piece or another decoy
        spans = sorted((o, o + len(b)) for o, b in kind)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (layout, "pieces overlap")
    return real + decoys, np.asarray(new_off, np.uint64), N_BYTES


def decoy_view(data, off, new_off, fields, A, aln_flip=None):
    """the case's bytes (same chunk table `off`) as a kernel that drops the high half of its offsets reads them: every byte that
    `place` put at or behind 2^32 is the decoy's"""
    walked = walk(data, off, fields, A)
    out = bytearray(data)
    for o, no, ch in zip(off, new_off, chunk_bytes(data, off, walked)):
        o, no = int(o), int(no)
        if no + len(ch) > FAR:
            skip = max(0, FAR - no)
            out[o + skip:o + len(ch)] = decoy(ch, fields, A, aln_flip)[skip:]
    return bytes(out)


def where(data, off, new_off, fields, A):
    """(chunk, record, field, byte within the field) of byte 2^32: field is "nbytes" / "nrec" for the chunk header (record None),
    "na", a field's name, or ("aln", j); None when the byte lies in no chunk."""
    H = head_bytes(fields)
    for c, ((nb, recs), no) in enumerate(zip(walk(data, off, fields, A), new_off)):
        j = FAR - int(no)
        if not 0 <= j < nb:
            continue
        if j < 8:
            return c, None, ("nbytes", "nrec")[j // 4], j % 4
        r = max(i for i, (q, _) in enumerate(recs) if q <= j)
        k = j - recs[r][0]
        if k < 4:
            return c, r, "na", k
        at = 4
        for name, w in fields:
            if k < at + w:
                return c, r, name, k - at
            at += w
        return c, r, ("aln", (k - H) // A), (k - H) % A
    return None


def far_chunks(new_off):
    """the chunks that begin at or behind 2^32"""
    return [i for i, o in enumerate(new_off) if int(o) >= FAR]


def decode(data, off, fields, A):
    """per chunk the records as (field values ..., [alignment bytes, ...])"""
    H, out = head_bytes(fields), []
    for o, (_, recs) in zip(off, walk(data, off, fields, A)):
        o, chunk = int(o), []
        for q, na in recs:
            vals, at = [], o + q + 4
            for _, w in fields:
                vals.append(u(data, at, w))
                at += w
            chunk.append(tuple(vals) + ([bytes(data[o + q + H + A * j:o + q + H + A * (j + 1)]) for j in range(na)],))
        out.append(chunk)
    return out


def canon(x):
    """a result as plain comparable Python: arrays as lists, dicts as sorted item lists"""
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, dict):
        return [(k, canon(x[k])) for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [canon(v) for v in x]
    if isinstance(x, (np.integer,)):
        return int(x)
    return x


# ------------------------------------------------------------------------------------------------------------------ families
def _rna_alns(alns):
    return [(u(a, 0, 4) & 0x7FFFFFFF, u(a, 0, 4) >> 31 == 1) for a in alns]


def _atac_alns(alns):
    return [(u(a, 0, 4), a[4], u(a, 5, 4), u(a, 9, 2)) for a in alns]


def _tiles_chunks(chunks, size_of, tile, small=3):
    """[a few records], [the records of every chunk over and over until they span more than three and a half tiles], [a few records]"""
    flat = [r for recs in chunks for r in recs]
    big, n = [], 0
    while n <= 3 * tile + tile // 2:
        for r in flat:
            big.append(r)
            n += size_of(r)
    return [flat[:small], big, flat[-small:]]


class Family:
    """name; limits() (None: the pass has no tiles); oris; layouts; cases(lim) -> {name: case}; layout(case) -> (fields, A);
    want(case, ori, lim): the family's existing judge on the case; from_bytes(case, data, ori, lim): the same judge on other bytes
    under the case's chunk table and tables"""
    oris = (None,)
    layouts = LAYOUTS
    limits = None
    aln_flip = (3, 0x80)   # (see `decoy`: the orientation bit of an RNA alignment word)

    def tile(self):
        return self.limits()["parse_tile"] if self.limits else None


class Gpl(Family):
    name, oris = "gpl", tuple(G.ORIS)
    limits = staticmethod(pkg.gpl_limits)

    def cases(self, lim):
        w = G.widths_case(8, 8, 8)
        return {"widths": w, "long": G.long_case("last"),
                "tiles": G.parse_case(_tiles_chunks(w["chunks"], lambda r: G.rec_size(len(r[2]), 8, 8, 8), lim["parse_tile"]), 8, 8, 8)}

    def layout(self, c):
        return [("bc", c["bc_bytes"]), ("umi", c["umi_bytes"])], 4 + c["pos_bytes"]

    def want(self, c, ori, lim):
        return G.want_hist(c, ori)

    def from_bytes(self, c, data, ori, lim):
        chunks = [[(bc, umi, _rna_alns(a)) for bc, umi, a in recs] for recs in decode(data, c["off"], *self.layout(c))]
        return G.want_hist({"chunks": chunks}, ori)


class GplMulti(Family):
    name, oris = "gpl multi", tuple(MC.ORIS)
    limits = staticmethod(pkg.gpl_multi_limits)

    def cases(self, lim):
        w = MC.widths_case(4, 4, 8, pos_bytes=8)
        return {"widths": w, "long": MC.long_case("last"),
                "tiles": MC.multi_case(_tiles_chunks(w["chunks"], lambda r: MC.rec_size(len(r[3]), 20, 8), lim["parse_tile"]), w["entries"], 4, 4, 8, 8)}

    def layout(self, c):
        return [("b0", c["b0_bytes"]), ("b1", c["b1_bytes"]), ("umi", c["umi_bytes"])], 4 + c["pos_bytes"]

    def want(self, c, ori, lim):
        return MC.want_pairs(c, ori)

    def from_bytes(self, c, data, ori, lim):
        chunks = [[(b0, b1, umi, _rna_alns(a)) for b0, b1, umi, a in recs] for recs in decode(data, c["off"], *self.layout(c))]
        return MC.want_pairs({"chunks": chunks, "entries": c["entries"]}, ori)


class AtacGpl(Family):
    aln_flip = (5, 1)   # the low bit of the start position
    name = "atac gpl"
    limits = staticmethod(pkg.atac_gpl_limits)
    layouts = tuple(x for x in LAYOUTS if x != "straddle-list")
    REF_LEN = [250001, 900, 99993]

    def cases(self, lim):
        out = {}
        for name, chunks in (("widths", AG.mixed_chunks(lim, 8, self.REF_LEN)[:40]), ("narrow", AG.mixed_chunks(lim, 1, self.REF_LEN)[:12])):
            bcb = 8 if name == "widths" else 1
            data, off = pkg.rad.encode_atac_chunks(chunks, bc_bytes=bcb)
            out[name] = {"chunks": chunks, "data": data, "off": off, "bc_bytes": bcb, "blens": AG.blens_of(self.REF_LEN)}
        return out

    def layout(self, c):
        return [("bc", c["bc_bytes"])], 11

    def want(self, c, ori, lim):
        return AG.want_of(c["chunks"], c["blens"])

    def from_bytes(self, c, data, ori, lim):
        return AG.want_of([[(bc, _atac_alns(a)) for bc, a in recs] for recs in decode(data, c["off"], *self.layout(c))], c["blens"])


class AtacSort(Family):
    aln_flip = (5, 1)   # the low bit of the start position
    name = "atac sort"
    limits = staticmethod(pkg.atac_sort_limits)
    layouts = tuple(x for x in LAYOUTS if x != "straddle-list")

    def cases(self, lim):
        out = {"widths": AS.long_records_case(lim, 8), "halo": AS.halo_case(lim, 8, "last_byte")}
        for name, w in (("tiles", 8), ("narrow", 1)):   # tile_full_case with its chunk of kept records in front of AND behind the other
            t = AS.tile_full_case(lim, w)
            c0, c1 = t["chunks"]
            out[name] = AS._case_of_chunks([c1, c0, c1], t["obs"], t["cor"], t["ref_lengths"], w)
        return out

    def layout(self, c):
        return [("bc", c["bc_bytes"])], 11

    def want(self, c, ori, lim):
        return AS.want_of(c)

    def from_bytes(self, c, data, ori, lim):
        cols, _ = AS.flat([[(bc, _atac_alns(a)) for bc, a in recs] for recs in decode(data, c["off"], *self.layout(c))])
        return AS.expected(*cols, c["obs"], c["cor"])


class Collate(Family):
    name, oris = "collate", tuple(CC.ORIS)
    limits = staticmethod(pkg.collate_limits)

    def cases(self, lim):
        w = CC.widths_case(8, 8, 8)
        return {"widths": w, "route": CC.route_case(lim, 4),
                "tiles": CC.planned(_tiles_chunks(w["chunks"], lambda r: G.rec_size(len(r[2]), 8, 8, 8), lim["parse_tile"]), 8, 8, 8, seed=9)}

    def layout(self, c):
        return [("bc", c["bc_bytes"]), ("umi", c["umi_bytes"])], 4 + c["pos_bytes"]

    def want(self, c, ori, lim):
        return CC.want(c, ori, lim["lane_alns"])

    def from_bytes(self, c, data, ori, lim):
        return CJ.collate(data, c["off"], c["bc_bytes"], c["umi_bytes"], c["pos_bytes"], ori, c["corrections"], c["cells"], lim["lane_alns"])


class CollateMulti(Family):
    name, oris = "collate multi", tuple(CM.ORIS)
    limits = staticmethod(pkg.collate_multi_limits)

    def cases(self, lim):
        mc = MC.widths_case(4, 4, 8, pos_bytes=8)
        tiles = MC.multi_case(_tiles_chunks(mc["chunks"], lambda r: MC.rec_size(len(r[3]), 20, 8), lim["parse_tile"]), mc["entries"], 4, 4, 8, 8)
        return {"widths": CM.planned(mc, seed=4), "long": CM.long_case("last"), "route": CM.route_case(lim, 4), "tiles": CM.planned(tiles, seed=5)}

    def layout(self, c):
        return [("b0", c["b0_bytes"]), ("b1", c["b1_bytes"]), ("umi", c["umi_bytes"])], 4 + c["pos_bytes"]

    def want(self, c, ori, lim):
        return CM.want(c, ori, lim["lane_alns"])

    def from_bytes(self, c, data, ori, lim):
        return CM.want(dict(c, data=data), ori, lim["lane_alns"])


class AtacCollate(Family):
    aln_flip = (5, 1)   # the low bit of the start position
    name = "atac collate"
    limits = staticmethod(pkg.atac_collate_limits)
    layouts = tuple(x for x in LAYOUTS if x != "straddle-list")

    def cases(self, lim):
        w = AC.widths_case(8)
        tiles = AC.planned(_tiles_chunks(w["chunks"], lambda r: 12 + 11 * len(r[1]), lim["parse_tile"]), 8, seed=6)
        return {"widths": w, "long": AC.long_record_case(lim, 3)[0], "tiles": tiles}

    def layout(self, c):
        return [("bc", c["bc_bytes"])], AC.ALN

    def want(self, c, ori, lim):
        return AC.want(c)

    def from_bytes(self, c, data, ori, lim):
        return AC.want(dict(c, data=data))


class AtacDedup(Family):
    aln_flip = (5, 1)   # the low bit of the start position
    """collated input: a chunk is a cell.  The judge gives the rows and tallies; the cells' barcodes are the case's own (what
    same_as_judge compares bc with), read back here from the records' heads.  The rows do not depend on the barcode, so the decoys
    flip of the low bit of every start position is what tells a cell whose tail alone is read from its decoy: it has other rows,
    whichever of its two barcodes a kernel would report."""
    name = "atac dedup"
    layouts = ("low-high", "start-on", "straddle-head", "descending")

    def cases(self, lim):
        return {"widths": AD.get_case("parse_8_0"), "narrow": AD.get_case("parse_1_3"), "fallback": AD.get_case("fallback_4")}

    def layout(self, c):
        return [("bc", c["bc_bytes"])], 11

    def _judged(self, cells):
        j = ADJ.judge_cells([recs for _, recs in cells])
        return {"rows": [list(r) for r in j.rows], "cell_ptr": list(j.cell_ptr), "tallies": {k: getattr(j, k) for k in AD.TALLIES},
                "bc": [bc for bc, recs in cells if recs]}   # (a barcode, or the several a half-decoy cell holds)

    def want(self, c, ori, lim):
        return self._judged(c["cells"])

    def from_bytes(self, c, data, ori, lim):
        cells = []
        for recs in decode(data, c["off"], *self.layout(c)):
            bcs = sorted({bc for bc, _ in recs})
            cells.append((bcs[0] if len(bcs) == 1 else bcs, [_atac_alns(a) for _, a in recs]))
        return self._judged(cells)


FAMILIES = {f.name: f for f in (Gpl(), GplMulti(), AtacGpl(), AtacSort(), Collate(), CollateMulti(), AtacCollate(), AtacDedup())}
PADS = {"low-high": (0, 3), "descending": (1,)}   # the pad bytes the layouts that take one run with


def placements(fam, lim):
    """every (case name, layout, pad) of a family that applies, with what `place` returns and the case: the GPU test's list, and the
    CPU test's.  Every layout of the family applies to at least one of its cases."""
    out = []
    cases = fam.cases(lim)
    for layout in fam.layouts:
        hit = 0
        for name, c in cases.items():
            fields, A = fam.layout(c)
            data = c["data"].tobytes() if isinstance(c["data"], np.ndarray) else c["data"]
            for pad in PADS.get(layout, (0,)):
                p = place(data, c["off"], layout, fields, A, pad, fam.tile(), fam.aln_flip)
                if p is not None:
                    out.append((name, layout, pad, c, p))
                    hit += 1
        assert hit, (fam.name, layout, "applies to no case")
    return out


# ------------------------------------------------------------------------------------------------------------------ the chunk table
# afq_collated_chunk_table hops a collated stream that lies on the device.  The stream here: CT_FIRST bytes of prelude, two chunks
# of about 2^31 bytes each whose bodies are the buffer's zeros, thirty small chunks up to a header that stands at `at` - one of
# CT_HEADERS_AT, all around byte 2^32 - and some three hundred chunks behind it, one longer than the hop's tile, the last one of 15
# bytes: its 8 bytes at + 12 run past the stream's end, behind which CT_GUARD bytes of 0xff stand in the buffer (never the hop's to
# read).  DECOYS: 2^32 below every byte at or behind 2^32 of a chunk's nbytes, nrec and 8 bytes at + 12 stands the byte of another
# nbytes (+ 4), nrec (+ 1) and barcode (every bit flipped); they lie in the prelude and the first large chunk's body, which the hop
# does not look at.  A hop that drops the high half of an address reads them: chunk_table_view(truncated=True).
CT_FIRST = 37
CT_HEADERS_AT = (FAR - 20, FAR - 15, FAR - 8, FAR - 4, FAR - 1)   # (the chunk at FAR - 20 is one of 20 bytes: the next header stands at FAR)
CT_WHERE = {FAR - 20: ("nbytes", 0), FAR - 15: ("first_bc", 3), FAR - 8: ("record", 0), FAR - 4: ("nrec", 0), FAR - 1: ("nbytes", 1)}
CT_BIG = (1 << 31) + 12345
CT_GUARD = 16


def chunk_table_placement(at, tile, no_record=False):
    """-> dict: pieces (for a zeroed buffer of N_BYTES), n (the stream's bytes), off / nbytes (every chunk's, Python ints), k_at (the
    index of the chunk at `at`), n_whole (the stream's bytes without its last, 15-byte chunk).  no_record: chunk k_at + 2, which
    lies behind byte 2^32, says nrec = 0."""
    import chunk_table_cases as T

    rng = np.random.default_rng(int(FAR - at))
    front = [int(x) for x in rng.integers(20, 900, 30)]
    back = [20 if at == FAR - 20 else 333] + [int(x) for x in rng.integers(20, 900, 300)] + [15]
    back[150] = tile + 777
    small0 = at - sum(front)
    sizes = [CT_BIG, small0 - CT_FIRST - CT_BIG] + front + back
    off = _from(sizes, CT_FIRST)
    k_at, n = 2 + len(front), off[-1] + sizes[-1]
    assert off[k_at] == at and off[2] == small0 and (1 << 30) < sizes[1] < FAR and n + CT_GUARD + 3 <= N_BYTES
    nrec = [1, 1] + [nb & 7 or 1 for nb in sizes[2:]]
    if no_record:
        assert off[k_at + 2] > FAR
        nrec[k_at + 2] = 0
    chunks = [T.chunk(nb, nr, rng) for nb, nr in zip(sizes[2:], nrec[2:])]
    far = b"".join(chunks)
    head = lambda nb, nr: int(nb).to_bytes(4, "little") + int(nr).to_bytes(4, "little")
    low = bytearray(n - FAR)
    low[:CT_FIRST] = rng.integers(0, 256, CT_FIRST, dtype=np.uint8).tobytes()
    for p, ch, nb, nr in zip(off[2:], chunks, sizes[2:], nrec[2:]):
        fields = head(nb + 4, nr + 1) + ch[8:12] + bytes(x ^ 0xFF for x in ch[12:20])
        for j in list(range(8)) + list(range(12, len(fields))):
            if p + j >= FAR:
                low[p + j - FAR] = fields[j]
    low[CT_FIRST:CT_FIRST + 8] = head(sizes[0], 1)
    pieces = [(0, bytes(low)), (off[1], head(sizes[1], 1)), (small0, far), (n, b"\xff" * CT_GUARD)]
    return {"pieces": pieces, "n": n, "off": off, "nbytes": sizes, "nrec": nrec, "k_at": k_at, "n_whole": off[-1], "at": at}


def chunk_table_view(pl, n=None, truncated=False):
    """the stream's first n bytes (all of them by default) as the hop reads them - chunk_table_cases.host_hop takes it"""
    import chunk_table_cases as T

    return T.Sparse(pl["n"] if n is None else n, pl["pieces"], wrap=FAR if truncated else None)


def chunk_table_where(pl):
    """(field, byte within it) of byte 2^32: nbytes, nrec, "record" (the 4 bytes behind the header), first_bc or "body" """
    c = max(i for i, o in enumerate(pl["off"]) if o <= FAR)
    j = FAR - pl["off"][c]
    assert j < pl["nbytes"][c]
    for name, a, b in (("nbytes", 0, 4), ("nrec", 4, 8), ("record", 8, 12), ("first_bc", 12, 20)):
        if a <= j < b:
            return name, j - a
    return "body", j - 20


# ------------------------------------------------------------------------------------------------------------------ convert
# afq_convert_bam_rad walks every byte of an inflated BAM record stream, so what lies between the low records and the records at byte
# 2^32 are records too: two FILLERS, unmapped (flag 0x4, dropped by the walk), every other fixed field zero, block_size about 2^31,
# each in a span of its own; only their 36 fixed bytes are written, their bodies are the buffer's zeros and are never parsed.  The
# stream: a pad (one unmapped record), the DECOYS, [one more low record], filler, filler, the high records.  Decoy j stands exactly
# 2^32 below high record j and has its sizes; every character of its name and every base of its CR and UR is another one, its refID is
# the next one, its AS has the low bit flipped.  The decoys are records of the stream like any other (the judge states them too): a
# kernel that drops the high half of an offset reads a decoy where it owes a high record and writes the decoy's run twice.
BAM_N_REF, BAM_BW, BAM_UW = 7, 4, 4
BAM_PLACEMENTS = ("block_size", "l_read_name", "flag", "name", "CR", "UR", "AS", "start-on", "run-across")
_BASE = str.maketrans("ACGTN", "CGTAC")


def bam_filler_bytes(block_size):
    import struct

    return struct.pack("<I", block_size) + struct.pack("<iiBBHHHIiii", 0, 0, 0, 0, 0, 0, 0x4, 0, 0, 0, 0)


def bam_decoy(r):
    aux = []
    for t, ty, v in r.get("aux", []):
        if t in ("CR", "UR") and ty == "Z":
            v = v.translate(_BASE)
        elif t == "AS" and ty in "cCsSiI":
            v ^= 1
        aux.append((t, ty, v))
    return dict(r, name="".join(chr(ord(ch) ^ 1) for ch in r["name"]), ref=(r.get("ref", 0) + 1) % BAM_N_REF, aux=aux)


def bam_high_records(lim):
    """the records that stand around byte 2^32: the runs of bam_cases' `names`, `scores`, `aux` and `n_and_lengths` (every one with an
    integer AS, so that every placement runs with and without filter_best) -> (records, the index of the target: a run's head with CR,
    UR and a 4-byte AS)"""
    import bam_cases as B

    by_name = {c["name"]: c for c in B.name_cases() + B.device_cases(lim)}
    recs = [r for name in ("names", "scores", "aux", "n_and_lengths") for r in by_name[name]["records"]]
    t = next(i for i, r in enumerate(recs) if r["name"] == "tied")
    return recs, t


def bam_field_at(r, k):
    """the field of record r (its bytes: block_size first) that byte k lies in: a fixed field's name, "name", or (tag, "tag" / "value")"""
    import bam_cases as B

    fixed = (("block_size", 4), ("refID", 4), ("pos", 4), ("l_read_name", 1), ("mapq", 1), ("bin", 2), ("n_cigar_op", 2), ("flag", 2), ("l_seq", 4), ("next_refID", 4),
             ("next_pos", 4), ("tlen", 4))
    at = 0
    for name, w in fixed:
        if k < at + w:
            return name
        at += w
    if k < at + len(r["name"]) + 1:
        return "name"
    at += len(r["name"]) + 1 + 4 * len(r.get("cigar", [])) + (r.get("seq_len", 0) + 1) // 2 + r.get("seq_len", 0)
    assert k >= at, "the placements aim at no CIGAR or sequence"
    for f in r.get("aux", []):
        n = len(B.aux_bytes([f]))
        if k < at + n:
            return f[0], "tag" if k < at + 3 else "value"
        at += n
    return "tail"


def bam_offset_of(r, field):
    """the first byte, from the record's first, of a fixed field, of the name, or of an aux tag's value"""
    import bam_cases as B

    n = len(B.record_bytes(r))
    return next(k for k in range(n) if bam_field_at(r, k) in (field, (field, "value")))


def bam_placement(where, lim, tail=None):
    """-> dict: pieces, n_bytes, span_off, records (the judge's list, the fillers as small unmapped records), high0 (the index of the
    first high record), offs (every record's offset), target (the index of the record that byte 2^32 lies in), decoyed (the indices of
    the high records that have a decoy 2^32 below).  tail: a record put behind the last high record (the refusals')."""
    import bam_cases as B

    high, t = bam_high_records(lim)
    low_extra = []
    if where == "run-across":   # a run of three with distinct scores: its head the last low record, the others the first high ones
        run = [B.rec("across", ref=i + 2, score=s, flag=0x10 * (i & 1)) for i, s in enumerate((3, 9, 9))]
        low_extra, high, t = run[:1], run[1:] + high, 0
    high = high + ([tail] if tail is not None else [])
    hb = [B.record_bytes(r) for r in high]
    within = {"block_size": 2, "l_read_name": bam_offset_of(high[t], "l_read_name"), "flag": bam_offset_of(high[t], "flag"), "name": bam_offset_of(high[t], "name") + 2,
              "CR": bam_offset_of(high[t], "CR") + 5, "UR": bam_offset_of(high[t], "UR") + 5, "AS": bam_offset_of(high[t], "AS") + 2, "start-on": 0, "run-across": -5}[where]
    h_off = _around([len(b) for b in hb], t, FAR - within)
    # the low side: a pad up to the first decoy, the decoys 2^32 below their high records
    j0 = next(j for j, o in enumerate(h_off) if o == FAR or o - FAR >= 64)   # (the pad is a record: bam_cases.filler makes none below 54 bytes)
    n_dec = len(high) - j0 - (tail is not None)   # (the refusals' record has no decoy: the lowest record in error is the one named)
    decoys = [bam_decoy(r) for r in high[j0:j0 + n_dec]]
    assert [len(B.record_bytes(d)) for d in decoys] == [len(b) for b in hb[j0:j0 + n_dec]]
    pad = [B.filler(h_off[j0] - FAR, name="pad")] if h_off[j0] > FAR else []
    low = pad + decoys + low_extra
    lb = [B.record_bytes(r) for r in low]
    low_end, high_end = sum(len(b) for b in lb), h_off[-1] + len(hb[-1])
    f1, f2 = low_end, low_end + 36 + CT_BIG
    sizes = [len(b) for b in lb] + [f2 - f1, h_off[0] - f2] + [len(b) for b in hb]
    offs = _from(sizes, 0)
    high0 = len(low) + 2
    assert offs[high0:] == h_off and all(offs[len(pad) + j] == h_off[j0 + j] - FAR for j in range(len(decoys))) and high_end + 16 + 3 <= N_BYTES
    unmapped = dict(name="", flag=0x4)
    pieces = [(0, b"".join(lb)), (f1, bam_filler_bytes(f2 - f1 - 4)), (f2, bam_filler_bytes(h_off[0] - f2 - 4)), (h_off[0], b"".join(hb))]
    span_off = sorted({0, f1, f2, h_off[0]} | {o for o in h_off[7::7]} | ({FAR} if where == "start-on" else set()))
    return {"where": where, "pieces": pieces, "n_bytes": high_end, "span_off": span_off, "records": low + [unmapped, unmapped] + high, "high0": high0, "offs": offs,
            "target": high0 + t, "decoyed": list(range(high0 + j0, high0 + j0 + n_dec)), "n_pad": len(pad), "fillers": (high0 - 2, high0 - 1)}


def bam_truncated_records(pl):
    """the record list a kernel states that reads every record at its offset mod 2^32: the decoys where the decoyed high records stand"""
    recs = list(pl["records"])
    for j, i in enumerate(pl["decoyed"]):
        recs[i] = pl["records"][pl["n_pad"] + j]
    return recs


def bam_refusals(lim):
    """(name, placement, record index named): a record behind byte 2^32 whose aux fields overrun its end; a last record whose block_size
    reaches past the span's end.  Both are refused through the error word; neither makes a kernel read outside [0, n_bytes)."""
    import bam_cases as B

    a = bam_placement("block_size", lim, tail=dict(B.rec("overrun", ref=1, score=1), raw_tail=b"XY"))
    b = bam_placement("block_size", lim, tail=dict(B.rec("past", ref=1, score=1), block_size=4000))
    return [("aux past the record's end", a, len(a["records"]) - 1), ("block_size past the span's end", b, len(b["records"]) - 1)]
