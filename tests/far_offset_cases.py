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
into the structures the family's judge takes."""
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
