"""Case builders for the `atac collate` tests: inputs of afq_atac_collate_rad (chunks of an uncollated scATAC RAD, a correction map,
the cells in output order), each at the smallest shape at which the kernels can go wrong.  A case is a dict: chunks / data / off,
bc_bytes, corrections {observed: corrected}, cells [barcode, ...].  Records are (bc, [(ref, type, start, frag_len), ...]) as
rad.encode_atac_chunks takes them; every alignment of a case differs from every other, so a record that lands in the wrong place or
carries a neighbour's bytes shows.  Every size comes from atac_collate_limits(), handed in as the dict `lim`."""
import random

import numpy as np

import atac_collate_judge as J
from atac_sort_cases import _with_home, table_slots
from util import pkg

rad = pkg.rad
WIDTHS = [1, 2, 4, 8]
ONES = 0xFFFFFFFFFFFFFFFF
ALN = J.ALN


class Alns:
    """a source of alignments that all differ: every field, the type byte and the high bytes included, is busy"""
    def __init__(self, seed=0):
        self.k = seed * 1000003

    def one(self):
        self.k += 1
        v = (self.k * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
        return ((v >> 32) | 0x80000000 if self.k % 3 == 0 else v >> 40, 1 + self.k % 4, (v & 0xFFFFFFFF) | (0xFF000000 if self.k % 5 == 0 else 0), (v >> 16) & 0xFFFF)

    def many(self, na):
        return [self.one() for _ in range(na)]


def case(chunks, corrections, cells, bc_bytes=4, pad=0):
    data, off = rad.encode_atac_chunks(chunks, bc_bytes=bc_bytes)
    return {"chunks": chunks, "data": b"\xEE" * pad + data, "off": off + np.uint64(pad), "bc_bytes": bc_bytes, "corrections": dict(corrections), "cells": list(cells)}


def want(c):
    return J.collate(c["data"], c["off"], c["bc_bytes"], c["corrections"], c["cells"])


def plan_for(chunks, rng, extra_cell=None):
    """a correction map over the barcodes the chunks carry: about half of them are cells (mapped onto themselves), a third of the
    others are corrected onto a cell, the rest are not in the map; the cells in a shuffled order, `extra_cell` (never observed: it
    stays empty) among them"""
    bcs = sorted({r[0] for recs in chunks for r in recs})
    cells = [b for i, b in enumerate(bcs) if i % 2 == 0] or bcs[:1]
    corr = {b: b for b in cells}
    for i, b in enumerate(x for x in bcs if x not in corr):
        if i % 3 == 0:
            corr[b] = rng.choice(cells)
    if extra_cell is not None and extra_cell not in corr:
        cells.append(extra_cell)
    rng.shuffle(cells)
    return corr, cells


def planned(chunks, bc_bytes, pad=0, seed=0, extra_cell=None):
    corr, cells = plan_for(chunks, random.Random(seed), extra_cell)
    return case(chunks, corr, cells, bc_bytes, pad)


def record_spans(out, chunk_off, bc_bytes):
    """(start, end) byte offsets of every record of a collated output"""
    R = 4 + bc_bytes + ALN
    return [(int(o) + 8 + R * k, int(o) + 8 + R * (k + 1)) for o in chunk_off[:-1] for k in range(int.from_bytes(out[int(o) + 4:int(o) + 8], "little"))]


def kept_input(c):
    """the (corrected barcode, alignment bytes) of the records a case's map keeps, straight from the record tuples"""
    out = []
    for recs in c["chunks"]:
        for bc, alns in recs:
            if len(alns) == 1 and bc in c["corrections"]:
                ref, ty, start, fl = alns[0]
                out.append((c["corrections"][bc], int(ref).to_bytes(4, "little") + bytes([ty]) + int(start).to_bytes(4, "little") + int(fl).to_bytes(2, "little")))
    return out


# ------------------------------------------------------------------------------------------------------------------ widths
def widths_case(bc_bytes):
    """chunks of 133, 70, 1 and 0 records with na in 0, 1, 1, 1, 2, 3 over 24 barcodes, barcode 0 and the all-ones barcode of the
    width among them"""
    rng, A = random.Random(bc_bytes), Alns(bc_bytes)
    top = (1 << (8 * bc_bytes)) - 1
    pool = sorted({0, top} | {rng.randrange(top + 1) for _ in range(22)})
    chunks = [[(rng.choice(pool), A.many(rng.choice([0, 1, 1, 1, 2, 3]))) for _ in range(n)] for n in (133, 70, 1, 0)]
    return planned(chunks, bc_bytes, seed=bc_bytes)


def alignment_case(pad):
    rng, A = random.Random(pad), Alns(10 + pad)
    chunks = [[(rng.randrange(40), A.many(rng.choice([0, 1, 1, 2]))) for _ in range(n)] for n in (90, 3, 41)]
    return planned(chunks, 2, pad=pad, seed=pad)


# ------------------------------------------------------------------------------------------------------------------ tile edges
def fill(n_bytes, H):
    """na values of records of head H that tile exactly n_bytes, as many of them with one alignment as can be"""
    R = H + ALN
    for a in range(n_bytes // R, -1, -1):
        if (n_bytes - a * R) % H == 0:
            b = (n_bytes - a * R) // H
            nas = [1] * a + [0] * b
            random.Random(n_bytes).shuffle(nas)
            return nas
    raise ValueError((n_bytes, H))


def tile_edge_case(lim, delta, bc_bytes=1):
    """a kept record whose HEAD ends at the first tile's end + delta (-1, 0, +1: for 0 its alignment lies wholly in the halo, for +1
    the head's last byte does too); records behind it make a second tile.  -> (case, offset of that record in the chunk's payload)"""
    H, A = 4 + bc_bytes, Alns(20 + delta)
    q = lim["parse_tile"] + delta - H
    recs = [(i % 5, A.many(na)) for i, na in enumerate(fill(q, H))]
    recs.append((3, A.many(1)))
    recs += [(i % 5, A.many(i % 3)) for i in range(30)]
    return case([recs, [(4, A.many(1))]], {0: 0, 1: 1, 3: 3, 4: 3}, [3, 1, 0], bc_bytes), q


def halo_case(lim, bc_bytes=8):
    """the widest kept record starting on the tile's LAST byte: all of it but one byte lies in the halo, and it ends in the last
    dword of the staged bytes"""
    H, A = 4 + bc_bytes, Alns(30)
    q = lim["parse_tile"] - 1
    assert lim["parse_tile"] + lim["parse_halo"] - 4 < q + H + ALN <= lim["parse_tile"] + lim["parse_halo"]
    recs = [(i % 3, A.many(na)) for i, na in enumerate(fill(q, H))]
    recs += [(ONES, A.many(1)), (1, A.many(1)), (2, A.many(2)), (ONES, A.many(1))]
    return case([recs], {0: 0, 1: 1, ONES: ONES}, [ONES, 0, 1], bc_bytes), q


def one_tile_chunk_case(lim, extra):
    """a chunk whose records fill exactly one tile (extra 0) or one tile and a byte (extra 1: the last record began in the tile and
    ends on the halo's first byte); an nrec = 0 chunk and a one-record chunk behind it"""
    A = Alns(40 + extra)
    recs = [(i % 7, A.many(na)) for i, na in enumerate(fill(lim["parse_tile"] + extra, 4 + 2))]
    return planned([recs, [], [(3, A.many(1))]], 2, seed=extra)


def long_record_case(lim, tiles):
    """a multi-mapped record LONGER than `tiles` tiles, begun in the middle of a tile behind kept records and followed by kept records"""
    A = Alns(50 + tiles)
    na = tiles * lim["parse_tile"] // ALN + 1
    assert ALN * na > tiles * lim["parse_tile"]
    recs = [(i % 3, A.many(1)) for i in range(100)] + [(1, A.many(na)), (2, A.many(1)), (0, A.many(1)), (1, A.many(2)), (1, A.many(1))]
    return case([recs, [(0, A.many(na)), (2, A.many(1))]], {0: 0, 1: 1, 2: 1}, [1, 0], 4), na


def na_case():
    """na = 0, 1 and 2 side by side under one barcode"""
    A = Alns(60)
    return case([[(5, A.many(0)), (5, A.many(1)), (5, A.many(2)), (5, A.many(1)), (5, A.many(0))]], {5: 5}, [5], 4)


# ------------------------------------------------------------------------------------------------------------------ placement
def many_cells_case(n_cells, seed=3):
    """one record per cell, cells and records both in shuffled orders: the cell word takes one radix pass up to 255 cells, two up to
    65 535, three from 65 536 on (the dropped records' word is n_cells itself)"""
    rng, A = random.Random(seed + n_cells), Alns(n_cells)
    cells = [(i * 2654435761 + 11) % (1 << 32) for i in range(n_cells)]
    assert len(set(cells)) == n_cells
    recs = [(b, A.many(1)) for b in cells]
    rng.shuffle(recs)
    rng.shuffle(cells)
    third = max(1, len(recs) // 3)
    assert cells[0] ^ 1 not in set(cells)   # (a barcode that is not in the map)
    return case([recs[:third], recs[third:] + [(cells[0] ^ 1, A.many(1))]], {b: b for b in cells}, cells, 4)


EMPTY = ["first", "middle", "last", "every second", "all"]


def empty_cells_case(which):
    """nine cells of which `which` keep no record (their reads are unmapped, multi-mapped, or there are none)"""
    A = Alns(70)
    cells = list(range(100, 109))
    idle = {"first": {0}, "middle": {4}, "last": {8}, "every second": {1, 3, 5, 7}, "all": set(range(9))}[which]
    recs = []
    for rep in range(3):
        for i, b in enumerate(cells):
            recs.append((b, A.many(rep * 2 if i in idle else 1)))   # an idle cell's reads: na 0, 2, 4
    return case([recs[:10], recs[10:]], {b: b for b in cells}, cells, 2), sorted(idle)


def barcode_case():
    """8-byte barcodes: the all-ones barcode observed (corrected onto another cell) and as a CELL (another barcode is corrected onto
    it); self-corrections; thirty observed barcodes onto one cell; a barcode that is not in the map"""
    A = Alns(80)
    a, b = 0x1111111111111111, 0x8000000000000001
    crowd = [(7 << 56) | i for i in range(30)]
    corr = {a: a, b: b, ONES: b, a ^ 1: ONES, **{x: a for x in crowd}}
    recs = [(x, A.many(1)) for x in [a, ONES, b, a ^ 1, 0x55, ONES] + crowd + [a ^ 1, b]]
    random.Random(8).shuffle(recs)
    return case([recs[:11], recs[11:]], corr, [ONES, a, b], 8)


def chain_case(n_corr=16, n_chain=12, n_absent=4):
    """a correction table of n_corr entries (capacity 2 n_corr) in which n_chain observed barcodes share ONE home slot: the last of them
    is found after n_chain probes, and n_absent barcodes with that home that are NOT in the map are refused only at the chain's end.
    -> (case, the chain's barcodes, {barcode: (home, slot)})"""
    slot_fn = pkg.atac_sort_table_slot
    home = slot_fn(12345, n_corr)[0]
    found, _ = _with_home(slot_fn, n_corr, {home}, n_chain + n_absent, 1 << 40)
    chain, absent = found[:n_chain], found[n_chain:]
    others = [(1 << 50) + i for i in range(n_corr - n_chain)]
    obs = chain + others
    cells = [9000 + i for i in range(5)]
    corr = {b: cells[i % 5] for i, b in enumerate(obs)}
    where, cap = table_slots(obs, n_corr, slot_fn)
    A = Alns(90)
    recs = [(b, A.many(1)) for b in obs + absent + chain[::-1]]
    return case([recs], corr, cells, 8), chain, where


def skew_case(lim):
    """one cell holds all the records - more than a radix workgroup takes -, the other four none"""
    A = Alns(95)
    n = lim["radix_block"] + 300
    recs = [(7 + (i % 2), A.many(1)) for i in range(n)]
    return case([recs[:n // 2], recs[n // 2:]], {7: 42, 8: 42}, [40, 41, 42, 43, 44], 1)


def malformed_case(kind):
    """chunk 2 of four is broken: `head_cut` (the last record's head runs past the chunk), `alns_cut` (its alignments do), `junk` (an
    na of 2^31), `nrec_low` / `nrec_high` (the header's count is one off).  -> (bytes, off)"""
    A = Alns(99)
    chunks = [[(1, A.many(1)), (2, A.many(0))], [(1, A.many(2))], [(1, A.many(1)), (2, A.many(1)), (1, A.many(1))], [(2, A.many(1))]]
    data, off = rad.encode_atac_chunks(chunks, bc_bytes=4)
    b, o2 = bytearray(data), int(off[2])
    last = o2 + 8 + 2 * 19   # chunk 2's third record
    if kind == "head_cut":
        b[o2:o2 + 4] = (8 + 2 * 19 + 5).to_bytes(4, "little")     # nbytes ends inside the third record's head
    elif kind == "alns_cut":
        b[last:last + 4] = (2).to_bytes(4, "little")
    elif kind == "junk":
        b[last:last + 4] = (1 << 31).to_bytes(4, "little")
    elif kind == "nrec_low":
        b[o2 + 4:o2 + 8] = (2).to_bytes(4, "little")
    elif kind == "nrec_high":
        b[o2 + 4:o2 + 8] = (4).to_bytes(4, "little")
    else:
        raise ValueError(kind)
    return bytes(b), off
