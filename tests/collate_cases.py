"""Case builders for the collate tests: inputs of afq_collate_rad (chunks of an uncollated RNA RAD, a correction map, the cells in
output order), each at the smallest shape at which the kernels can go wrong.  A case is a dict: data / off (the bytes), bc_bytes,
umi_bytes, pos_bytes, corrections {observed: corrected}, cells [barcode, ...].  Records are (bc, umi, [(ref, fw), ...]) as in
tests/gpl_cases.py; the encoder here writes NON-ZERO position bytes that differ from alignment to alignment, so that a kept
alignment can be told from a dropped one."""
import random

import numpy as np

import collate_judge as J
import gpl_cases as G

WIDTHS = [1, 2, 4, 8]
ORIS = ["both", "fw", "rc"]
ONES = 0xFFFFFFFFFFFFFFFF


def position(counter, pos_bytes):
    """the position bytes of the counter-th alignment of a file: non-zero, and distinct as far as the width allows"""
    v = ((counter + 1) * 0x9E3779B97F4A7C15) & ((1 << (8 * pos_bytes)) - 1)
    return (v or 1).to_bytes(pos_bytes, "little")


def encode(chunks, bc_bytes=4, umi_bytes=4, pos_bytes=0, pad=0):
    out, offs, ctr = bytearray(b"\xEE" * pad), [], 0
    for recs in chunks:
        offs.append(len(out))
        body = bytearray()
        for bc, umi, alns in recs:
            body += len(alns).to_bytes(4, "little") + int(bc).to_bytes(bc_bytes, "little") + int(umi).to_bytes(umi_bytes, "little")
            for ref, fw in alns:
                body += ((int(ref) & 0x7FFFFFFF) | (0x80000000 if fw else 0)).to_bytes(4, "little")
                if pos_bytes:
                    body += position(ctr, pos_bytes)
                ctr += 1
        out += (len(body) + 8).to_bytes(4, "little") + len(recs).to_bytes(4, "little") + body
    return bytes(out), np.asarray(offs, dtype=np.uint64)


def case(chunks, corrections, cells, bc_bytes=4, umi_bytes=4, pos_bytes=0, pad=0):
    data, off = encode(chunks, bc_bytes, umi_bytes, pos_bytes, pad)
    return {"chunks": chunks, "data": data, "off": off, "bc_bytes": bc_bytes, "umi_bytes": umi_bytes, "pos_bytes": pos_bytes,
            "corrections": dict(corrections), "cells": list(cells)}


def want(c, ori, lane_alns=None):
    return J.collate(c["data"], c["off"], c["bc_bytes"], c["umi_bytes"], c["pos_bytes"], ori, c["corrections"], c["cells"], lane_alns)


def plan_for(chunks, rng, extra_cell=None):
    """a correction map over the barcodes the chunks carry: about half of them are cells (mapped onto themselves), a third of the
    others are corrected onto a cell, the rest are not in the map; the cells in a shuffled order, `extra_cell` (never observed, so
    its chunk stays empty) among them"""
    bcs = sorted({r[0] for recs in chunks for r in recs})
    cells = [b for i, b in enumerate(bcs) if i % 2 == 0] or bcs[:1]
    corr = {b: b for b in cells}
    for i, b in enumerate(x for x in bcs if x not in corr):
        if i % 3 == 0 and cells:
            corr[b] = rng.choice(cells)
    if extra_cell is not None and extra_cell not in corr:
        cells.append(extra_cell)
    rng.shuffle(cells)
    return corr, cells


def planned(chunks, bc_bytes, umi_bytes, pos_bytes, pad=0, seed=0, extra_cell=None):
    corr, cells = plan_for(chunks, random.Random(seed), extra_cell)
    return case(chunks, corr, cells, bc_bytes, umi_bytes, pos_bytes, pad)


# ------------------------------------------------------------------------------------------------------------------ widths
def widths_case(bc_bytes, umi_bytes, pos_bytes):
    """the GPL width case's chunks (133, 70, 1 and 0 records of na 0..5, every orientation mix, barcode 0 and the all-ones barcode
    of the width) with a plan over their barcodes"""
    return planned(G.widths_case(bc_bytes, umi_bytes, pos_bytes)["chunks"], bc_bytes, umi_bytes, pos_bytes, seed=bc_bytes * 8 + umi_bytes)


def record_spans(out, chunk_off, bc_bytes, umi_bytes, pos_bytes):
    """(start, end) byte offsets of every record of a collated output"""
    H, A = 4 + bc_bytes + umi_bytes, 4 + pos_bytes
    spans = []
    for o in chunk_off[:-1]:
        o = int(o)
        nrec = int.from_bytes(out[o + 4:o + 8], "little")
        p = o + 8
        for _ in range(nrec):
            n = H + A * int.from_bytes(out[p:p + 4], "little")
            spans.append((p, p + n))
            p += n
    return spans


# ------------------------------------------------------------------------------------------------------------------ tile edges
def alignment_case(pad):
    return planned(G.alignment_case(pad)["chunks"], 1, 2, 0, pad=pad, seed=pad)


def tile_edge_case(lim, delta):
    """G.tile_edge_case: the first tile's records end at its end (0), a byte before it (-1: the next record starts on the tile's
    last byte) or a byte behind it (+1); a second tile follows"""
    c, _ = G.tile_edge_case(lim, delta)
    return planned(c["chunks"], c["bc_bytes"], c["umi_bytes"], 0, seed=delta + 5)


def one_tile_chunk_case(lim, extra):
    """a chunk whose records fill exactly one tile (extra 0) or one tile and a byte (extra 1: the last record ends in the halo);
    heads of 7 bytes, alignments of 5; a one-record chunk behind it"""
    rng = random.Random(60 + extra)
    nas = G.fill_nas(lim["parse_tile"] + extra, 7, 5)
    recs = [G.rand_record(rng, 2, 1, na) for na in nas]
    return planned([recs, [(3, 1, [(1, True)])]], 2, 1, 1, seed=extra)


def halo_case(lim, na):
    """G.halo_case: the widest record on the tile's last four bytes with `na` alignments of which only the last is forward"""
    c, _ = G.halo_case(lim, na)
    corr, cells = plan_for(c["chunks"], random.Random(na))
    corr[ONES] = ONES   # the record in question is kept
    if ONES not in cells:
        cells.append(ONES)
    return case(c["chunks"], corr, cells, 8, 8, 8)


# ------------------------------------------------------------------------------------------------------------------ routes
def route_nas(lim):
    L = lim["lane_alns"]
    return [0, 1, L, L + 1, 64, 65, 129]


def route_case(lim, pos_bytes=4, bc_bytes=4, umi_bytes=2):
    """every na of route_nas with orientation bits such that the number of fitting words is 0, 1, na - 1 and na, the only fitting
    word at index 0, 63, 64 and last; two cells and a barcode corrected onto one of them take the records in turn, a fourth
    barcode is not in the map"""
    recs, k = [], 0
    for na in route_nas(lim):
        pats = [[True] * na, [False] * na]
        for only in sorted({0, 63, 64, na - 1}):
            if 0 <= only < na:
                pats.append([j == only for j in range(na)])
                pats.append([j != only for j in range(na)])
        for pat in pats:
            recs.append(((k % 4) + 10, k, [(100 + j, fw) for j, fw in enumerate(pat)]))
            k += 1
    cuts = [0, len(recs) // 3, len(recs) // 3 + 1, len(recs)]
    chunks = [recs[a:b] for a, b in zip(cuts, cuts[1:])]
    return case(chunks, {10: 10, 11: 11, 12: 11}, [11, 10], bc_bytes, umi_bytes, pos_bytes)


# ------------------------------------------------------------------------------------------------------------------ placement
def interleave_case():
    """cell 7's records spread over three input chunks between those of cells 8 and 9: their order in cell 7's chunk is the input's
    (the UMIs number them)"""
    def rec(bc, umi):
        return (bc, umi, [(umi, umi % 2 == 0)] * (1 + umi % 3))
    chunks = [[rec(7, 0), rec(8, 1), rec(7, 2), rec(9, 3), rec(7, 4)], [rec(9, 5), rec(7, 6), rec(8, 7)], [rec(7, 8), rec(7, 9), rec(8, 10), rec(9, 11), rec(7, 12)]]
    return case(chunks, {7: 7, 8: 8, 9: 9}, [9, 7, 8], 4, 4, 0)


def many_cells_case(n_cells, seed=3):
    """one record per cell, cells and records both in shuffled orders: n_cells 1, 2 (one radix digit), 256, 257 (two), 65 537 (three)"""
    rng = random.Random(seed + n_cells)
    cells = [(i * 2654435761 + 11) % (1 << 32) for i in range(n_cells)]
    assert len(set(cells)) == n_cells
    recs = [(b, i & 0xFFFF, [(i & 0xFFFF, True)]) for i, b in enumerate(cells)]
    rng.shuffle(recs)
    rng.shuffle(cells)
    third = max(1, len(recs) // 3)
    return case([recs[:third], recs[third:]], {b: b for b in cells}, cells, 4, 2, 0)


def big_cell_case(lim):
    """one cell with more records than a radix workgroup takes, between the records of two small cells"""
    n = lim["radix_block"] + 100
    recs = []
    for i in range(n):
        recs.append((5, i, [(i, True)] * (i % 3)))
        if i % 50 == 0:
            recs.append((6 + (i // 50) % 2, i, [(1, False)]))
    cut = lim["radix_block"] - 7
    return case([recs[:cut], recs[cut:]], {5: 5, 6: 6, 7: 7}, [6, 5, 7], 4, 4, 0)


def corrected_case():
    """8-byte barcodes: a cell with no record (its chunk is a header), an observed barcode corrected onto ANOTHER cell, the all-ones
    barcode as an observed key, a barcode that is not in the map"""
    a, b, empty = 0x1111111111111111, 0x2222222222222222, 0x3333333333333333
    chunks = [[(a, 1, [(1, True)]), (ONES, 2, [(2, False), (3, True)]), (0x55, 3, [(4, True)]), (a ^ 1, 4, [(5, True)])], [(ONES, 5, []), (b, 6, [(6, True)])]]
    return case(chunks, {a: a, b: b, ONES: b, a ^ 1: a, empty: empty}, [empty, b, a], 8, 4, 2)


# ------------------------------------------------------------------------------------------------------------------ whole command
def cells_and_corrections(permit_freq, permit_map):
    """what `afquant collate` derives from a GPL output directory: the cells in output order, the map"""
    return J.cell_order(permit_freq), dict(permit_map)
