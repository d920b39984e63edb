"""Case builders for the multi-barcode collate tests: inputs of afq_collate_multi_rad (chunks of an uncollated two-barcode RNA RAD, a
sample table, a cell table, the cells in output order), each at the smallest shape at which the kernels can go wrong.
tests/test_collate_multi_cases_cpu.py shows without a device that every case reaches the edge it names; tests/test_gpu_collate_multi.py
runs them against tests/collate_multi_judge.py.  A case is a dict: chunks (records (b0, b1, umi, [(ref, fw), ...])), data / off (the
bytes), b0_bytes, b1_bytes, umi_bytes, pos_bytes, sample_table {observed b0: sample}, cell_table {(sample, observed b1): corrected},
cells [(sample, barcode)] in output order, b0_out {sample: value written into b0}, n_samples."""
import random

import numpy as np

import collate_cases as CC
import collate_multi_judge as J
import gpl_cases as G
import gpl_multi_cases as MC
from util import pkg

B_WIDTHS = MC.B_WIDTHS
U_WIDTHS = MC.U_WIDTHS
ORIS = ["both", "fw", "rc"]
top = MC.top


def encode(chunks, b0_bytes, b1_bytes, umi_bytes, pos_bytes=0, pad=0):
    """rad.encode_multi_bc_chunks with NON-ZERO position bytes that differ from alignment to alignment, behind `pad` bytes of 0xEE"""
    out, offs, ctr = bytearray(b"\xEE" * pad), [], 0
    for recs in chunks:
        offs.append(len(out))
        body = bytearray()
        for b0, b1, umi, alns in recs:
            body += len(alns).to_bytes(4, "little") + int(b0).to_bytes(b0_bytes, "little") + int(b1).to_bytes(b1_bytes, "little") + int(umi).to_bytes(umi_bytes, "little")
            if pos_bytes == 0 and len(alns) > 64:
                a = np.asarray(alns, dtype=np.int64).reshape(-1, 2)
                body += ((a[:, 0] & 0x7FFFFFFF) | (a[:, 1].astype(bool).astype(np.int64) << 31)).astype("<u4").tobytes()
                continue
            for ref, fw in alns:
                body += ((int(ref) & 0x7FFFFFFF) | (0x80000000 if fw else 0)).to_bytes(4, "little")
                if pos_bytes:
                    body += CC.position(ctr, pos_bytes)
                ctr += 1
        out += (len(body) + 8).to_bytes(4, "little") + len(recs).to_bytes(4, "little") + body
    return bytes(out), np.asarray(offs, dtype=np.uint64)


def ordinals(cells):
    """the dense ordinals of the samples that have a cell, in sample order"""
    return {s: i for i, s in enumerate(sorted({s for s, _ in cells}))}


def case(chunks, sample_table, cell_table, cells, n_samples, b0_bytes=2, b1_bytes=4, umi_bytes=4, pos_bytes=0, pad=0, b0_out=None):
    data, off = encode(chunks, b0_bytes, b1_bytes, umi_bytes, pos_bytes, pad)
    return {"chunks": chunks, "data": data, "off": off, "b0_bytes": b0_bytes, "b1_bytes": b1_bytes, "umi_bytes": umi_bytes, "pos_bytes": pos_bytes,
            "sample_table": dict(sample_table), "cell_table": dict(cell_table), "cells": list(cells), "n_samples": n_samples,
            "b0_out": dict(ordinals(cells) if b0_out is None else b0_out)}


def want(c, ori, lane_alns=None):
    return J.collate_multi(c["data"], c["off"], c["b0_bytes"], c["b1_bytes"], c["umi_bytes"], ori, c["sample_table"], c["cell_table"], c["cells"], c["b0_out"],
                           c["pos_bytes"], lane_alns)


def args(c):
    """the arrays of Quantifier.collate_multi_rad, in its argument order after chunk_off"""
    so = sorted(c["sample_table"])
    ck = sorted(c["cell_table"])
    b0o = [c["b0_out"].get(s, 0) for s in range(c["n_samples"])]
    return (so, [c["sample_table"][b] for b in so], [s for s, _ in ck], [b for _, b in ck], [c["cell_table"][k] for k in ck], [s for s, _ in c["cells"]],
            [b for _, b in c["cells"]], b0o)


def plan_for(chunks, entries, rng, b1_bytes):
    """tables over what the chunks carry.  Entry i of the sorted routing entries routes to sample n - 1 - i of n = len(entries) + 2
    samples: sample 0 and sample 1 receive nothing; sample 1 has two cells all the same (header-only chunks), sample 0 has none
    (the ordinals skip it, so a written ordinal is below its sample index).  Per (sample, b1): about a sixth have
    no correction, half of the rest are cells mapped onto themselves, the others are corrected onto a cell of their sample."""
    entries = sorted(entries)
    n = len(entries) + 2
    sample_table = {b: n - 1 - i for i, b in enumerate(entries)}
    seen = {}
    for recs in chunks:
        for b0, b1, _, _ in recs:
            if b0 in sample_table:
                seen.setdefault(sample_table[b0], set()).add(b1)
    cell_table, cells = {}, [(1, 5 % (top(b1_bytes) + 1)), (1, top(b1_bytes))]
    for s in sorted(seen):
        b1s = sorted(seen[s])
        own = [b for i, b in enumerate(b1s) if i % 2 == 0]
        cells += [(s, b) for b in own]
        for b in own:
            cell_table[(s, b)] = b
        for i, b in enumerate(x for x in b1s if x not in own):
            if i % 3 != 2:
                cell_table[(s, b)] = rng.choice(own)
    rng.shuffle(cells)
    return sample_table, cell_table, cells, n


def planned(mc, seed=0, pad=0, pos_bytes=None):
    """a gpl_multi_cases parse case (its chunks and routing entries) with tables over them"""
    pb = mc["pos_bytes"] if pos_bytes is None else pos_bytes
    st, ct, cells, n = plan_for(mc["chunks"], mc["entries"], random.Random(seed), mc["b1_bytes"])
    return case(mc["chunks"], st, ct, cells, n, mc["b0_bytes"], mc["b1_bytes"], mc["umi_bytes"], pb, pad)


def record_spans(out, chunk_off, c):
    """(start, end) byte offsets of every record of a collated output"""
    H, A = 4 + c["b0_bytes"] + c["b1_bytes"] + c["umi_bytes"], 4 + c["pos_bytes"]
    spans = []
    for o in chunk_off[:-1]:
        o = int(o)
        p = o + 8
        for _ in range(int.from_bytes(out[o + 4:o + 8], "little")):
            n = H + A * int.from_bytes(out[p:p + 4], "little")
            spans.append((p, p + n))
            p += n
    return spans


# ------------------------------------------------------------------------------------------------------------------ widths, edges
def widths_case(b0_bytes, b1_bytes, umi_bytes):
    """MC.widths_case's chunks (three chunks of about 40 records, na 0..5, every orientation mix, b0 and b1 of 0 and all-ones)"""
    return planned(MC.widths_case(b0_bytes, b1_bytes, umi_bytes), seed=b0_bytes * 64 + b1_bytes * 8 + umi_bytes)


def alignment_case(pad):
    """the first chunk at byte alignment `pad`; records of 7 + 4 na bytes put later chunks, tiles and output records at every alignment"""
    return planned(MC.alignment_case(pad), seed=pad, pad=pad)


def tile_edge_case(lim, delta):
    """MC.tile_edge_case: the first tile's records end at its end (0), a byte before it (-1: the next record starts on the tile's last
    byte) or a byte behind it (+1).  Returns (case, index of the first record behind the filled bytes)."""
    mc, at = MC.tile_edge_case(lim, delta)
    return planned(mc, seed=delta + 5), at


def one_tile_chunk_case(lim):
    """a chunk whose records fill exactly one tile (heads of 4 + 1 + 2 + 1 bytes, alignments of 4); a one-record chunk behind it"""
    rng = random.Random(61)
    nas = G.fill_nas(lim["parse_tile"], 8, 4)
    recs = [MC.rand_record(rng, [3, 4, 9], 2, 1, na) for na in nas]
    return planned(MC.multi_case([recs, [(3, 1, 1, [(1, True)])]], [3, 9], 1, 2, 1), seed=2)


def halo_case(lim, na):
    """MC.halo_case: the widest record (4-byte b0 and b1, 8-byte UMI, 8 position bytes) on the tile's last four bytes with `na`
    alignments of which only the last is forward; it is kept.  Returns (case, index of that record)."""
    mc, at = MC.halo_case(lim, na)
    c = planned(mc, seed=na, pos_bytes=8)
    s = c["sample_table"][0xFFFFFFFF]
    if (s, 0xFFFFFFFF) not in c["cells"]:
        c["cells"].append((s, 0xFFFFFFFF))
    c["cell_table"][(s, 0xFFFFFFFF)] = 0xFFFFFFFF
    c["b0_out"] = ordinals(c["cells"])
    return c, at


def long_case(where):
    """MC.long_case (records of 2 500 and 3 000 alignments; the only forward word first, last or absent): b0 = 12 is sample 2, and of
    its long records b1 = 2 is kept, b1 = 4 is reverse-only (dropped under fw), b1 = 8 has no correction; the long record of b0 = 99 has
    no sample.  Under fw with where = "last" the only fitting word of the kept record lies beyond the first 64-lane trip."""
    mc = MC.long_case(where)
    st = {11: 3, 12: 2, 16: 1}
    ct = {(3, 1): 1, (2, 0): 2, (2, 2): 2, (2, 4): 2, (1, 7): 7}
    return case(mc["chunks"], st, ct, [(1, 7), (2, 2), (3, 1)], 4, mc["b0_bytes"], mc["b1_bytes"], mc["umi_bytes"])


def no_alignment_case():
    """records without an alignment beside records with one: kept under both, dropped under fw / rc"""
    return planned(MC.no_alignment_case(), seed=3)


# ------------------------------------------------------------------------------------------------------------------ routes
ROUTE_FATES = ("kept", "corrected", "unrouted", "uncorrected")


def route_case(lim, pos_bytes=4, b0_bytes=2, b1_bytes=4, umi_bytes=2):
    """CC.route_case over the head na, b0, b1, umi: every na of CC.route_nas with orientation bits such that all, none, only the word
    at index 0 / 63 / 64 / last, and all but that word fit; the UMI numbers the records.  Record k takes fate k % 4 of ROUTE_FATES:
    kept (b0 = 40 is sample 2, b1 = 10 its cell), corrected onto another cell of its sample (b1 = 12 -> 11), unrouted (b0 = 41 has no
    sample), uncorrected (b1 = 13 has no correction in sample 2).  Three chunks, the middle one a single record; the position bytes
    are non-zero and differ from alignment to alignment.  Sample 1 has a cell and no record."""
    recs, k = [], 0
    for na in CC.route_nas(lim):
        pats = [[True] * na, [False] * na]
        for only in sorted({0, 63, 64, na - 1}):
            if 0 <= only < na:
                pats.append([j == only for j in range(na)])
                pats.append([j != only for j in range(na)])
        for pat in pats:
            b0, b1 = [(40, 10), (40, 12), (41, 10), (40, 13)][k % 4]
            recs.append((b0, b1, k, [(100 + j, fw) for j, fw in enumerate(pat)]))
            k += 1
    cuts = [0, len(recs) // 3, len(recs) // 3 + 1, len(recs)]
    chunks = [recs[a:b] for a, b in zip(cuts, cuts[1:])]
    return case(chunks, {40: 2, 43: 1}, {(2, 10): 10, (2, 11): 11, (2, 12): 11, (1, 10): 10}, [(2, 11), (1, 10), (2, 10)], 3, b0_bytes, b1_bytes, umi_bytes, pos_bytes)


# ------------------------------------------------------------------------------------------------------------------ the lookup
def lookup_case():
    """5 samples, 4-byte fields.  b1 = 0x77 is observed in samples 1 and 4 and corrected to DIFFERENT cells; the barcode 0xC0FFEE is a
    cell of samples 1 and 4; b0 = 900 has no sample; b1 = 0x99 is corrected in sample 4 only and observed in sample 1; b1 = all ones is
    a key in sample 0 and in sample 4 (the highest); no b0 equals its sample index or its ordinal; sample 2 has cells and no record;
    sample 3 has no cell, so the ordinals are 0, 1, 2, 3 for samples 0, 1, 2, 4."""
    ones = 0xFFFFFFFF
    st = {500: 0, 501: 1, 7: 1, 502: 2, 503: 3, 0: 4, ones: 4}
    ct = {(1, 0x77): 0xA1, (4, 0x77): 0xC0FFEE, (1, 0xC0FFEE): 0xC0FFEE, (4, 0x99): 0xB4, (0, ones): ones, (4, ones): 0xB4, (1, 0xA1): 0xA1, (2, 5): 5}
    cells = [(0, ones), (1, 0xA1), (1, 0xC0FFEE), (2, 5), (2, 6), (4, 0xB4), (4, 0xC0FFEE)]
    f, r = [(1, True)], [(2, False), (3, True)]
    chunks = [[(501, 0x77, 1, f), (0, 0x77, 2, r), (900, 0x77, 3, f), (7, 0x99, 4, f), (ones, 0x99, 5, r), (500, ones, 6, f)],
              [(0, ones, 7, r), (501, 0xC0FFEE, 8, f), (503, 5, 9, f), (ones, 0x77, 10, f), (7, 0xA1, 11, r), (500, 0x77, 12, f)]]
    return case(chunks, st, ct, cells, 5, 4, 4, 4)


def keys_homing_at(slot, n_keys, count, make, seed=5, exclude=()):
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        v = rng.randrange(1 << 32)
        if v not in exclude and v not in out and pkg.atac_sort_table_slot(make(v), n_keys)[0] == slot:
            out.append(v)
    return sorted(out)


def chain_case(n_entries=48, n_corr=40, chain=5):
    """probe chains that wrap the end of BOTH tables.  `chain` sample barcodes home at the LAST slot of the sample table of n_entries,
    and two more values with that home are no entries (their lookup walks the chain into slot 0 and on to a free slot).  In sample 3,
    `chain` cell barcodes have keys 3 << 32 | b1 that home at the last slot of the cell table of n_corr corrections, and two more
    with that home have no correction.  Returns (case, the chained b0s, the b0 misses, the chained b1s, the b1 misses)."""
    scap = pkg.atac_sort_table_slot(0, n_entries)[1]
    ccap = pkg.atac_sort_table_slot(0, n_corr)[1]
    b0s = keys_homing_at(scap - 1, n_entries, chain + 2, lambda v: v)
    b0_chain, b0_miss = b0s[:chain], b0s[chain:]
    b1s = keys_homing_at(ccap - 1, n_corr, chain + 2, lambda v: (3 << 32) | v, seed=6)
    b1_chain, b1_miss = b1s[:chain], b1s[chain:]
    rng = random.Random(8)
    st = {b: 3 for b in b0_chain}
    while len(st) < n_entries:
        b = rng.randrange(1 << 32)
        if b not in b0s:
            st[b] = rng.choice([1, 2, 4])
    ct = {(3, b): b1_chain[0] for b in b1_chain}
    cells = [(3, b1_chain[0]), (1, 9), (2, 9), (4, 9)]
    while len(ct) < n_corr:
        s, b = rng.choice([1, 2, 4]), rng.randrange(1 << 32)
        ct[(s, b)] = 9
    recs = [(b0, b1, i, [(1, True)]) for i, (b0, b1) in enumerate([(x, y) for x in b0_chain + b0_miss for y in b1_chain[:2] + b1_miss[:1]] +
                                                                  [(b0_chain[-1], y) for y in b1_chain + b1_miss])]
    others = [(b, s) for b, s in sorted(st.items()) if s != 3][:6]
    keys = sorted(k for k in ct if k[0] != 3)
    recs += [(b, next(k[1] for k in keys if k[0] == s), 0, [(2, True)]) for b, s in others]
    rng.shuffle(recs)
    return case([recs[:17], recs[17:]], st, ct, cells, 5, 4, 4, 1), b0_chain, b0_miss, b1_chain, b1_miss


# ------------------------------------------------------------------------------------------------------------------ placement
def many_cells_case(n_cells, n_records=600, seed=3):
    """n_cells cells over three samples and n_records records that reach the first cell, the last cell and cells between them, a few per
    cell; cells and records in shuffled orders.  n_cells 255, 256 (one radix digit - the dropped records' word n_cells takes a second
    at 256), 257 (two), 65 537 (three)."""
    rng = random.Random(seed + n_cells)
    cells = [(1 + i % 3, (i * 2654435761 + 11) % (1 << 32)) for i in range(n_cells)]
    assert len(set(cells)) == n_cells
    rng.shuffle(cells)
    hit = sorted({0, n_cells - 1, n_cells // 2} | {rng.randrange(n_cells) for _ in range(min(n_cells, n_records // 3))})
    st = {1000 + s: s for s in (1, 2, 3)}
    ct = {cells[j]: cells[j][1] for j in hit}
    recs = [(1000 + cells[j][0], cells[j][1], i & 0xFFFF, [(i & 0xFFFF, True)]) for i, j in enumerate(hit * 3)][:max(n_records, 9)]
    recs.append((1000 + 1, 12345, 0, [(1, True)]))   # (no correction: it sorts behind every cell)
    rng.shuffle(recs)
    third = max(1, len(recs) // 3)
    return case([recs[:third], recs[third:]], st, ct, cells, 4, 2, 4, 2), hit


def interleave_case():
    """the records of cell (1, 7) spread over three input chunks between those of two other cells: their order in its chunk is the
    input's (the UMIs number them)"""
    def rec(b0, b1, umi):
        return (b0, b1, umi, [(umi, umi % 2 == 0)] * (1 + umi % 3))
    chunks = [[rec(21, 7, 0), rec(22, 7, 1), rec(21, 7, 2), rec(21, 9, 3), rec(21, 7, 4)], [rec(21, 9, 5), rec(21, 7, 6), rec(22, 7, 7)],
              [rec(21, 7, 8), rec(21, 7, 9), rec(22, 7, 10), rec(21, 9, 11), rec(21, 7, 12)]]
    return case(chunks, {21: 1, 22: 2}, {(1, 7): 7, (2, 7): 7, (1, 9): 9}, [(1, 9), (1, 7), (2, 7)], 3)


def big_cell_case(lim):
    """one cell takes every record, and more of them than a radix workgroup takes; a second cell stays empty"""
    n = lim["radix_block"] + 100
    recs = [(5, i % 7, i, [(i, True)] * (i % 3)) for i in range(n)]
    cut = lim["radix_block"] - 7
    return case([recs[:cut], recs[cut:]], {5: 1}, {(1, b): 3 for b in range(7)}, [(1, 3), (1, 4)], 2, 1, 1, 4)


# ------------------------------------------------------------------------------------------------------------------ malformed
MALFORMED_KINDS = ("head_cut", "alns_cut", "nrec_low", "nrec_high")


def malformed_case(kind):
    """MC.malformed_case: four chunks of which chunk 2 is malformed, read as records of 2-byte b0 and b1 and a 4-byte UMI.
    head_cut: a head past the chunk; alns_cut: alignments past the chunk; nrec_low: more records than the header says; nrec_high:
    fewer.  Returns (data, off)."""
    return MC.malformed_case(kind)
