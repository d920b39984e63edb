"""A seeded combination sweep of the seven record passes (gpl, gpl multi, atac gpl, atac sort, collate, collate multi, atac collate):
`draw(family, seed, lim)` returns a case of the family's own shape, built with the family's existing encoder and case() / plan_for()
helpers and judged by its existing judge (`want`).  The hand-built cases of the families move one dimension at a time; a draw moves
them together: field widths, position bytes, 0..3 pad bytes, 1..6 chunks of 0 records to three and a half tiles (one may be empty
between the others), na mostly 0..5 with about 5 % around lane_alns and 1 % in [60, 200] (the ATAC families: their own 0 / 1 / 2 /
5), orientation bits at random, barcodes from a pool of twelve that holds 0 and the width's all-ones value, a fifth of the records
on barcodes that the tables do not hold.  tests/test_rad_pass_sweep_cpu.py shows what the fixed seeds reach together;
tests/test_gpu_rad_pass_sweep.py runs every family x seed x orientation.

The slowest want() over a family's eight draws and orientations, measured on the CPU these tests were written on (a 4096-byte tile:
a draw holds at most 86 kB of records, the fixed ones at most 32 kB): gpl 0.001 s, gpl multi 0.001 s, atac gpl 0.001 s, atac sort
0.001 s, collate 0.003 s, collate multi 0.003 s, atac collate 0.001 s; the seven families' 56 draws together take 0.4 s."""
import random

import numpy as np

import atac_collate_cases as AC
import atac_gpl_cases as AG
import atac_sort_cases as AS
import collate_cases as CC
import collate_multi_cases as CM
import gpl_cases as G
import gpl_multi_cases as MC
from util import pkg

FAMILIES = ("gpl", "gpl multi", "atac gpl", "atac sort", "collate", "collate multi", "atac collate")
LIMITS = {"gpl": pkg.gpl_limits, "gpl multi": pkg.gpl_multi_limits, "atac gpl": pkg.atac_gpl_limits, "atac sort": pkg.atac_sort_limits,
          "collate": pkg.collate_limits, "collate multi": pkg.collate_multi_limits, "atac collate": pkg.atac_collate_limits}
RNA = ("gpl", "gpl multi", "collate", "collate multi")
ORIS = {f: (tuple(G.ORIS) if f in RNA else (None,)) for f in FAMILIES}
# the position bytes the family's hand-built cases already use
POS_BYTES = {"gpl": (0, 4, 8), "gpl multi": (0, 4, 8), "collate": (0, 1, 4, 8), "collate multi": (0, 1, 2, 4, 8)}
ATAC_WIDTHS = (1, 2, 4, 8)
ATAC_NAS = (0, 1, 1, 1, 2, 5)
REF_LEN = [250001, 900, 99993]
# eight seeds a family; tests/test_rad_pass_sweep_cpu.py shows what their union reaches (change the seeds, not the witnesses)
SEEDS = {"gpl": (2, 4, 28, 29, 49, 55, 68, 70), "gpl multi": (2, 4, 28, 29, 49, 55, 68, 70), "atac gpl": (2, 4, 28, 29, 49, 55, 68, 70),
         "atac sort": (12, 14, 21, 23, 34, 47, 48, 57), "collate": (2, 4, 28, 29, 49, 55, 68, 70), "collate multi": (14, 25, 27, 33, 34, 53, 54, 56),
         "atac collate": (9, 16, 18, 33, 42, 58, 61, 64)}


def _pool(rng, width, n=12):
    """(the barcodes the tables are planned over, the strangers they never hold): twelve values of the width, 0 and all-ones among them"""
    top = (1 << (8 * width)) - 1
    vals = {0, top}
    while len(vals) < n:
        vals.add(rng.randrange(top + 1))
    vals = sorted(vals)
    rng.shuffle(vals)
    return vals[n // 5:], vals[:n // 5]


def _barcode(rng, inside, strangers):
    return rng.choice(strangers) if rng.random() < 0.2 else rng.choice(inside)


def _na(rng, L):
    r = rng.random()
    if r < 0.01:
        return rng.randrange(60, 201)
    if r < 0.06:
        return rng.randrange(L - 1, L + 3)
    return rng.randrange(0, 6)


def _rna_alns(rng, na):
    p = rng.choice([0.0, 0.5, 0.5, 1.0])
    return [(rng.randrange(1 << 20), rng.random() < p) for _ in range(na)]


def _chunks(rng, tile, record, size_of):
    """1..6 chunks; one of the inner ones may be empty; the others hold records up to a drawn size between a few bytes and three
    and a half tiles"""
    n = rng.randrange(1, 7)
    empty = rng.randrange(1, n - 1) if n >= 3 and rng.random() < 0.6 else None
    chunks = []
    for i in range(n):
        recs, size = [], 0
        target = 0 if i == empty else (rng.randrange(1, 3 * tile + tile // 2) if rng.random() < 0.6 else rng.randrange(1, 300))
        while size < target:
            r = record()
            recs.append(r)
            size += size_of(r)
        chunks.append(recs)
    return chunks


def _without(chunks, strangers):
    return [[r for r in recs if r[0] not in strangers] for recs in chunks]


def draw(family, seed, lim):
    rng = random.Random(seed * 7919 + FAMILIES.index(family))
    tile = lim["parse_tile"]
    pad = rng.randrange(4)
    if family in ("gpl", "collate"):
        bw, uw, pb = rng.choice(G.WIDTHS), rng.choice(G.WIDTHS), rng.choice(POS_BYTES[family])
        inside, strangers = _pool(rng, bw)
        chunks = _chunks(rng, tile, lambda: (_barcode(rng, inside, strangers), rng.randrange(1 << (8 * uw)), _rna_alns(rng, _na(rng, lim["lane_alns"]))),
                         lambda r: G.rec_size(len(r[2]), bw, uw, pb))
        if family == "gpl":
            return G.parse_case(chunks, bw, uw, pb, pad)
        corr, cells = CC.plan_for(_without(chunks, strangers), random.Random(seed))
        return CC.case(chunks, corr, cells, bw, uw, pb, pad)
    if family in ("gpl multi", "collate multi"):
        b0w, b1w, uw, pb = rng.choice(MC.B_WIDTHS), rng.choice(MC.B_WIDTHS), rng.choice(MC.U_WIDTHS), rng.choice(POS_BYTES[family])
        entries, unrouted = _pool(rng, b0w, 8)
        b1s = sum(_pool(rng, b1w), [])
        H = 4 + b0w + b1w + uw
        chunks = _chunks(rng, tile, lambda: (_barcode(rng, entries, unrouted), rng.choice(b1s), rng.randrange(1 << (8 * uw)), _rna_alns(rng, _na(rng, lim["lane_alns"]))),
                         lambda r: MC.rec_size(len(r[3]), H, pb))
        if family == "gpl multi":
            return MC.multi_case(chunks, entries, b0w, b1w, uw, pb, pad)
        st, ct, cells, n = CM.plan_for(chunks, entries, random.Random(seed), b1w)
        return CM.case(chunks, st, ct, cells, n, b0w, b1w, uw, pb, pad)
    bw = rng.choice(ATAC_WIDTHS)
    inside, strangers = _pool(rng, bw)
    if family == "atac collate":
        alns = AC.Alns(seed)
        chunks = _chunks(rng, tile, lambda: (_barcode(rng, inside, strangers), alns.many(rng.choice(ATAC_NAS))), lambda r: 4 + bw + AC.ALN * len(r[1]))
        corr, cells = AC.plan_for(_without(chunks, strangers), random.Random(seed))
        return AC.case(chunks, corr, cells, bw, pad)

    def aln():
        r = rng.randrange(len(REF_LEN))
        return (r, rng.randrange(1, 5), rng.randrange(REF_LEN[r]), rng.randrange(20, 2500))

    chunks = _chunks(rng, tile, lambda: (_barcode(rng, inside, strangers), [aln() for _ in range(rng.choice(ATAC_NAS))]), lambda r: 4 + bw + 11 * len(r[1]))
    if family == "atac gpl":
        data, off = pkg.rad.encode_atac_chunks(chunks, bc_bytes=bw)
        return {"chunks": chunks, "data": b"\xEE" * pad + data, "off": off + np.uint64(pad), "bc_bytes": bw, "ref_lengths": REF_LEN, "blens": AG.blens_of(REF_LEN)}
    assert family == "atac sort"
    obs = list(inside)
    cor = obs[:len(obs) // 2] + [rng.choice(obs[:len(obs) // 2]) for _ in obs[len(obs) // 2:]]   # half onto themselves, half onto one of those
    c = AS._case_of_chunks(chunks, obs, cor, REF_LEN, bw)
    c["data"], c["off"] = b"\xEE" * pad + c["data"], c["off"] + np.uint64(pad)
    return c


def want(family, c, ori, lim):
    """the family's existing judge on a drawn case"""
    if family == "gpl":
        return G.want_hist(c, ori)
    if family == "gpl multi":
        return MC.want_pairs(c, ori)
    if family == "atac gpl":
        return AG.want_of(c["chunks"], c["blens"])
    if family == "atac sort":
        return AS.want_of(c)
    if family == "collate":
        return CC.want(c, ori, lim["lane_alns"])
    if family == "collate multi":
        return CM.want(c, ori, lim["lane_alns"])
    return AC.want(c)
