"""Time multi-barcode collate's device half against single-barcode collate: per kernel group (cfg.profile, HIP events) and end to end
(host clock around calls that end in a device synchronise and hand the output to the host), the median of 5 warm calls, all five
values kept so that the spread can be read.  The two collates alternate call by call inside one process.

Input: a Flex-like synthetic map.rad body - `--records` records (5 * 10^7 by default) of one forward alignment each (u16 sample
barcode, u32 cell barcode, u32 UMI: 18 bytes a record), 5 000 to a chunk; 16 samples of 8 rotations each (8-base sample barcodes),
96 % of the reads on a rotation, 3 % one substitution away, 1 % uniformly random; `--cells` cells (1.1 * 10^4 by default) dealt over
the samples, 3 % of the reads one substitution away from their cell.  The sample table is the rotations and their structurally unique
neighbours; the cell table holds every cell and its one-substitution neighbours that reach one cell of the sample only.

Yardstick, same process: afq_collate_rad on single-barcode records (u32 barcode, u32 UMI: 16 bytes) with the SAME record count, the
same alignments per record and the same cell barcodes, its map being the union of the samples' maps.  Placement and scan are the same
kernels over the same number of sort words; the walks differ by the second barcode's bytes and the dependent second lookup.

    python profiles/collate_multi_time.py [--records 50000000] [--out FILE]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("GPU_FORCE_BLIT_COPY_SIZE", "0")
pkg = importlib.import_module("alevin-fry_amd")
from gpl_multi_time import HBM_BYTES_PER_S, SAMPLE_L, chunked   # noqa: E402

N_SAMPLES, ROTS, CELL_L = 16, 8, 16


def neighbours(v, L):
    """every one-substitution neighbour of the packed barcodes v: (len(v) * 3 L,) with the source index beside it"""
    out, src = [], []
    for pos in range(L):
        for x in (1, 2, 3):
            out.append(v ^ np.uint64(x << (2 * pos)))
            src.append(np.arange(len(v)))
    return np.concatenate(out), np.concatenate(src)


def unique_map(obs, tgt):
    """(obs, tgt) pairs -> those whose obs reaches ONE target"""
    order = np.lexsort((tgt, obs))
    obs, tgt = obs[order], tgt[order]
    first = np.r_[True, obs[1:] != obs[:-1]]
    grp = np.cumsum(first) - 1
    lo, hi = np.minimum.reduceat(tgt, np.flatnonzero(first)), np.maximum.reduceat(tgt, np.flatnonzero(first))
    ok = (lo == hi)[grp] & first
    return obs[ok], tgt[ok]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=50_000_000)
    ap.add_argument("--cells", type=int, default=11_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.records
    t0 = time.perf_counter()
    rng = np.random.default_rng(13)
    rot = np.unique(rng.integers(0, 1 << (2 * SAMPLE_L), size=N_SAMPLES * ROTS, dtype=np.uint64))
    rot_sample = (np.arange(len(rot)) // ROTS).astype(np.uint64)
    nb, src = neighbours(rot, SAMPLE_L)
    n_obs, n_idx = unique_map(nb, rot_sample[src])
    fresh = ~np.isin(n_obs, rot)   # (a rotation routes to its own sample whatever it neighbours)
    s_obs, s_idx = np.concatenate([rot, n_obs[fresh]]), np.concatenate([rot_sample, n_idx[fresh]])
    cells = np.unique(rng.integers(0, 1 << 32, size=a.cells, dtype=np.uint64))
    cell_sample = rng.integers(0, N_SAMPLES, size=len(cells)).astype(np.uint64)
    order = np.lexsort((cells, cell_sample))
    cells, cell_sample = cells[order], cell_sample[order]
    # reads: a cell, its sample's rotation, errors on both
    pick = rng.integers(0, len(cells), size=n)
    b1 = cells[pick].copy()
    smp = cell_sample[pick].astype(np.int64)
    b0 = rot[np.minimum(smp * ROTS + rng.integers(0, ROTS, size=n), len(rot) - 1)].copy()
    near = rng.random(n) < 0.03
    b0[near] ^= (rng.integers(1, 4, size=int(near.sum()), dtype=np.uint64) << (np.uint64(2) * rng.integers(0, SAMPLE_L, size=int(near.sum()), dtype=np.uint64)))
    far = rng.random(n) < 0.01
    b0[far] = rng.integers(0, 1 << (2 * SAMPLE_L), size=int(far.sum()), dtype=np.uint64)
    err = rng.random(n) < 0.03
    b1[err] ^= (rng.integers(1, 4, size=int(err.sum()), dtype=np.uint64) << (np.uint64(2) * rng.integers(0, CELL_L, size=int(err.sum()), dtype=np.uint64)))
    umi = rng.integers(0, 1 << 24, size=n, dtype=np.uint32)
    aln = rng.integers(0, 100000, size=n, dtype=np.uint32) | np.uint32(0x80000000)
    flex = np.dtype([("na", "<u4"), ("b0", "<u2"), ("b1", "<u4"), ("umi", "<u4"), ("aln", "<u4")])
    rna = np.dtype([("na", "<u4"), ("bc", "<u4"), ("umi", "<u4"), ("aln", "<u4")])
    data, off = chunked(flex, {"na": 1, "b0": b0.astype(np.uint16), "b1": b1.astype(np.uint32), "umi": umi, "aln": aln}, n)
    rdata, roff = chunked(rna, {"na": 1, "bc": b1.astype(np.uint32), "umi": umi, "aln": aln}, n)
    del b0, b1, near, far, err, pick, smp, umi, aln
    # the cell table: per sample, a cell and its one-substitution neighbours that reach one cell of the sample only
    cnb, csrc = neighbours(cells, CELL_L)
    key = np.concatenate([cell_sample << np.uint64(32) | cells, cell_sample[csrc] << np.uint64(32) | cnb])
    tgt = np.concatenate([np.arange(len(cells)), csrc]).astype(np.uint64)
    ckey, ctgt = unique_map(key, tgt)
    corr_sample, corr_obs, corr_cor = (ckey >> np.uint64(32)).astype(np.uint32), ckey & np.uint64(0xFFFFFFFF), cells[ctgt.astype(np.int64)]
    # the yardstick's map: the union over the samples (an observed barcode of two samples keeps its first target), its cells
    u_obs, first = np.unique(corr_obs, return_index=True)
    u_cor = corr_cor[first]
    u_cells = np.unique(u_cor)
    prep_s = time.perf_counter() - t0

    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=True)
    q = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    res = {"records": n, "alignments_per_record": 1, "chunks": int(len(off)), "samples": N_SAMPLES, "cells": int(len(cells)), "sample_entries": int(len(s_obs)),
           "cell_corrections": int(len(corr_obs)), "input_bytes_multi": int(len(data)), "input_bytes_single": int(len(rdata)), "prepare_s": round(prep_s, 1)}
    out = {}
    try:
        def run_multi():
            out["m"] = q.collate_multi_rad(data, off, s_obs, s_idx.astype(np.uint32), corr_sample, corr_obs, corr_cor, cell_sample.astype(np.uint32), cells,
                                           np.arange(N_SAMPLES, dtype=np.uint32), b0_bytes=2, b1_bytes=4, umi_bytes=4, expected_ori="fw")
            return q.kernel_times()

        def run_single():
            out["s"] = q.collate_rad(rdata, roff, u_obs, u_cor, u_cells, bc_bytes=4, umi_bytes=4, expected_ori="fw")
            return q.kernel_times()

        run_multi(); run_single()
        rows = {"multi": ([], []), "single": ([], [])}
        for _ in range(5):
            for name, fn in (("multi", run_multi), ("single", run_single)):
                t1 = time.perf_counter()
                k = fn()
                rows[name][0].append((time.perf_counter() - t1) * 1e3)
                rows[name][1].append(k)
        for name, pre, nbytes, what in (("multi", "k_collate_multi_", len(data), out["m"]), ("single", "k_collate_", len(rdata), out["s"])):
            e2e, kern = rows[name]
            ms = lambda k, part: k.get(pre + part, (0.0, 0))[0]
            med = {part: statistics.median(ms(k, part) for k in kern) for part in ("table", "measure", "sort", "scan", "write")}
            io = nbytes + what["stats"]["out_bytes"]
            total = sum(med.values())
            res["collate_" + name] = {"e2e_ms_median_of_5": round(statistics.median(e2e), 3), "e2e_ms_all": [round(x, 3) for x in e2e],
                                      "kernel_ms": {k: round(v, 3) for k, v in med.items()}, "kernels_ms": round(total, 3),
                                      "measure_ms_all": [round(ms(k, "measure"), 3) for k in kern], "write_ms_all": [round(ms(k, "write"), 3) for k in kern],
                                      "walks_ms": round(med["measure"] + med["write"], 3), "placement_ms": round(med["sort"] + med["scan"], 3),
                                      "io_share_of_hbm": round(io / max(total, 1e-9) * 1e3 / HBM_BYTES_PER_S, 4), "stats": what["stats"]}
        m, s = res["collate_multi"], res["collate_single"]
        res["multi_over_single"] = {k: round(m["kernel_ms"][k] / max(s["kernel_ms"][k], 1e-9), 3) for k in ("measure", "write", "sort", "scan")}
        res["multi_over_single"]["bytes"] = round(len(data) / len(rdata), 3)
    finally:
        q.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
