"""Time `atac collate`'s device half: per kernel group (cfg.profile, HIP events) and end to end (host clock around calls that end in a
device synchronise and hand the output to the host), the medians of `--steps` calls after `--warmup`.

Input: that of profiles/atac_sort_time.py - the scATAC synthetic of config 5 (synth_native.generate_atac), its records dealt into
chunks of 5 000 under a fixed permutation, an identity correction map plus 1 % corrected barcodes.  The cells are the corrected
barcodes, by (kept records descending, barcode ascending) as permit_freq.bin orders them.

Yardstick, same process, same bytes: k_sort_parse (afq_atac_sort_rad).  Each of collate's two walks is that kernel's walk - without
its range checks and key build - plus, in the write walk, one scattered store of R = 19 bytes per kept record.  Printed beside it: the
table, the measure walk, the placement (radix passes + cell runs + scan + heads + destinations), the write walk, end to end.

    python profiles/atac_collate_time.py [--records 20000000] [--steps 20] [--warmup 5] [--out profiles/atac_collate_time.json]
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
sn = importlib.import_module("alevin-fry_amd.synth_native")
from atac_sort_time import deal, record_starts   # noqa: E402


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    e2e, kern = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        k = fn()
        e2e.append((time.perf_counter() - t0) * 1e3)
        kern.append(k)
    names = sorted({n for k in kern for n in k})
    return statistics.median(e2e), {n: statistics.median(k.get(n, (0.0, 0))[0] for k in kern) for n in names}, e2e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    frags = 20000
    n_cells = max(1, a.records // frags)
    n_refs, ref_len = 25, 150_000_000
    t0 = time.perf_counter()
    data, off = sn.generate_atac(seed=5, n_cells=n_cells, frags_per_cell=frags, n_refs=n_refs, ref_len=ref_len, n_threads=min(16, os.cpu_count() or 1))
    pos, na, bc = record_starts(data, off)
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(pos))
    mixed, moff, _, na_p = deal(data, pos, na, perm)
    cells = np.unique(bc).astype(np.uint64)
    obs, cor = cells.copy(), cells.copy()
    k = max(1, len(cells) // 100)
    pick = rng.permutation(len(cells))[:2 * k]
    cor[pick[:k]] = cells[pick[k:2 * k]]             # 1 % of the barcodes are corrected onto other permitted ones
    # the cells in permit_freq.bin's order: kept records descending, barcode ascending
    kept_bc = bc[perm][na_p == 1].astype(np.uint64)
    tgt, cnt = np.unique(cor[np.searchsorted(obs, kept_bc)], return_counts=True)
    out_cells = tgt[np.lexsort((tgt, -cnt.astype(np.int64)))]
    ref_lengths = np.full(n_refs, ref_len, np.uint32)
    del data, off, pos, na, bc, kept_bc
    prep_s = time.perf_counter() - t0
    n_rec = len(perm)

    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=True)
    q = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    res = {"records": n_rec, "chunks": int(len(moff)), "input_bytes": int(len(mixed)), "cells": int(len(out_cells)), "corrections": int(len(obs)),
           "steps": a.steps, "warmup": a.warmup, "prepare_s": round(prep_s, 1)}
    keep = {}
    try:
        def run_sort():
            keep["sort"] = q.atac_sort_rad(mixed, moff, obs, cor, ref_lengths)["stats"]
            return q.kernel_times()

        def run_collate():
            keep["out"] = q.atac_collate_rad(mixed, moff, obs, cor, out_cells, bc_bytes=4)
            return q.kernel_times()

        _, kern, _ = timed(run_sort, 1, 5)
        parse_ms = kern.get("k_sort_parse", 0.0)
        res["yardstick_k_sort_parse_ms"] = round(parse_ms, 3)
        e2e, kern, all_e2e = timed(run_collate, a.warmup, a.steps)
        st = keep["out"]["stats"]
        assert st["n_kept"] == keep["sort"]["n_kept"] and st["n_cells_out"] == len(out_cells), "collate and sort keep different records"
        g = lambda k_: kern.get(k_, 0.0)
        res["atac_collate"] = {"e2e_ms_median": round(e2e, 3), "e2e_ms_min_max": [round(min(all_e2e), 3), round(max(all_e2e), 3)],
                               "kernel_ms": {k_: round(v, 3) for k_, v in kern.items()}, "kernels_ms": round(sum(kern.values()), 3), "stats": st,
                               "measure_over_k_sort_parse": round(g("k_atac_collate_measure") / max(parse_ms, 1e-9), 2),
                               "write_over_k_sort_parse": round(g("k_atac_collate_write") / max(parse_ms, 1e-9), 2),
                               "write_over_measure": round(g("k_atac_collate_write") / max(g("k_atac_collate_measure"), 1e-9), 2),
                               "ns_per_record_kernels": round(sum(kern.values()) * 1e6 / n_rec, 3), "ns_per_record_e2e": round(e2e * 1e6 / n_rec, 3)}
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
