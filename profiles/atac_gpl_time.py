"""Time the record pass of `atac generate-permit-list` (afq_atac_gpl_hist_rad): per kernel group (cfg.profile, HIP events) and end to end
(host clock around calls that end in a device synchronise and hand the histogram and the bins to the host), the medians of `--steps`
calls after `--warmup`.

Input: that of profiles/atac_sort_time.py - the scATAC synthetic of config 5 (synth_native.generate_atac), its records dealt into
chunks of 5 000 under a fixed permutation.  25 references of 150 Mb give 37 500 bins of 100 kb (a human genome has about 31 000).

Yardstick, same process, same bytes: k_sort_parse (afq_atac_sort_rad under an identity correction map).  The record pass's walk is that
kernel's walk; it stores a barcode for EVERY record where the sort parse stores a key and a bin for the kept ones, probes no table, and
adds one global atomic per record with one alignment.  Printed beside it: the walk, the bins' widening pass, the counting table
(k_gpl_count, k_gpl_compact), end to end.

    python profiles/atac_gpl_time.py [--records 200000000] [--steps 10] [--warmup 3] [--out profiles/atac_gpl_time.json]
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

BIN_SIZE = 100000


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
    ap.add_argument("--records", type=int, default=200_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
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
    ref_lengths = np.full(n_refs, ref_len, np.uint32)
    bin_base = np.concatenate(([0], np.cumsum(np.ceil(ref_lengths.astype(np.float32) / np.float32(BIN_SIZE)).astype(np.uint64)))).astype(np.uint64)
    n_rec, n_one = len(perm), int((na_p == 1).sum())
    del data, off, pos, na, bc
    prep_s = time.perf_counter() - t0

    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=True)
    q = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    res = {"records": n_rec, "chunks": int(len(moff)), "input_bytes": int(len(mixed)), "barcodes": int(len(cells)), "bins": int(bin_base[-1]),
           "steps": a.steps, "warmup": a.warmup, "prepare_s": round(prep_s, 1)}
    keep = {}
    try:
        def run_sort():
            keep["sort"] = q.atac_sort_rad(mixed, moff, cells, cells, ref_lengths)["stats"]
            return q.kernel_times()

        def run_gpl():
            keep["out"] = q.atac_gpl_hist_rad(mixed, moff, bin_base, bc_bytes=4, bin_size=BIN_SIZE)
            return q.kernel_times()

        _, kern, _ = timed(run_sort, 1, 3)
        parse_ms = kern.get("k_sort_parse", 0.0)
        res["yardstick_k_sort_parse_ms"] = round(parse_ms, 3)
        e2e, kern, all_e2e = timed(run_gpl, a.warmup, a.steps)
        bcs, count, bins, st = keep["out"]
        assert st["n_records"] == n_rec and st["n_binned"] == n_one == int(bins.sum()) and int(count.sum()) == n_rec and len(bcs) == len(cells), "the record pass lost records"
        assert st["n_binned"] == keep["sort"]["n_kept"], "the record pass and the sort parse see different single-alignment records"
        g = lambda k_: kern.get(k_, 0.0)
        res["atac_gpl"] = {"e2e_ms_median": round(e2e, 3), "e2e_ms_min_max": [round(min(all_e2e), 3), round(max(all_e2e), 3)],
                           "kernel_ms": {k_: round(v, 3) for k_, v in kern.items()}, "kernels_ms": round(sum(kern.values()), 3), "stats": st,
                           "parse_over_k_sort_parse": round(g("k_atac_gpl_parse") / max(parse_ms, 1e-9), 2),
                           "parse_GBps": round(len(mixed) / max(g("k_atac_gpl_parse"), 1e-9) / 1e6, 1),
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
