"""Time generate-permit-list's device half: per-kernel (cfg.profile, HIP events) and end to end (host clock around calls that end in
a device synchronise), the median of 5 warm calls.

Input: a PBMC-like synthetic map.rad body - `--records` records (4 * 10^8 by default) of one alignment each (u32 barcode, u32 UMI:
16 bytes a record), 5 000 to a chunk, 1.1 * 10^4 cells with a 3 % rate of one-substitution errors, and uniformly random 16-base
barcodes on 0.1 % of the reads (about 10^6 distinct observed barcodes at the full size).  Printed: the parse,
count (+ compact) and correct kernel groups, the end-to-end times of the histogram, of the correction of the observed barcodes
and of the full theoretical neighbourhood; the parse's input bytes per second beside the device's HBM bandwidth.  Yardstick, same
process: k_sort_parse (afq_atac_sort_rad) on scATAC records of the same byte volume, since the walk is the same.

    python profiles/gpl_time.py [--records 400000000] [--out FILE]
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
os.environ.setdefault("GPU_FORCE_BLIT_COPY_SIZE", "0")
pkg = importlib.import_module("alevin-fry_amd")

PER_CHUNK = 5000
L = 16
HBM_BYTES_PER_S = 8.0e12   # MI355X: 8 TB/s


def chunked(rec_dtype, fields, n):
    """n records of a fixed size, PER_CHUNK to a chunk (the last one shorter): (bytes, chunk_off)"""
    rs = rec_dtype.itemsize
    n_full, rest = divmod(n, PER_CHUNK)
    parts, offs, at = [], [], 0
    rec = np.zeros(n, rec_dtype)
    for k, v in fields.items():
        rec[k] = v
    raw = rec.view(np.uint8).reshape(n, rs)
    if n_full:
        blk = np.zeros((n_full, 8 + PER_CHUNK * rs), np.uint8)
        blk[:, 0:4] = np.frombuffer(np.uint32(8 + PER_CHUNK * rs).tobytes(), np.uint8)
        blk[:, 4:8] = np.frombuffer(np.uint32(PER_CHUNK).tobytes(), np.uint8)
        blk[:, 8:] = raw[:n_full * PER_CHUNK].reshape(n_full, PER_CHUNK * rs)
        parts.append(blk.ravel())
        offs.append(np.arange(n_full, dtype=np.uint64) * np.uint64(8 + PER_CHUNK * rs))
        at = n_full * (8 + PER_CHUNK * rs)
    if rest:
        tail = np.zeros(8 + rest * rs, np.uint8)
        tail[0:4] = np.frombuffer(np.uint32(8 + rest * rs).tobytes(), np.uint8)
        tail[4:8] = np.frombuffer(np.uint32(rest).tobytes(), np.uint8)
        tail[8:] = raw[n_full * PER_CHUNK:].ravel()
        parts.append(tail)
        offs.append(np.asarray([at], np.uint64))
    return np.concatenate(parts), np.concatenate(offs)


def neighbours(src):
    """every retained barcode and all its substitution-or-shift-1 neighbours (for_each_neighbor), distinct, ascending"""
    out = [src]
    for pos in range(L):
        sh = np.uint64(2 * pos)
        cleared = src & ~(np.uint64(3) << sh)
        for rep in range(4):
            out.append(cleared | (np.uint64(rep) << sh))
    for b in range(1, L):
        lower_mask = np.uint64((1 << (2 * b)) - 1)
        upper, lower = src & ~lower_mask, src & lower_mask
        for adm in range(4):
            out.append(upper | (np.uint64(adm) << np.uint64(2 * (b - 1))) | (lower >> np.uint64(2)))
            out.append(upper | np.uint64(adm) | (lower << np.uint64(2)))
    return np.unique(np.concatenate(out))


def timed(fn, warm=1, reps=5):
    for _ in range(warm):
        fn()
    e2e, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        k = fn()
        e2e.append((time.perf_counter() - t0) * 1e3)
        kern.append(k)
    names = sorted({n for k in kern for n in k})
    return statistics.median(e2e), {n: statistics.median(k.get(n, (0.0, 0))[0] for k in kern) for n in names}, e2e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=400_000_000)
    ap.add_argument("--cells", type=int, default=11_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.records
    t0 = time.perf_counter()
    rng = np.random.default_rng(7)
    cells = np.unique(rng.integers(0, 1 << 32, size=a.cells, dtype=np.uint64))
    bc = cells[rng.integers(0, len(cells), size=n)]
    err = rng.random(n) < 0.03
    bc[err] ^= (rng.integers(1, 4, size=int(err.sum()), dtype=np.uint64) << (np.uint64(2) * rng.integers(0, L, size=int(err.sum()), dtype=np.uint64)))
    noise = rng.random(n) < 0.001
    bc[noise] = rng.integers(0, 1 << 32, size=int(noise.sum()), dtype=np.uint64)
    rna = np.dtype([("na", "<u4"), ("bc", "<u4"), ("umi", "<u4"), ("aln", "<u4")])
    data, off = chunked(rna, {"na": 1, "bc": bc.astype(np.uint32), "umi": rng.integers(0, 1 << 24, size=n, dtype=np.uint32),
                              "aln": rng.integers(0, 100000, size=n, dtype=np.uint32) | np.uint32(0x80000000)}, n)
    # the yardstick's input: scATAC records (na, u32 barcode, ref, type, start, frag_len: 19 bytes) of the same byte volume
    atac = np.dtype([("na", "<u4"), ("bc", "<u4"), ("ref", "<u4"), ("type", "u1"), ("start", "<u4"), ("flen", "<u2")])
    n_atac = len(data) // atac.itemsize
    adata, aoff = chunked(atac, {"na": 1, "bc": cells[rng.integers(0, len(cells), size=n_atac)].astype(np.uint32), "ref": rng.integers(0, 25, size=n_atac, dtype=np.uint32),
                                 "type": 0, "start": rng.integers(0, 100_000_000, size=n_atac, dtype=np.uint32), "flen": rng.integers(50, 600, size=n_atac, dtype=np.uint16)}, n_atac)
    del bc, err, noise
    prep_s = time.perf_counter() - t0

    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=True)
    q = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    res = {"records": n, "chunks": int(len(off)), "input_bytes": int(len(data)), "cells": int(len(cells)), "prepare_s": round(prep_s, 1)}
    keep = {}
    try:
        def run_hist():
            keep["hist"] = q.gpl_hist_rad(data, off, bc_bytes=4, umi_bytes=4, expected_ori="fw")
            return q.kernel_times()

        e2e, kern, all_e2e = timed(run_hist)
        h = keep["hist"]
        parse_ms = kern.get("k_gpl_parse", 0.0)
        res["hist"] = {"e2e_ms_median_of_5": round(e2e, 3), "e2e_ms_all": [round(x, 3) for x in all_e2e], "kernel_ms": {k: round(v, 3) for k, v in kern.items()},
                       "distinct_observed": int(len(h["bc"])), "stats": h["stats"], "parse_GBps": round(len(data) / max(parse_ms, 1e-9) / 1e6, 1),
                       "parse_share_of_hbm": round(len(data) / max(parse_ms, 1e-9) * 1e3 / HBM_BYTES_PER_S, 4)}
        # retained: the barcodes with at least a tenth of the mean cell's reads (what a knee would find on this input)
        thr = max(1, int(n / len(cells) / 10))
        ret = h["bc"][h["count"] >= thr]
        ret_cnt = h["count"][h["count"] >= thr]
        res["retained"] = int(len(ret))
        for res_name, kw in (("unique", {}), ("frequency", {"resolution": "frequency"})):
            def run_correct():
                keep["c"] = q.gpl_correct(h["bc"], h["count"], ret, ret_cnt, L, neighborhood="substitution-or-shift-1", **kw)
                return q.kernel_times()
            e2e, kern, all_e2e = timed(run_correct)
            res["correct_observed_" + res_name] = {"e2e_ms_median_of_5": round(e2e, 3), "kernel_ms": {k: round(v, 3) for k, v in kern.items()}, "stats": keep["c"]["stats"]}
        t1 = time.perf_counter()
        theo = neighbours(ret)
        res["full_neighbourhood"] = {"barcodes": int(len(theo)), "host_list_ms": round((time.perf_counter() - t1) * 1e3, 1)}
        zeros = np.zeros(len(theo), np.uint64)

        def run_full():
            q.gpl_correct(theo, zeros, ret, ret_cnt, L, neighborhood="substitution-or-shift-1")
            return q.kernel_times()
        e2e, kern, _ = timed(run_full)
        res["full_neighbourhood"].update({"e2e_ms_median_of_5": round(e2e, 3), "kernel_ms": {k: round(v, 3) for k, v in kern.items()}})
        res["end_to_end_ms"] = round(res["hist"]["e2e_ms_median_of_5"] + res["correct_observed_unique"]["e2e_ms_median_of_5"] + res["full_neighbourhood"]["host_list_ms"] +
                                     res["full_neighbourhood"]["e2e_ms_median_of_5"], 1)

        def run_sort():
            q.atac_sort_rad(adata, aoff, cells, cells, np.full(25, 150_000_000, np.uint32))
            return q.kernel_times()
        e2e, kern, _ = timed(run_sort, reps=3)
        sp = kern.get("k_sort_parse", 0.0)
        res["yardstick_k_sort_parse"] = {"input_bytes": int(len(adata)), "records": int(n_atac), "k_sort_parse_ms": round(sp, 3), "parse_GBps": round(len(adata) / max(sp, 1e-9) / 1e6, 1)}
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
