"""Time multi-barcode generate-permit-list's record pass: per-kernel (cfg.profile, HIP events) and end to end (host clock around calls
that end in a device synchronise), the median of 5 warm calls, with all five values kept so that the spread can be read.

Input: a Flex-like synthetic map.rad body - `--records` records (5 * 10^7 by default) of one alignment each (u16 sample barcode, u32
cell barcode, u32 UMI: 18 bytes a record), 5 000 to a chunk; 16 samples of 8 rotations each (8-base sample barcodes), 96 % of the reads
on a rotation, 3 % one substitution away, 1 % uniformly random; 1.1 * 10^4 cells per experiment with a 3 % rate of one-substitution
errors.  The routing entries are what sample correction `unique` over hamming-1 gives: the rotations and their structurally unique
neighbours.  Yardstick, same process: afq_gpl_hist_rad on single-barcode records (u32 barcode, u32 UMI: 16 bytes) of the same byte
volume - the same walk without the table probe.

    python profiles/gpl_multi_time.py [--records 50000000] [--out FILE]
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
SAMPLE_L = 8
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


def unique_neighbours(rot, target):
    """the rotations and every one-substitution neighbour that reaches rotations of ONE sample only (what `unique` over hamming-1 routes)"""
    reach = {}
    for b, t in zip(rot.tolist(), target.tolist()):
        for pos in range(SAMPLE_L):
            for rep in range(4):
                nb = (b & ~(3 << (2 * pos))) | (rep << (2 * pos))
                if nb != b:
                    reach.setdefault(nb, set()).add(t)
    src = set(rot.tolist())
    return np.asarray(sorted(src | {b for b, ts in reach.items() if b not in src and len(ts) == 1}), np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=50_000_000)
    ap.add_argument("--cells", type=int, default=11_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.records
    t0 = time.perf_counter()
    rng = np.random.default_rng(11)
    rot = np.unique(rng.integers(0, 1 << (2 * SAMPLE_L), size=16 * 8, dtype=np.uint64))
    target = rot[(np.arange(len(rot)) // 8) * 8]
    entries = unique_neighbours(rot, target)
    b0 = rot[rng.integers(0, len(rot), size=n)]
    near = rng.random(n) < 0.03
    b0[near] ^= (rng.integers(1, 4, size=int(near.sum()), dtype=np.uint64) << (np.uint64(2) * rng.integers(0, SAMPLE_L, size=int(near.sum()), dtype=np.uint64)))
    far = rng.random(n) < 0.01
    b0[far] = rng.integers(0, 1 << (2 * SAMPLE_L), size=int(far.sum()), dtype=np.uint64)
    cells = np.unique(rng.integers(0, 1 << 32, size=a.cells, dtype=np.uint64))
    b1 = cells[rng.integers(0, len(cells), size=n)]
    err = rng.random(n) < 0.03
    b1[err] ^= (rng.integers(1, 4, size=int(err.sum()), dtype=np.uint64) << (np.uint64(2) * rng.integers(0, 16, size=int(err.sum()), dtype=np.uint64)))
    umi = rng.integers(0, 1 << 24, size=n, dtype=np.uint32)
    aln = rng.integers(0, 100000, size=n, dtype=np.uint32) | np.uint32(0x80000000)
    flex = np.dtype([("na", "<u4"), ("b0", "<u2"), ("b1", "<u4"), ("umi", "<u4"), ("aln", "<u4")])
    assert flex.itemsize == 18
    data, off = chunked(flex, {"na": 1, "b0": b0.astype(np.uint16), "b1": b1.astype(np.uint32), "umi": umi, "aln": aln}, n)
    # the yardstick's input: single-barcode records (16 bytes) of the same byte volume
    rna = np.dtype([("na", "<u4"), ("bc", "<u4"), ("umi", "<u4"), ("aln", "<u4")])
    n_rna = len(data) // rna.itemsize
    pick = rng.integers(0, n, size=n_rna)
    rdata, roff = chunked(rna, {"na": 1, "bc": b1[pick].astype(np.uint32), "umi": umi[pick], "aln": aln[pick]}, n_rna)
    del b0, b1, near, far, err, pick
    prep_s = time.perf_counter() - t0

    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=True)
    q = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    res = {"records": n, "chunks": int(len(off)), "input_bytes": int(len(data)), "routing_entries": int(len(entries)), "rotations": int(len(rot)), "cells": int(len(cells)),
           "prepare_s": round(prep_s, 1)}
    keep = {}
    try:
        def run_multi():
            keep["m"] = q.gpl_multi_hist_rad(data, off, entries, b0_bytes=2, b1_bytes=4, umi_bytes=4, expected_ori="fw")
            return q.kernel_times()

        def run_single():
            keep["s"] = q.gpl_hist_rad(rdata, roff, bc_bytes=4, umi_bytes=4, expected_ori="fw")
            return q.kernel_times()

        # the two passes alternate call by call inside one process: whatever else the host or the device does meets both alike
        run_multi(); run_single()
        rows = {"multi": ([], []), "single": ([], [])}
        for _ in range(5):
            for name, fn in (("multi", run_multi), ("single", run_single)):
                t1 = time.perf_counter()
                k = fn()
                rows[name][0].append((time.perf_counter() - t1) * 1e3)
                rows[name][1].append(k)
        for name, parse, nbytes, what in (("multi", "k_gpl_multi_parse", len(data), keep["m"]), ("single", "k_gpl_parse", len(rdata), keep["s"])):
            e2e, kern = rows[name]
            names = sorted({k2 for k in kern for k2 in k})
            med = {k2: statistics.median(k.get(k2, (0.0, 0))[0] for k in kern) for k2 in names}
            p = med.get(parse, 0.0)
            res["hist_" + name if name == "multi" else "yardstick_gpl_hist_rad"] = {
                "input_bytes": int(nbytes), "e2e_ms_median_of_5": round(statistics.median(e2e), 3), "e2e_ms_all": [round(x, 3) for x in e2e],
                "kernel_ms": {k2: round(v, 3) for k2, v in med.items()}, "parse_ms_all": [round(k.get(parse, (0.0, 0))[0], 3) for k in kern],
                "parse_GBps": round(nbytes / max(p, 1e-9) / 1e6, 1), "parse_share_of_hbm": round(nbytes / max(p, 1e-9) * 1e3 / HBM_BYTES_PER_S, 4),
                "distinct": int(len(what["count"])), "stats": what["stats"]}
        m, s = res["hist_multi"], res["yardstick_gpl_hist_rad"]
        res["parse_ms_multi_minus_single"] = round(m["kernel_ms"]["k_gpl_multi_parse"] - s["kernel_ms"]["k_gpl_parse"], 3)
        res["parse_ms_spread"] = {"multi": round(max(m["parse_ms_all"]) - min(m["parse_ms_all"]), 3), "single": round(max(s["parse_ms_all"]) - min(s["parse_ms_all"]), 3)}
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
