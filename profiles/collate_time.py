"""Time collate's device half: per kernel group (cfg.profile, HIP events) and end to end (host clock around calls that end in a
device synchronise and hand the output to the host), the median of 5 warm calls.

Input: the generator of profiles/gpl_time.py - `--records` records (5 * 10^7 by default) of one forward alignment each (u32 barcode,
u32 UMI: 16 bytes a record), 5 000 to a chunk, 1.1 * 10^4 cells with a 3 % rate of one-substitution errors and uniformly random
barcodes on 0.1 % of the reads.  The correction map and the cell order are made the way the pipeline makes them: gpl_hist_rad, the
retained set, gpl_correct, cells by (count descending, barcode ascending).

Printed: the kernel groups (table, measure, sort passes, scan + heads, write), end to end, input + output bytes over the kernels'
time as a fraction of HBM bandwidth.  Yardstick, same process, same bytes: k_gpl_parse.  Collate walks the input twice, so the two
walks are compared against 2 x that time; the placement is compared against the bytes it moves (a radix pass reads the sort words
twice and writes them once: 24 bytes a record; the scan reads the sorted words and gathers the lengths twice and writes two
offsets: 48 bytes a record).

    python profiles/collate_time.py [--records 50000000] [--out profiles/collate_time.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("GPU_FORCE_BLIT_COPY_SIZE", "0")
pkg = importlib.import_module("alevin-fry_amd")
from gpl_time import HBM_BYTES_PER_S, L, chunked, timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=50_000_000)
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
    del bc, err, noise
    prep_s = time.perf_counter() - t0

    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=True)
    q = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    res = {"records": n, "chunks": int(len(off)), "input_bytes": int(len(data)), "prepare_s": round(prep_s, 1)}
    keep = {}
    try:
        def run_hist():
            keep["hist"] = q.gpl_hist_rad(data, off, bc_bytes=4, umi_bytes=4, expected_ori="fw")
            return q.kernel_times()

        _, kern, _ = timed(run_hist)
        parse_ms = kern.get("k_gpl_parse", 0.0)
        res["yardstick_k_gpl_parse_ms"] = round(parse_ms, 3)
        h = keep["hist"]
        thr = max(1, int(n / len(cells) / 10))
        sel = h["count"] >= thr
        ret, ret_cnt = h["bc"][sel], h["count"][sel]
        c = q.gpl_correct(h["bc"], h["count"], ret, ret_cnt, L, neighborhood="substitution-or-shift-1")
        has = c["target"] != pkg._abi.GPL_NO_TARGET
        observed, corrected = h["bc"][has], ret[c["target"][has]]
        permitted = c["target_count"] > 0
        order = np.lexsort((ret[permitted], -c["target_count"][permitted].astype(np.int64)))
        out_cells = ret[permitted][order]
        res.update({"cells": int(len(out_cells)), "corrections": int(len(observed))})

        def run_collate():
            keep["out"] = q.collate_rad(data, off, observed, corrected, out_cells, bc_bytes=4, umi_bytes=4, expected_ori="fw")
            return q.kernel_times()

        e2e, kern, all_e2e = timed(run_collate)
        o = keep["out"]
        assert o["stats"]["n_kept"] == int(c["target_count"].sum()), "kept records != the sum of the permit list"   # collate.rs:615
        g = lambda k: kern.get(k, 0.0)
        walks, place, total = g("k_collate_measure") + g("k_collate_write"), g("k_collate_sort") + g("k_collate_scan"), sum(kern.values())
        passes = max(1, (int(len(out_cells)).bit_length() + 7) // 8)
        moved = n * (24 * passes + 48)
        io = len(data) + o["stats"]["out_bytes"]
        res["collate"] = {"e2e_ms_median_of_5": round(e2e, 3), "e2e_ms_all": [round(x, 3) for x in all_e2e], "kernel_ms": {k: round(v, 3) for k, v in kern.items()},
                          "kernels_ms": round(total, 3), "stats": o["stats"], "io_GBps_over_kernels": round(io / max(total, 1e-9) / 1e6, 1),
                          "io_share_of_hbm": round(io / max(total, 1e-9) * 1e3 / HBM_BYTES_PER_S, 4),
                          "walks_ms": round(walks, 3), "walks_over_two_gpl_parses": round(walks / max(2 * parse_ms, 1e-9), 2),
                          "radix_passes": passes, "placement_ms": round(place, 3), "placement_bytes_moved": int(moved),
                          "placement_GBps": round(moved / max(place, 1e-9) / 1e6, 1)}
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
