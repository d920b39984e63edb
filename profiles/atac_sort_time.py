"""Time `atac sort` on the device: per-kernel (cfg.profile, HIP events) and end to end (host clock around calls that end in a
device synchronise), the median of 5 warm calls.

Input: the scATAC synthetic of config 5 (synth_native.generate_atac) at 2*10^7 records, its records dealt into chunks of 5 000
under a fixed permutation - what a mapper's map.rad looks like: barcodes mixed inside every chunk - with an identity correction
map plus 1 % corrected barcodes.  A skewed variant puts 10 % of the fragments on one 16.5 kb reference (a mitochondrial bin).
Next to them, from the same process: `atac deduplicate` (afq_atac_dedup_rad) on the collated chunks the records came from - the one
yardstick there is; its output is per cell, so the two are different problems of the same size.

    python profiles/atac_sort_time.py [--records 20000000] [--out FILE]
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
sn = importlib.import_module("alevin-fry_amd.synth_native")

H = 8            # na:u32 + a u32 barcode
PER_CHUNK = 5000


def u32_at(data, pos):
    p = pos.astype(np.int64)
    return (data[p].astype(np.uint32) | (data[p + 1].astype(np.uint32) << 8) | (data[p + 2].astype(np.uint32) << 16) | (data[p + 3].astype(np.uint32) << 24))


def put_u32(data, pos, v):
    p = pos.astype(np.int64)
    for k in range(4):
        data[p + k] = ((v >> (8 * k)) & 0xFF).astype(np.uint8)


def record_starts(data, off):
    """start offset, na and barcode of every record of collated chunks (every record of a chunk carries the chunk's barcode: the
    positions whose barcode field matches are the records when their sizes chain from the chunk's start to its end - checked)"""
    n = len(data)
    ends = np.append(off[1:], n).astype(np.int64)
    starts, nas, bcs = [], [], []
    for c0 in range(0, len(off), 64):   # a block of cells at a time keeps the index arrays small
        lo, hi = int(off[c0]), int(ends[min(c0 + 64, len(off)) - 1])
        for c in range(c0, min(c0 + 64, len(off))):
            a, b = int(off[c]), int(ends[c])
            nrec = int(u32_at(data, np.array([a + 4]))[0])
            if nrec == 0:
                continue
            bc = data[a + 12:a + 16]
            seg = data[a + 8:b]
            m = (seg[4:len(seg) - 3] == bc[0]) & (seg[5:len(seg) - 2] == bc[1]) & (seg[6:len(seg) - 1] == bc[2]) & (seg[7:] == bc[3])
            cand = np.flatnonzero(m).astype(np.int64) + a + 8
            na = u32_at(data, cand).astype(np.int64)
            nxt = cand + H + 11 * na
            ok = len(cand) == nrec and cand[0] == a + 8 and np.array_equal(nxt[:-1], cand[1:]) and nxt[-1] == b
            if not ok:   # a field that happens to spell the barcode: walk this chunk
                p, cl = a + 8, []
                while p < b:
                    cl.append(p)
                    p += H + 11 * int(u32_at(data, np.array([p]))[0])
                cand = np.asarray(cl, np.int64)
                na = u32_at(data, cand).astype(np.int64)
                assert len(cand) == nrec
            starts.append(cand)
            nas.append(na)
            bcs.append(np.full(len(cand), int(u32_at(data, np.array([a + 12]))[0]), np.uint32))
        del lo, hi
    return np.concatenate(starts), np.concatenate(nas), np.concatenate(bcs)


def deal(data, pos, na, perm):
    """the records in the order perm, PER_CHUNK to a chunk: bytes, chunk_off, the new start of every record"""
    pos, na = pos[perm], na[perm]
    sz = H + 11 * na
    n = len(pos)
    n_chunks = (n + PER_CHUNK - 1) // PER_CHUNK
    new = np.cumsum(sz) - sz + 8 * (np.arange(n) // PER_CHUNK + 1)
    total = int(new[-1] + sz[-1])
    out = np.zeros(total, np.uint8)
    off = np.zeros(n_chunks, np.uint64)
    for c in range(n_chunks):
        a, b = c * PER_CHUNK, min((c + 1) * PER_CHUNK, n)
        o = int(new[a]) - 8
        off[c] = o
        nb = int(new[b - 1] + sz[b - 1]) - o
        out[o:o + 4] = np.frombuffer(int(nb).to_bytes(4, "little"), np.uint8)
        out[o + 4:o + 8] = np.frombuffer(int(b - a).to_bytes(4, "little"), np.uint8)
    for s in np.unique(sz):
        idx = np.flatnonzero(sz == s)
        for i0 in range(0, len(idx), 1 << 21):
            ii = idx[i0:i0 + (1 << 21)]
            ar = np.arange(int(s), dtype=np.int64)
            out[(new[ii][:, None] + ar).ravel()] = data[(pos[ii][:, None] + ar).ravel()]
    return out, off, new, na


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
    ap.add_argument("--records", type=int, default=20_000_000)
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
    mixed, moff, new, na_p = deal(data, pos, na, perm)
    cells = np.unique(bc).astype(np.uint64)
    obs, cor = cells.copy(), cells.copy()
    k = max(1, len(cells) // 100)
    pick = rng.permutation(len(cells))[:2 * k]
    cor[pick[:k]] = cells[pick[k:2 * k]]             # 1 % of the barcodes are corrected onto other permitted ones
    ref_lengths = np.full(n_refs, ref_len, np.uint32)
    # the skewed variant: 10 % of the single-alignment records on a 16.5 kb reference of its own
    skew = mixed.copy()
    one = np.flatnonzero(na_p == 1)
    hit = one[rng.random(len(one)) < 0.10]
    put_u32(skew, new[hit] + H, np.full(len(hit), n_refs, np.uint32))
    put_u32(skew, new[hit] + H + 5, rng.integers(0, 16000, size=len(hit)).astype(np.uint32))
    skew_lengths = np.append(ref_lengths, np.uint32(16500))
    prep_s = time.perf_counter() - t0
    n_rec = len(pos)

    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=True)
    q = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    res = {"records": n_rec, "chunks": int(len(moff)), "input_bytes": int(len(mixed)), "cells": int(n_cells), "corrections": int(len(obs)), "prepare_s": round(prep_s, 1)}
    try:
        def run_sort(b, rl):
            def f():
                r = q.atac_sort_rad(b, moff, obs, cor, rl)
                run_sort.stats = r["stats"]
                return q.kernel_times()
            return f

        def run_dedup():
            q.atac_dedup_rad(data, off, copy=False)
            return q.kernel_times()

        for name, fn in (("atac_sort", run_sort(mixed, ref_lengths)), ("atac_sort_skewed", run_sort(skew, skew_lengths)), ("atac_deduplicate", run_dedup)):
            e2e, kern, all_e2e = timed(fn)
            res[name] = {"e2e_ms_median_of_5": round(e2e, 3), "e2e_ms_all": [round(x, 3) for x in all_e2e], "ns_per_record_e2e": round(e2e * 1e6 / n_rec, 3),
                         "kernel_ms": {k_: round(v, 3) for k_, v in kern.items()}, "kernel_ms_sum": round(sum(kern.values()), 3),
                         "ns_per_record_kernels": round(sum(kern.values()) * 1e6 / n_rec, 3)}
            if name.startswith("atac_sort"):
                res[name]["stats"] = run_sort.stats
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
