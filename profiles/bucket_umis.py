"""Keys and distinct UMIs per bucket of the configs[1] sample, on the CPU: how many 64-lane rounds the hash resolve needs
per key (ceil(n / 64)) and per UMI (ceil(U / 64)).  The same 320 cells as r09_bucket_fill.txt (seed 2, 11 000 cells; 8 cells at
each of 40 points of the size order) from the sample generator's host twin; a record's keys are its distinct genes; bucket_of
restated in numpy.   python profiles/bucket_umis.py > profiles/r12_bucket_umis.txt"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sn = importlib.import_module("alevin-fry_amd.synth_native")


def records(w, bc):
    """(umi, na, first ref word) of every record of one chunk's words (after its 8-byte header): record = na, bc, umi, na refs"""
    cand = np.flatnonzero((w[1:] == bc) & (w[:-1] >= 1) & (w[:-1] <= 64))
    na = w[cand].astype(np.int64)
    end = cand + 3 + na   # every word pair that looks like a record's head is one when they chain from word 0 to the end
    if len(cand) and np.array_equal(end[:-1], cand[1:]) and cand[0] == 0 and end[-1] == len(w):
        return w[cand + 2], na, cand + 3
    starts, out, pos = set(cand.tolist()), [], 0
    while pos < len(w):   # a ref or UMI word looked like a head: walk the chunk
        assert pos in starts
        out.append(pos)
        pos += 3 + int(w[pos])
    c = np.asarray(out, dtype=np.int64)
    return w[c + 2], w[c].astype(np.int64), c + 3


def main():
    p = sn.params()
    sizes = sn.cell_sizes(p)
    pts = np.linspace(0, p.n_cells - 8, 40).astype(int)
    n_all, u_all, keys, refs_total = [], [], 0, 0
    for c0 in pts:
        d = sn.generate(cell_range=(int(c0), int(c0) + 8), sizes=sizes, p=p)
        words = d.data.view(np.uint32)
        offs = (d.chunk_off // 4).astype(np.int64).tolist() + [len(words)]
        for ci in range(8):
            w = words[offs[ci] + 2:offs[ci + 1]]
            umi, na, r0 = records(w, w[1])
            assert len(umi) == words[offs[ci] + 1] and na.max() <= 3
            n_ref = int(na.sum())
            refs_total += n_ref
            g = np.full((len(umi), 3), -1, np.int64)
            for j in range(3):
                m = na > j
                g[m, j] = d.tid_to_gid[w[r0[m] + j] & 0x7FFFFFFF]
            g[(g[:, 1] == g[:, 0]), 1] = -1
            g[(g[:, 2] == g[:, 0]) | (g[:, 2] == g[:, 1]), 2] = -1
            ku = np.repeat(umi, 3)[(g >= 0).ravel()].astype(np.uint64)
            keys += len(ku)
            lg = 0
            while (256 << lg) < n_ref:
                lg += 1
            h = (ku * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
            b = (h >> np.uint64(32 - lg)).astype(np.int64) if lg else np.zeros(len(ku), np.int64)
            n_b = np.bincount(b, minlength=1 << lg)
            bu = np.unique(b * (1 << 32) + ku.astype(np.int64))
            u_b = np.bincount(bu >> 32, minlength=1 << lg)
            if lg:   # (single-bucket cells are the sort path's)
                n_all.append(n_b)
                u_all.append(u_b)
    n = np.concatenate(n_all)
    u = np.concatenate(u_all)
    print("# Round 12, step 1: keys (n) and distinct UMIs (U) per bucket of the configs[1] sample, on the CPU (no GPU call)\n")
    print(f"320 cells (seed 2, 11 000 cells; 8 at each of 40 points of the size order), {keys} keys / {refs_total} refs = {keys / refs_total:.3f}; "
          f"{len(n)} buckets of multi-bucket cells under the planner's rule (256 << lg >= n_ref).\n")
    print("| buckets | count | mean n | mean U | U / n | mean ceil(n/64) | mean ceil(U/64) | rounds saved |")
    print("|---|---|---|---|---|---|---|---|")
    for name, m in (("all", n >= 0), ("the table's (0 < n <= 256)", (n > 0) & (n <= 256))):
        rn, ru = -(-n[m] // 64), -(-u[m] // 64)
        print(f"| {name} | {m.sum()} | {n[m].mean():.1f} | {u[m].mean():.1f} | {u[m].sum() / n[m].sum():.3f} | {rn.mean():.3f} | {ru.mean():.3f} | {(rn - ru).mean():.3f} |")
    m = (n > 0) & (n <= 256)
    rn, ru = -(-n[m] // 64), -(-u[m] // 64)
    print("\nThe table's buckets by rounds, % of them (rows: ceil(n/64), columns: ceil(U/64)):\n")
    print("| key rounds | 1 | 2 | 3 | 4 | all |")
    print("|---|---|---|---|---|---|")
    for a in range(1, 5):
        print(f"| {a} | " + " | ".join(f"{100.0 * ((rn == a) & (ru == c)).mean():.2f}" for c in range(1, 5)) + f" | {100.0 * (rn == a).mean():.2f} |")
    print("| all | " + " | ".join(f"{100.0 * (ru == c).mean():.2f}" for c in range(1, 5)) + " | 100 |")
    print(f"\nU per bucket: sd {u[m].std():.1f}, max {u[m].max()}; U > 64: {100.0 * (u[m] > 64).mean():.2f} %, U > 128: {100.0 * (u[m] > 128).mean():.3f} %.")


if __name__ == "__main__":
    main()
