"""Time the device snappy frame encoder (csrc/afq_snappy.hip) and what it does to collate's copy down.

Two inputs:
  - the bench's PBMC-like sample (synth_native.generate_device: a collated RAD in HBM, `--cells` cells): the bytes a collate leaves
    on the device.  Measured: afq_snappy_frame_encode from the device pointer to stream bytes on the host (host clock around a call
    that ends in a device synchronise), its two kernel groups (cfg.profile, HIP events), stream bytes over input bytes, and - the
    thing to compare with - a plain copy of the same bytes down into fresh host memory, which is what the collates do with the
    setter off (the parent commit's behaviour).
  - collate input made by profiles/collate_time.py's generator (`--records` records): afq_collate_rad with
    afq_set_collate_compress off and on, alternating in one process; per call the time behind the write walk - end to end less
    the collate kernels - is the time from the end of the write walk to bytes on the host.
On a prefix of the PBMC-like bytes (`--google-bytes`): Google's snappy through pyarrow.Codec("snappy"), one thread, a block per
frame chunk, framed as rad.snappy_frame_encode frames a compressed chunk (8 bytes a chunk, 10 in front), beside this encoder's
stream of the same prefix.

    python profiles/snappy_time.py [--steps 20] [--warmup 5] [--cells 11000] [--records 50000000] [--out profiles/snappy_time.json]
"""
import argparse
import ctypes as C
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
from gpl_time import L, chunked   # noqa: E402


def med(xs):
    return round(statistics.median(xs), 3)


def encode_device(q, lib, d_ptr, n):
    """afq_snappy_frame_encode on device bytes; the stream is freed at once -> (ms, stats, kernel times)"""
    o_b, o_n, st = C.POINTER(C.c_uint8)(), C.c_uint64(), pkg._abi.AfqSnappyStats()
    t0 = time.perf_counter()
    q._check(lib.afq_snappy_frame_encode(q._h, C.c_void_p(d_ptr), n, 1, C.byref(o_b), C.byref(o_n), C.byref(st)))
    ms = (time.perf_counter() - t0) * 1e3
    lib.afq_free(o_b)
    return ms, {k: int(getattr(st, k)) for k, _ in st._fields_}, q.kernel_times()


def collate_device(q, lib, d_ptr, n, off, observed, corrected, cells):
    """afq_collate_rad on device bytes, its arrays freed at once (none of the binding's numpy copies) -> (ms, bytes handed out, stats)"""
    u64p = C.POINTER(C.c_uint64)
    o_b, o_n, o_off, o_nrec, st = C.POINTER(C.c_uint8)(), C.c_uint64(), u64p(), C.POINTER(C.c_uint32)(), pkg._abi.AfqCollateStats()
    t0 = time.perf_counter()
    q._check(lib.afq_collate_rad(q._h, C.c_void_p(d_ptr), n, off.ctypes.data_as(u64p), len(off), 4, 4, pkg._abi.GPL_ORI["fw"], 1, observed.ctypes.data_as(u64p),
                                 corrected.ctypes.data_as(u64p), len(observed), cells.ctypes.data_as(u64p), len(cells), C.byref(o_b), C.byref(o_n), C.byref(o_off),
                                 C.byref(o_nrec), C.byref(st)))
    ms = (time.perf_counter() - t0) * 1e3
    for p_ in (o_b, o_off, o_nrec):
        lib.afq_free(p_)
    return ms, int(o_n.value), {k: int(getattr(st, k)) for k, _ in st._fields_}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cells", type=int, default=11_000, help="cells of the PBMC-like sample")
    ap.add_argument("--records", type=int, default=50_000_000, help="records of the collate input")
    ap.add_argument("--google-bytes", type=int, default=256 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = pkg.load_library()
    sn = importlib.import_module("alevin-fry_amd.synth_native")
    res = {"steps": a.steps, "warmup": a.warmup}
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=True)
    q = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    try:
        # ---- the PBMC-like sample: encoder against the plain copy down, alternating (--cells 0: the collate part alone)
        if a.cells:
            pbmc_like(a, q, lib, sn, res)
        collate_off_on(a, q, lib, res)
    finally:
        q.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


def pbmc_like(a, q, lib, sn, res):
    rad = sn.generate_device(device=0, seed=2, n_cells=a.cells, median_reads=30000.0, sigma=0.6, num_genes=36601, usa=False, umi_err=0.01, ref_count=199138)
    n = int(rad.n_bytes)
    slib = sn._lib()
    enc, blocks, pack, plain = [], [], [], []
    st = None
    for i in range(a.warmup + a.steps):
        ms, st, kt = encode_device(q, lib, rad.d_ptr, n)
        host = np.empty(n, np.uint8)   # fresh pages, as the malloc'd block of the collates' copy down
        t0 = time.perf_counter()
        rc = slib.afq_synth_device_read(0, C.c_void_p(rad.d_ptr), n, C.c_void_p(host.ctypes.data))
        t1 = (time.perf_counter() - t0) * 1e3
        assert rc == 0
        if i >= a.warmup:
            enc.append(ms)
            plain.append(t1)
            blocks.append(kt.get("k_snappy_blocks", (0.0, 0))[0])
            pack.append(kt.get("k_snappy_pack", (0.0, 0))[0])
    k_ms = statistics.median(blocks) + statistics.median(pack)
    res["pbmc_like"] = {"cells": a.cells, "input_bytes": n, "stats": st, "stream_over_input": round(st["n_out"] / max(n, 1), 4),
                        "k_snappy_blocks_ms": med(blocks), "k_snappy_pack_ms": med(pack), "encoder_GBps_of_input_over_kernels": round(n / max(k_ms, 1e-9) / 1e6, 1),
                        "encode_to_host_ms": med(enc), "encode_to_host_ms_min_max": [round(min(enc), 3), round(max(enc), 3)],
                        "plain_copy_down_ms": med(plain), "plain_copy_down_ms_min_max": [round(min(plain), 3), round(max(plain), 3)]}
    # ---- Google's snappy on a prefix of the same bytes, one thread
    m = min(n, a.google_bytes)
    B = pkg.snappy_limits()["block"]
    pre = host[:m].copy()
    del host
    try:
        import pyarrow as pa
        codec = pa.Codec("snappy") if pa.Codec.is_available("snappy") else None
    except ImportError:
        codec = None
    ours, ost = q.snappy_frame_encode(pre)
    g = {"prefix_bytes": m, "this_encoder_stream_bytes": len(ours), "this_encoder_stream_over_input": round(len(ours) / max(m, 1), 4), "this_encoder_stored_chunks": ost["n_blocks_stored"]}
    if codec is not None:
        mv = memoryview(pre)
        t0 = time.perf_counter()
        sizes = [len(codec.compress(mv[i:i + B], asbytes=True)) for i in range(0, m, B)]
        dt = time.perf_counter() - t0
        total = 10 + sum(8 + s for s in sizes)
        g.update({"google_stream_bytes": total, "google_stream_over_input": round(total / max(m, 1), 4), "google_one_thread_GBps": round(m / dt / 1e9, 3),
                  "this_over_google_stream": round(len(ours) / total, 4)})
    else:
        g["google"] = "pyarrow without snappy: not measured"
    res["google_snappy_same_bytes"] = g
    rad.free()


def collate_off_on(a, q, lib, res):
    """collate: setter off and on, alternating"""
    import torch

    nrec = a.records
    rng = np.random.default_rng(7)
    cells = np.unique(rng.integers(0, 1 << 32, size=11_000, dtype=np.uint64))
    bc = cells[rng.integers(0, len(cells), size=nrec)]
    err = rng.random(nrec) < 0.03
    bc[err] ^= (rng.integers(1, 4, size=int(err.sum()), dtype=np.uint64) << (np.uint64(2) * rng.integers(0, L, size=int(err.sum()), dtype=np.uint64)))
    rna = np.dtype([("na", "<u4"), ("bc", "<u4"), ("umi", "<u4"), ("aln", "<u4")])
    data, off = chunked(rna, {"na": 1, "bc": bc.astype(np.uint32), "umi": rng.integers(0, 1 << 24, size=nrec, dtype=np.uint32),
                              "aln": rng.integers(0, 100000, size=nrec, dtype=np.uint32) | np.uint32(0x80000000)}, nrec)
    del bc, err
    h = q.gpl_hist_rad(data, off, bc_bytes=4, umi_bytes=4, expected_ori="fw")
    sel = h["count"] >= max(1, int(nrec / len(cells) / 10))
    ret, ret_cnt = h["bc"][sel], h["count"][sel]
    c = q.gpl_correct(h["bc"], h["count"], ret, ret_cnt, L, neighborhood="substitution-or-shift-1")
    has = c["target"] != pkg._abi.GPL_NO_TARGET
    observed, corrected = h["bc"][has], ret[c["target"][has]]
    permitted = c["target_count"] > 0
    order = np.lexsort((ret[permitted], -c["target_count"][permitted].astype(np.int64)))
    out_cells = np.ascontiguousarray(ret[permitted][order], dtype=np.uint64)
    observed, corrected, off = (np.ascontiguousarray(x, dtype=np.uint64) for x in (observed, corrected, off))
    d = torch.from_numpy(data).cuda()   # the input on the device: no upload inside the timed calls
    torch.cuda.synchronize()
    t = {False: {"e2e": [], "tail": [], "snappy": []}, True: {"e2e": [], "tail": [], "snappy": []}}
    sizes = {}
    for i in range(a.warmup + a.steps):
        for on in (False, True):
            q.set_collate_compress(on)
            ms, handed, cst = collate_device(q, lib, d.data_ptr(), len(data), off, observed, corrected, out_cells)
            kt = q.kernel_times()
            sizes[on] = (handed, cst["out_bytes"])
            if i >= a.warmup:
                kern = sum(v[0] for k, v in kt.items() if k.startswith("k_collate"))
                t[on]["e2e"].append(ms)
                t[on]["tail"].append(ms - kern)
                t[on]["snappy"].append(sum(v[0] for k, v in kt.items() if k.startswith("k_snappy")))
    q.set_collate_compress(False)
    res["collate"] = {"records": nrec, "input_bytes": int(len(data)), "out_bytes": sizes[False][1], "stream_bytes": sizes[True][0],
                      "stream_over_out_bytes": round(sizes[True][0] / max(sizes[False][1], 1), 4),
                      "setter_off": {"e2e_ms": med(t[False]["e2e"]), "behind_the_write_walk_ms": med(t[False]["tail"]),
                                     "behind_the_write_walk_ms_min_max": [round(min(t[False]["tail"]), 3), round(max(t[False]["tail"]), 3)]},
                      "setter_on": {"e2e_ms": med(t[True]["e2e"]), "behind_the_write_walk_ms": med(t[True]["tail"]),
                                    "behind_the_write_walk_ms_min_max": [round(min(t[True]["tail"]), 3), round(max(t[True]["tail"]), 3)],
                                    "snappy_kernels_ms": med(t[True]["snappy"])},
                      "note": "behind_the_write_walk = e2e - the k_collate_* kernels: the status reads, the copy down (off) or encoder + copy down (on)"}


if __name__ == "__main__":
    main()
