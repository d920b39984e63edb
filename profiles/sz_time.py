"""Time the device snappy frame decoder (csrc/afq_snappy.hip, k_snappy_decode), the chunk-table hop (k_collated_chunk_table) and
what --sz-on-device does to `afquant quant` end to end.

The stream: the bench's PBMC-like sample (synth_native.generate_device, `--cells` cells) compressed by the device encoder - what
`collate -c` writes: the frame stream of the prelude, then the frame stream of the chunks.

  (a) the decoder: afq_snappy_frame_decode_device of the chunks' stream from host memory to bytes resident on the device - wall
      (upload included) and the k_snappy_decode launches alone (HIP events, upload excluded) - beside the library's host decoder
      afq_snappy_frame_decode on the same stream (it takes min(8, cores) threads; the closed door's own lap, all `-t` threads, is
      in (b)).
  (b) end to end: `afquant quant -r cr-like -t <threads>` on the directory, door closed and door open, alternating, a fresh
      process per run, with AFQ_HOST_TIMING's laps of the last run of each.  `--parent-cli PATH`: the closed door is run by that
      binary - an `afquant` built from the parent commit (`git worktree add DIR HEAD~1 && make -C DIR/alevin-fry_amd/csrc`).
  (c) the hop: afq_collated_chunk_table on the decoded sample, and on a stream of `--small-cells` cells of 352 bytes.

    python profiles/sz_time.py [--steps 5] [--warmup 1] [--cells 4000] [--threads 16] [--parent-cli PATH] [--out profiles/sz_time.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_FORCE_BLIT_COPY_SIZE", "0")
pkg = importlib.import_module("alevin-fry_amd")
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")


def summary(xs, nd=3):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def decoder(a, q, lib, stream, n_out, res):
    dev, kern, host = [], [], []
    lib.afq_snappy_frame_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    lib.afq_snappy_frame_decode.restype = C.c_int64
    out = np.empty(n_out, np.uint8)
    st = None
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        ptr, n, st = q.snappy_frame_decode(stream, shift=0, on_device=True)
        t1 = time.perf_counter()
        assert n == n_out
        k = q.kernel_times().get("k_snappy_decode", (0.0, 0))
        t2 = time.perf_counter()
        assert lib.afq_snappy_frame_decode(stream.ctypes.data, len(stream), out.ctypes.data, n_out) == n_out
        t3 = time.perf_counter()
        if i >= a.warmup:
            dev.append((t1 - t0) * 1e3), kern.append(k[0]), host.append((t3 - t2) * 1e3)
    gb = n_out / 1e6
    res["decoder"] = {"stream_bytes": int(len(stream)), "decoded_bytes": int(n_out), "stats": st, "launches": int(k[1]),
                      "device_wall_ms_upload_included": summary(dev), "device_GBps_of_output_upload_included": round(gb / statistics.median(dev), 2),
                      "k_snappy_decode_ms_sum_of_launches": summary(kern), "device_GBps_of_output_kernels_alone": round(gb / max(statistics.median(kern), 1e-9), 2),
                      "host_decoder_ms": summary(host), "host_decoder_GBps_of_output": round(gb / statistics.median(host), 2),
                      "host_decoder_threads": min(8, os.cpu_count() or 1), "removed_round3_device_decoder_GBps": 9.4}
    return ptr


def hop(a, q, d_ptr, n, first_chunk, what, res):
    ms, kms, nc = [], [], 0
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        off, _, _, _ = q.collated_chunk_table(d_ptr, n, first_chunk, 12)
        t1 = time.perf_counter()
        nc = len(off)
        if i >= a.warmup:
            ms.append((t1 - t0) * 1e3), kms.append(q.kernel_times().get("k_collated_chunk_table", (0.0, 0))[0])
    res.setdefault("chunk_table", {})[what] = {"bytes": int(n), "cells": nc, "mean_cell_bytes": round(n / max(nc, 1), 1), "call_ms": summary(ms), "kernel_ms": summary(kms),
                                               "kernel_us_per_cell": round(statistics.median(kms) * 1e3 / max(nc, 1), 4)}


def end_to_end(a, d, tg, n_reads, res):
    runs = {"closed": [], "open": []}
    laps = {}
    env = {**os.environ, "AFQ_HOST_TIMING": "1"}
    for i in range(a.warmup + a.steps):
        for door in ("closed", "open"):
            o = os.path.join(d, "out_" + door)
            shutil.rmtree(o, ignore_errors=True)
            t0 = time.perf_counter()
            p = subprocess.run([a.parent_cli if door == "closed" and a.parent_cli else CLI, "quant", "-i", d, "-m", tg, "-o", o, "-r", "cr-like", "-t", str(a.threads)] + (["--sz-on-device"] if door == "open" else []),
                               capture_output=True, text=True, env=env)
            dt = time.perf_counter() - t0
            if p.returncode != 0:
                res["end_to_end"] = {"error": door + ": " + p.stderr[-600:]}
                return
            laps[door] = [ln for ln in p.stderr.splitlines() if ln.startswith("[afquant]")]
            if i >= a.warmup:
                runs[door].append(dt)
    same = all(open(os.path.join(d, "out_closed", f), "rb").read() == open(os.path.join(d, "out_open", f), "rb").read()
               for f in ("alevin/quants_mat.mtx", "alevin/quants_mat_rows.txt", "featureDump.txt"))
    res["end_to_end"] = {"command": f"afquant quant -r cr-like -t {a.threads}, a fresh process per run, the file in the page cache", "reads": int(n_reads),
                         "door_closed_binary": "built from the parent commit" if a.parent_cli else "this tree's",
                         "door_closed_wall_s": summary(runs["closed"]), "door_open_wall_s": summary(runs["open"]),
                         "open_over_closed_median": round(statistics.median(runs["open"]) / statistics.median(runs["closed"]), 3),
                         "open_inside_closed_range": min(runs["closed"]) <= statistics.median(runs["open"]) <= max(runs["closed"]),
                         "outputs_identical": same, "laps_door_closed": laps["closed"], "laps_door_open": laps["open"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cells", type=int, default=4000, help="cells of the PBMC-like sample")
    ap.add_argument("--small-cells", type=int, default=200_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-cli", default=None, help="an afquant built from the parent commit: it runs the closed door")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    lib = pkg.load_library()
    sn = importlib.import_module("alevin-fry_amd.synth_native")
    res = {"steps": a.steps, "warmup": a.warmup, "cells": a.cells}
    q = pkg.Quantifier(pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=True), np.zeros(1, np.uint32), device=0)
    work = tempfile.mkdtemp(prefix="sz_time_")
    try:
        rad = sn.generate_device(device=0, seed=2, n_cells=a.cells, median_reads=30000.0, sigma=0.6, num_genes=36601, usa=False, umi_err=0.01, ref_count=199138)
        n = int(rad.n_bytes)
        body, _ = q.snappy_frame_encode(None, d_ptr=rad.d_ptr, n_bytes=n)
        stream = np.frombuffer(body, np.uint8)
        # ---- the directory `collate -c` would leave
        names = [f"t{i}" for i in range(len(rad.tid_to_gid))]
        prelude = pkg.rad.rad_prelude(names, len(rad.cell_nrec), 16, 12)
        d = os.path.join(work, "in")
        tg = pkg.rad.write_quant_input_dir(d, b"", len(rad.cell_nrec), names, [(names[i], f"g{int(g)}") for i, g in enumerate(rad.tid_to_gid)], cblen=16, ulen=12, prelude=prelude)
        os.remove(os.path.join(d, "map.collated.rad"))
        with open(os.path.join(d, "map.collated.rad.sz"), "wb") as f:
            f.write(q.snappy_frame_encode(prelude)[0])
            f.write(body)
        with open(os.path.join(d, "collate.json"), "w") as f:
            json.dump({"cmd": "sz_time", "version_str": "0.18.0", "compressed_output": True}, f)
        n_reads = int(np.asarray(rad.cell_nrec).astype(np.int64).sum())
        rad.free()
        del body
        os.sync()
        # ---- (a) and (c)
        d_ptr = decoder(a, q, lib, stream, n, res)
        hop(a, q, d_ptr, n, 0, "pbmc_like", res)
        small = np.random.default_rng(1).integers(0, 256, (a.small_cells, 352), dtype=np.uint8)
        small[:, :8] = np.frombuffer(np.array([352, 20], "<u4").tobytes(), np.uint8)
        t = torch.from_numpy(small.reshape(-1)).cuda()
        torch.cuda.synchronize()
        hop(a, q, t.data_ptr(), t.numel(), 0, "cells_of_352_bytes", res)
        del t
    finally:
        q.close()
    try:
        end_to_end(a, d, tg, n_reads, res)   # (b): the processes have the device to themselves
    finally:
        shutil.rmtree(work, ignore_errors=True)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
