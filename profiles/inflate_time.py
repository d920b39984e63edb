"""Time the device BGZF inflater (csrc/afq_inflate.hip, k_bgzf_inflate) and what --inflate-on-device does to `afquant convert`
end to end.

The file: a BAM of about `--gib` GiB inflated, of tests/bam_cases.py's record writer at zlib level 6 - a unit of `--unit-mib` MiB of
records with random names, barcodes, UMIs and references, cut into BGZF blocks of 65280 bytes and written as often as it takes
(BGZF blocks are independent, so the unit's blocks are compressed once).

  (a) the inflater: afq_bgzf_inflate_device of the file from host memory to bytes resident on the device - wall (upload
      included) and the k_bgzf_inflate launches alone (HIP events, upload excluded).
  (b) end to end: `afquant convert -t <threads>` on the file, door closed and door open, alternating, a fresh process per run,
      with AFQ_HOST_TIMING's laps of the last run of each.  `--parent-cli PATH`: the closed door is also run by that binary - an
      `afquant` built from the parent commit (`git worktree add DIR HEAD~1 && make -C DIR/alevin-fry_amd/csrc`).

    python profiles/inflate_time.py [--steps 3] [--warmup 1] [--gib 1.0] [--threads 16] [--parent-cli PATH] [--out profiles/inflate_time.json]
"""
import argparse
import importlib
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("GPU_FORCE_BLIT_COPY_SIZE", "0")
pkg = importlib.import_module("alevin-fry_amd")
import bam_cases as B  # noqa: E402

CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")
REFS = ["tx%05d" % i for i in range(2000)]


def summary(xs, nd=3):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def write_bam(path, gib, unit_mib, seed=1):
    """returns (file bytes, inflated bytes, BGZF blocks)"""
    rng = random.Random(seed)
    unit = bytearray()
    i = 0
    while len(unit) < unit_mib << 20:
        name = "A00%d:%d:HXXX:%d:%d:%d:%d" % (rng.randrange(9), rng.randrange(400), rng.randrange(1, 5), rng.randrange(1101, 2679), rng.randrange(32768), rng.randrange(32768))
        cr, ur = "".join(rng.choice("ACGT") for _ in range(16)), "".join(rng.choice("ACGT") for _ in range(12))
        # (the writer's own sequence and quality bytes are constant: a read's bases and qualities ride in two aux strings, so that
        # the file compresses about as a real one does)
        bases, quals = "".join(rng.choice("ACGT") for _ in range(91)), "".join(rng.choice("FFFFFFFF:F,") for _ in range(91))
        for _ in range(rng.choice([1, 1, 1, 2, 3])):
            unit += B.record_bytes(B.rec(name, ref=rng.randrange(len(REFS)), flag=rng.choice([0, 16]), cr=cr, ur=ur, score=rng.randrange(60, 92), pos=rng.randrange(5000),
                                         cigar=[(91 << 4)], seq_len=91, after=[("NH", "C", 1), ("HI", "C", 1), ("XB", "Z", bases), ("XQ", "Z", quals)]))
        i += 1
    unit = bytes(unit)
    blocks = [B.bgzf_block(unit[a:a + 65280]) for a in range(0, len(unit), 65280)]
    unit_z = b"".join(blocks)
    reps = max(1, round(gib * (1 << 30) / len(unit)))
    head = B.header_bytes(REFS)
    with open(path, "wb") as f:
        f.write(B.bgzf_block(head))
        for _ in range(reps):
            f.write(unit_z)
        f.write(B.BGZF_EOF)
    return os.path.getsize(path), len(head) + reps * len(unit), 2 + reps * len(blocks)


def inflater(a, q, data, n_out, res):
    wall, kern, st, k = [], [], None, (0.0, 0)
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        (_, n), st = q.bgzf_inflate(data, shift=0, on_device=True)
        t1 = time.perf_counter()
        assert n == n_out
        k = q.kernel_times().get("k_bgzf_inflate", (0.0, 0))
        if i >= a.warmup:
            wall.append((t1 - t0) * 1e3), kern.append(k[0])
    gb = n_out / 1e6
    res["inflater"] = {"file_bytes": int(len(data)), "inflated_bytes": int(n_out), "stats": st, "launches": int(k[1]),
                       "device_wall_ms_upload_included": summary(wall), "device_GBps_of_output_upload_included": round(gb / statistics.median(wall), 2),
                       "k_bgzf_inflate_ms_sum_of_launches": summary(kern), "device_GBps_of_output_kernels_alone": round(gb / max(statistics.median(kern), 1e-9), 2)}


def end_to_end(a, bam, work, res):
    doors = [("closed", CLI, []), ("open", CLI, ["--inflate-on-device"])] + ([("closed_parent", a.parent_cli, [])] if a.parent_cli else [])
    runs, laps = {d: [] for d, _, _ in doors}, {}
    env = {**os.environ, "AFQ_HOST_TIMING": "1"}
    for i in range(a.warmup + a.steps):
        for door, cli, flags in doors:
            o = os.path.join(work, door + ".rad")
            t0 = time.perf_counter()
            p = subprocess.run([cli, "convert", "-b", bam, "-o", o, "-t", str(a.threads)] + flags, capture_output=True, text=True, env=env)
            dt = time.perf_counter() - t0
            if p.returncode != 0:
                res["end_to_end"] = {"error": door + ": " + p.stderr[-600:]}
                return
            laps[door] = [ln for ln in p.stderr.splitlines() if ln.startswith("[afquant]")]
            if i >= a.warmup:
                runs[door].append(dt)
    same = all(open(os.path.join(work, "closed.rad"), "rb").read() == open(os.path.join(work, d + ".rad"), "rb").read() for d, _, _ in doors[1:])
    res["end_to_end"] = {"command": f"afquant convert -t {a.threads}, a fresh process per run, the file in the page cache",
                         "wall_s": {d: summary(runs[d]) for d in runs}, "open_over_closed_median": round(statistics.median(runs["open"]) / statistics.median(runs["closed"]), 3),
                         "outputs_identical": same, "laps": laps}
    if a.parent_cli:
        res["end_to_end"]["open_over_parent_median"] = round(statistics.median(runs["open"]) / statistics.median(runs["closed_parent"]), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gib", type=float, default=1.0, help="inflated size of the BAM")
    ap.add_argument("--unit-mib", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-cli", default=None, help="an afquant built from the parent commit: it runs the closed door too")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"steps": a.steps, "warmup": a.warmup, "threads": a.threads}
    work = tempfile.mkdtemp(prefix="inflate_time_")
    try:
        bam = os.path.join(work, "reads.bam")
        t0 = time.perf_counter()
        n_file, n_out, n_blocks = write_bam(bam, a.gib, a.unit_mib)
        res["bam"] = {"file_bytes": n_file, "inflated_bytes": n_out, "bgzf_blocks": n_blocks, "zlib_level": 6, "written_in_s": round(time.perf_counter() - t0, 1)}
        data = np.fromfile(bam, np.uint8)
        q = pkg.Quantifier(pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=True), np.zeros(1, np.uint32), device=0)
        try:
            inflater(a, q, data, n_out, res)
        finally:
            q.close()
        del data
        end_to_end(a, bam, work, res)   # the processes have the device to themselves
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
