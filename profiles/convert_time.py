"""`python profiles/convert_time.py [REPS] [--out FILE]`: builds a synthetic BAM with the case writer of tests/bam_cases.py (one piece of
66 000 reads, 1-6 alignments each, STARsolo-like records of about 300 bytes; the piece's BGZF blocks are written REPS times, 72 by
default: about 10^7 records) into a temporary directory and runs `afquant convert` on it under AFQ_HOST_TIMING: one warm-up, then
five runs without -f and three with.  Every run is a fresh process, so its wall time holds the process start and the device's
initialisation; the laps are the host's phases (seconds) and, inside "convert: device", the entry point's own (milliseconds)."""
import os
import random
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_cases as B  # noqa: E402

CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 72
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
PIECE_READS = 66000
REFS = ["ENST%011d.1" % i for i in range(2000)]


def piece(seed=3):
    rng = random.Random(seed)
    recs = []
    for i in range(PIECE_READS):
        n = rng.choice([1, 1, 1, 1, 2, 2, 3, 6])
        cr = "".join(rng.choice("ACGT") for _ in range(16))
        ur = "".join(rng.choice("ACGT") for _ in range(12))
        best = rng.randrange(n)
        name = "A00123:45:HXXXXXXX:1:%04d:%05d:%05d" % (i % 10000, rng.randrange(100000), i)
        for j in range(n):
            recs.append(dict(name=name, ref=rng.randrange(len(REFS)),
                             flag=(0x10 if rng.random() < 0.1 else 0) | (0x100 if j else 0), pos=rng.randrange(5000), mapq=255 if n == 1 else 3, cigar=[(91 << 4)], seq_len=91,
                             aux=[("NH", "C", n), ("HI", "C", j + 1), ("AS", "C", 89 if j == best else 80 + rng.randrange(9)), ("nM", "C", 0), ("CR", "Z", cr), ("UR", "Z", ur),
                                  ("CY", "Z", "F" * 16), ("UY", "Z", "F" * 12)]))
    return recs


def blocks_of(data):
    return b"".join(B.bgzf_block(data[a:a + 60000]) for a in range(0, len(data), 60000))


def main():
    log = open(OUT, "w") if OUT else None
    def say(s):
        print(s, flush=True)
        if log:
            log.write(s + "\n")
            log.flush()
    t0 = time.time()
    recs = piece()
    body = b"".join(B.record_bytes(r) for r in recs)
    with tempfile.TemporaryDirectory() as d:
        bam = os.path.join(d, "synthetic.bam")
        comp = blocks_of(body)
        with open(bam, "wb") as f:
            f.write(B.bgzf_block(B.header_bytes(REFS)))
            for _ in range(REPS):
                f.write(comp)
            f.write(B.BGZF_EOF)
        say(f"BAM: {len(recs) * REPS} records in {PIECE_READS * REPS} reads, {len(body) * REPS} bytes inflated, {os.path.getsize(bam)} bytes on disk, built in {time.time() - t0:.1f} s")
        for label, extra, runs in (("warm-up", [], 1), ("no filter", [], 5), ("-f", ["-f"], 3)):
            for k in range(runs):
                t = time.time()
                r = subprocess.run([CLI, "convert", "-b", bam, "-o", os.path.join(d, "out.rad"), "-t", "16"] + extra, capture_output=True, text=True,
                                   env=dict(os.environ, AFQ_HOST_TIMING="1"), timeout=400)
                wall = time.time() - t
                if r.returncode:
                    say(f"{label} {k}: FAILED rc={r.returncode}: {r.stderr[-600:]}")
                    return 1
                laps = re.findall(r"\[(afquant|afq host)\] (.*?)\s+([0-9.]+) (s|ms)", r.stderr)
                say(f"{label} {k}: wall {wall:.3f} s (process start and device init included); " + "; ".join(f"{w.strip()} = {v} {u}" for _, w, v, u in laps))
                if k == 0:
                    say("    " + r.stderr.strip().splitlines()[-1])
    return 0


if __name__ == "__main__":
    sys.exit(main())
