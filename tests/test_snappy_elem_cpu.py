"""The device snappy decoder's element parser (csrc/afq_snappy_elem.h) on the host: tests/snappy_elem_check.cpp decodes chunks with
the parser and a serial executor, built with the address and undefined-behaviour sanitizers and run as a program of its own.  Every
chunk of tests/snappy_streams.py and 10^4 seeded mutations of them: the program's verdict and bytes are the judge's
(tests/snappy_judge.py), and no mutation makes it touch a byte outside the body or the output."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import snappy_streams as ss

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "snappy_elem_check.cpp")
HDR = os.path.join(HERE, "..", "alevin-fry_amd", "csrc", "afq_snappy_elem.h")
BIN = os.path.join(HERE, "_build", "snappy_elem_check")
N_MUTATIONS = 10_000


@pytest.fixture(scope="module")
def checker():
    """(path, sanitized): the sanitizer build where the machine has the sanitizers' runtime, a plain one otherwise"""
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    probe = os.path.join(os.path.dirname(BIN), "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([cxx, *san, probe, "-o", probe + ".out"], capture_output=True, text=True)
    sanitized = r.returncode == 0 and subprocess.run([probe + ".out"], capture_output=True).returncode == 0
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + (san if sanitized else [])
    r = subprocess.run([cxx, *flags, SRC, "-o", BIN], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print("snappy_elem_check:", "address + undefined sanitizers" if sanitized else "PLAIN build - no sanitizer runtime on this machine")
    return BIN, sanitized


def run(checker, chunks, tmp_path):
    path = tmp_path / "chunks.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(chunks)))
        for c in chunks:
            f.write(struct.pack("<III", c.planned_ulen(), 1 if c.compressed else 0, len(c.body)) + c.body)
    r = subprocess.run([checker[0], str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(chunks)
    return [(ln.split()[0] == "ok", int(ln.split()[1], 16 if ln.startswith("ok") else 10)) for ln in lines]


def test_every_case_of_the_streams(checker, tmp_path):
    chunks, want = [], []
    for case in ss.VALID:
        for c in case.chunks:
            chunks.append(c)
            want.append((True, ss.sj.crc32c(c.data)))
    for case in ss.CORRUPT:
        for i, c in enumerate(case.chunks):
            ok, crc = ss.judge_chunk(c)
            if i == case.bad and case.code != ss.CRC_MISMATCH:
                assert not ok, case.name
                want.append((False, case.code))
            elif ok:   # (a CRC case decodes: the checksum is the frame's, not the block's)
                want.append((True, crc))
            else:      # the second of two bad chunks
                assert "two bad chunks" in case.name and i > case.bad
                want.append((False, ss.OFFSET_ZERO))
            chunks.append(c)
    for c, code in ss.CHUNKS_ONLY:
        assert ss.judge_chunk(c) == (False, None)
        chunks.append(c)
        want.append((False, code))
    got = run(checker, chunks, tmp_path)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)
    assert {w[1] for w in want if not w[0]} == set(range(1, 8)), "every code of the parser is met"


def mutate(rng, c):
    b = bytearray(c.body)
    ulen = c.planned_ulen()
    kind = rng.integers(0, 8)
    if kind == 0 and len(b) > 1:
        del b[int(rng.integers(1, len(b))):]                                   # cut off
    elif kind == 1:
        b += rng.integers(0, 256, int(rng.integers(1, 6)), dtype=np.uint8).tobytes()   # bytes behind the end
    elif kind == 2:
        ulen = max(0, min(65536, ulen + int(rng.integers(-3, 4))))            # the plan says another length
    else:
        for _ in range(int(rng.integers(1, 4))):
            if b:
                i = int(rng.integers(0, len(b)))
                b[i] = int(rng.integers(0, 256)) if rng.integers(0, 2) else b[i] ^ (1 << int(rng.integers(0, 8)))
    return ss.DataChunk(c.compressed, bytes(b), b"", ulen=ulen)


def test_seeded_mutations(checker, tmp_path):
    base = [c for case in ss.VALID + ss.CORRUPT for c in case.chunks if len(c.body) <= 700] + [c for c, _ in ss.CHUNKS_ONLY]
    base = list({(c.compressed, c.body, c.planned_ulen()): c for c in base}.values())
    assert len(base) >= 60
    rng = np.random.default_rng(20260)
    chunks = [mutate(rng, base[int(rng.integers(0, len(base)))]) for _ in range(N_MUTATIONS)]
    got = run(checker, chunks, tmp_path)
    n_ok = 0
    for k, (c, g) in enumerate(zip(chunks, got)):
        ok, crc = ss.judge_chunk(c)
        assert g[0] == ok, (k, c.compressed, c.body.hex(), c.planned_ulen(), g)
        if ok:
            assert g[1] == crc, (k, c.body.hex())
            n_ok += 1
        else:
            assert 1 <= g[1] <= 7, g
    assert N_MUTATIONS // 20 < n_ok < N_MUTATIONS * 19 // 20, n_ok   # both verdicts are exercised
    print(f"{N_MUTATIONS} mutations of {len(base)} chunks: {n_ok} decode, {N_MUTATIONS - n_ok} are refused; sanitizers: {checker[1]}")
