"""The device inflater's parser (csrc/afq_inflate_elem.h) on the host: tests/inflate_elem_check.cpp decodes payloads with the
parser and a serial executor, built with the address and undefined-behaviour sanitizers and run as a program of its own.  Every
payload of tests/deflate_streams.py and its 10^4 seeded mutations: the program's verdict, code, tallies and the CRC-32 of its
bytes are the judge's (tests/inflate_judge.py), and no mutation makes it touch a byte outside the payload, the output or the
decode tables."""
import os
import shutil
import struct
import subprocess

import pytest

import deflate_streams as ds
import inflate_judge as ij

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "inflate_elem_check.cpp")
BIN = os.path.join(HERE, "_build", "inflate_elem_check")


@pytest.fixture(scope="module")
def checker():
    """(path, sanitized): the sanitizer build where the machine has the sanitizers' runtime, a plain one otherwise"""
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    probe = os.path.join(os.path.dirname(BIN), "inflate_probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([cxx, *san, probe, "-o", probe + ".out"], capture_output=True, text=True)
    sanitized = r.returncode == 0 and subprocess.run([probe + ".out"], capture_output=True).returncode == 0
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + (san if sanitized else [])
    r = subprocess.run([cxx, *flags, SRC, "-o", BIN], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print("inflate_elem_check:", "address + undefined sanitizers" if sanitized else "PLAIN build - no sanitizer runtime on this machine")
    return BIN, sanitized


def run(checker, payloads, tmp_path):
    """payloads: (body, isize) each -> ("ok", crc, tallies) or ("err", code, produced) each"""
    path = tmp_path / "payloads.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(payloads)))
        for body, isize in payloads:
            f.write(struct.pack("<II", isize, len(body)) + body)
    r = subprocess.run([checker[0], str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(payloads)
    out = []
    for ln in lines:
        w = ln.split()
        out.append(("ok", int(w[1], 16), tuple(int(x) for x in w[2:])) if w[0] == "ok" else ("err", int(w[1]), int(w[2])))
    return out


def judged(t):
    if t.code:
        return ("err", t.code, t.produced)
    return ("ok", ij.crc32(t.data), (t.n_stored, t.n_fixed, t.n_dynamic, t.n_literals, t.n_copies))


def test_every_payload_of_the_cases(checker, tmp_path):
    payloads = [(p.body, p.isize) for p in ds.all_payloads()]
    want = [judged(ij.inflate(b, n)) for b, n in payloads]   # (without the trailer's CRC: the parser does not see it)
    got = run(checker, payloads, tmp_path)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)
    assert {w[1] for w in want if w[0] == "err"} == set(range(1, ij.CODE_COUNT)) - {ij.CRC_MISMATCH}, "every code of the parser is met"
    assert sum(w[0] == "ok" for w in want) >= sum(len(c.payloads) for c in ds.VALID)


def test_seeded_mutations(checker, tmp_path):
    muts, tallies = ds.mutations()
    got = run(checker, muts, tmp_path)
    n_ok = 0
    for k, ((body, isize), t, g) in enumerate(zip(muts, tallies, got)):
        assert g == judged(t), (k, body.hex(), isize, g, judged(t))
        n_ok += g[0] == "ok"
    assert ds.N_MUTATIONS // 20 <= n_ok <= ds.N_MUTATIONS * 19 // 20, n_ok   # both verdicts are exercised
    print(f"{ds.N_MUTATIONS} mutations: {n_ok} decode, {ds.N_MUTATIONS - n_ok} are refused; sanitizers: {checker[1]}")
