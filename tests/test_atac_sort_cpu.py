"""CPU tests of the host side of `atac sort` (no GPU calls): the readers of correction_plan.bin and the legacy
permit_map.bin (include/afquant_host.h) against the writers of rad.py, and what `afquant atac sort` refuses before any
device work (src/atac/sort.rs:189-222 of the reference)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from util import ROOT, pkg

rad = pkg.rad
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")


@pytest.fixture(scope="module")
def lib():
    L = pkg.load_library()
    u64p = C.POINTER(C.c_uint64)
    L.afq_parse_correction_plan.argtypes = [C.c_char_p, C.c_size_t, u64p, u64p, C.c_size_t, C.POINTER(C.c_uint32)]
    L.afq_parse_correction_plan.restype = C.c_int64
    L.afq_parse_permit_map.argtypes = [C.c_char_p, C.c_size_t, u64p, u64p, C.c_size_t]
    L.afq_parse_permit_map.restype = C.c_int64
    L.afq_host_last_error.restype = C.c_char_p
    return L


def _pairs(n, seed=1):
    """n (observed, corrected) pairs, observed distinct, in no particular order; every other barcode has bit 63 set"""
    rng = np.random.default_rng(seed)
    obs = rng.permutation(np.unique(rng.integers(0, 1 << 62, size=2 * n + 8, dtype=np.uint64)))[:n]
    cor = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    top = np.uint64(1) << np.uint64(63)
    obs[::2] |= top
    cor[1::2] |= top
    assert len(obs) == n
    return list(zip(obs.tolist(), cor.tolist()))


def _read(lib, which, blob):
    """(count or negative code, observed, corrected, cell barcode length, message) - sized with NULL first, as a caller would"""
    u64p = C.POINTER(C.c_uint64)
    blen = C.c_uint32(0)
    if which == "plan":
        n = lib.afq_parse_correction_plan(blob, len(blob), None, None, 0, C.byref(blen))
    else:
        n = lib.afq_parse_permit_map(blob, len(blob), None, None, 0)
    if n < 0:
        return n, None, None, None, lib.afq_host_last_error().decode()
    obs, cor = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
    if which == "plan":
        m = lib.afq_parse_correction_plan(blob, len(blob), obs.ctypes.data_as(u64p), cor.ctypes.data_as(u64p), n, None)
    else:
        m = lib.afq_parse_permit_map(blob, len(blob), obs.ctypes.data_as(u64p), cor.ctypes.data_as(u64p), n)
    assert m == n
    return n, obs[:n], cor[:n], blen.value, ""


@pytest.mark.parametrize("n", [0, 1, 5000])
@pytest.mark.parametrize("spec", ["unique", ("frequency", (9, 10), 3)])
def test_correction_plan_round_trip(lib, n, spec):
    pairs = _pairs(n)
    if n:
        assert max(o for o, _ in pairs) >> 63 == 1   # barcodes with bit 63 set
    blob = rad.correction_plan_bytes(pairs, barcode_len=32, spec=spec)
    got_n, obs, cor, blen, _ = _read(lib, "plan", blob)
    assert got_n == n and blen == 32
    want = sorted(pairs)   # (the plan is written in observed order, correction_plan.rs:137-141)
    assert obs.tolist() == [o for o, _ in want] and cor.tolist() == [c for _, c in want]


@pytest.mark.parametrize("n", [0, 1, 5000])
def test_permit_map_round_trip(lib, n):
    pairs = _pairs(n, seed=2)
    got_n, obs, cor, _, _ = _read(lib, "map", rad.permit_map_bytes(pairs))
    assert got_n == n
    assert obs.tolist() == [o for o, _ in pairs] and cor.tolist() == [c for _, c in pairs]


def test_a_short_output_array_is_not_overrun(lib):
    pairs = _pairs(10)
    blob = rad.permit_map_bytes(pairs)
    u64p = C.POINTER(C.c_uint64)
    obs, cor = np.full(10, 7, np.uint64), np.full(10, 7, np.uint64)
    assert lib.afq_parse_permit_map(blob, len(blob), obs.ctypes.data_as(u64p), cor.ctypes.data_as(u64p), 4) == 10
    assert obs[:4].tolist() == [o for o, _ in pairs[:4]] and (obs[4:] == 7).all() and (cor[4:] == 7).all()


def test_malformed_files_are_refused_each_with_its_own_message(lib):
    good = rad.correction_plan_bytes(_pairs(3), barcode_len=16)
    cases = {
        "truncated header": good[:5],
        "invalid magic": b"NOTCORR\0" + good[8:],
        "unsupported format version 2": rad.correction_plan_bytes(_pairs(3), version=2),
        "truncated or malformed": good[:-7],
        "trailing data": good + b"\0",
        "sample-scoped": rad.correction_plan_bytes(_pairs(3), sample_barcode_len=8, sample_scopes=[(5, _pairs(2))]),
    }
    seen = set()
    for want, blob in cases.items():
        n, _, _, _, msg = _read(lib, "plan", blob)
        assert n == pkg._abi.AFQ_ERR_BAD_INPUT and want in msg, (want, n, msg)
        seen.add(msg)
    assert len(seen) == len(cases)
    m = rad.permit_map_bytes(_pairs(3))
    seen = set()
    for want, blob in {"truncated length": m[:4], "truncated entries": m[:-3], "trailing data": m + b"\0\0"}.items():
        n, _, _, _, msg = _read(lib, "map", blob)
        assert n == pkg._abi.AFQ_ERR_BAD_INPUT and want in msg, (want, n, msg)
        seen.add(msg)
    assert len(seen) == 3


def test_every_proper_prefix_of_a_file_is_refused(lib):
    plan = rad.correction_plan_bytes(_pairs(4), barcode_len=16, spec=("frequency", (9, 10), 2))
    for k in range(len(plan)):
        assert _read(lib, "plan", plan[:k])[0] == pkg._abi.AFQ_ERR_BAD_INPUT, k
    pm = rad.permit_map_bytes(_pairs(4))
    for k in range(len(pm)):
        assert _read(lib, "map", pm[:k])[0] == pkg._abi.AFQ_ERR_BAD_INPUT, k
    # a length field that promises more entries than the file can hold is not believed
    huge = (1 << 60).to_bytes(8, "little") + pm[8:]
    assert _read(lib, "map", huge)[0] == pkg._abi.AFQ_ERR_BAD_INPUT


def _input_dir(path, version_str=True, bins=True):
    os.makedirs(path, exist_ok=True)
    meta = {"gpl_options": {"rc": True}, "num-chunks": 0}
    if version_str:
        meta["version_str"] = "0.18.0"
    with open(os.path.join(path, "generate_permit_list.json"), "w") as f:
        json.dump(meta, f)
    if bins:
        for name in ("bin_recs.bin", "bin_lens.bin"):
            with open(os.path.join(path, name), "wb") as f:
                f.write((0).to_bytes(8, "little"))
    with open(os.path.join(path, "permit_freq.bin"), "wb") as f:
        f.write(rad.permit_freq_header(16))


def test_cli_refuses_before_any_device_work(tmp_path):
    """No map.rad exists in any of these directories, and none of the messages is about it: the refusals come first."""
    if not os.path.exists(CLI):
        import __graft_entry__ as ge

        ge.build()
    ok = str(tmp_path / "ok")
    _input_dir(ok)
    r = subprocess.run([CLI, "atac", "sort", "-i", ok], capture_output=True, text=True)
    assert r.returncode == 2 and "--rad-dir" in r.stderr
    nobins = str(tmp_path / "nobins")
    _input_dir(nobins, bins=False)
    r = subprocess.run([CLI, "atac", "sort", "-i", nobins, "-r", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 1 and "bin file containing records does not exist" in r.stderr
    nover = str(tmp_path / "nover")
    _input_dir(nover, version_str=False)
    r = subprocess.run([CLI, "atac", "sort", "-i", nover, "-r", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 1 and "does not contain a version_str field" in r.stderr
    for d in (nobins, nover):
        assert not os.path.exists(os.path.join(d, "sort.json")) and not os.path.exists(os.path.join(d, "map.bed"))
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "atac sort -i <input-dir> -r <rad-dir>" in r.stderr
