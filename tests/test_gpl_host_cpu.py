"""CPU tests of generate-permit-list's host half (csrc/afq_gpl_host.h behind include/afquant_host.h): the retained-set rules and the
knee, the confidence and barcode-list parsers and the file writers, through host-only entry points against tests/gpl_judge.py;
and the same code in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

import gpl_judge as J
from util import ROOT, pkg

rad = pkg.rad
INVALID_ARG, BAD_INPUT = pkg._abi.AFQ_ERR_INVALID_ARG, pkg._abi.AFQ_ERR_BAD_INPUT
KNEE, EXPECT, FORCE, VALID_BC, UNFILTERED = range(5)
u64p = C.POINTER(C.c_uint64)


class GplOpts(C.Structure):
    _fields_ = [("input_dir", C.c_char_p), ("output_dir", C.c_char_p), ("expected_ori", C.c_uint32), ("method", C.c_uint32), ("method_count", C.c_uint64),
                ("list_file", C.c_char_p), ("min_reads", C.c_uint64), ("frequency", C.c_uint32), ("neighborhood", C.c_int32), ("conf_num", C.c_uint64),
                ("conf_den", C.c_uint64), ("num_threads", C.c_uint32), ("device", C.c_uint32), ("cmdline", C.c_char_p), ("fill_bytes", C.c_uint64),
                ("corrected_out", u64p)]


class GplTables(C.Structure):
    _fields_ = [("barcode_len", C.c_uint32), ("neighborhood", C.c_uint32), ("frequency", C.c_uint32), ("filtered", C.c_uint32), ("conf_num", C.c_uint64),
                ("conf_den", C.c_uint64), ("pseudocount", C.c_uint64), ("freq_bc", u64p), ("freq_count", u64p), ("n_freq", C.c_uint64), ("all_bc", u64p),
                ("all_count", u64p), ("n_all", C.c_uint64), ("map_obs", u64p), ("map_cor", u64p), ("n_map", C.c_uint64), ("plan_obs", u64p),
                ("plan_cor", u64p), ("n_plan", C.c_uint64), ("stats", C.c_uint64 * 8), ("max_ambig", C.c_uint64)]


@pytest.fixture(scope="module")
def lib():
    l = pkg.load_library()
    l.afq_host_last_error.restype = C.c_char_p
    l.afq_gpl_parse_confidence.argtypes = [C.c_char_p, u64p, u64p]
    l.afq_gpl_parse_barcode_list.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_uint32, u64p, C.c_size_t, C.POINTER(C.c_uint32)]
    l.afq_gpl_parse_barcode_list.restype = C.c_int64
    l.afq_gpl_knee.argtypes = [u64p, C.c_size_t]
    l.afq_gpl_knee.restype = C.c_int64
    l.afq_gpl_select_retained.argtypes = [u64p, u64p, C.c_size_t, C.c_uint32, C.c_uint64, u64p, C.c_size_t]
    l.afq_gpl_select_retained.restype = C.c_int64
    l.afq_gpl_write_outputs.argtypes = [C.POINTER(GplOpts), C.POINTER(GplTables)]
    return l


def err(lib):
    return (lib.afq_host_last_error() or b"").decode()


def arr(v):
    return np.ascontiguousarray(v, dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(u64p)


# ------------------------------------------------------------------------------------------------------------- confidence
def confidence(lib, text):
    n, d = C.c_uint64(), C.c_uint64()
    rc = lib.afq_gpl_parse_confidence(text.encode(), C.byref(n), C.byref(d))
    return rc, (int(n.value), int(d.value))


def test_confidence_parser(lib):
    assert confidence(lib, "0.975") == (0, (39, 40))
    assert confidence(lib, "39/40") == (0, (39, 40))
    assert confidence(lib, "90/100") == (0, (9, 10))
    assert confidence(lib, "1") == (0, (1, 1))
    assert confidence(lib, "0") == (0, (0, 1))
    assert confidence(lib, " 0.5 ") == (0, (1, 2))
    assert confidence(lib, "0.123456789012345678") == (0, (61728394506172839, 500000000000000000))   # 18 digits still fit
    for bad in ("1.5", "3/0", "1.01", "41/40", "NaN", "", ".5", "0.1234567890123456789", "-0.5", "1/2/3", "0x1", "1e-1"):
        rc, _ = confidence(lib, bad)
        assert rc == INVALID_ARG, bad
    assert confidence(lib, "1.5")[0] == INVALID_ARG and "between zero and one (got 15/10)" in err(lib)   # (as the reference: before reduction)
    assert confidence(lib, "0.1234567890123456789")[0] == INVALID_ARG and "invalid barcode-correction confidence" in err(lib)


# ------------------------------------------------------------------------------------------------------------ barcode lists
def parse_list(lib, text, unfiltered, L):
    b = text.encode()
    first = C.c_uint32()
    n = lib.afq_gpl_parse_barcode_list(b, len(b), int(unfiltered), L, None, 0, C.byref(first))
    if n < 0:
        return int(n), err(lib)
    out = np.zeros(max(int(n), 1), np.uint64)
    assert lib.afq_gpl_parse_barcode_list(b, len(b), int(unfiltered), L, ptr(out), int(n), None) == n
    return out[:n].tolist(), int(first.value)


def test_barcode_list_parsing(lib):
    enc = rad.seq_to_int
    for unf in (True, False):
        got, first = parse_list(lib, "ACGT\nTTTT\nAAAA\nACGT\n", unf, 4)
        assert got == [enc("ACGT"), enc("TTTT"), 0, enc("ACGT")] == J.parse_barcode_list("ACGT\nTTTT\nAAAA\nACGT\n", unf, 4)   # file order, duplicates kept
        if unf:
            assert first == 4
    # CRLF, and no newline behind the last line
    for text in ("ACGT\r\nTTTT\r\n", "ACGT\r\nTTTT", "acgt\ntttt\n"):
        for unf in (True, False):
            assert parse_list(lib, text, unf, 4)[0] == [enc("ACGT"), enc("TTTT")] == J.parse_barcode_list(text, unf, 4)
    # an empty file
    assert parse_list(lib, "", True, 4) == ([], 0) and parse_list(lib, "", False, 4)[0] == []
    # -u: a line with N contributes nothing; -b: it is an error
    assert parse_list(lib, "ACGT\nACNT\nTTTT\n", True, 4)[0] == [enc("ACGT"), enc("TTTT")] == J.parse_barcode_list("ACGT\nACNT\nTTTT\n", True, 4)
    rc, msg = parse_list(lib, "ACGT\nACNT\nTTTT\n", False, 4)
    assert rc == BAD_INPUT and "can't extract kmer" in msg
    with pytest.raises(ValueError):
        J.parse_barcode_list("ACGT\nACNT\nTTTT\n", False, 4)
    # -u: mixed lengths are an error; -b takes the first valid window of a longer line
    rc, msg = parse_list(lib, "ACGT\nACG\n", True, 4)
    assert rc == BAD_INPUT and "found barcodes of different lengths 4 and 3" in msg
    with pytest.raises(ValueError, match="different lengths 4 and 3"):
        J.parse_barcode_list("ACGT\nACG\n", True, 4)
    assert parse_list(lib, "NACGTA\nACGT\n", False, 4)[0] == [enc("ACGT")] * 2 == J.parse_barcode_list("NACGTA\nACGT\n", False, 4)
    # the first base is the most significant; 32 bases fill the u64
    assert parse_list(lib, "T" + "A" * 31 + "\n", True, 32)[0] == [3 << 62]
    assert parse_list(lib, "C" * 33 + "\n", True, 0) == ([], 33)   # (no k-mer of 33 bases)


# ------------------------------------------------------------------------------------------------------------ retained set
def select(lib, hist, method, arg=0):
    bcs = sorted(hist)
    bc, cnt = arr(bcs), arr([hist[b] for b in bcs])
    n = lib.afq_gpl_select_retained(ptr(bc), ptr(cnt), len(bcs), method, arg, None, 0)
    if n < 0:
        return int(n), err(lib)
    out = np.zeros(max(int(n), 1), np.uint64)
    assert lib.afq_gpl_select_retained(ptr(bc), ptr(cnt), len(bcs), method, arg, ptr(out), int(n)) == n
    return out[:n].tolist()


def two_population_hist(seed=1, n_cells=60, n_bg=300):
    rng = random.Random(seed)
    hist = {}
    while len(hist) < n_cells:
        hist[rng.randrange(1 << 32)] = rng.randrange(800, 1500)
    while len(hist) < n_cells + n_bg:
        hist.setdefault(rng.randrange(1 << 32), rng.randrange(1, 12))
    return hist


def test_knee_against_the_judge(lib):
    for seed in (1, 2, 3):
        hist = two_population_hist(seed)
        freqs = sorted(hist.values(), reverse=True)
        a = arr(freqs)
        knee = lib.afq_gpl_knee(ptr(a), len(a))
        assert knee == J.get_knee(freqs) and 40 <= knee <= 80      # the knee sits at the end of the cell population
        assert select(lib, hist, KNEE) == J.select_retained(hist, "knee")
    for freqs in ([100, 90, 80, 5, 4, 3, 2, 1, 1, 1], [4, 2, 1, 1], [10, 9, 8, 7, 6, 5, 4, 3, 2, 1]):
        a = arr(freqs)
        assert lib.afq_gpl_knee(ptr(a), len(a)) == J.get_knee(freqs), freqs


def test_knee_refusals_carry_the_references_sentence(lib):
    for freqs in ([7], [5, 5]):
        a = arr(freqs)
        assert lib.afq_gpl_knee(ptr(a), len(a)) == BAD_INPUT
        assert "the list of putative cells is only of length 1. Cannot proceed. Please check the mapping rate." in err(lib)
        with pytest.raises(ValueError, match="only of length 1"):
            J.get_knee(freqs)
    assert select(lib, {1: 7}, KNEE)[0] == BAD_INPUT
    assert select(lib, {}, KNEE) == []   # an empty histogram retains nothing (cellfilter.rs:750-752)


def test_force_and_expect_cells(lib):
    hist = {10: 50, 11: 40, 12: 40, 13: 40, 14: 3, 15: 1}
    for n in (0, 1, 2, 3, 4, 5, 6, 7, 99):
        assert select(lib, hist, FORCE, n) == J.select_retained(hist, "force", n), n
    assert select(lib, hist, FORCE, 2) == [10, 11, 12, 13] and select(lib, hist, FORCE, 0) == [] and len(select(lib, hist, FORCE, 99)) == 6
    # 150 * 0.99 = 148.5 rounds half away from zero to index 149
    big = {i: (1000 if i < 148 else 100 if i == 148 else 40 if i == 149 else 5 + i % 5) for i in range(200)}
    assert select(lib, big, EXPECT, 150) == J.select_retained(big, "expect", 150) == list(range(200))
    for n in (1, 2, 3, 50, 148, 149, 151, 1000):
        assert select(lib, big, EXPECT, n) == J.select_retained(big, "expect", n), n
    assert select(lib, {1: 4, 2: 3, 3: 1}, EXPECT, 3) == [1, 2, 3]   # a threshold that rounds to 0 is lifted to 1
    hist = two_population_hist(4)
    assert select(lib, hist, EXPECT, 60) == J.select_retained(hist, "expect", 60)
    assert select(lib, hist, UNFILTERED, 10) == J.select_retained(hist, "unfiltered", min_reads=10)


# ------------------------------------------------------------------------------------------------------------------ writers
def tables_for(want, L, resolution):
    """the judge's maps as the C tables (every list ascending)"""
    t = GplTables()
    keep = []
    def put(name_a, name_b, name_n, pairs):
        a, b = arr([p[0] for p in pairs]), arr([p[1] for p in pairs])
        keep.extend([a, b])
        setattr(t, name_a, ptr(a)); setattr(t, name_b, ptr(b)); setattr(t, name_n, len(pairs))
    put("freq_bc", "freq_count", "n_freq", sorted(want["permit_freq"].items()))
    if want["all_freq"] is not None:
        put("all_bc", "all_count", "n_all", sorted(want["all_freq"].items()))
    put("map_obs", "map_cor", "n_map", sorted(want["permit_map"].items()))
    put("plan_obs", "plan_cor", "n_plan", want["plan"])
    t.barcode_len, t.neighborhood, t.filtered = L, rad.NEIGHBORHOOD_TAGS[want["neighborhood"]], int(want["all_freq"] is not None)
    t.frequency = int(resolution != "unique")
    if resolution != "unique":
        t.conf_num, t.conf_den, t.pseudocount = resolution[1][0], resolution[1][1], resolution[2]
    for i, k in enumerate(f"{d}_{x}" for d in (J.EXACT, J.CORRECTED, J.AMBIGUOUS, J.NOT_FOUND) for x in ("distinct", "reads")):
        t.stats[i] = want["stats"][k]
    t.max_ambig = want["max_ambig"]
    return t, keep


def read_outputs(d):
    out = {}
    for name in ("permit_freq.bin", "all_freq.bin", "permit_map.bin", "correction_plan.bin"):
        p = os.path.join(d, name)
        out[name] = open(p, "rb").read() if os.path.exists(p) else None
    out["json"] = json.load(open(os.path.join(d, "generate_permit_list.json")))
    return out


def check_outputs(d, want, L, resolution):
    """the five files of directory d against the judge's maps (shared with tests/test_gpu_gpl_cli.py)"""
    f = read_outputs(d)
    assert rad.read_permit_freq(f["permit_freq.bin"]) == (1, L, want["permit_freq"])
    if want["all_freq"] is None:
        assert f["all_freq.bin"] is None
    else:
        assert rad.read_permit_freq(f["all_freq.bin"]) == (1, L, want["all_freq"])
    assert rad.read_permit_map(f["permit_map.bin"]) == want["permit_map"]
    plan = rad.read_correction_plan(f["correction_plan.bin"])
    assert plan == {"barcode_len": L, "neighborhood": want["neighborhood"], "resolution": resolution, "corrections": want["plan"]}
    j = f["json"]
    assert set(j) == {"velo_mode", "expected_ori", "version_str", "max-ambig-record", "cmd", "permit-list-type", "gpl_options", "resolved_cell_bc_neighborhood",
                      "resolved_cell_bc_confidence", "correction_stats"}
    assert j["velo_mode"] is False and j["version_str"] == "0.18.0" and j["max-ambig-record"] == want["max_ambig"]
    assert j["permit-list-type"] == want["permit_list_type"] and j["resolved_cell_bc_neighborhood"] == want["neighborhood"]
    assert j["correction_stats"] == want["stats"]
    return j


@pytest.mark.parametrize("method", ["force", "unfiltered"])
@pytest.mark.parametrize("resolution", ["unique", ("frequency", (19, 20), 1)], ids=["unique", "frequency"])
def test_writers_round_trip_the_judges_maps(lib, tmp_path, method, resolution):
    rng = random.Random(5)
    cells = [rng.randrange(1 << 16) for _ in range(5)]
    recs = [(rng.choice(cells) ^ (1 << rng.randrange(16) if rng.random() < 0.2 else 0), 0, [(1, True)] * rng.choice([1, 1, 2, 7])) for _ in range(400)]
    kw = {"arg": 4} if method == "force" else {"listed": cells + [12345], "min_reads": 3}
    want = J.gpl_outputs([recs], "fw", method, 8, resolution=resolution, **kw)
    assert want["stats"]["corrected_distinct"] > 0 and len(want["permit_map"]) > len(want["permit_freq"])
    t, keep = tables_for(want, 8, resolution)
    out = str(tmp_path / "deep" / "out")
    o = GplOpts(input_dir=b"in dir", output_dir=out.encode(), expected_ori=1, method=FORCE if method == "force" else UNFILTERED, method_count=4,
                list_file=b'a "quoted" list', min_reads=3, frequency=int(resolution != "unique"), neighborhood=-1, num_threads=2, cmdline=b"afquant generate-permit-list -k")
    if resolution != "unique":
        o.conf_num, o.conf_den = resolution[1]
    assert lib.afq_gpl_write_outputs(C.byref(o), C.byref(t)) == 0, err(lib)
    j = check_outputs(out, want, 8, resolution)
    assert j["expected_ori"] == "fw" and j["cmd"] == "afquant generate-permit-list -k"
    assert j["resolved_cell_bc_confidence"] == ("19/20" if resolution != "unique" else "39/40")
    g = j["gpl_options"]
    assert g["input_dir"] == "in dir" and g["cell_bc_neighborhood"] is None and g["cell_bc_correction"] == ("unique" if resolution == "unique" else "frequency")
    assert g["fmeth"] == ({"ForceCells": 4} if method == "force" else {"UnfilteredExternalList": ['a "quoted" list', 3]})
    # the project's own readers take the files (afq_parse_permit_map and the plan reader)
    lib.afq_parse_permit_map.restype = C.c_int64
    lib.afq_parse_correction_plan.restype = C.c_int64
    lib.afq_parse_permit_map.argtypes = [C.c_char_p, C.c_size_t, u64p, u64p, C.c_size_t]
    lib.afq_parse_correction_plan.argtypes = [C.c_char_p, C.c_size_t, u64p, u64p, C.c_size_t, C.POINTER(C.c_uint32)]
    pm = open(os.path.join(out, "permit_map.bin"), "rb").read()
    n = len(want["permit_map"])
    a, b = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    assert lib.afq_parse_permit_map(pm, len(pm), ptr(a), ptr(b), n) == n and dict(zip(a.tolist(), b.tolist())) == want["permit_map"]
    cp = open(os.path.join(out, "correction_plan.bin"), "rb").read()
    n = len(want["plan"])
    a, b, cl = np.zeros(n, np.uint64), np.zeros(n, np.uint64), C.c_uint32()
    assert lib.afq_parse_correction_plan(cp, len(cp), ptr(a), ptr(b), n, C.byref(cl)) == n, err(lib)
    assert list(zip(a.tolist(), b.tolist())) == want["plan"] and cl.value == 8


def test_rad_writers_and_readers_agree():
    pairs = [(9, 2), (3, 3), (5, 3)]
    assert rad.read_permit_freq(rad.permit_freq_bytes(16, pairs)) == (1, 16, dict(pairs))
    assert rad.permit_freq_bytes(16, [])[:16] == rad.permit_freq_header(16)[:16]
    assert rad.read_permit_map(rad.permit_map_bytes(pairs)) == dict(pairs)
    for nbh in ("hamming-1", "substitution-or-shift-1"):
        for spec in ("unique", ("frequency", (39, 40), 1)):
            got = rad.read_correction_plan(rad.correction_plan_bytes(pairs, 12, spec, neighborhood=nbh))
            assert got == {"barcode_len": 12, "neighborhood": nbh, "resolution": spec, "corrections": sorted(pairs)}
    with pytest.raises(ValueError):
        rad.read_permit_map(rad.permit_map_bytes(pairs) + b"\0")


# ------------------------------------------------------------------------------------------------------------ chunk table
def refused(lib, tmp_path, code, sentence, num_chunks=2, cut=0):
    """afq_generate_permit_list on a map.rad of two one-record chunks less its last `cut` bytes, whose prelude announces num_chunks"""
    os.makedirs(tmp_path / "map")
    body, _ = rad.encode_chunks([[(0x11, 1, [(1, True)])], [(0x22, 2, [(0, True)])]])
    blob = rad.rad_prelude(["t0", "t1"], num_chunks, 16, 12, 4, 4) + body
    (tmp_path / "map" / "map.rad").write_bytes(blob[:len(blob) - cut])
    lib.afq_generate_permit_list.argtypes = [C.POINTER(GplOpts)]
    o = GplOpts(input_dir=str(tmp_path / "map").encode(), output_dir=str(tmp_path / "out").encode(), expected_ori=1, method=KNEE, neighborhood=-1)
    rc = lib.afq_generate_permit_list(C.byref(o))
    assert rc == code and sentence in err(lib), (rc, err(lib))
    assert not (tmp_path / "out").exists()


def test_a_truncated_chunk_table(lib, tmp_path):
    """the prelude promises three chunks and the file holds two; the last chunk's nbytes runs past the file's end.  Both are refused
    before a device is opened."""
    refused(lib, tmp_path / "a", BAD_INPUT, "map.rad ends before chunk 2 of 3", num_chunks=3)
    refused(lib, tmp_path / "b", BAD_INPUT, "corrupt chunk header (chunk 1)", cut=4)


# ---------------------------------------------------------------------------------------------------------------- sanitizers
SAN_MAIN = r'''
#include "afq_gpl_host.h"
#include "afq_chunk_table.h"
#include <cassert>
using namespace afq::gplhost;
int main(int argc, char** argv) {
    std::string err;
    // ---- list parser: exact-size heap copies, so that a read past the text is seen
    const char* texts[] = {"", "\n", "\r\n", "ACGT", "ACGT\r", "ACGT\r\nTTTT", "ACNT\nACGT\n", "NNNN", "A", "ACGTACGTACGTACGTACGTACGTACGTACGTA\n", "\n\nACGT"};
    for (const char* t : texts)
        for (int unf = 0; unf < 2; ++unf)
            for (uint32_t L : {1u, 4u, 32u}) {
                const size_t n = std::strlen(t);
                std::vector<uint8_t> heap(t, t + n);
                uint32_t first = 0;
                const int64_t k = parse_barcode_list(heap.data(), n, unf, L, nullptr, 0, &first, err);
                if (k > 0) {
                    std::vector<uint64_t> out((size_t)k);
                    assert(parse_barcode_list(heap.data(), n, unf, L, out.data(), out.size(), nullptr, err) == k);
                    std::vector<uint64_t> less((size_t)k - 1 + 1);   // a smaller cap writes no more than cap
                    parse_barcode_list(heap.data(), n, unf, L, less.data(), (size_t)k - 1, nullptr, err);
                }
            }
    // ---- confidence
    uint64_t a = 0, b = 0;
    for (const char* t : {"0.975", "39/40", "1", "0", "1.5", "3/0", "0.1234567890123456789", "18446744073709551615/18446744073709551615", "18446744073709551616/1", "18446744073709551615.5", ""})
        parse_confidence(t, &a, &b, err);
    assert(parse_confidence("0.975", &a, &b, err) == 0 && a == 39 && b == 40);
    // ---- knee and selection at the edges
    const uint64_t one[1] = {7}, flat[3] = {5, 5, 5}, top[2] = {~0ull >> 1, ~0ull >> 1};
    assert(knee(one, 1, err) < 0 && knee(nullptr, 0, err) < 0);
    knee(flat, 3, err); knee(top, 2, err);
    const uint64_t bc[4] = {1, 2, 3, 4}, cnt[4] = {9, 9, 1, 5};
    uint64_t out[4];
    for (uint32_t m : {0u, 1u, 2u, 4u}) for (uint64_t arg : {0ull, 1ull, 2ull, 1000ull, ~0ull}) select_retained(bc, cnt, 4, m, arg, out, 4, err);
    assert(select_retained(bc, cnt, 4, AFQ_GPL_FORCE, 2, out, 1, err) == 2);   // counts beyond cap, writes cap
    // ---- neighbours at both ends of the u64
    std::vector<uint64_t> nb;
    for (uint32_t L : {1u, 2u, 31u, 32u}) for (uint64_t x : {0ull, ~0ull >> (64 - 2 * L)}) { gpl_push_neighbors(x, L, true, nb); }
    // ---- writers
    if (argc > 1) {
        afq_gpl_opts o{};
        o.input_dir = "in"; o.output_dir = argv[1]; o.method = AFQ_GPL_UNFILTERED; o.list_file = "list \"x\"\n"; o.min_reads = 10; o.neighborhood = -1;
        afq_gpl_tables t{};
        t.barcode_len = 16; t.frequency = 1; t.conf_num = 39; t.conf_den = 40; t.pseudocount = 1;
        std::vector<uint64_t> k = {1, 2, 3}, v = {4, 5, 6};
        t.freq_bc = k.data(); t.freq_count = v.data(); t.n_freq = 3; t.map_obs = k.data(); t.map_cor = v.data(); t.n_map = 3; t.plan_obs = k.data(); t.plan_cor = v.data(); t.n_plan = 3;
        assert(write_outputs(&o, &t, err) == 0);
        afq_gpl_tables e{};   // empty tables: null pointers with zero lengths
        e.barcode_len = 1; e.filtered = 1;
        assert(write_outputs(&o, &e, err) == 0);
    }
    // ---- chunk-table checks at wrapping sizes
    using namespace afq;
    assert(!chunk_header_inside(~0ull, ~0ull) && !chunk_header_inside(0, 7) && chunk_header_inside(~0ull - 8, ~0ull));
    assert(check_chunk_header(~0ull - 7, 8, 0, ~0ull, 6) == kChunkSize);
    assert(check_chunk_header(0, 0xFFFFFFFFu, 0xFFFFFFFFu, 1ull << 40, 20) == kChunkRecords);
    assert(check_chunk_header(0, 0xFFFFFFFFu, 0, 0xFFFFFFFEull, 6) == kChunkSize);
    assert(check_chunk_header((1ull << 40) - 8, 8, 0, 1ull << 40, 6) == kChunkOk);
    const uint64_t offs[3] = {0, ~0ull, 8};
    assert(first_chunk_outside(offs, 3, 64) == 1);
    std::puts("clean");
    return 0;
}
'''


def test_host_pieces_under_the_sanitizers(tmp_path):
    """a stand-alone program with its own main over csrc/afq_gpl_host.h and csrc/afq_chunk_table.h, built with
    -fsanitize=address,undefined and run here (nothing is loaded into python under a sanitizer)"""
    src = tmp_path / "san.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "san"
    csrc = os.path.join(ROOT, "alevin-fry_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", csrc, "-o", str(exe), str(src)], check=True, capture_output=True)
    out = tmp_path / "out"
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "clean", r.stdout + r.stderr
    assert rad.read_permit_freq((out / "permit_freq.bin").read_bytes()) == (1, 1, {})
