"""CPU tests of multi-barcode generate-permit-list's host half (csrc/afq_gpl_host.h behind include/afquant_host.h): the sample list and
its error sentences, the routing entries against tests/gpl_multi_judge.py, the prelude refusals of afq_generate_permit_list_multi (they
precede any device work), the argument checks of afq_gpl_multi_hist_rad that precede device work, and the same code in a stand-alone
program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpl_judge as J
import gpl_multi_cases as MC
import gpl_multi_judge as M
from util import ROOT, pkg

rad = pkg.rad
INVALID_ARG, BAD_INPUT, UNSUPPORTED = pkg._abi.AFQ_ERR_INVALID_ARG, pkg._abi.AFQ_ERR_BAD_INPUT, pkg._abi.AFQ_ERR_UNSUPPORTED
u64p = C.POINTER(C.c_uint64)
MODES = {"exact": 0, "unique": 1, "frequency": 2, "1-edit": 3}
NBH = {J.HAMMING: 0, J.SHIFT: 1}


@pytest.fixture(scope="module")
def lib():
    l = pkg.load_library()
    l.afq_host_last_error.restype = C.c_char_p
    l.afq_gpl_multi_routing.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, u64p, u64p, C.POINTER(C.c_uint8), C.c_size_t,
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    l.afq_gpl_multi_routing.restype = C.c_int64
    l.afq_gpl_multi_check_args.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p, C.c_uint64]
    l.afq_gpl_multi_check_args.restype = C.c_int
    return l


def err(lib):
    return (lib.afq_host_last_error() or b"").decode()


def routing(lib, text, mode="exact", nbh=J.HAMMING, reverse=False):
    b = text.encode()
    L, ns = C.c_uint32(), C.c_uint32()
    n = lib.afq_gpl_multi_routing(b, len(b), int(reverse), MODES[mode], NBH[nbh], None, None, None, 0, C.byref(L), C.byref(ns))
    if n < 0:
        return int(n), err(lib)
    ent, tgt, kind = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint8)
    assert lib.afq_gpl_multi_routing(b, len(b), int(reverse), MODES[mode], NBH[nbh], ent.ctypes.data_as(u64p), tgt.ctypes.data_as(u64p),
                                     kind.ctypes.data_as(C.POINTER(C.c_uint8)), n, None, None) == n
    return {"entry": ent[:n].tolist(), "target": tgt[:n].tolist(), "kind": kind[:n].tolist(), "L": int(L.value), "n_samples": int(ns.value)}


def want_routing(text, mode, nbh, reverse=False):
    info = M.load_sample_list(text, reverse)
    r = M.build_routing(info, M.sample_spec(mode, nbh))
    kind = [2 if b in r["deferred"] else (0 if b in info["rotations"] else 1) for b in r["entries"]]
    return {"entry": r["entries"], "target": [r["permit_map"].get(b, 0) for b in r["entries"]], "kind": kind, "L": info["L"], "n_samples": len(info["canonical"])}


# ------------------------------------------------------------------------------------------------------------ sample list
@pytest.mark.parametrize("text, sentence", [
    ("ACGT\tACG\tx\n", "sample barcode 'ACGT' and its canonical barcode 'ACG' have different lengths"),
    ("A" * 33 + "\n", "sample barcode length 33 is unsupported; expected 1 through 32 bases"),
    ("ACGT\nACG\n", "sample barcode file mixes lengths 4 and 3"),
    ("ACNT\n", "couldn't pack sample barcode: ACNT"),
    ("ACGT\tACNT\tx\n", "couldn't pack sample barcode: ACNT"),
    ("ACGT\tAAAA\ts1\nACGT\tCCCC\ts2\n", "sample construction barcode 'ACGT' is assigned to conflicting canonical barcodes"),
    ("ACGT\tAAAA\ts1\nACGA\tAAAA\ts2\n", "canonical sample barcode 'AAAA' is assigned conflicting names 's1' and 's2'"),
    ("# nothing\n\n", "contains no barcodes"),
    ("", "contains no barcodes"),
])
def test_every_sample_list_error_sentence(lib, text, sentence):
    rc, msg = routing(lib, text)
    assert rc == BAD_INPUT and sentence in msg, msg
    with pytest.raises(ValueError) as e:   # the judge bails with the same sentence
        M.load_sample_list(text)
    assert sentence in str(e.value)


def test_reverse_complements_before_it_packs(lib):
    # under reverse the conflict sentences quote the reverse-complemented text, as the reference's do
    rc, msg = routing(lib, "ACGT\tAAAA\ts1\nACGA\tAAAA\ts2\n", reverse=True)
    assert rc == BAD_INPUT and "canonical sample barcode 'TTTT' is assigned conflicting names 's1' and 's2'" in msg


def test_unknown_modes_are_refused(lib):
    assert lib.afq_gpl_multi_routing(b"ACGT\n", 5, 0, 4, 0, None, None, None, 0, None, None) == INVALID_ARG
    assert lib.afq_gpl_multi_routing(b"ACGT\n", 5, 0, 1, 2, None, None, None, 0, None, None) == INVALID_ARG


LISTS = {
    "one column": "# c\nACGT\n\nTTTT\r\nACGA\n",
    "two columns": "ACGT\tfirst sample\n  TTTT\tsecond\t\nACGA\tthird\n",
    "rotations": "ACGT\tAAAA\ts1\textra\nAAAC\tAAAA\ts1\nTTTT\tTTTT\ts2\nTTTA\tTTTT\ts2\nACGA\tGGGG\ts3\n",
    "length 1": "A\nG\n",
    "design": MC.sample_rows(MC.routing_design()[0]),
    "design reversed": MC.sample_rows(MC.routing_design()[0], reverse=True),
}


@pytest.mark.parametrize("name", sorted(LISTS))
@pytest.mark.parametrize("mode", M.SAMPLE_MODES)
@pytest.mark.parametrize("nbh", [J.HAMMING, J.SHIFT])
def test_routing_entries_against_the_judge(lib, name, mode, nbh):
    rev = name == "design reversed"
    got, want = routing(lib, LISTS[name], mode, nbh, rev), want_routing(LISTS[name], mode, nbh, rev)
    assert got == want
    assert got["entry"] == sorted(set(got["entry"])) and (2 in got["kind"]) <= (mode == "frequency")


def test_the_design_has_every_kind_of_sample_barcode(lib):
    rows, kinds = MC.routing_design()
    got = routing(lib, MC.sample_rows(rows), "frequency")
    kind = dict(zip(got["entry"], got["kind"]))
    assert all(kind[b] == 0 for b in kinds["exact"]) and all(kind[b] == 1 for b in kinds["unique"])
    assert all(kind[b] == 2 for b in kinds["ambig_a0_b0"] + kinds["ambig_a1_b1"]) and not any(b in kind for b in kinds["none"])
    assert routing(lib, MC.sample_rows(rows, reverse=True), "frequency", reverse=True) == got and got["n_samples"] == 3 and got["L"] == 8


# --------------------------------------------------------------------------------------------------------------- arguments
def check_args(lib, entries, b0=2, b1=4, umi=4, ori=0):
    a = np.ascontiguousarray(entries, dtype=np.uint64)
    return lib.afq_gpl_multi_check_args(b0, b1, umi, ori, a.ctypes.data_as(u64p), len(a))


def test_argument_checks_that_precede_device_work(lib):
    assert check_args(lib, []) == 0 and check_args(lib, [0, 1, 0xFFFF]) == 0 and check_args(lib, [0xFFFFFFFF], b0=4) == 0
    for kw in ({"b0": 3}, {"b0": 8}, {"b1": 8}, {"b1": 0}, {"umi": 3}, {"ori": 3}):
        assert check_args(lib, [1], **kw) == INVALID_ARG, kw
    for ent in ([2, 1], [1, 1], [0, 5, 5]):
        assert check_args(lib, ent) == INVALID_ARG and "ascend without duplicates" in err(lib)
    assert check_args(lib, [1, 0x10000]) == BAD_INPUT and "packed sample barcode 65536 does not fit 2 bytes" in err(lib)
    assert check_args(lib, [256], b0=1) == BAD_INPUT and check_args(lib, [1 << 32], b0=4) == BAD_INPUT
    assert lib.afq_gpl_multi_check_args(2, 4, 4, 0, None, 1) == INVALID_ARG
    one = np.zeros(1, np.uint64)   # (the count is checked before any entry is read)
    assert lib.afq_gpl_multi_check_args(4, 4, 4, 0, one.ctypes.data_as(u64p), (1 << 31) + 1) == UNSUPPORTED
    # without a context nothing runs
    l = pkg.load_library()
    assert l.afq_gpl_multi_hist_rad(None, None, 0, None, 0, 2, 4, 4, 0, 0, None, 0, None, None, None, None, None) == INVALID_ARG


# ----------------------------------------------------------------------------------------------------------------- prelude
def write_dir(path, prelude, body=b""):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "map.rad"), "wb") as f:
        f.write(prelude + body)
    return str(path)


def multi(tmp_path, in_dir, **kw):
    lst = tmp_path / "samples.tsv"
    if not lst.exists():
        lst.write_text("ACGTACGT\ts1\n")
    with pytest.raises(pkg.AfqError) as e:
        pkg.generate_permit_list_multi(in_dir, str(tmp_path / "out"), kw.pop("sample_bc_list", str(lst)), **kw)
    assert not (tmp_path / "out").exists()   # a refusal leaves nothing behind
    return e.value


def test_prelude_refusals(tmp_path):
    refs = ["t0", "t1"]
    e = multi(tmp_path, write_dir(tmp_path / "single", rad.rad_prelude(refs, 0, 16, 12)))
    assert e.code == UNSUPPORTED and "single-barcode RAD file" in str(e)
    e = multi(tmp_path, write_dir(tmp_path / "atac", rad.rad_prelude_atac(refs, [1000, 2000], 0)))
    assert e.code == UNSUPPORTED and "scATAC RAD file" in str(e)
    good = rad.rad_prelude_multi_bc(refs, 0, 8, 16, 12, b_bytes=4, umi_bytes=4, b0_bytes=2)
    e = multi(tmp_path, write_dir(tmp_path / "three", good.replace((2).to_bytes(2, "little") + (8).to_bytes(2, "little") + (16).to_bytes(2, "little"),
                                                                   (3).to_bytes(2, "little") + (8).to_bytes(2, "little") + (16).to_bytes(2, "little"))))
    assert e.code == UNSUPPORTED and "only two barcode levels" in str(e)
    e = multi(tmp_path, write_dir(tmp_path / "wide", rad.rad_prelude_multi_bc(refs, 0, 8, 16, 12, b_bytes=8, umi_bytes=4, b0_bytes=2)))
    assert e.code == UNSUPPORTED and "1, 2 or 4 bytes" in str(e)
    e = multi(tmp_path, write_dir(tmp_path / "nolen", good.replace(b"b1len", b"b1xxx")))
    assert e.code == BAD_INPUT and "b1len" in str(e)
    pos = good.replace((1).to_bytes(2, "little") + (20).to_bytes(2, "little") + b"compressed_ori_refid\x03",
                       (2).to_bytes(2, "little") + (20).to_bytes(2, "little") + b"compressed_ori_refid\x03" + (3).to_bytes(2, "little") + b"pos\x03")
    assert pos != good
    e = multi(tmp_path, write_dir(tmp_path / "pos", pos))
    assert e.code == UNSUPPORTED and "alignment positions" in str(e)
    e = multi(tmp_path, str(tmp_path / "missing"))
    assert e.code == BAD_INPUT and "does not exist" in str(e)


def test_a_truncated_chunk_table(tmp_path):
    """the prelude promises three chunks and the file holds two; the last chunk's nbytes runs past the file's end"""
    body, _ = rad.encode_multi_bc_chunks([[(1, 0x11, 1, [(0, True)])], [(1, 0x22, 2, [(0, True)])]])
    e = multi(tmp_path, write_dir(tmp_path / "three", rad.rad_prelude_multi_bc(["t0"], 3, 8, 16, 12, b_bytes=4, umi_bytes=4, b0_bytes=2), body))
    assert e.code == BAD_INPUT and "map.rad ends before chunk 2 of 3" in str(e)
    e = multi(tmp_path, write_dir(tmp_path / "cut", rad.rad_prelude_multi_bc(["t0"], 2, 8, 16, 12, b_bytes=4, umi_bytes=4, b0_bytes=2), body[:-4]))
    assert e.code == BAD_INPUT and "corrupt chunk header (chunk 1)" in str(e)


def test_option_and_list_refusals_precede_the_device(tmp_path):
    good = write_dir(tmp_path / "good", rad.rad_prelude_multi_bc(["t0"], 0, 8, 16, 12, b_bytes=4, umi_bytes=4, b0_bytes=2))
    assert multi(tmp_path, good, method="unfiltered").code == INVALID_ARG                                     # no list file
    (tmp_path / "wl.txt").write_text("ACGTACGTACGTACGT\n")
    e = multi(tmp_path, good, method="unfiltered", list_file=str(tmp_path / "wl.txt"), min_reads=0)
    assert e.code == INVALID_ARG and "min-reads < 1 is not supported" in str(e)
    assert multi(tmp_path, good, confidence=(3, 2)).code == INVALID_ARG and multi(tmp_path, good, sample_confidence=(1, 0)).code == INVALID_ARG
    assert multi(tmp_path, good, sample_correction=4).code == INVALID_ARG and multi(tmp_path, good, sample_bc_ori=2).code == INVALID_ARG
    e = multi(tmp_path, good, sample_bc_list=str(tmp_path / "no_such_list"))
    assert e.code == BAD_INPUT and "couldn't open sample barcode list" in str(e)
    (tmp_path / "bad.tsv").write_text("ACGT\nACG\n")
    e = multi(tmp_path, good, sample_bc_list=str(tmp_path / "bad.tsv"))
    assert e.code == BAD_INPUT and "sample barcode file mixes lengths 4 and 3" in str(e)
    (tmp_path / "long.tsv").write_text("ACGTACGTA\n")   # 9 bases do not fit a 2-byte b0
    e = multi(tmp_path, good, sample_bc_list=str(tmp_path / "long.tsv"))
    assert e.code == BAD_INPUT and "do not fit the 2-byte b0 field" in str(e)


# ---------------------------------------------------------------------------------------------------------------- sanitizers
SAN_MAIN = r'''
#include "afq_gpl_host.h"
#include <cassert>
using namespace afq::gplhost;
int main() {
    std::string err;
    // ---- the sample list: exact-size heap copies, so that a read past the text is seen
    const char* texts[] = {"", "\n", "\t", "#", "ACGT", "ACGT\r", "ACGT\tx", "ACGT\t", "\tACGT", "ACGT\tAAAA\tn\tmore\n", "ACGT\tAAA\tn", "ACNT", "ACGT\nAC", "ACGT\tAAAA\ta\nACGT\tCCCC\tb",
                           "ACGT\tAAAA\ta\nACGA\tAAAA\tb", "ACGTACGTACGTACGTACGTACGTACGTACGTA", "ACGTACGTACGTACGTACGTACGTACGTACGT\nTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT\n"};
    for (const char* t : texts)
        for (int rev = 0; rev < 2; ++rev) {
            const std::string heap(t);
            SampleList sl;
            if (parse_sample_list(heap, rev != 0, sl, err)) continue;
            for (uint32_t mode = 0; mode < 4; ++mode)
                for (uint32_t nbh = 0; nbh < 2; ++nbh) {
                    SampleRouting r;
                    build_sample_routing(sl, mode, nbh, r);
                    assert(r.entry.size() == r.target.size() && r.entry.size() == r.kind.size() && std::is_sorted(r.entry.begin(), r.entry.end()));
                    SampleIndex ix = sample_index(sl, mode, nbh);
                    for (auto& s : ix.src) s.count = ~0ull >> 10;   // large priors: the 128-bit products
                    uint64_t tgt = 0;
                    for (uint64_t b : ix.theoretical()) ix.resolve(b, tgt);
                }
        }
    // ---- the index at both ends of the u64 (L = 32) and at L = 1
    for (uint32_t L : {1u, 2u, 31u, 32u}) {
        SampleIndex ix;
        ix.L = L; ix.shift = true; ix.frequency = true;
        ix.src = {SampleSource{0, 7, 5}, SampleSource{gpl_base_mask(L), 9, 3}};
        if (ix.src[0].source == ix.src[1].source) ix.src.pop_back();
        uint64_t tgt = 0;
        for (uint64_t b : ix.theoretical()) { ix.resolve(b, tgt); ix.structural(b, tgt); }
        std::vector<uint64_t> inv;
        gpl_push_inverse_shift(gpl_base_mask(L), L, inv); gpl_push_inverse_shift(0, L, inv);
    }
    // ---- argument checks and the plan
    const uint64_t ent[3] = {1, 2, 70000};
    assert(multi_check_args(2, 4, 4, 0, ent, 2, err) == 0 && multi_check_args(2, 4, 4, 0, ent, 3, err) == AFQ_ERR_BAD_INPUT && multi_check_args(4, 4, 4, 0, nullptr, 0, err) == 0);
    const PlanSpec ss{8, 0, 1, 39, 40, 1}, cs{16, 1, 0, 0, 1, 0};
    const uint64_t o[2] = {1, 2}, c[2] = {3, 3};
    const std::vector<PlanScope> scopes{PlanScope{true, 5, cs, o, c, 2}, PlanScope{true, 9, cs, nullptr, nullptr, 0}};
    assert(plan_bytes(8, 16, &ss, o, c, 2, scopes).size() == 8 + 2 + 3 + 1 + 33 + 8 + 32 + 8 + (9 + 9 + 8 + 32) + (9 + 9 + 8));
    assert(plan_bytes(-1, 16, nullptr, nullptr, nullptr, 0, {PlanScope{false, 0, cs, o, c, 2}}).size() == 8 + 2 + 3 + 8 + 8 + (1 + 9 + 8 + 32));
    std::puts("clean");
    return 0;
}
'''


def test_host_pieces_under_the_sanitizers(tmp_path):
    """a stand-alone program with its own main over csrc/afq_gpl_host.h, built with -fsanitize=address,undefined and run here (nothing
    is loaded into python under a sanitizer)"""
    src = tmp_path / "san.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "san"
    csrc = os.path.join(ROOT, "alevin-fry_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    "-o", str(exe), str(src)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "clean", r.stdout + r.stderr
