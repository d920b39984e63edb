"""CPU tests of `atac generate-permit-list`'s host half (afq_atac_generate_permit_list, include/afquant_host.h): everything that is refused
before the device runs, through ctypes, with its return code and sentence - the same with and without a GPU - and the two small host
helpers (the f32 bin lengths, the reverse complement) against tests/atac_gpl_judge.py."""
import ctypes as C
import gzip
import os

import pytest

import atac_gpl_judge as J
from util import pkg

rad = pkg.rad
INVALID_ARG, BAD_INPUT, UNSUPPORTED = pkg._abi.AFQ_ERR_INVALID_ARG, pkg._abi.AFQ_ERR_BAD_INPUT, pkg._abi.AFQ_ERR_UNSUPPORTED
Opts = pkg._abi.AfqAtacGplOpts
L = 16
A1 = (0, 4, 10, 50)
FILES = ("permit_freq.bin", "permit_map.bin", "correction_plan.bin", "bin_recs.bin", "bin_lens.bin", "generate_permit_list.json")


@pytest.fixture(scope="module")
def lib():
    l = pkg.load_library()
    l.afq_atac_gpl_bin_lens.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64)]
    l.afq_atac_gpl_bin_lens.restype = None
    l.afq_gpl_reverse_complement.argtypes = [C.c_uint64, C.c_uint32]
    l.afq_gpl_reverse_complement.restype = C.c_uint64
    return l


def mapper_dir(path, prelude=None, chunks=None, ref_lengths=(1000,), cut=0):
    os.makedirs(path)
    chunks = [[(0x11, [A1])], [(0x22, [A1])]] if chunks is None else chunks
    body, _ = rad.encode_atac_chunks(chunks)
    head = rad.rad_prelude_atac(["r%d" % i for i in range(len(ref_lengths))], list(ref_lengths), len(chunks), cblen=L) if prelude is None else prelude
    blob = head + body
    with open(os.path.join(path, "map.rad"), "wb") as f:
        f.write(blob[:len(blob) - cut])
    return str(path)


def list_file(path, text="A" * L + "\n"):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def gpl(lib, ind, out, lst, **kw):
    kw.setdefault("min_reads", 10)
    o = Opts(input_dir=ind.encode() if ind else None, output_dir=out.encode() if out else None, list_file=lst.encode() if lst else None, rc=1,
             cmdline=b"afquant atac generate-permit-list", **kw)
    rc = lib.afq_atac_generate_permit_list(C.byref(o))
    return rc, (lib.afq_host_last_error() or b"").decode()


def refused(lib, tmp_path, code, sentence, **kw):
    os.makedirs(tmp_path, exist_ok=True)
    out = str(tmp_path / "out")
    args = {"ind": kw.pop("ind", None) or mapper_dir(tmp_path / "map"), "lst": kw.pop("lst", None) or list_file(tmp_path / "list.txt")}
    rc, msg = gpl(lib, args["ind"], out, args["lst"], **kw)
    assert rc == code and sentence in msg, (rc, msg)
    assert not any(os.path.exists(os.path.join(out, f)) for f in FILES)


def test_null_options_and_min_reads(lib, tmp_path):
    assert lib.afq_atac_generate_permit_list(None) == INVALID_ARG
    ind, lst = mapper_dir(tmp_path / "map"), list_file(tmp_path / "l.txt")
    for a in ((None, str(tmp_path / "o"), lst), (ind, None, lst), (ind, str(tmp_path / "o"), None)):
        rc, msg = gpl(lib, *a)
        assert rc == INVALID_ARG and msg, a
    refused(lib, tmp_path / "a", INVALID_ARG, "min-reads < 1 is not supported, the value 0 was provided", min_reads=0)
    refused(lib, tmp_path / "b", INVALID_ARG, "unknown barcode neighbourhood", neighborhood=2)


def test_a_confidence_above_one_and_a_zero_denominator(lib, tmp_path):
    refused(lib, tmp_path / "a", INVALID_ARG, "barcode-correction confidence must be between zero and one (got 11/10)", conf_num=11, conf_den=10)
    refused(lib, tmp_path / "b", INVALID_ARG, "barcode-correction confidence must be between zero and one (got 1/0)", conf_num=1, conf_den=0)


def test_list_refusals(lib, tmp_path):
    refused(lib, tmp_path / "a", BAD_INPUT, "couldn't open input barcode file", lst=str(tmp_path / "nowhere.txt"))
    os.makedirs(tmp_path / "b")
    refused(lib, tmp_path / "b", BAD_INPUT, "found barcodes of different lengths 16 and 15", lst=list_file(tmp_path / "b" / "l.txt", "A" * 16 + "\n" + "C" * 15 + "\n"))
    # (the same through gzip: zlib reads both)
    os.makedirs(tmp_path / "c")
    with gzip.open(tmp_path / "c" / "l.txt.gz", "wt") as f:
        f.write("A" * 16 + "\n" + "C" * 17 + "\n")
    refused(lib, tmp_path / "c", BAD_INPUT, "found barcodes of different lengths 16 and 17", lst=str(tmp_path / "c" / "l.txt.gz"))
    # a listed barcode that does not fit 2 * cblen bits
    os.makedirs(tmp_path / "d")
    refused(lib, tmp_path / "d", BAD_INPUT, "does not fit declared length 16", lst=list_file(tmp_path / "d" / "l.txt", "C" + "A" * 16 + "\n"))
    refused(lib, tmp_path / "e", BAD_INPUT, "does not exist", ind=str(tmp_path / "no_such_dir"))


def test_an_rna_prelude_is_refused_and_names_generate_permit_list(lib, tmp_path):
    ind = mapper_dir(tmp_path / "map", prelude=rad.rad_prelude(["t0", "t1"], 1, L, 12, 4, 4))
    refused(lib, tmp_path, UNSUPPORTED, "generate-permit-list", ind=ind)
    rc, msg = gpl(lib, ind, str(tmp_path / "o"), list_file(tmp_path / "l2.txt"))
    assert rc == UNSUPPORTED and "RNA RAD" in msg


def _prelude_without(tag):
    """rad_prelude_atac's layout with one file tag left out"""
    def t(name, type_id, extra=b""):
        b = name.encode()
        return len(b).to_bytes(2, "little") + b + bytes([type_id]) + extra

    tags = [("cblen", t("cblen", 2), (L).to_bytes(2, "little")), ("ref_lengths", t("ref_lengths", 7, bytes([3, 3])), (1).to_bytes(4, "little") + (1000).to_bytes(4, "little"))]
    tags = [x for x in tags if x[0] != tag]
    out = bytes([1]) + (1).to_bytes(8, "little") + (2).to_bytes(2, "little") + b"r0" + (2).to_bytes(8, "little")
    out += len(tags).to_bytes(2, "little") + b"".join(x[1] for x in tags)
    out += (1).to_bytes(2, "little") + t("b", 3)
    out += (4).to_bytes(2, "little") + t("ref", 3) + t("type", 1) + t("start_pos", 3) + t("frag_len", 2)
    return out + b"".join(x[2] for x in tags)


def test_a_missing_cblen_or_ref_lengths(lib, tmp_path):
    refused(lib, tmp_path / "a", BAD_INPUT, "tag map must contain cblen", ind=mapper_dir(tmp_path / "a" / "map", prelude=_prelude_without("cblen")))
    refused(lib, tmp_path / "b", BAD_INPUT, "ref_lengths", ind=mapper_dir(tmp_path / "b" / "map", prelude=_prelude_without("ref_lengths")))
    # one entry per reference
    two = rad.rad_prelude_atac(["r0", "r1"], [1000], 2, cblen=L)
    refused(lib, tmp_path / "c", BAD_INPUT, "one entry per reference", ind=mapper_dir(tmp_path / "c" / "map", prelude=two))


def test_a_truncated_chunk_table(lib, tmp_path):
    three = rad.rad_prelude_atac(["r0"], [1000], 3, cblen=L)   # the prelude promises three chunks, the file holds two
    refused(lib, tmp_path / "a", BAD_INPUT, "map.rad ends before chunk 2 of 3", ind=mapper_dir(tmp_path / "a" / "map", prelude=three))
    refused(lib, tmp_path / "b", BAD_INPUT, "corrupt chunk header (chunk 1)", ind=mapper_dir(tmp_path / "b" / "map", cut=4))


def test_reference_lengths_without_a_bin(lib, tmp_path):
    refused(lib, tmp_path, BAD_INPUT, "bins should not be empty", ind=mapper_dir(tmp_path / "map", ref_lengths=(0, 0)))


def test_bin_lens_are_the_f32_ceiling(lib):
    for lens in ([200000001], [4294967295] * 3, [100000, 100001, 99999, 0, 1], [16777217, 33554433, 400000, 9000, 70], []):
        a = (C.c_uint32 * max(len(lens), 1))(*lens)
        out = (C.c_uint64 * (len(lens) + 1))()
        lib.afq_atac_gpl_bin_lens(a, len(lens), J.SIZE_RANGE, out)
        assert list(out) == J.bin_lens(lens), lens
    assert J.bin_lens([200000001]) == [0, 2000]


def test_reverse_complement(lib):
    for bc, k in ((1, 4), (191, 4), (0, 32), ((1 << 64) - 1, 32), (0x1234ABCD, 16), (1, 1), (0x0123456789ABCDEF, 32)):
        assert lib.afq_gpl_reverse_complement(bc, k) == J.reverse_complement(bc, k), (bc, k)
        assert lib.afq_gpl_reverse_complement(lib.afq_gpl_reverse_complement(bc, k), k) == bc


def test_limits_are_the_sort_parses(lib):
    g, s = pkg.atac_gpl_limits(), pkg.atac_sort_limits()
    assert (g["parse_tile"], g["parse_halo"]) == (s["parse_tile"], s["parse_halo"]) and g["private_bins"] >= 0
    assert g["parse_halo"] >= 4 + 8 + 9    # the widest head and ref, type, start_pos of one alignment
    assert pkg.Quantifier.atac_gpl_limits() == g


SAN_MAIN = r'''
#include "afq_gpl_host.h"
#include <cstdio>
#define CHECK(x) do { if (!(x)) { std::printf("failed: %s\n", #x); return 1; } } while (0)
int main(int argc, char** argv) {
    using namespace afq::gplhost;
    if (argc < 2) return 2;
    const uint32_t lens[5] = {200000001u, 4294967295u, 0u, 100001u, 1u};
    uint64_t out[6];
    atac_bin_lens(lens, 5, 100000, out);
    CHECK(out[1] == 2000 && out[2] == 2000 + 42950 && out[3] == out[2] && out[4] == out[3] + 2 && out[5] == out[4] + 1);
    uint64_t none[1] = {9};
    atac_bin_lens(nullptr, 0, 100000, none);
    CHECK(none[0] == 0);
    CHECK(reverse_complement(1, 4) == 191 && reverse_complement(0, 32) == ~0ull && reverse_complement(~0ull, 32) == 0);
    afq_atac_gpl_opts o{};
    o.input_dir = "in \"dir\""; o.output_dir = argv[1]; o.list_file = "list.txt"; o.min_reads = 3; o.rc = 1; o.conf_num = 9; o.conf_den = 10;
    afq_gpl_tables t{};
    t.barcode_len = 16;
    const uint64_t fb[2] = {1, 2}, fc[2] = {5, 6}, bins[3] = {1, 0, 7}, bl[2] = {0, 3};
    t.freq_bc = fb; t.freq_count = fc; t.n_freq = 2; t.map_obs = fb; t.map_cor = fb; t.n_map = 2; t.plan_obs = fb; t.plan_cor = fb; t.n_plan = 2;
    std::string err;
    CHECK(write_atac_outputs(&o, &t, bins, 3, bl, 2, 6, 7, err) == 0);
    CHECK(write_atac_outputs(nullptr, &t, bins, 3, bl, 2, 6, 7, err) != 0);
    o.output_dir = "/proc/nowhere/x";
    CHECK(write_atac_outputs(&o, &t, bins, 3, bl, 2, 6, 7, err) != 0 && !err.empty());
    std::puts("clean");
    return 0;
}
'''


def test_host_pieces_under_the_sanitizers(tmp_path):
    """a stand-alone program with its own main over the ATAC pieces of csrc/afq_gpl_host.h, built with -fsanitize=address,undefined and run
    here (nothing is loaded into python under a sanitizer); the files it writes are read back"""
    import json
    import subprocess

    from util import ROOT

    src = tmp_path / "san.cpp"
    src.write_text(SAN_MAIN)
    exe = tmp_path / "san"
    csrc = os.path.join(ROOT, "alevin-fry_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", csrc, "-o", str(exe), str(src)], check=True, capture_output=True)
    out = tmp_path / "out" / "deeper"
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "clean", r.stdout + r.stderr
    assert rad.read_permit_freq((out / "permit_freq.bin").read_bytes()) == (1, 16, {1: 5, 2: 6}) and rad.read_permit_map((out / "permit_map.bin").read_bytes()) == {1: 1, 2: 2}
    assert (out / "bin_recs.bin").read_bytes() == b"".join(v.to_bytes(8, "little") for v in (3, 1, 0, 7)) and (out / "bin_lens.bin").read_bytes() == b"".join(v.to_bytes(8, "little") for v in (2, 0, 3))
    j = json.loads((out / "generate_permit_list.json").read_text())
    assert j["gpl_options"]["input_dir"] == 'in "dir"' and j["gpl_options"]["rc"] is True and j["num-chunks"] == 6 and j["max-rec-in-bin"] == 7
