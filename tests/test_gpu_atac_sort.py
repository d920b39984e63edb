"""GPU tests of `atac sort` (afq_atac_sort_rad, `afquant atac sort`): the chunks of an uncollated scATAC RAD - a barcode per
record - in, the distinct (ref, start, frag_len, corrected barcode) rows in that order with their counts out.

The expected result is numpy on the decoded records (src/atac/sort.rs:47-59, 74, 121-123 of the reference): keep na == 1 with
the barcode in the map, map the barcode, np.lexsort((bc, frag_len, start, ref)), unique rows with counts.  Every comparison is
exact integer equality, array for array, in order.  Boundary shapes come from atac_sort_limits(), not from copied constants."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from atac_sort_cases import distinct, expected, flat, na1_chunks, same
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")
BAD_INPUT = pkg._abi.AFQ_ERR_BAD_INPUT


@pytest.fixture(scope="module")
def q():
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    qq = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    yield qq
    qq.close()


@pytest.fixture(scope="module")
def lim():
    L = pkg.atac_sort_limits()
    assert L["repartition_above"] >= L["leaf_cap"] > 1025 and L["parse_tile"] >= 64
    return L


# ---------------------------------------------------------------------------------------------------------------- helpers
# (expected - the judge of every result -, same, flat, na1_chunks and distinct live in tests/atac_sort_cases.py)
def rand_alns(rng, na, ref_lengths):
    out = []
    for _ in range(na):
        r = int(rng.integers(0, len(ref_lengths)))
        out.append((r, int(rng.integers(1, 5)), int(rng.integers(0, ref_lengths[r])), int(rng.integers(20, 2500))))
    return out


# ------------------------------------------------------------------------------------------------------------------ parse
@pytest.mark.parametrize("bc_bytes", [1, 2, 4, 8])
def test_parse_every_width_alignment_and_chunk_shape(q, lim, bc_bytes):
    """na in {0, 1, 2, 5} interleaved, a barcode per record; an empty chunk; chunks of three parse tiles whose records meet the
    tile edges at eight different phases (records, na fields and barcode fields straddle them); a one-record chunk; 300 chunks of
    1-3 records; and all of it at each of the four byte alignments of the chunk starts."""
    rng = np.random.default_rng(bc_bytes)
    S, tile = lim["bin_shift"], lim["parse_tile"]
    ref_lengths = [3 * (1 << S) + 5, 900, (1 << S) - 7]
    n_bc = min(200, 1 << (8 * bc_bytes))
    pool = distinct(rng, n_bc, min(8 * bc_bytes, 62))
    if bc_bytes == 8:
        pool[::3] |= np.uint64(1) << np.uint64(63)
    obs = pool[: n_bc * 3 // 4]                      # a quarter of the barcodes is not in the map
    cor = obs.copy()
    cor[::5] = obs[rng.integers(0, len(obs), size=len(cor[::5]))]

    def rec():
        return (int(pool[rng.integers(0, n_bc)]), rand_alns(rng, int(rng.choice([0, 1, 1, 1, 2, 5])), ref_lengths))

    chunks = [[rec() for _ in range(40)], [], [rec()]]
    for phase in range(8):   # ~2.5 tiles of records behind `phase` shortest records
        c = [(int(pool[0]), []) for _ in range(phase)]
        size = 8 + phase * (4 + bc_bytes)
        while size < 2 * tile + tile // 2:
            r = rec()
            c.append(r)
            size += 4 + bc_bytes + 11 * len(r[1])
        assert 2 * tile < size < 3 * tile
        chunks.append(c)
    chunks += [[rec() for _ in range(int(rng.integers(1, 4)))] for _ in range(300)]
    data, off = rad.encode_atac_chunks(chunks, bc_bytes=bc_bytes)
    cols, (n, n0, nm) = flat(chunks)
    want = expected(*cols, obs, cor)
    assert want["n_kept"] > 500 and want["n_uncorrected"] > 100 and n0 > 100 and nm > 100
    for al in range(4):
        got = q.atac_sort_rad(b"\xEE" * al + data, off + np.uint64(al), obs, cor, ref_lengths, bc_bytes=bc_bytes)
        same(got, want, f"alignment {al}")
        st = got["stats"]
        assert (st["n_records"], st["n_unmapped"], st["n_multimapped"]) == (n, n0, nm)


def test_nothing_in_nothing_out(q):
    got = q.atac_sort_rad(b"", np.zeros(0, np.uint64), [1], [1], [100])
    assert all(len(got[k]) == 0 for k in ("ref", "start", "frag_len", "bc", "count")) and got["stats"]["n_records"] == 0
    data, off = rad.encode_atac_chunks([[], [(5, [])]])
    got = q.atac_sort_rad(data, off, [], [], [100])
    assert len(got["ref"]) == 0 and got["stats"]["n_records"] == 1 and got["stats"]["n_unmapped"] == 1


# ------------------------------------------------------------------------------------------------------------- correction
def test_correction_map_shapes(q):
    rl = [1000]
    # two observed barcodes onto one corrected: the fragments are equal only AFTER correction -> one row, count 2; 9 is absent
    chunks = [[(7, [(0, 4, 10, 50)]), (9, [(0, 4, 10, 50)]), (8, [(0, 4, 10, 50)]), (3, [(0, 4, 10, 50)])]]
    data, off = rad.encode_atac_chunks(chunks)
    got = q.atac_sort_rad(data, off, [7, 8, 3], [7, 7, 3], rl)
    same(got, expected(*flat(chunks)[0], [7, 8, 3], [7, 7, 3]))
    assert got["bc"].tolist() == [3, 7] and got["count"].tolist() == [1, 2] and got["stats"]["n_uncorrected"] == 1
    # a table of one entry (and the same pair twice is one entry)
    got = q.atac_sort_rad(data, off, [8, 8], [123, 123], rl)
    assert got["bc"].tolist() == [123] and got["count"].tolist() == [1] and got["stats"]["n_uncorrected"] == 3
    # corrected barcodes whose integer order is the reverse of the observed order and of the order in the file
    obs = np.arange(1, 41, dtype=np.uint64)
    cor = np.uint64(1000) - obs
    chunks = [[(int(b), [(0, 4, 10, 50)]) for b in obs]]
    data, off = rad.encode_atac_chunks(chunks)
    got = q.atac_sort_rad(data, off, obs, cor, rl)
    same(got, expected(*flat(chunks)[0], obs, cor))
    assert got["bc"].tolist() == sorted(cor.tolist())
    # barcodes that differ only above bit 32, and the all-ones barcode, in 8-byte fields
    hi = [(k << 32) | 5 for k in (3, 1, 2, 0)] + [0xFFFFFFFFFFFFFFFF, 1 << 63]
    chunks = [[(b, [(0, 4, 10, 50)]) for b in hi + [(9 << 32) | 5]]]
    data, off = rad.encode_atac_chunks(chunks, bc_bytes=8)
    got = q.atac_sort_rad(data, off, hi, hi, rl, bc_bytes=8)
    same(got, expected(*flat(chunks)[0], hi, hi))
    assert got["bc"].tolist() == sorted(hi) and got["stats"]["n_uncorrected"] == 1


def test_correction_table_of_5000_entries(q):
    rng = np.random.default_rng(5)
    obs = distinct(rng, 5000, 32)
    cor = obs.copy()
    cor[::7] = obs[rng.integers(0, 5000, size=len(cor[::7]))]
    n = 30000
    bc = np.concatenate((obs[rng.integers(0, 5000, size=n - 3000)], rng.integers(0, 1 << 32, size=3000).astype(np.uint64)))
    ref, start, fl = np.zeros(n, np.uint32), rng.integers(0, 400, size=n), rng.integers(30, 40, size=n)
    data, off = na1_chunks(bc, ref, start, fl, 1000, bc_bytes=4)
    got = q.atac_sort_rad(data, off, obs, cor, [400])
    want = expected(bc, ref, start, fl, obs, cor)
    assert want["count"].max() > 1 and want["n_uncorrected"] > 2000
    same(got, want)


def test_one_observed_barcode_with_two_corrections_is_refused(q):
    data, off = rad.encode_atac_chunks([[(7, [(0, 4, 10, 50)])]])
    for obs in ([7, 5, 7], [0xFFFFFFFFFFFFFFFF, 5, 0xFFFFFFFFFFFFFFFF]):
        with pytest.raises(pkg.AfqError) as e:
            q.atac_sort_rad(data, off, obs, [1, 2, 3], [100], bc_bytes=4)
        assert e.value.code == BAD_INPUT and "two different corrected" in str(e.value)
    assert q.atac_sort_rad(data, off, [7], [1], [100])["bc"].tolist() == [1]


# ----------------------------------------------------------------------------------------------------------- order and bins
def test_order_across_bins_and_references(q, lim):
    S = lim["bin_shift"]
    B = 1 << S
    rl = [3 * B + 5, B - 7, 100, 2 * B, 0, 1]   # not a multiple of 2^S; shorter than 2^S; one bin exactly; without a bin
    recs = []
    for k in (1, 2, 3):
        recs += [(11, [(0, 4, k * B - 1, 60)]), (11, [(0, 4, k * B, 60)])]        # either side of a bin edge
    recs += [(11, [(0, 4, 3 * B + 4, 60)]), (11, [(1, 4, B - 8, 60)]), (11, [(5, 4, 0, 60)])]   # the last base of a reference
    recs += [(12, [(r, 4, 77, 60)]) for r in (3, 2, 1, 0)]                            # equal start on consecutive refs
    recs += [(12, [(3, 4, 500, f)]) for f in (300, 20, 2000, 1999, 65535, 20)]        # equal (ref, start), different frag_len
    recs += [(b, [(3, 4, B + 9, 100)]) for b in (13, 11, 12, 11)]                     # equal triple under three barcodes
    recs += [(13, [(2, ty, 5, 80)]) for ty in (1, 2, 3, 4)]                           # every map type is kept (sort.rs has no type filter)
    rng = np.random.default_rng(3)
    recs = [recs[i] for i in rng.permutation(len(recs))]
    chunks = [recs[:9], recs[9:20], recs[20:]]
    data, off = rad.encode_atac_chunks(chunks)
    obs = [11, 12, 13]
    want = expected(*flat(chunks)[0], obs, obs)
    got = q.atac_sort_rad(data, off, obs, obs, rl)
    same(got, want)
    rows = list(zip(got["ref"].tolist(), got["start"].tolist(), got["frag_len"].tolist(), got["bc"].tolist(), got["count"].tolist()))
    assert (2, 5, 80, 13, 4) in rows and (3, 500, 20, 12, 2) in rows and (3, B + 9, 100, 11, 2) in rows
    assert (3, 500, 1999, 12, 1) in rows and (3, 500, 2000, 12, 1) in rows and got["stats"]["n_long_fragments"] == 2
    assert got["stats"]["n_kept"] == len(recs) and got["stats"]["n_repartitioned_bins"] == 0


def test_reference_ids_above_65535(q):
    n_ref = 70000
    rng = np.random.default_rng(8)
    ref = np.concatenate((rng.integers(0, n_ref, size=5000), [65535, 65536, 65536, n_ref - 1, 0])).astype(np.uint32)
    n = len(ref)
    start, fl, bc = rng.integers(0, 100, size=n), rng.integers(30, 33, size=n), rng.integers(0, 4, size=n).astype(np.uint64)
    data, off = na1_chunks(bc, ref, start, fl, 700, bc_bytes=2)
    want = expected(bc, ref, start, fl, [0, 1, 2, 3], [3, 2, 1, 0])
    got = q.atac_sort_rad(data, off, [0, 1, 2, 3], [3, 2, 1, 0], np.full(n_ref, 100, np.uint32), bc_bytes=2)
    same(got, want)
    assert got["ref"].max() == n_ref - 1 and (got["ref"] > 65535).sum() > 100


def test_count_is_not_sixteen_bits(q):
    n = 70000
    z = np.zeros(n, np.uint32)
    data, off = na1_chunks(z + 9, z, z + 123, z + 50, 5000, bc_bytes=1)
    got = q.atac_sort_rad(data, off, [9], [9], [1000], bc_bytes=1)
    assert got["count"].tolist() == [70000] and got["count"].dtype == np.uint32   # (as u16: 4 464)
    assert (got["ref"].tolist(), got["start"].tolist(), got["frag_len"].tolist(), got["bc"].tolist()) == ([0], [123], [50], [9])


# ------------------------------------------------------------------------------------------------------------------ leaves
def test_bins_at_the_leaf_boundaries(q, lim):
    """bins of exactly leaf cap - 1, leaf cap, leaf cap + 1 distinct keys and of 1 024 / 1 025 keys, empty bins between them"""
    S, cap = lim["bin_shift"], lim["leaf_cap"]
    B = 1 << S
    assert cap + 1 <= B
    sizes = [cap - 1, cap, cap + 1, 1024, 1025]
    rng = np.random.default_rng(4)
    start = np.concatenate([2 * i * B + rng.permutation(B)[:n] for i, n in enumerate(sizes)]).astype(np.uint32)   # distinct starts: distinct keys
    n = len(start)
    perm = rng.permutation(n)
    start = start[perm]
    ref, fl, bc = np.zeros(n, np.uint32), rng.integers(20, 900, size=n), rng.integers(0, 30, size=n).astype(np.uint64)
    data, off = na1_chunks(bc, ref, start, fl, 5000, bc_bytes=4)
    ident = np.arange(30, dtype=np.uint64)
    want = expected(bc, ref, start, fl, ident, ident)
    assert len(want["ref"]) == n
    got = q.atac_sort_rad(data, off, ident, ident, [2 * len(sizes) * B])
    same(got, want)
    assert got["stats"]["n_repartitioned_bins"] == sum(s > lim["repartition_above"] for s in sizes)


# -------------------------------------------------------------------------------------------------------------------- skew
def test_skewed_bins_are_partitioned_again(q, lim):
    """one bin of 12 x leaf cap keys over 200 distinct starts, one of 3 x leaf cap identical keys; twice, for the same arrays"""
    S, cap = lim["bin_shift"], lim["leaf_cap"]
    B = 1 << S
    rng = np.random.default_rng(6)
    n1, n2 = 12 * cap, 3 * cap
    starts200 = rng.choice(B, size=200, replace=False)
    start = np.concatenate((B + starts200[rng.integers(0, 200, size=n1)], np.full(n2, 3 * B + 17), rng.integers(0, 5 * B, size=3000))).astype(np.uint32)
    fl = np.concatenate((rng.integers(30, 700, size=n1), np.full(n2, 150), rng.integers(30, 700, size=3000)))
    bc = np.concatenate((rng.integers(0, 40, size=n1), np.full(n2, 21), rng.integers(0, 40, size=3000))).astype(np.uint64)
    n = len(start)
    perm = rng.permutation(n)
    start, fl, bc = start[perm], fl[perm], bc[perm]
    ref = np.ones(n, np.uint32)
    data, off = na1_chunks(bc, ref, start, fl, 5000, bc_bytes=4)
    ident = np.arange(40, dtype=np.uint64)
    want = expected(bc, ref, start, fl, ident, ident[::-1].copy())
    got = q.atac_sort_rad(data, off, ident, ident[::-1].copy(), [10, 5 * B])
    same(got, want)
    assert got["stats"]["n_repartitioned_bins"] == 2 and got["count"].max() >= n2
    again = q.atac_sort_rad(data, off, ident, ident[::-1].copy(), [10, 5 * B])
    same(again, want)
    assert again["stats"] == got["stats"]


# ------------------------------------------------------------------------------------------------------------------ errors
def test_malformed_chunks_are_refused_by_name_and_the_context_survives(q):
    rl = [1000, 50]
    good = [[(1, [(0, 4, 5, 60)]), (2, [])], [(1, [(1, 4, 49, 60)]), (2, [(0, 4, 7, 60), (0, 4, 8, 60)]), (1, [(0, 4, 999, 60)])], [(2, [(0, 4, 1, 30)])]]
    data, off = rad.encode_atac_chunks(good)
    o1 = int(off[1])

    def patched(at, value, width=4):
        b = bytearray(data)
        b[at:at + width] = int(value).to_bytes(width, "little")
        return bytes(b)

    rec0 = o1 + 8                       # chunk 1, record 0: na at +0, bc at +4, ref at +8, type at +12, start at +13
    cases = {
        "na pointing past the chunk end": (patched(rec0 + 19 + 30, 1000), "do not tile"),   # the na of the chunk's last record
        "nrec off by one (more)": (patched(o1 + 4, 4), "do not tile"),
        "nrec off by one (fewer)": (patched(o1 + 4, 2), "do not tile"),
        "ref = ref_count": (patched(rec0 + 8, 2), "reference id"),
        "start = ref_len": (patched(rec0 + 13, 50), "start position"),
    }
    assert data[rec0 + 49:rec0 + 53] == (1).to_bytes(4, "little")
    want = expected(*flat(good)[0], [1, 2], [1, 2])
    for what, (blob, msg) in cases.items():
        with pytest.raises(pkg.AfqError) as e:
            q.atac_sort_rad(blob, off, [1, 2], [1, 2], rl)
        assert e.value.code == BAD_INPUT and "chunk 1:" in str(e.value) and msg in str(e.value), (what, str(e.value))
        same(q.atac_sort_rad(data, off, [1, 2], [1, 2], rl), want, "after " + what)


# ------------------------------------------------------------------------------------------------------------ input routes
def test_pageable_host_bytes_and_device_bytes_agree(q):
    import torch

    rng = np.random.default_rng(12)
    n = 20000
    rl = [300000, 5000]
    ref = rng.integers(0, 2, size=n).astype(np.uint32)
    start = (rng.integers(0, 5000, size=n) * (1 + 50 * (1 - ref))).astype(np.uint32)
    fl, bc = rng.integers(30, 60, size=n), rng.integers(0, 50, size=n).astype(np.uint64)
    data, off = na1_chunks(bc, ref, start, fl, 1500, bc_bytes=2)
    ident = np.arange(45, dtype=np.uint64)
    want = expected(bc, ref, start, fl, ident, ident)
    same(q.atac_sort_rad(data, off, ident, ident, rl, bc_bytes=2), want, "host bytes")
    for al in (0, 3):   # (a device buffer that starts off a dword boundary: nothing in front of it is read)
        t = torch.from_numpy(np.frombuffer(b"\0" * al + data, np.uint8).copy()).cuda()
        same(q.atac_sort_rad(None, off, ident, ident, rl, bc_bytes=2, d_ptr=t.data_ptr() + al, n_bytes=len(data)), want, f"device bytes + {al}")


# --------------------------------------------------------------------------------------------------------------------- CLI
def _bc_string(bc, n, rc):
    if rc:
        r = 0
        for _ in range(n):
            r = (r << 2) | (3 - (bc & 3))
            bc >>= 2
        bc = r
    return "".join("ACGT"[(bc >> (2 * (n - 1 - i))) & 3] for i in range(n))


@pytest.fixture(scope="module")
def cli_case():
    """6 chunks, 3 refs, 40 barcodes of which 5 are corrected (onto other permitted ones), unmapped and multi-mapped records"""
    rng = np.random.default_rng(21)
    rl = [400000, 9000, 70]
    names = ["chr1", "chrM", "tiny"]
    pool = distinct(rng, 48, 32)
    obs = pool[:40]
    cor = obs.copy()
    cor[35:] = obs[:5]
    alt = obs.copy()                       # the legacy map's differing contents
    alt[30:35] = obs[5:10]
    chunks = []
    for _ in range(6):
        c = []
        for _ in range(int(rng.integers(150, 250))):
            c.append((int(pool[rng.integers(0, 48)]), rand_alns(rng, int(rng.choice([0, 1, 1, 1, 1, 2])), rl)))
        c += [c[0], c[1], c[2]]            # exact duplicates
        chunks.append(c)
    unmapped = [(int(pool[i]), 3 + i) for i in (0, 36, 45, 0, 1)]
    return {"rl": rl, "names": names, "obs": obs, "cor": cor, "alt": alt, "chunks": chunks, "unmapped": unmapped}


@pytest.mark.parametrize("maps", ["plan", "legacy", "both"])
@pytest.mark.parametrize("rc,gz", [(True, False), (False, False), (True, True)])
def test_cli_writes_the_sorted_bed(cli_case, tmp_path, maps, rc, gz):
    c = cli_case
    ind, radd = str(tmp_path / "gpl"), str(tmp_path / "map")
    os.makedirs(ind)
    os.makedirs(radd)
    data, _ = rad.encode_atac_chunks(c["chunks"])
    with open(os.path.join(radd, "map.rad"), "wb") as f:
        f.write(rad.rad_prelude_atac(c["names"], c["rl"], len(c["chunks"]), cblen=16) + data)
    with open(os.path.join(radd, "unmapped_bc_count.bin"), "wb") as f:
        f.write(b"".join(b.to_bytes(8, "little") + n.to_bytes(4, "little") for b, n in c["unmapped"]))
    with open(os.path.join(ind, "generate_permit_list.json"), "w") as f:
        json.dump({"version_str": "0.18.0", "gpl_options": {"rc": rc, "other": 1}, "num-chunks": len(c["chunks"])}, f)
    for name in ("bin_recs.bin", "bin_lens.bin"):
        with open(os.path.join(ind, name), "wb") as f:
            f.write((0).to_bytes(8, "little"))
    with open(os.path.join(ind, "permit_freq.bin"), "wb") as f:
        f.write(rad.permit_freq_header(16))
    used = c["cor"] if maps in ("plan", "both") else c["alt"]
    if maps in ("plan", "both"):
        with open(os.path.join(ind, "correction_plan.bin"), "wb") as f:
            f.write(rad.correction_plan_bytes(zip(c["obs"].tolist(), c["cor"].tolist()), barcode_len=16, spec=("frequency", (9, 10), 1)))
    if maps in ("legacy", "both"):
        with open(os.path.join(ind, "permit_map.bin"), "wb") as f:
            f.write(rad.permit_map_bytes(zip(c["obs"].tolist(), c["alt"].tolist())))
    r = subprocess.run([CLI, "atac", "sort", "-i", ind, "-r", radd, "-t", "3", "-m", "1000"] + (["-c"] if gz else []), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cols, (n, n0, nm) = flat(c["chunks"])
    want = expected(*cols, c["obs"], used)
    lines = [f"{c['names'][r_]}\t{s}\t{s + f}\t{_bc_string(int(b), 16, rc)}\t{k}"
             for r_, s, f, b, k in zip(want["ref"].tolist(), want["start"].tolist(), want["frag_len"].tolist(), want["bc"].tolist(), want["count"].tolist()) if f < 2000]
    assert len(lines) < len(want["ref"]) and max(want["count"]) > 1
    if gz:
        assert not os.path.exists(os.path.join(ind, "map.bed"))
        text = gzip.open(os.path.join(ind, "map.bed.gz"), "rt").read()
    else:
        assert not os.path.exists(os.path.join(ind, "map.bed.gz"))
        text = open(os.path.join(ind, "map.bed")).read()
    assert text.split("\n") == lines + [""]
    meta = json.load(open(os.path.join(ind, "sort.json")))
    assert set(meta) == {"cmd", "version_str", "compressed_output"} and meta["compressed_output"] is gz and "atac sort" in meta["cmd"]
    blob = open(os.path.join(ind, "unmapped_bc_count_collated.bin"), "rb").read()
    m = int.from_bytes(blob[:8], "little")
    assert len(blob) == 8 + 12 * m
    coll = {int.from_bytes(blob[8 + 12 * i:16 + 12 * i], "little"): int.from_bytes(blob[16 + 12 * i:20 + 12 * i], "little") for i in range(m)}
    cmap = dict(zip(c["obs"].tolist(), used.tolist()))
    exp = {}
    for b, k in c["unmapped"]:
        if b in cmap:
            exp[cmap[b]] = exp.get(cmap[b], 0) + k
    assert coll == exp and len(exp) >= 2
    for label, v in (("processed", n), ("without a mapping", n0), ("greater than 1 mapping", nm), ("not in the correction map", want["n_uncorrected"]),
                     ("fragments sorted", want["n_kept"]), ("Number of rows", len(want["ref"])),
                     ("frag length >= 2000", int((want["frag_len"] >= 2000).sum()))):
        hit = [ln for ln in r.stderr.split("\n") if label in ln]
        assert len(hit) == 1 and str(v) in hit[0].replace(",", "").split(), (label, v, r.stderr)
