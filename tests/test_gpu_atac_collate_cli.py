"""GPU end-to-end tests of `afquant atac collate` in fresh child processes: a mapper directory and a permit-list directory written with
rad.py in, map.collated.rad / collate.json / unmapped_bc_count_collated.bin out, each compared with tests/atac_collate_judge.py; then
`afquant atac deduplicate` on the output, against tests/atac_dedup_judge.py on the judge's cells and against atac_sort_rad on the same
uncollated bytes - two independent paths through the project that must agree."""
import json
import os
import random
import subprocess
from collections import Counter

import numpy as np
import pytest

import atac_collate_judge as J
import atac_dedup_judge as D
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
CLI = os.path.join(ROOT, "alevin-fry_amd", "csrc", "afquant")
L = 16
NAMES, REF_LEN = ["chr1", "chrM", "tiny"], [400000, 9000, 70]
ABSENT = "retained barcodes produced no collated records (every read was unmapped or multi-mapping) and are absent from the output."


def run(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)


def dataset(seed, all_pairs=False, idle_cells=0):
    """six chunks over 40 cells and 8 stray barcodes; 5 observed barcodes are corrected onto cells; duplicates within and across
    chunks; `idle_cells` cells whose reads are all unmapped or multi-mapped.  all_pairs: every alignment has map type 4.
    -> (chunks, freq {cell: count}, corrections {observed: corrected}, unmapped [(barcode, count)])"""
    rng = random.Random(seed)
    pool = rng.sample(range(1, 1 << 32), 53)
    cells, near, stray = pool[:40], pool[40:45], pool[45:]
    corr = {b: b for b in cells}
    corr.update({n: cells[i] for i, n in enumerate(near)})
    idle = set(cells[10:10 + idle_cells])

    def alns(na):
        out = []
        for _ in range(na):
            r = rng.randrange(3)
            out.append((r, 4 if all_pairs else rng.choice([4, 4, 4, 1, 2, 3]), rng.randrange(REF_LEN[r]) // 7 * 7, rng.choice([40, 41, 150, 1999, 2000, 2500])))
        return out

    chunks = []
    for _ in range(6):
        c = []
        for _ in range(rng.randrange(150, 250)):
            b = rng.choice(pool)
            c.append((b, alns(rng.choice([0, 2]) if b in idle else rng.choice([0, 1, 1, 1, 1, 2]))))
        c += [c[0], c[1], c[2], c[0]]   # exact duplicates
        chunks.append(c)
    kept = Counter(corr[b] for c in chunks for b, a in c if len(a) == 1 and b in corr)
    freq = {b: kept.get(b, 0) + 1 for b in cells}   # (the reference does not compare these counts with what it retains; they order the cells)
    unmapped = [(pool[i], 3 + i) for i in (0, 41, 47, 0, 1)]
    return chunks, freq, corr, unmapped


def write_dirs(tmp_path, chunks, freq, corr, unmapped, legacy=False, num_chunks=None, extra_chunks=()):
    ind, rd = str(tmp_path / "gpl"), str(tmp_path / "map")
    os.makedirs(ind)
    os.makedirs(rd)
    body, off = rad.encode_atac_chunks(list(chunks) + list(extra_chunks))
    head = rad.rad_prelude_atac(NAMES, REF_LEN, len(chunks) + len(extra_chunks), cblen=L)
    with open(os.path.join(rd, "map.rad"), "wb") as f:
        f.write(head + body)
    if unmapped is not None:
        with open(os.path.join(rd, "unmapped_bc_count.bin"), "wb") as f:
            f.write(b"".join(b.to_bytes(8, "little") + n.to_bytes(4, "little") for b, n in unmapped))
    with open(os.path.join(ind, "generate_permit_list.json"), "w") as f:
        json.dump({"version_str": "0.18.0", "gpl_options": {"rc": False}, "num-chunks": len(chunks) if num_chunks is None else num_chunks}, f)
    with open(os.path.join(ind, "permit_freq.bin"), "wb") as f:
        f.write(rad.permit_freq_bytes(L, freq.items()))
    with open(os.path.join(ind, "permit_map.bin" if legacy else "correction_plan.bin"), "wb") as f:
        f.write(rad.permit_map_bytes(corr.items()) if legacy else rad.correction_plan_bytes(corr.items(), barcode_len=L))
    n_in = len(chunks) if num_chunks is None else num_chunks
    return ind, rd, head, body[:int(off[n_in])] if n_in < len(off) else body, off[:n_in]


def judged_files(ind, head, want, corr, unmapped):
    """the three files against the judge"""
    got = open(os.path.join(ind, "map.collated.rad"), "rb").read()
    n_out = len(want["nrec"])
    want_head = rad.rad_prelude_atac(NAMES, REF_LEN, n_out, cblen=L)
    assert len(want_head) == len(head) and got[:len(head)] == want_head
    assert got[len(head):] == want["bytes"]
    j = json.load(open(os.path.join(ind, "collate.json")))
    assert set(j) == {"cmd", "version_str", "compressed_output"} and j["compressed_output"] is False and j["version_str"] == "0.18.0" and "atac collate" in j["cmd"]
    blob = open(os.path.join(ind, "unmapped_bc_count_collated.bin"), "rb").read()
    m = int.from_bytes(blob[:8], "little")
    assert len(blob) == 8 + 12 * m
    coll = {int.from_bytes(blob[8 + 12 * i:16 + 12 * i], "little"): int.from_bytes(blob[16 + 12 * i:20 + 12 * i], "little") for i in range(m)}
    exp = {}
    for b, k in unmapped or []:
        if b in corr:
            exp[corr[b]] = exp.get(corr[b], 0) + k
    assert coll == exp


@pytest.mark.parametrize("legacy,idle_cells", [(False, 0), (False, 4), (True, 0)])
def test_atac_collate_writes_the_judges_files(tmp_path, legacy, idle_cells):
    chunks, freq, corr, unmapped = dataset(31 + idle_cells, idle_cells=idle_cells)
    ind, rd, head, body, off = write_dirs(tmp_path, chunks, freq, corr, unmapped, legacy=legacy)
    r = run("atac", "collate", "-i", ind, "-r", rd, "-t", 4, "-m", 1000)
    assert r.returncode == 0, r.stderr
    cells = J.cell_order(freq)
    want = J.collate(body, off, 4, corr, cells)
    assert want["stats"]["n_kept"] > 500 and want["stats"]["n_uncorrected"] > 50 and want["stats"]["n_unmapped"] > 50 and want["stats"]["n_multimapped"] > 50
    judged_files(ind, head, want, corr, unmapped)
    # the absent-cells warning exactly when cells are absent, with both counts; the legacy warning exactly on the legacy path
    assert want["stats"]["n_cells_empty"] == idle_cells
    assert (ABSENT in r.stderr) == (idle_cells > 0)
    if idle_cells:
        assert f"{idle_cells} of {len(cells)} {ABSENT}" in r.stderr
    assert ("No correction_plan.bin was found; loading legacy permit_map.bin for ATAC collation" in r.stderr) == legacy
    assert f"writing num output chunks ({len(cells) - idle_cells}) to header" in r.stderr


def test_num_chunks_of_the_json_is_what_is_walked(tmp_path):
    """map.rad holds eight chunks, the JSON says six: six are collated"""
    chunks, freq, corr, unmapped = dataset(33)
    ind, rd, head, body, off = write_dirs(tmp_path, chunks, freq, corr, unmapped, num_chunks=6, extra_chunks=chunks[:2])
    assert len(off) == 6 and len(body) < os.path.getsize(os.path.join(rd, "map.rad")) - len(head)
    r = run("atac", "collate", "-i", ind, "-r", rd)
    assert r.returncode == 0, r.stderr
    judged_files(ind, head, J.collate(body, off, 4, corr, J.cell_order(freq)), corr, unmapped)


def test_a_missing_unmapped_file_is_an_empty_map_and_an_empty_permit_list_an_empty_rad(tmp_path):
    chunks, freq, corr, _ = dataset(34)
    ind, rd, head, body, off = write_dirs(tmp_path / "a", chunks, freq, corr, None)
    r = run("atac", "collate", "-i", ind, "-r", rd)
    assert r.returncode == 0, r.stderr
    judged_files(ind, head, J.collate(body, off, 4, corr, J.cell_order(freq)), corr, None)
    assert open(os.path.join(ind, "unmapped_bc_count_collated.bin"), "rb").read() == bytes(8)
    ind, rd, head, body, off = write_dirs(tmp_path / "b", chunks, {}, {}, None)
    r = run("atac", "collate", "-i", ind, "-r", rd)
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(ind, "map.collated.rad"), "rb").read() == rad.rad_prelude_atac(NAMES, REF_LEN, 0, cblen=L) and ABSENT not in r.stderr


def collated_cells(want, bc_bytes=4):
    """the judge's output as atac_dedup_judge reads it: [(barcode, records)]"""
    out = []
    for o in want["chunk_off"][:-1]:
        bc, records, _ = D.read_chunk(want["bytes"], o, bc_bytes)
        out.append((bc, records))
    return out


@pytest.mark.parametrize("all_pairs", [False, True])
def test_atac_collate_then_atac_deduplicate(tmp_path, all_pairs):
    chunks, freq, corr, unmapped = dataset(35, all_pairs=all_pairs, idle_cells=2)
    ind, rd, head, body, off = write_dirs(tmp_path, chunks, freq, corr, unmapped)
    r = run("atac", "collate", "-i", ind, "-r", rd)
    assert r.returncode == 0, r.stderr
    r = run("atac", "deduplicate", "-i", ind, "-t", 3, "-d", "fw")
    assert r.returncode == 0, r.stderr
    got = open(os.path.join(ind, "map.bed")).read().splitlines()
    # against the dedup judge applied to the collate judge's cells
    want = J.collate(body, off, 4, corr, J.cell_order(freq))
    cells = collated_cells(want)
    batch = D.judge_cells([recs for _, recs in cells])
    exp = []
    for i, (bc, _) in enumerate(cells):
        exp += D.bed_lines(batch.rows[batch.cell_ptr[i]:batch.cell_ptr[i + 1]], bc, NAMES, L, False)
    assert Counter(got) == Counter(exp)
    assert len(got) == len(batch.rows) - batch.n_long_fragments > 200 and batch.n_deduplicated > 5 and batch.n_long_fragments > 5   # (the dataset reaches them)
    assert (batch.n_not_mapped_pair > 0) == (not all_pairs) and batch.n_multimapped == 0   # (collate kept only records with one alignment)
    for line in D.log_lines(batch):
        assert line + "\n" in r.stderr, (line, r.stderr)
    if not all_pairs:
        return
    # every alignment a proper pair: `atac sort` of the same uncollated bytes yields the same (barcode, ref, start, frag_len, count)
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    q = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    try:
        obs = sorted(corr)
        s = q.atac_sort_rad(body, off, obs, [corr[b] for b in obs], REF_LEN, bc_bytes=4)
    finally:
        q.close()
    assert int(s["count"].max()) < 65536 and int(s["count"].max()) > 1
    sort_lines = [f"{NAMES[r_]}\t{st}\t{st + fl}\t{D.bc_string(int(b), L, False)}\t{k}"
                  for r_, st, fl, b, k in zip(s["ref"].tolist(), s["start"].tolist(), s["frag_len"].tolist(), s["bc"].tolist(), s["count"].tolist()) if fl < 2000]
    assert Counter(got) == Counter(sort_lines)
