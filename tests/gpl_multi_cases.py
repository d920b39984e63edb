"""Case builders for the multi-barcode generate-permit-list tests: inputs of afq_gpl_multi_hist_rad (chunks of an uncollated
two-barcode RNA RAD and a list of routing entries), each at the smallest shape at which the kernel can go wrong, and the small
experiment of the whole step.  tests/test_gpl_multi_cases_cpu.py shows without a device that every case reaches what it claims;
tests/test_gpu_gpl_multi.py and tests/test_gpu_gpl_multi_chain.py run them against tests/gpl_multi_judge.py.  A parse case is a dict:
chunks (the judge's view: records (b0, b1, umi, alns)), data / off (the bytes), entries, b0_bytes, b1_bytes, umi_bytes, pos_bytes."""
import os
import random

import numpy as np

import gpl_cases as G
import gpl_judge as J
import gpl_multi_judge as M
from util import pkg

rad = pkg.rad
B_WIDTHS = [1, 2, 4]
U_WIDTHS = [1, 2, 4, 8]
ORIS = G.ORIS


def top(width):
    return (1 << (8 * width)) - 1


def multi_case(chunks, entries, b0_bytes=2, b1_bytes=4, umi_bytes=4, pos_bytes=0, pad=0):
    data, off = rad.encode_multi_bc_chunks(chunks, b0_bytes, b1_bytes, umi_bytes, pos_bytes=pos_bytes, pad=pad)
    return {"chunks": chunks, "data": data, "off": off, "entries": sorted(entries), "b0_bytes": b0_bytes, "b1_bytes": b1_bytes, "umi_bytes": umi_bytes,
            "pos_bytes": pos_bytes}


def want_pairs(case, ori):
    pairs, st = M.pair_histogram(case["chunks"], case["entries"], ori)
    ks = sorted(pairs)
    return {"entry": np.asarray([k[0] for k in ks], np.uint32), "cell": np.asarray([k[1] for k in ks], np.uint64),
            "count": np.asarray([pairs[k] for k in ks], np.uint64), "stats": st}


def same_pairs(got, want, what=""):
    for k in ("entry", "cell", "count"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k][:8], want[k][:8])
    st = {k: got["stats"][k] for k in want["stats"]}
    assert st == want["stats"], (what, got["stats"], want["stats"])
    assert got["stats"]["n_routed"] == int(got["count"].sum()) and got["stats"]["n_routed"] + got["stats"]["n_unrouted"] == got["stats"]["n_compatible"], what


def rec_size(na, case_or_head, pos_bytes=0):
    head = case_or_head if isinstance(case_or_head, int) else 4 + case_or_head["b0_bytes"] + case_or_head["b1_bytes"] + case_or_head["umi_bytes"]
    return head + na * (4 + pos_bytes)


def rand_record(rng, b0_pool, b1_bytes, umi_bytes, na, p_fw=0.5, n_cells=9):
    t1 = top(b1_bytes)
    b1 = rng.choice([0, t1, t1 - 1, 1]) if rng.random() < 0.3 else (rng.randrange(n_cells) * 0x9E3779B1 + 7) % (t1 + 1)
    return (rng.choice(b0_pool), b1, rng.randrange(1 << (8 * umi_bytes)), G.rand_alns(rng, na, p_fw))


# ------------------------------------------------------------------------------------------------------------------ parse
def widths_case(b0_bytes, b1_bytes, umi_bytes, edges="entries", pos_bytes=0, seed=1):
    """3 chunks of about 40 mixed records (na 0..5, every orientation mix).  The smallest (0) and the largest b0 of the width are
    routing entries (edges = "entries") or misses beside entries 1 and top - 1 ("misses"); the pairs (0, 0) and (all-ones, all-ones)
    occur in both."""
    rng = random.Random(seed * 10000 + b0_bytes * 1000 + b1_bytes * 100 + umi_bytes * 10 + pos_bytes)
    t0 = top(b0_bytes)
    mid = [5, 77, 100, 201]
    entries = ([0, t0] if edges == "entries" else [1, t0 - 1]) + mid[:3]
    pool = [0, t0, 1, t0 - 1] + mid   # (201 is never an entry)
    chunks = [[rand_record(rng, pool, b1_bytes, umi_bytes, rng.choice([0, 1, 1, 2, 3, 5]), p_fw=rng.choice([0.0, 0.5, 1.0])) for _ in range(n)] for n in (39, 1, 44)]
    chunks[0] += [(t0, top(b1_bytes), 3, [(1, True), (2, False)]), (0, 0, 4, [(1, False), (2, True)])]
    return multi_case(chunks, entries, b0_bytes, b1_bytes, umi_bytes, pos_bytes)


def alignment_case(pad):
    """the first chunk at byte alignment `pad` of the buffer; 1-byte barcodes and 1-byte UMIs give records of 7 + 4 na bytes, so the
    later chunks (and the tiles inside a chunk) start at other alignments"""
    rng = random.Random(40 + pad)
    chunks = [[rand_record(rng, [3, 4, 9, 250], 1, 1, rng.choice([0, 1, 2, 3])) for _ in range(n)] for n in (5, 6, 7, 300)]
    return multi_case(chunks, [3, 9, 250], 1, 1, 1, pad=pad)


def tile_edge_case(lim, delta):
    """one chunk whose records end exactly at the first tile's end (delta 0), one byte before it (-1: the next record starts on the
    tile's last byte) or one byte after it (+1: the last record of the tile straddles its end); a second tile follows.  Returns
    (case, index of the first record behind the filled bytes)."""
    rng = random.Random(7 + delta)
    H, A = 4 + 1 + 1 + 1, 4
    nas = G.fill_nas(lim["parse_tile"] + delta, H, A) + [2, 0, 1, 3, 1]
    pool = [3, 4, 9, 250]
    recs = [rand_record(rng, pool, 1, 1, na) for na in nas]
    recs[len(nas) - 5] = (9, 0xAB, 1, recs[len(nas) - 5][3])   # the record at the edge is routed: its pair must be counted
    return multi_case([recs], [3, 9, 250], 1, 1, 1), len(nas) - 5


def halo_case(lim, na, pos_bytes=8):
    """the widest record (4-byte b0 and b1, 8-byte UMI, 8 position bytes) starting on the tile's LAST FOUR BYTES (every size is a
    multiple of 4 at these widths: no later start exists) with `na` alignments of which only the last is forward: na = lane_alns
    reaches farthest into the halo and is read from LDS, lane_alns + 1 is a long record.  Returns (case, index of that record)."""
    rng = random.Random(90 + na)
    H, A = 4 + 4 + 4 + 8, 4 + pos_bytes
    nas = G.fill_nas(lim["parse_tile"] - 4, H, A)
    pool = [0xFFFFFFFF, 17, 0xCAFE0001]
    recs = [rand_record(rng, pool, 4, 8, n, p_fw=0.0) for n in nas]
    recs.append((0xFFFFFFFF, 0xFFFFFFFF, 5, [(9, False)] * (na - 1) + [(9, True)]))
    recs += [rand_record(rng, pool, 4, 8, 1, p_fw=0.0) for _ in range(3)]
    return multi_case([recs], [17, 0xFFFFFFFF], 4, 4, 8, pos_bytes), len(nas)


def long_case(where, na=2500, decoy_na=3000):
    """long records under fw: the only forward alignment is the first, the last, or absent (where = "first" / "last" / "absent");
    the same under rc by symmetry (the test runs both orientations against the judge).  The long records are routed (b0 = 12 is an
    entry); a longer one with only REVERSE alignments is routed too and must not count under fw; one long record is a miss."""
    def alns(n, pos, fw):
        return [(i, (i == pos) == fw) for i in range(n)]
    pos = {"first": 0, "last": na - 1, "absent": -1}[where]
    recs = [(11, 1, 1, [(3, True)]), (12, 2, 2, alns(na, pos, True)), (13, 3, 3, [(4, False), (5, True)]), (12, 4, 4, [(1, False)] * decoy_na),
            (12, 8, 5, alns(na, pos, False)), (15, 6, 6, []), (99, 2, 7, alns(na, pos, True))]
    return multi_case([[(12, 0, 0, [(1, True)])], recs, [(16, 7, 7, [(2, True)] * 40)]], [11, 12, 16])


def no_alignment_case():
    """records without an alignment beside records with one: na == 0 counts only under `both`"""
    recs = [(7, 1, 0, []), (7, 1, 1, [(1, True)]), (8, 2, 2, []), (7, 1, 3, [(1, False)]), (9, 3, 4, []), (7, 2, 5, [])]
    return multi_case([recs, [(7, 1, 6, [])]], [7, 9], 1, 2, 2)


def malformed_case(kind):
    """gpl_cases.malformed_case's bytes (four chunks of which chunk 2 is malformed; 4-byte barcode, 4-byte UMI) read as two-barcode
    records of the same head: b0 and b1 of 2 bytes each.  Returns (data, off)."""
    return G.malformed_case(kind)


# ------------------------------------------------------------------------------------------------------------ entry table
def n_entries_case(n, seed=4):
    """n routing entries (2-byte values at a stride); the records hit the first, the last and a middle one, and miss beside them.
    n = 64 fills the entry table exactly half (capacity 128); 65 takes the next capacity."""
    entries = [257 * i + 3 for i in range(n)]
    rng = random.Random(seed + n)
    pool = ([entries[0], entries[-1], entries[n // 2]] if n else []) + [2, 4, 60000]
    chunks = [[rand_record(rng, pool, 2, 2, rng.choice([1, 2])) for _ in range(k)] for k in (30, 12)]
    return multi_case(chunks, entries, 2, 2, 2)


def values_homing_at(slot, n_entries, count, seed=5, exclude=()):
    rng = random.Random(seed)
    out = set()
    while len(out) < count:
        b = rng.randrange(1 << 32)
        if b not in exclude and pkg.atac_sort_table_slot(b, n_entries)[0] == slot:
            out.add(b)
    return sorted(out)


def entry_chain_case(wrap, n_entries=48, chain=6):
    """`chain` entries with one home slot in the entry table of n_entries (capacity from afq_atac_sort_table_slot); wrap: the home
    slot is the table's last, so the probe chain wraps to slot 0.  Two more values with that home slot are NOT entries: their lookup
    walks the whole chain before it meets a free slot.  Returns (case, chain entries, the two misses, capacity, slot)."""
    cap = pkg.atac_sort_table_slot(0, n_entries)[1]
    slot = cap - 1 if wrap else cap // 3
    homed = values_homing_at(slot, n_entries, chain + 2)
    ch, misses = homed[:chain], homed[chain:]
    rng = random.Random(8)
    entries = set(ch)
    while len(entries) < n_entries:
        b = rng.randrange(1 << 32)
        if b not in homed:
            entries.add(b)
    recs = [(b, i % 5, i, [(1, True)]) for i, b in enumerate((ch + misses) * 3)]
    recs += [(b, 1, 0, [(1, True)]) for b in sorted(entries - set(ch))[:10]]
    rng.shuffle(recs)
    return multi_case([recs[:20], recs[20:]], entries, 4, 1, 1), ch, misses, cap, slot


# --------------------------------------------------------------------------------------------------------- counting table
def hot_case(n=70000, n_chunks=70):
    """one pair on 70 000 records spread over many chunks (one counter takes every add), two other pairs and a miss beside it"""
    per = n // n_chunks
    chunks = [[(500, 0xABCDEF01, i, [(1, True)]) for i in range(per)] + [(0, 0, 1, [(2, True)]), (500, 0xFFFFFFFF, 2, [(2, False)]), (501, 1, 3, [(1, True)])]
              for _ in range(n_chunks)]
    return multi_case(chunks, [0, 500, 600])


def keys_homing_at(slot, n_routed, entry, count, seed=6):
    rng = random.Random(seed)
    out = set()
    while len(out) < count:
        b1 = rng.randrange(1 << 32)
        if pkg.gpl_table_slot((entry << 32) | b1, n_routed, 8)[0] == slot:
            out.add(b1)
    return sorted(out)


def count_chain_case(n_routed=48, chain=4):
    """`chain` pairs whose keys entry << 32 | b1 home at the LAST slot of the counting table of n_routed records (capacity from
    afq_gpl_table_slot): the probe chain wraps to slot 0.  Every pair occurs three times; filler pairs make n_routed.
    Returns (case, the pairs, capacity)."""
    entries = [10, 20, 30]
    cap = pkg.gpl_table_slot(0, n_routed, 8)[1]
    cells = keys_homing_at(cap - 1, n_routed, 1, chain)
    recs = [(20, b1, i, [(1, True)]) for i, b1 in enumerate(cells * 3)]
    rng = random.Random(9)
    while len(recs) < n_routed:
        recs.append((rng.choice(entries), rng.randrange(1 << 32), 0, [(1, True)]))
    recs += [(11, 5, 0, [(1, True)])] * 3   # (misses: they take no slot)
    rng.shuffle(recs)
    return multi_case([recs[:20], recs[20:]], entries), [(1, b1) for b1 in cells], cap


def two_fill_cases():
    """two fills of one context over the same entries with a pair present in both (the caller merges the sorted outputs)"""
    ent = [5, 7]
    a = multi_case([[(5, 1, 0, [(1, True)]), (7, 1, 0, [(1, True)]), (5, 1, 1, [(1, True), (2, False)]), (6, 1, 0, [(1, True)])]], ent)
    b = multi_case([[(7, 1, 0, [(1, True)] * 3), (7, 9, 0, [(1, True)])], [(5, 1, 2, [(1, True)]), (8, 1, 0, [(1, True)])]], ent)
    return a, b


def merge_pairs(ga, gb):
    m = {}
    for g in (ga, gb):
        for e, c, n in zip(g["entry"].tolist(), g["cell"].tolist(), g["count"].tolist()):
            m[(e, c)] = m.get((e, c), 0) + n
    return m


# ------------------------------------------------------------------------------------------------------------ whole step
def seq(v, L):
    return rad.int_to_seq(v, L)


def sample_rows(rows, reverse=False):
    """the text of a three-column sample list: rows of (observed, canonical, name) as packed 8-mers.  reverse: the file holds the
    reverse complements (what --sample-bc-ori reverse undoes)"""
    def s(v):
        t = seq(v, 8)
        return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[ch] for ch in reversed(t)) if reverse else t
    return "# observed\tcanonical\tname\n\n" + "".join(f"{s(o)}\t{s(c)}\t{n}\n" for o, c, n in rows)


def routing_design():
    """Three samples of two rotations each over 8-base sample barcodes, built so that under hamming-1 there are barcodes of every
    kind: exact sources, structurally unique neighbours, structurally AMBIGUOUS ones (one substitution from rotations of two
    samples), and barcodes that reach no source.  Sample "gamma" is never observed.  b0 is a0 with another last base and b1 is a1
    with another fifth base, so the two remaining bases at either position lie between alpha and beta.
    Returns (rows, kinds): kinds maps "exact" / "unique" / "ambig_a0_b0" / "ambig_a1_b1" / "none" to sample barcodes."""
    a0, a1 = M.pack("ACGTACGT"), M.pack("TTGGCCAA")
    b0, b1 = M.pack("ACGTACGA"), M.pack("TTGGACAA")
    g0, g1 = M.pack("CATGCATG"), M.pack("TGCATGCA")
    rows = [(a0, a0, "alpha"), (a1, a0, "alpha"), (b0, b0, "beta"), (b1, b0, "beta"), (g0, g0, "gamma"), (g1, g0, "gamma")]
    kinds = {"exact": [a0, a1, b0, b1], "unique": [a1 ^ 1, b1 ^ (2 << 4), a0 ^ (1 << 10)],
             "ambig_a0_b0": [M.pack("ACGTACGC"), M.pack("ACGTACGG")], "ambig_a1_b1": [M.pack("TTGGGCAA"), M.pack("TTGGTCAA")],
             "none": [M.pack("GGGGGGGG"), M.pack("CCCCAAAA")]}
    return rows, kinds


def chain_dataset(seed=9, L=16, n_cells=30, n_noise=150):
    """The small experiment of the whole step: per observed sample about n_cells cells (30-60 reads, a tenth carrying one
    substitution) and n_noise noise barcodes (1-3 reads), sample barcodes of every kind of routing_design, records of every
    orientation mix over chunks of uneven size.  Rotation b0 of beta is read exactly three times while a0 is read hundreds of times,
    and a1 and b1 are both read hundreds of times: under Frequency at 39/40 the barcodes between a0 and b0 are accepted for alpha
    and those between a1 and b1 are rejected.  Returns (chunks, rows, kinds, cells per sample name)."""
    rng = random.Random(seed)
    rows, kinds = routing_design()
    full = (1 << (2 * L)) - 1
    a0, a1, b0, b1 = kinds["exact"]
    rots = {"alpha": [a0, a1], "beta": [b1]}
    near = {"alpha": [kinds["unique"][0], kinds["unique"][2]], "beta": [kinds["unique"][1]]}
    recs, cells = [], {}

    def alns():
        r = rng.random()
        if r < 0.05:
            return []
        if r < 0.15:
            return [(rng.randrange(100), False)] * rng.choice([1, 3])
        return [(rng.randrange(100), rng.random() < 0.8) for _ in range(rng.choice([1, 1, 1, 2, 4, 30]))]

    def sample_bc(name):
        r = rng.random()
        if r < 0.80:
            return rng.choice(rots[name])
        if r < 0.90:
            return rng.choice(near[name])
        if r < 0.96:
            return rng.choice(kinds["ambig_a0_b0"] + kinds["ambig_a1_b1"])
        return rng.choice(kinds["none"])

    for name in ("alpha", "beta"):
        cells[name] = sorted({rng.randrange(full + 1) for _ in range(n_cells)})
        for c in cells[name]:
            for _ in range(rng.randrange(30, 60)):
                b = c
                if rng.random() < 0.1:
                    b = rng.choice(J.substitutions(c, L))
                recs.append((sample_bc(name), b, rng.randrange(1 << 24), alns()))
        for _ in range(n_noise):
            b = rng.randrange(full + 1)
            recs += [(sample_bc(name), b, rng.randrange(1 << 24), alns()) for _ in range(rng.randrange(1, 4))]
    recs += [(b0, cells["beta"][i], i, [(1, True), (2, False)]) for i in range(3)]
    # a midpoint between a heavy cell of alpha and a sibling that is never observed (unique: ambiguous on a -b list; frequency: the heavy one)
    h = cells["alpha"][0]
    recs += [(a0, h, rng.randrange(1 << 24), [(1, True), (1, False)]) for _ in range(45)]
    recs += [(a0, h ^ 1, 7, [(2, True), (2, False)]), (a0, h ^ 1, 8, [(3, True), (3, False)])]
    for k in ("ambig_a0_b0", "ambig_a1_b1", "none", "unique"):   # every kind at least once on a record compatible with every orientation
        for b in kinds[k]:
            recs.append((b, cells["alpha"][1], 1, [(1, True), (2, False)]))
    rng.shuffle(recs)
    cuts = [0, 1, 400, 401, 1200, len(recs)]
    return [recs[a:b] for a, b in zip(cuts, cuts[1:])], rows, kinds, cells


def write_chain_dir(path, chunks, L=16, sample_L=8, b0_bytes=2, b1_bytes=4, umi_bytes=4):
    os.makedirs(path, exist_ok=True)
    data, _off = rad.encode_multi_bc_chunks(chunks, b0_bytes, b1_bytes, umi_bytes)
    with open(os.path.join(path, "map.rad"), "wb") as f:
        f.write(rad.rad_prelude_multi_bc(["t%d" % i for i in range(100)], len(chunks), sample_L, L, 12, b_bytes=b1_bytes, umi_bytes=umi_bytes, b0_bytes=b0_bytes))
        f.write(data)
    return path


# the whole step's cases: the five filter methods, sample correction exact / unique / frequency (and the deprecated 1-edit), both sample
# orientations, cell correction unique and frequency, every expected orientation, and one run in several device fills
CHAIN_CASES = [
    dict(name="knee_exact", method="knee", sample_correction="exact"),
    dict(name="expect_unique", method="expect", method_count=30, sample_correction="unique"),
    dict(name="force_frequency", method="force", method_count=20, sample_correction="frequency"),
    dict(name="valid_bc_frequency_cell_frequency", method="valid_bc", sample_correction="frequency", correction="frequency"),
    dict(name="unfiltered_unique", method="unfiltered", min_reads=10, sample_correction="unique"),
    dict(name="unfiltered_frequency_reverse_cell_frequency", method="unfiltered", min_reads=5, sample_correction="frequency", sample_bc_ori="reverse",
         correction="frequency", confidence=(9, 10)),
    dict(name="knee_one_edit_rc", method="knee", sample_correction="1-edit", expected_ori="rc"),
    dict(name="knee_unique_shift_both", method="knee", sample_correction="unique", sample_neighborhood=J.SHIFT, neighborhood=J.SHIFT, expected_ori="both"),
    dict(name="force_frequency_reverse_fills", method="force", method_count=25, sample_correction="frequency", sample_bc_ori="reverse", sample_confidence=(78, 80),
         fill_bytes=20000),
]


def chain_lists(cells):
    """the -b list (most cells of both samples and a sibling of alpha's heavy cell that is never observed) and the -u whitelist (the
    cells; the noise barcodes and the cells' one-substitution errors are NOT listed) as packed barcodes"""
    h = cells["alpha"][0]
    valid = cells["alpha"][:25] + cells["beta"][:25] + [h ^ 1 ^ (1 << 10)]
    white = cells["alpha"] + cells["beta"] + [h ^ 1 ^ (1 << 10)]
    return valid, white


def chain_want(case, chunks, rows, cells, list_file=None, cmdline=""):
    """the judge's outputs for one case of CHAIN_CASES"""
    valid, white = chain_lists(cells)
    meth = case["method"]
    reverse = case.get("sample_bc_ori", "forward") == "reverse"
    return M.gpl_multi_outputs(chunks, case.get("expected_ori", "fw"), sample_rows(rows, reverse), 16, meth, arg=case.get("method_count"),
                               listed={"valid_bc": valid, "unfiltered": white}.get(meth), min_reads=case.get("min_reads", 0) if meth == "unfiltered" else 0,
                               list_file=list_file, sample_mode=case["sample_correction"], sample_neighborhood=case.get("sample_neighborhood", J.HAMMING),
                               sample_confidence=case.get("sample_confidence", M.RNA_CONF), reverse=reverse, cell_correction=case.get("correction", "unique"),
                               cell_neighborhood=case.get("neighborhood"), cell_confidence=case.get("confidence", M.RNA_CONF), cmdline=cmdline)
