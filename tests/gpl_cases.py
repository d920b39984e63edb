"""Case builders for the generate-permit-list tests: inputs of afq_gpl_hist_rad (chunks of an uncollated RNA RAD) and of
afq_gpl_correct (observed / retained barcode lists), each at the smallest shape at which the kernels can go wrong.
tests/test_gpl_cases_cpu.py shows without a device that every case reaches what it claims; tests/test_gpu_gpl.py runs them
against tests/gpl_judge.py.  A parse case is a dict: chunks (the judge's view), data / off (the bytes), bc_bytes, umi_bytes,
pos_bytes.  A correct case is a dict: L, neighborhood, resolution, retained {bc: count}, observed [(bc, count)] ascending."""
import random

import numpy as np

import gpl_judge as J
from util import pkg

rad = pkg.rad
WIDTHS = [1, 2, 4, 8]
ORIS = ["both", "fw", "rc"]


def parse_case(chunks, bc_bytes=4, umi_bytes=4, pos_bytes=0, pad=0):
    data, off = rad.encode_chunks(chunks, bc_bytes=bc_bytes, umi_bytes=umi_bytes, pos_bytes=pos_bytes, pad=pad)
    return {"chunks": chunks, "data": data, "off": off, "bc_bytes": bc_bytes, "umi_bytes": umi_bytes, "pos_bytes": pos_bytes}


def want_hist(case, ori):
    hist, n_rec, n_compat, max_ambig = J.histogram(case["chunks"], ori)
    bcs = sorted(hist)
    return {"bc": np.asarray(bcs, np.uint64), "count": np.asarray([hist[b] for b in bcs], np.uint64), "n_records": n_rec,
            "n_compatible": n_compat, "max_ambig": max_ambig}


def same_hist(got, want, what=""):
    assert np.array_equal(got["bc"], want["bc"]), (what, "barcodes", got["bc"][:8], want["bc"][:8])
    assert np.array_equal(got["count"], want["count"]), (what, "counts")
    st = got["stats"]
    assert (st["n_records"], st["n_compatible"], st["max_ambig"]) == (want["n_records"], want["n_compatible"], want["max_ambig"]), (what, st, want)


def rec_size(na, bc_bytes, umi_bytes, pos_bytes=0):
    return 4 + bc_bytes + umi_bytes + na * (4 + pos_bytes)


def rand_alns(rng, na, p_fw=0.5):
    return [(rng.randrange(1 << 20), rng.random() < p_fw) for _ in range(na)]


def rand_record(rng, bc_bytes, umi_bytes, na, n_bc=12, p_fw=0.5):
    top = (1 << (8 * bc_bytes)) - 1
    bc = rng.choice([0, top, top - 1, 1]) if rng.random() < 0.3 else (rng.randrange(n_bc) * 0x9E3779B1 + 7) % (top + 1)
    return (bc, rng.randrange(1 << (8 * umi_bytes)), rand_alns(rng, na, p_fw))


# ------------------------------------------------------------------------------------------------------------------ parse
def widths_case(bc_bytes, umi_bytes, pos_bytes, seed=1):
    """a few chunks of mixed records (na 0..5, every orientation mix, barcode 0 and the all-ones barcode of the width)"""
    rng = random.Random(seed * 1000 + bc_bytes * 100 + umi_bytes * 10 + pos_bytes)
    chunks = [[rand_record(rng, bc_bytes, umi_bytes, rng.choice([0, 1, 1, 2, 3, 5]), p_fw=rng.choice([0.0, 0.5, 1.0])) for _ in range(n)] for n in (70, 1, 0, 133)]
    return parse_case(chunks, bc_bytes, umi_bytes, pos_bytes)


def alignment_case(pad):
    """the first chunk at byte alignment `pad` of the buffer; 1-byte barcodes and 2-byte UMIs give odd record sizes, so the later
    chunks (and the tiles inside a chunk) start at other alignments"""
    rng = random.Random(40 + pad)
    chunks = [[rand_record(rng, 1, 2, rng.choice([0, 1, 2, 3])) for _ in range(n)] for n in (5, 6, 7, 300)]
    return parse_case(chunks, 1, 2, 0, pad=pad)


def fill_nas(target, H, A, avg=2):
    """alignment counts of records (head H, alignment A bytes) whose sizes sum to exactly `target` bytes"""
    k = max(1, target // (H + avg * A))
    while (target - k * H) % A or target - k * H < 0:
        k -= 1
        assert k >= 1, (target, H, A)
    total = (target - k * H) // A
    nas = [total // k + (1 if i < total % k else 0) for i in range(k)]
    assert sum(H + A * n for n in nas) == target
    return nas


def tile_edge_case(lim, delta, bc_bytes=2, umi_bytes=1):
    """one chunk whose records end exactly at the first tile's end (delta 0), one byte before it (-1: the next record starts on
    the tile's last byte) or one byte after it (+1: the last record of the tile straddles its end); a second tile follows"""
    rng = random.Random(7 + delta)
    H, A = 4 + bc_bytes + umi_bytes, 4
    nas = fill_nas(lim["parse_tile"] + delta, H, A) + [2, 0, 1, 3, 1]
    recs = [rand_record(rng, bc_bytes, umi_bytes, na) for na in nas]
    return parse_case([recs], bc_bytes, umi_bytes), len(nas) - 5


def halo_case(lim, na, pos_bytes=8):
    """the widest record (8-byte barcode and UMI, 8 position bytes) starting on the tile's LAST FOUR BYTES (every size is a multiple
    of 4 at these widths: no later start exists) with `na` alignments of which only the last is forward: na = lane_alns reaches
    farthest into the halo and is read from LDS, lane_alns + 1 is a long record"""
    rng = random.Random(90 + na)
    H, A = 20, 4 + pos_bytes
    nas = fill_nas(lim["parse_tile"] - 4, H, A)
    recs = [rand_record(rng, 8, 8, n, p_fw=0.0) for n in nas]
    recs.append((0xFFFFFFFFFFFFFFFF, 5, [(9, False)] * (na - 1) + [(9, True)]))
    recs += [rand_record(rng, 8, 8, 1, p_fw=0.0) for _ in range(3)]
    return parse_case([recs], 8, 8, pos_bytes), len(nas)


def long_case(where, na=2500, decoy_na=3000):
    """long records under fw: the only forward alignment is the first, the last, or absent (where = "first" / "last" / "absent");
    the same under rc by symmetry (the test flips nothing: it runs both orientations against the judge).  A record with the
    largest na of the file (decoy_na) has only REVERSE alignments: under fw it is not compatible and must not set max-ambig."""
    def alns(n, pos, fw):
        return [(i, (i == pos) == fw) for i in range(n)]
    pos = {"first": 0, "last": na - 1, "absent": -1}[where]
    recs = [(11, 1, [(3, True)]), (12, 2, alns(na, pos, True)), (13, 3, [(4, False), (5, True)]), (14, 4, [(1, False)] * decoy_na), (12, 5, alns(na, pos, False)),
            (15, 6, [])]
    return parse_case([[(10, 0, [(1, True)])], recs, [(16, 7, [(2, True)] * 40)]])


def malformed_case(kind):
    """four chunks of which chunk 2 is malformed; returns (data, off).  kinds: head_cut (nbytes ends inside the last record's head),
    alns_cut (... inside its alignment list), junk (3 bytes behind the last record), nrec_low / nrec_high (the header's count)."""
    rng = random.Random(3)
    chunks = [[rand_record(rng, 4, 4, rng.choice([1, 2, 40])) for _ in range(n)] for n in (3, 4, 300, 2)]
    c = parse_case(chunks)
    data, off = bytearray(c["data"]), c["off"].copy()
    o2, o3 = int(off[2]), int(off[3])
    nb = int.from_bytes(data[o2:o2 + 4], "little")
    nrec = int.from_bytes(data[o2 + 4:o2 + 8], "little")
    last = rec_size(len(chunks[2][-1][2]), 4, 4)
    def set_hdr(nbytes, n):
        data[o2:o2 + 4] = int(nbytes).to_bytes(4, "little")
        data[o2 + 4:o2 + 8] = int(n).to_bytes(4, "little")
    if kind == "head_cut":
        set_hdr(nb - last + 7, nrec)
    elif kind == "alns_cut":
        assert last > 12 + 2
        set_hdr(nb - 2, nrec)
    elif kind == "junk":
        data[o3:o3] = b"\x00\x00\x00"
        off[3] += 3
        set_hdr(nb + 3, nrec)
    elif kind == "nrec_low":
        set_hdr(nb, nrec - 1)
    elif kind == "nrec_high":
        set_hdr(nb, nrec + 1)
    else:
        raise ValueError(kind)
    return bytes(data), off


# ------------------------------------------------------------------------------------------------------------------ count
def hot_case(n=70000, n_chunks=70):
    """one barcode on 70 000 records spread over many chunks (one counter takes every add), barcode 0 and the all-ones barcode beside it"""
    per = n // n_chunks
    chunks = [[(0xABCDEF0123, i, [(1, True)]) for i in range(per)] + [(0, 1, [(2, True)]), (0xFFFFFFFFFFFFFFFF, 2, [(2, False)])] for _ in range(n_chunks)]
    return parse_case(chunks, 8, 4)


def barcodes_homing_at(slot, n_kept, count, bc_bytes=8, seed=5):
    rng = random.Random(seed)
    out = set()
    while len(out) < count:
        b = rng.randrange(1 << 62)
        if pkg.gpl_table_slot(b, n_kept, bc_bytes)[0] == slot:
            out.add(b)
    return sorted(out)


def chain_case(wrap, n_kept=48, chain=6):
    """`chain` distinct barcodes with one home slot in the table of n_kept records (capacity from the slot helper); wrap: the home
    slot is the table's last, so the probe chain wraps to slot 0.  Every barcode occurs more than once; filler barcodes make n_kept."""
    cap = pkg.gpl_table_slot(0, n_kept)[1]
    slot = cap - 1 if wrap else cap // 3
    bcs = barcodes_homing_at(slot, n_kept, chain)
    recs = [(b, i, [(1, True)]) for i, b in enumerate(bcs * 3)]
    rng = random.Random(8)
    while len(recs) < n_kept:
        recs.append((rng.randrange(1 << 40), 0, [(1, True)]))
    rng.shuffle(recs)
    return parse_case([recs[:20], recs[20:]], 8, 4), bcs, cap, slot


def capacity_step_case(n):
    """n records with n DISTINCT barcodes: at n a power of two the table is exactly half full; n + 1 takes the next capacity"""
    return parse_case([[(1000003 * (i + 1), i, [(1, True)]) for i in range(n)]], 8, 4)


def two_fill_cases():
    """two fills of one context with a barcode present in both (the caller merges the sorted histograms)"""
    a = parse_case([[(5, 0, [(1, True)]), (7, 0, [(1, True)]), (5, 1, [(1, True), (2, False)])]], 4, 4)
    b = parse_case([[(7, 0, [(1, True)] * 3), (9, 0, [(1, True)])], [(7, 2, [(1, True)])]], 4, 4)
    return a, b


def merge_hists(ha, hb):
    m = {}
    for h in (ha, hb):
        for b, n in zip(h["bc"].tolist(), h["count"].tolist()):
            m[b] = m.get(b, 0) + n
    ks = sorted(m)
    return np.asarray(ks, np.uint64), np.asarray([m[k] for k in ks], np.uint64)


# ------------------------------------------------------------------------------------------------------------------ correct
RNA = ("frequency", (39, 40), 1)


def correct_case(L, neighborhood, resolution, retained, observed):
    return {"L": L, "neighborhood": neighborhood, "resolution": resolution, "retained": dict(retained), "observed": sorted(dict(observed).items())}


def want_correct(case):
    """what afq_gpl_correct returns for the case: per observed barcode the decision and the target's index in the sorted retained
    list, the stats over the OBSERVED barcodes, the target counts.  (The identity entries of never-observed retained barcodes are
    the compilation's: J.Index.compile_distinct_observed_with_target_counts.)"""
    idx = J.identity_index(case["L"], case["neighborhood"], case["resolution"], case["retained"])
    ret = sorted(case["retained"])
    pos = {b: i for i, b in enumerate(ret)}
    code = {J.EXACT: 0, J.CORRECTED: 1, J.AMBIGUOUS: 2, J.NOT_FOUND: 3}
    dec, tgt, tc, stats = [], [], [0] * len(ret), J.Index.new_stats()
    for b, n in case["observed"]:
        d, t = idx.resolve(b)
        J.Index._tally(stats, d, n)
        dec.append(code[d])
        tgt.append(0xFFFFFFFF if t is None else pos[t])
        if t is not None:
            tc[pos[t]] += n
    return {"decision": np.asarray(dec, np.uint8), "target": np.asarray(tgt, np.uint32), "target_count": np.asarray(tc, np.uint64), "stats": stats,
            "retained": np.asarray(ret, np.uint64), "retained_count": np.asarray([case["retained"][b] for b in ret], np.uint64)}


def same_correct(got, want, what=""):
    for k in ("decision", "target", "target_count"):
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8])
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


L4_RETAINED = [
    {},                                                     # nothing retained: everything is not found
    {0x1B: 5},                                              # one source
    {0x00: 3, 0xFF: 0, 0x55: 9, 0xAA: 9},                   # the four homopolymers (shift candidates repeat)
    {0x1B: 38, 0x1A: 0, 0x2B: 0, 0xE4: 7, 0x6C: 2, 0x6D: 2},   # neighbours of one another: collisions of every kind
    {b: (2000 if b % 4 == 0 else (b * 7) % 5) for b in range(0, 256, 11)},   # dense, a few heavy: several candidates, and priors that decide
]


def l4_case(k, neighborhood, resolution):
    """L = 4, exhaustive: all 256 barcodes observed (counts 0..10) against retained set k"""
    return correct_case(4, neighborhood, resolution, L4_RETAINED[k], {b: (b * 7 + 3) % 11 for b in range(256)})


def random_case(L, neighborhood, resolution, n_ret=40, seed=2, top_bit=False):
    """retained barcodes at random (with bit 2L-1 set on half of them when top_bit), observed: every neighbour of the first 6, the
    retained ones themselves bar a few (never observed), and random others"""
    rng = random.Random(seed * 100 + L)
    full = (1 << (2 * L)) - 1
    ret = {}
    while len(ret) < n_ret:
        b = rng.randrange(full + 1)
        if top_bit and len(ret) % 2:
            b |= 1 << (2 * L - 1)
        ret[b] = rng.choice([0, 1, 5, 37, 38, 1000])
    srcs = sorted(ret)
    # a close pair, so that some observed barcodes have two retained neighbours
    ret[srcs[0] ^ 1] = 3
    obs = {}
    for s in srcs[:6]:
        for nb in J.neighbors(s, L, J.SHIFT):
            obs[nb] = rng.randrange(1, 20)
    for s in srcs[3:]:
        obs[s] = rng.randrange(0, 50)
    for _ in range(200):
        obs[rng.randrange(full + 1)] = rng.randrange(1, 5)
    if L == 32:
        obs[full] = 2
        obs[0] = 1
    return correct_case(L, neighborhood, resolution, ret, obs)


def boundary_case_l32(resolution="unique"):
    """L = 32, 8-byte barcodes: sources with bit 63 set and the all-ones barcode; the observed barcodes are their shift neighbours at
    boundaries 1 and 31 (the masks' two ends) and their substitutions at base 31"""
    srcs = {0xFFFFFFFFFFFFFFFF: 4, 0x8000000000000001: 2, 0xC3C3C3C3C3C3C3C3: 7, 0x1B1B1B1B1B1B1B1B: 1}
    obs = {}
    for s in srcs:
        for boundary in (1, 31):
            lower_mask = (1 << (2 * boundary)) - 1
            upper, lower = s & ~lower_mask & J.U64, s & lower_mask
            for adm in range(4):
                obs[upper | (adm << (2 * (boundary - 1))) | (lower >> 2)] = 3
                obs[(upper | adm | (lower << 2)) & J.U64] = 2
        for rep in range(4):
            obs[(s & ~(3 << 62) & J.U64) | (rep << 62)] = 1
    return correct_case(32, J.SHIFT, resolution, srcs, obs)


def frequency_cases():
    """name -> (case, observed barcode, expected decision, expected target or None); L = 4, hamming-1 unless said"""
    x, a, b = 0x00, 0x01, 0x02   # a and b are substitutions of x at base 0
    out = {
        "39_of_40_accepted": (correct_case(4, J.HAMMING, RNA, {a: 38, b: 0}, {x: 6}), x, J.CORRECTED, a),
        "38_of_39_ambiguous": (correct_case(4, J.HAMMING, RNA, {a: 37, b: 0}, {x: 6}), x, J.AMBIGUOUS, None),
        "tie_at_half_goes_to_greatest": (correct_case(4, J.HAMMING, ("frequency", (1, 2), 1), {a: 4, b: 4}, {x: 6}), x, J.CORRECTED, b),
        "confidence_0": (correct_case(4, J.HAMMING, ("frequency", (0, 1), 1), {a: 0, b: 0, 0x03: 0}, {x: 1}), x, J.CORRECTED, 0x03),
        "confidence_1_two_targets": (correct_case(4, J.HAMMING, ("frequency", (1, 1), 1), {a: 1000, b: 0}, {x: 1}), x, J.AMBIGUOUS, None),
        "confidence_1_one_target": (correct_case(4, J.HAMMING, ("frequency", (1, 1), 1), {a: 0}, {x: 1}), x, J.CORRECTED, a),
    }
    # a source S reachable from x by a substitution AND by a shift weighs once: weight 20 against 1 is 20/21 < 39/40 (ambiguous);
    # counted twice it would be 40/41 >= 39/40 (corrected)
    for xx in range(256):
        both = set(J.substitutions(xx, 4)) & set(J.inverse_shift_candidates(xx, 4))
        only_sub = [s for s in J.substitutions(xx, 4) if s not in J.inverse_shift_candidates(xx, 4)]
        if both and only_sub:
            s, t = sorted(both)[0], only_sub[0]
            out["sub_and_shift_once"] = (correct_case(4, J.SHIFT, RNA, {s: 19, t: 0}, {xx: 2}), xx, J.AMBIGUOUS, None)
            break
    return out


def never_observed_case():
    """a -b list with a barcode that was never observed: identity entry, exact_distinct counted, absent from permit_freq"""
    return correct_case(4, J.HAMMING, "unique", {0x10: 0, 0x33: 0}, {0x33: 5, 0x32: 2, 0xC0: 1})


# ------------------------------------------------------------------------------------------------------------------ whole command
def cli_dataset(seed=9, L=16, n_cells=40, n_noise=150):
    """a small experiment for the sub-command: two populations of barcodes (cells with 30-60 reads, noise with 1-3), a tenth of
    the cells' reads carrying one substitution or a shift, records of every orientation mix over chunks of uneven size.  Returns
    (chunks, cells, (heavy, sibling, midpoint)): `midpoint` is observed and lies one substitution from the cell `heavy` and one
    from `sibling`, which is never observed - on a -b list, unique calls the midpoint ambiguous and frequency gives it to `heavy`."""
    rng = random.Random(seed)
    full = (1 << (2 * L)) - 1
    cells = sorted({rng.randrange(full + 1) for _ in range(n_cells)})
    recs = []
    def alns():
        r = rng.random()
        if r < 0.05:
            return []
        if r < 0.15:
            return [(rng.randrange(100), False)] * rng.choice([1, 3])
        return [(rng.randrange(100), rng.random() < 0.8) for _ in range(rng.choice([1, 1, 1, 2, 4, 30]))]
    for c in cells:
        for _ in range(rng.randrange(30, 60)):
            b = c
            if rng.random() < 0.1:
                b = rng.choice(J.neighbors(c, L, J.SHIFT))
            recs.append((b, rng.randrange(1 << 24), alns()))
    for _ in range(n_noise):
        b = rng.randrange(full + 1)
        recs += [(b, rng.randrange(1 << 24), alns()) for _ in range(rng.randrange(1, 4))]
    heavy = cells[0]
    recs += [(heavy, rng.randrange(1 << 24), [(1, True)]) for _ in range(40)]   # (at least 39 exact reads: weight 40 of 41 >= 39/40)
    midpoint, sibling = heavy ^ 1, heavy ^ 1 ^ (1 << 10)
    recs += [(midpoint, 7, [(2, True)]), (midpoint, 8, [(3, True)])]
    rng.shuffle(recs)
    cuts = [0, 1, 400, 401, 1200, len(recs)]
    return [recs[a:b] for a, b in zip(cuts, cuts[1:])], cells, (heavy, sibling, midpoint)
