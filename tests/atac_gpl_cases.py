"""Inputs of `atac generate-permit-list` for tests/test_gpu_atac_gpl.py (the record pass) and tests/test_gpu_atac_gpl_chain.py (the
front-end), built on rad.encode_atac_chunks / rad.rad_prelude_atac and on the tile, halo and edge builders of tests/atac_sort_cases.py
(the record pass walks a chunk as the `atac sort` parse does).  The JUDGE of every result is tests/atac_gpl_judge.py on the
python-level chunks; nothing here decides whether a result is right.  Sizes come from atac_gpl_limits(), handed in as `lim`."""
import os
import random

import numpy as np

import atac_gpl_judge as J
import atac_sort_cases as S
from util import pkg

rad = pkg.rad
ONES = (1 << 64) - 1


def sort_lim(lim):
    """atac_sort_cases' builders take the `atac sort` limits dict: the same walk, with this record pass's tile and halo"""
    out = dict(pkg.atac_sort_limits())
    out.update(parse_tile=lim["parse_tile"], parse_halo=lim["parse_halo"])
    return out


# ------------------------------------------------------------------------------------------------------------- the judge's view
def want_of(chunks, blens, bin_size=J.SIZE_RANGE):
    """what afq_atac_gpl_hist_rad owes for python-level chunks: the judge's record pass as arrays"""
    hist, bins, max_ambig, n = J.record_pass(chunks, list(blens), bin_size)
    n0 = sum(1 for c in chunks for _, a in c if len(a) == 0)
    n1 = sum(1 for c in chunks for _, a in c if len(a) == 1)
    keys = sorted(hist)
    return {"bc": np.asarray(keys, np.uint64), "count": np.asarray([hist[k] for k in keys], np.uint64), "bins": np.asarray(bins, np.uint64),
            "stats": {"n_records": n, "n_unmapped": n0, "n_multimapped": n - n0 - n1, "n_binned": n1, "max_ambig": max_ambig, "max_bin": max(bins) if bins else 0}}


def same(got, want, what=""):
    bc, count, bins, stats = got
    for name, g in (("bc", bc), ("count", count), ("bins", bins)):
        assert g.dtype == np.uint64 and np.array_equal(g, want[name]), (what, name, len(g), len(want[name]))
    assert stats == want["stats"], (what, stats, want["stats"])
    assert int(count.sum()) == stats["n_records"] and int(bins.sum()) == stats["n_binned"], what


def blens_of(ref_lengths):
    return J.bin_lens([int(x) for x in ref_lengths])


# --------------------------------------------------------------------------------------------------------------------- the walk
def pool_of(bc_bytes, n=40, seed=0):
    rng = np.random.default_rng(200 + bc_bytes + seed)
    pool = S.distinct(rng, min(n, 1 << (8 * bc_bytes)), min(8 * bc_bytes, 63))
    if bc_bytes == 8:
        pool[::3] |= np.uint64(1) << np.uint64(63)
    return [int(x) for x in pool]


def mixed_chunks(lim, bc_bytes, ref_lengths):
    """na in {0, 1, 2, 400} interleaved (400 alignments are longer than tile + halo), a barcode per record; a header-only chunk; a
    one-record chunk; chunks of ~2.5 tiles at eight phases against the tile edges; a chunk that ENDS with an na == 0 record, one that
    ends with the na == 400 record, and 100 chunks of 1-3 records."""
    rng = np.random.default_rng(bc_bytes)
    pool = pool_of(bc_bytes)
    tile = lim["parse_tile"]
    assert 4 + 8 + 11 * 400 > tile + lim["parse_halo"]

    def alns(na):
        out = []
        for _ in range(na):
            r = int(rng.integers(0, len(ref_lengths)))
            out.append((r, int(rng.integers(1, 5)), int(rng.integers(0, max(ref_lengths[r], 1))), int(rng.integers(20, 2500))))
        return out

    def rec(na=None):
        return (pool[int(rng.integers(0, len(pool)))], alns(int(rng.choice([0, 1, 1, 1, 2])) if na is None else na))

    chunks = [[rec() for _ in range(40)], [], [rec(1)]]
    for phase in range(8):
        c = [(pool[0], []) for _ in range(phase)]
        size = 8 + phase * (4 + bc_bytes)
        while size < 2 * tile + tile // 2:
            r = rec()
            c.append(r)
            size += 4 + bc_bytes + 11 * len(r[1])
        chunks.append(c)
    chunks.append([rec(1), rec(400), rec(1), rec(2), rec(0)])          # ... an na == 0 record last
    chunks.append([rec(0), rec(1), rec(400)])                           # ... the long record last
    chunks.append([rec(0)])
    chunks += [[rec() for _ in range(int(rng.integers(1, 4)))] for _ in range(100)]
    return chunks


def walk_cases(lim, bc_bytes=4):
    """{name: (chunks, ref_lengths)}: atac_sort_cases' edge builders - the chunk body ends at tile edge - 1 / 0 / + 1 and at two tiles; the
    last record starts on the tile's last byte (head and alignment in the halo), ends its head or itself with the tile, or begins the
    next; records longer than a tile between short ones; a tile as full of record starts as the width allows."""
    sl = sort_lim(lim)
    out = {}
    for kind in S.EDGE_KINDS:
        c = S.exact_edge_case(sl, kind, bc_bytes)
        out["edge " + kind] = (c["chunks"], c["ref_lengths"])
    for pos in S.HALO_POSITIONS:
        c = S.halo_case(sl, bc_bytes, pos)
        out["halo " + pos] = (c["chunks"], c["ref_lengths"])
    c = S.tile_full_case(sl, bc_bytes)
    out["tile full"] = (c["chunks"], c["ref_lengths"])
    return out


def malformed(lim, bc_bytes=4):
    """{kind: (bytes, chunk_off, index of the bad chunk)}: three chunks, the middle one spoilt five ways"""
    H = 4 + bc_bytes
    good = [(7, [(0, 4, 5, 60)]), (9, []), (7, [(0, 4, 6, 61), (0, 4, 7, 62)])]
    data, off = rad.encode_atac_chunks([good, good, good], bc_bytes=bc_bytes)
    o1, o2 = int(off[1]), int(off[2])
    nb = o2 - o1

    def patch(at, v):
        b = bytearray(data)
        b[at:at + 4] = int(v).to_bytes(4, "little")
        return bytes(b)

    def resized(delta, tail=b""):
        """chunk 1 with nbytes changed by delta (its bytes cut, or `tail` appended), the chunks behind it moved"""
        body = data[o1:o2][:nb + delta] if delta < 0 else data[o1:o2] + tail
        b = data[:o1] + (nb + delta).to_bytes(4, "little") + body[4:] + data[o2:]
        return b, np.asarray([0, o1, o2 + delta], np.uint64)

    last_na_at = o2 - (H + 22)
    assert int.from_bytes(data[last_na_at:last_na_at + 4], "little") == 2
    head_cut = resized(-(H + 22) + 2)                       # the last record's head is cut after two bytes
    aln_cut = resized(-5)                                   # its second alignment loses five bytes
    junk = resized(3, b"\x01\x02\x03")                      # three bytes behind the last record: no head fits
    nrec = int.from_bytes(data[o1 + 4:o1 + 8], "little")
    return {"head cut": (*head_cut, 1), "alignments cut": (*aln_cut, 1), "junk tail": (*junk, 1),
            "nrec low": (patch(o1 + 4, nrec - 1), off, 1), "nrec high": (patch(o1 + 4, nrec + 1), off, 1)}, (data, off, [good, good, good])


# -------------------------------------------------------------------------------------------------------------------- the table
def chain_chunks(n_chain=60, n_wrap=20, n_rand=120, reps=3):
    """8-byte barcodes for the counting table of n = reps * (n_chain + n_wrap + n_rand + 2) records: n_chain with ONE home slot, n_wrap
    whose home slots are the table's last three (their chain wraps to slot 0), random ones, 1 << 63 and the all-ones barcode (which
    travels beside the table); every barcode `reps` times, shuffled over chunks of 97 records.  -> (chunks, info)"""
    n_bc = n_chain + n_wrap + n_rand + 2
    n = reps * n_bc
    slot = lambda x, _n: pkg.gpl_table_slot(x, n, 8)
    cap = slot(0, n)[1]
    home = slot(12345, n)[0]
    chain, _ = S._with_home(slot, n, {home}, n_chain, 1 << 40)
    wrap, _ = S._with_home(slot, n, {cap - 1, cap - 2, cap - 3}, n_wrap, 1 << 41)
    rng = np.random.default_rng(7)
    used = set(chain + wrap)
    rnd = [int(x) for x in S.distinct(rng, n_rand + 8, 63) if int(x) not in used][:n_rand]
    bcs = chain + wrap + rnd + [1 << 63, ONES]
    assert len(set(bcs)) == n_bc
    recs = [(b, [(0, 4, 5 * i, 40)] if i % 3 else []) for i, b in enumerate(bcs * reps)]
    random.Random(3).shuffle(recs)
    chunks = [recs[a:a + 97] for a in range(0, len(recs), 97)]
    return chunks, {"cap": cap, "home": home, "chain": chain, "wrap": wrap, "n": n}


def capacity_step_chunks(n_bc):
    """n_bc records of n_bc distinct 8-byte barcodes: at 64 the table (capacity 128) is exactly half full, at 65 the capacity doubles"""
    rng = np.random.default_rng(n_bc)
    bcs = [int(x) for x in S.distinct(rng, n_bc, 63)]
    return [[(b, [(0, 4, 7, 40)]) for b in bcs[:n_bc // 2]], [(b, []) for b in bcs[n_bc // 2:]]]


# -------------------------------------------------------------------------------------------------------------- the front-end
L = 16
NAMES, REF_LEN = ["chr1", "chrM", "tiny"], [400000, 9000, 70]
MIN_READS = 3


def bc_line(bc, rc):
    """the line of a barcode list that packs to `bc` for a run under `rc` (rc: the list spells the reverse complement)"""
    return rad.int_to_seq(J.reverse_complement(bc, L) if rc else bc, L)


def sub(bc, pos, to):
    """bc with base `pos` (0 = last) replaced by one of the three other bases"""
    base = (bc >> (2 * pos)) & 3
    return (bc & ~(3 << (2 * pos))) | (((base + to) & 3) << (2 * pos))


def chain_dataset(seed=41):
    """6 chunks, 3 references, ~1 200 records, 48 barcodes.  40 are listed; of the listed, `rare` occurs MIN_READS - 1 times (below the
    threshold) and `edge` exactly MIN_READS times; of the 8 unlisted, `near` is one substitution from one listed barcode (corrected),
    `between` one substitution from two of them (ambiguous, whatever their counts: they are drawn alike), the rest are random (no
    candidate).  Every alignment is a proper pair (type 4) so that `atac deduplicate` keeps what `atac sort` keeps.
    -> dict: chunks, listed (the 40, packed), list_text(rc), absent (listed lines no read carries), near, between, rare, edge"""
    rng = random.Random(seed)
    pool = rng.sample(range(1, 1 << 32), 48)
    listed, stray = pool[:40], pool[40:]
    x = sub(listed[1], 3, 1)
    listed[2] = sub(x, 7, 2)             # listed[1] and listed[2] are both one substitution from x
    near, between = sub(listed[0], 0, 1), x
    stray[0], stray[1] = near, between
    rare, edge = listed[38], listed[39]
    absent = rng.sample(range(1, 1 << 32), 5)
    assert len(set(listed + stray + absent)) == 53
    common = [b for b in listed + stray if b not in (rare, edge)]

    def alns(na):
        out = []
        for _ in range(na):
            r = rng.randrange(3)
            out.append((r, 4, rng.randrange(REF_LEN[r]) // 7 * 7, rng.choice([40, 41, 150, 1999, 2000, 2500])))
        return out

    chunks = []
    for _ in range(6):
        c = [(rng.choice(common), alns(rng.choice([0, 1, 1, 1, 1, 2]))) for _ in range(rng.randrange(170, 230))]
        c += [c[0], c[1], c[2], c[0]]   # exact duplicates
        chunks.append(c)
    for k in range(MIN_READS - 1):
        chunks[k].append((rare, alns(1)))
    for k in range(MIN_READS):
        chunks[5 - k].insert(3, (edge, alns(1)))

    def list_text(rc):
        lines = [bc_line(b, rc) for b in listed[:20]] + ["ACGTACGTNACGTACG"] + [bc_line(b, rc) for b in listed[20:] + absent] + [bc_line(listed[4], rc)]
        return "\n".join(lines) + "\n"

    return {"chunks": chunks, "listed": listed, "list_text": list_text, "absent": absent, "near": near, "between": between, "rare": rare, "edge": edge}


def write_mapper_dir(path, chunks, ref_lengths=REF_LEN, names=NAMES, cblen=L, bc_bytes=4, unmapped=None):
    """a mapper's output directory: map.rad (and unmapped_bc_count.bin).  -> (prelude, body, chunk_off)"""
    os.makedirs(path, exist_ok=True)
    body, off = rad.encode_atac_chunks(chunks, bc_bytes=bc_bytes)
    head = rad.rad_prelude_atac(names, ref_lengths, len(chunks), cblen=cblen, bc_bytes=bc_bytes)
    with open(os.path.join(path, "map.rad"), "wb") as f:
        f.write(head + body)
    if unmapped is not None:
        with open(os.path.join(path, "unmapped_bc_count.bin"), "wb") as f:
            f.write(b"".join(int(b).to_bytes(8, "little") + int(n).to_bytes(4, "little") for b, n in unmapped))
    return head, body, off
