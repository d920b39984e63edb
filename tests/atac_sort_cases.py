"""Hand-built inputs at the limits of `atac sort` (csrc/afq_atac_sort.hip and the levelling loop of afq_atac_sort_rad), shared by
tests/test_atac_sort_cases_cpu.py (builders and witnesses, no device) and tests/test_gpu_atac_sort*.py (the device against them).

A case is a dict: "data" (the chunk bytes), "off" (chunk offsets), "obs" / "cor" (the correction map), "ref_lengths", "bc_bytes",
"cols" (the decoded (bc, ref, start, frag_len) columns of the single-alignment records) and "counts" (#records, #na == 0, #na > 1).
The JUDGE of a device result is `expected(*case["cols"], case["obs"], case["cor"])`: np.lexsort + unique-with-counts on the
decoded records, which knows nothing of tiles, tables, keys or levels.  Everything below that restates the kernels - `tile_walk`
(how k_sort_parse cuts a chunk into tiles), `level_model` (DESIGN 3.4b's levelling rule), `table_slots` (linear probing) - is a
WITNESS: it shows that a builder's input reaches the edge it names, and never decides whether a result is right.

Every size comes from atac_sort_limits() (afq_atac_sort_limits and afq_atac_sort_leaf_limits), handed in as the dict `lim`; nothing
here copies a kernel constant.  The run-head cases are built around the two leaf workgroups' thread counts (the slices in which a
leaf's run heads are compacted) and the small-leaf size; the leaf-class case brackets that switch with 2^k - 1, 2^k, 2^k + 1 without
using it."""
import numpy as np

from util import pkg

rad = pkg.rad


# ------------------------------------------------------------------------------------------------- the judge and the encoders
def expected(bc, ref, start, fl, obs, cor):
    """the rows `atac sort` owes for the single-alignment records (bc, ref, start, fl) under the map obs -> cor"""
    bc, ref, start, fl = (np.asarray(x, dt) for x, dt in ((bc, np.uint64), (ref, np.uint32), (start, np.uint32), (fl, np.uint16)))
    obs, cor = np.asarray(obs, np.uint64), np.asarray(cor, np.uint64)
    o = np.argsort(obs)
    so, sc = obs[o], cor[o]
    i = np.minimum(np.searchsorted(so, bc), max(len(so) - 1, 0))
    hit = so[i] == bc if len(so) else np.zeros(len(bc), bool)
    cbc, ref, start, fl = sc[i][hit] if len(so) else bc[:0], ref[hit], start[hit], fl[hit]
    k = np.lexsort((cbc, fl, start, ref))
    cbc, ref, start, fl = cbc[k], ref[k], start[k], fl[k]
    head = np.ones(len(k), bool)
    if len(k):
        head[1:] = (ref[1:] != ref[:-1]) | (start[1:] != start[:-1]) | (fl[1:] != fl[:-1]) | (cbc[1:] != cbc[:-1])
    pos = np.flatnonzero(head)
    cnt = np.diff(np.append(pos, len(k))).astype(np.uint32)
    return {"ref": ref[pos], "start": start[pos], "frag_len": fl[pos], "bc": cbc[pos], "count": cnt,
            "n_uncorrected": int((~hit).sum()), "n_kept": int(hit.sum())}


def same(got, want, what=""):
    for k in ("ref", "start", "frag_len", "bc", "count"):
        assert got[k].dtype == want[k].dtype, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, len(got[k]), len(want[k]))
    st = got["stats"]
    assert st["n_distinct"] == len(want["ref"]) and st["n_kept"] == want["n_kept"] and st["n_uncorrected"] == want["n_uncorrected"], (what, st)
    assert st["n_long_fragments"] == int((want["frag_len"] >= 2000).sum()), (what, st)


def flat(chunks):
    """(bc, ref, start, fl) of the single-alignment records of python-level chunks, plus (#records, #na == 0, #na > 1)"""
    one = [(bc, a[0]) for recs in chunks for bc, a in recs if len(a) == 1]
    n = sum(len(r) for r in chunks)
    n0 = sum(1 for recs in chunks for _, a in recs if len(a) == 0)
    cols = ([b for b, _ in one], [a[0] for _, a in one], [a[2] for _, a in one], [a[3] for _, a in one])
    return cols, (n, n0, n - n0 - len(one))


def na1_chunks(bc, ref, start, fl, per_chunk, ty=4, bc_bytes=8):
    """chunks of single-alignment records, encoded with numpy (the large shapes): bytes, chunk_off"""
    dt = np.dtype([("na", "<u4"), ("bc", "<u%d" % bc_bytes), ("ref", "<u4"), ("ty", "u1"), ("start", "<u4"), ("fl", "<u2")])
    assert dt.itemsize == 15 + bc_bytes
    r = np.zeros(len(bc), dt)
    r["na"], r["bc"], r["ref"], r["ty"], r["start"], r["fl"] = 1, bc, ref, ty, start, fl
    out, offs = bytearray(), []
    for a in range(0, max(len(r), 1), per_chunk):
        body = r[a:a + per_chunk].tobytes()
        offs.append(len(out))
        out += (len(body) + 8).to_bytes(4, "little") + len(r[a:a + per_chunk]).to_bytes(4, "little") + body
    return bytes(out), np.asarray(offs, np.uint64)


def distinct(rng, n, bits):
    """n distinct integers below 2^bits, in random order"""
    if bits <= 20:
        return rng.permutation(1 << bits)[:n].astype(np.uint64)
    v = np.unique(rng.integers(0, 1 << bits, size=2 * n + 16, dtype=np.uint64))
    assert len(v) >= n
    return rng.permutation(v)[:n]


def _case_of_chunks(chunks, obs, cor, ref_lengths, bc_bytes):
    data, off = rad.encode_atac_chunks(chunks, bc_bytes=bc_bytes)
    cols, counts = flat(chunks)
    return {"data": data, "off": off, "obs": np.asarray(obs, np.uint64), "cor": np.asarray(cor, np.uint64),
            "ref_lengths": np.asarray(ref_lengths, np.uint32), "bc_bytes": bc_bytes, "cols": cols, "counts": counts, "chunks": chunks}


def _case_of_columns(bc, ref, start, fl, obs, cor, ref_lengths, bc_bytes, per_chunk=5000, shuffle_seed=None):
    bc, ref, start, fl = np.asarray(bc, np.uint64), np.asarray(ref, np.uint32), np.asarray(start, np.uint32), np.asarray(fl, np.uint16)
    if shuffle_seed is not None:
        p = np.random.default_rng(shuffle_seed).permutation(len(bc))
        bc, ref, start, fl = bc[p], ref[p], start[p], fl[p]
    data, off = na1_chunks(bc, ref, start, fl, per_chunk, bc_bytes=bc_bytes)
    return {"data": data, "off": off, "obs": np.asarray(obs, np.uint64), "cor": np.asarray(cor, np.uint64),
            "ref_lengths": np.asarray(ref_lengths, np.uint32), "bc_bytes": bc_bytes, "cols": (bc, ref, start, fl), "counts": (len(bc), 0, 0)}


def want_of(case):
    return expected(*case["cols"], case["obs"], case["cor"])


# ------------------------------------------------------------------------------------------------- witness: the parse tiles
def tile_walk(data, chunk_off, bc_bytes, lim):
    """WITNESS.  How k_sort_parse cuts one chunk: a tile begins at a record start (the first at byte 8 of the chunk), the record
    starts q below parse_tile are its records, a record takes H + 11 na bytes, the next tile begins where the last one of them
    ends.  Returns [(p, [(q, na), ...]), ...] per tile and the byte at which the walk ended (== nbytes for a well-formed chunk)."""
    tile, H = lim["parse_tile"], 4 + bc_bytes
    o = int(chunk_off)
    nb = int.from_bytes(data[o:o + 4], "little")
    p, tiles = 8, []
    while p < nb:
        q, recs = 0, []
        while q < tile and p + q < nb:
            assert nb - (p + q) >= H
            na = int.from_bytes(data[o + p + q:o + p + q + 4], "little")
            assert na <= (nb - (p + q) - H) // 11
            recs.append((q, na))
            q += H + 11 * na
        tiles.append((p, recs))
        p += q
    return tiles, p


def _pool(bc_bytes, n=40):
    """n barcodes of the width, with distinct bytes where the width allows it; the first 3/4 are the map"""
    rng = np.random.default_rng(100 + bc_bytes)
    pool = distinct(rng, min(n, 1 << (8 * bc_bytes)), min(8 * bc_bytes, 63))
    if bc_bytes == 8:
        pool[::3] |= np.uint64(1) << np.uint64(63)
    k = len(pool) * 3 // 4
    return pool, pool[:k], pool[:k][::-1].copy()


# ------------------------------------------------------------------------------------------------------------- parse cases
def tile_full_case(lim, bc_bytes):
    """Two chunks of 3 * (parse_tile // H) + 7 records: the first all na == 0 (a tile as full of record starts as the width allows:
    parse_tile // 5 + 1 of them at H == 5, the last at parse_tile - 1), the second with every 64th and 65th record na == 1, so that
    kept records sit in the last lane of one 64-lane trip and the first lane of the next."""
    H = 4 + bc_bytes
    n = 3 * (lim["parse_tile"] // H) + 7
    pool, obs, cor = _pool(bc_bytes)
    rng = np.random.default_rng(bc_bytes)
    B = 1 << lim["bin_shift"]
    rl = [3 * B + 1]
    c0 = [(int(pool[i % len(pool)]), []) for i in range(n)]
    c1 = [(int(pool[(7 * i) % len(pool)]), [(0, 4, int(rng.integers(0, rl[0])), int(rng.integers(20, 3000)))] if i and i % 64 in (63, 0) else []) for i in range(n)]
    return _case_of_chunks([c0, c1], obs, cor, rl, bc_bytes)


def long_record_nas(lim):
    """na of the multi-alignment records: 2, the three around the first na with 8 + 11 na > parse_tile + parse_halo, and 400, 1 000, 5 000"""
    c = (lim["parse_tile"] + lim["parse_halo"] - 8) // 11 + 1
    return [2, c - 2, c - 1, c, c + 26, 1000, 5000]


def long_records_case(lim, bc_bytes):
    """Single-alignment records between records that are longer than a tile (and than tile + halo): q jumps past everything staged.
    Chunk 0 interleaves them, chunk 1 is one long record alone, chunk 2 ends with one, chunk 3 begins with one."""
    pool, obs, cor = _pool(bc_bytes)
    rng = np.random.default_rng(10 + bc_bytes)
    B = 1 << lim["bin_shift"]
    rl = [2 * B + 3, 77]

    def one():
        r = int(rng.integers(0, 2))
        return (int(pool[rng.integers(0, len(pool))]), [(r, 4, int(rng.integers(0, rl[r])), int(rng.integers(20, 2500)))])

    def multi(na):
        return (int(pool[rng.integers(0, len(pool))]), [(0, 4, 0xEEEEEEEE, 0xEEEE)] * na)   # (fields of a record that is not kept are not read)

    nas = long_record_nas(lim)
    c0 = [one()]
    for na in nas:
        c0 += [multi(na), one(), one()]
    chunks = [c0, [multi(nas[-1])], [one(), one(), multi(nas[3])], [multi(nas[2]), one()], [multi(nas[1])]]
    return _case_of_chunks(chunks, obs, cor, rl, bc_bytes)


HALO_POSITIONS = ("last_byte", "head_fits", "record_fits", "next_tile")


def halo_case(lim, bc_bytes, position):
    """One chunk whose LAST record is a kept record with distinctive fields (frag_len 65 535, a start and a barcode whose bytes all
    differ) that starts at q == parse_tile - 1 (its head and alignment lie in the halo), parse_tile - H (the head ends with the
    tile), parse_tile - H - 11 (the record ends with the tile) or parse_tile (the padding ends with the tile; the record begins
    the next one).  In front of it: na == 0 records, and as few na == 1 / na == 2 records as the arithmetic needs."""
    tile, H = lim["parse_tile"], 4 + bc_bytes
    assert H + 11 <= lim["parse_halo"]   # (the head and one alignment of a record on the tile's last byte are staged with the tile)
    target = {"last_byte": tile - 1, "head_fits": tile - H, "record_fits": tile - H - 11, "next_tile": tile}[position]
    for n1, n2 in ((a, b) for s in range(2 * H + 2) for a in range(s + 1) for b in (s - a,)):
        rest = target - n1 * (H + 11) - n2 * (H + 22)
        if rest >= 0 and rest % H == 0:
            break
    else:
        raise AssertionError((H, target))
    n0 = rest // H
    special_bc = 0x0807060504030201 & ((1 << (8 * bc_bytes)) - 1)
    pool, obs, cor = _pool(bc_bytes)
    obs, cor = np.append(obs, np.uint64(special_bc)), np.append(cor, np.uint64(special_bc ^ 0x80))
    keep = obs != np.uint64(special_bc)
    keep[-1] = True   # (a pool barcode that happens to equal the special one leaves the map: one correction per observed barcode)
    obs, cor = obs[keep], cor[keep]
    rl = [0x05000000, 9]
    pad = [(int(pool[i % len(pool)]), []) for i in range(n0)]
    step = max(n0 // (n1 + n2 + 1), 1)
    for j in range(n1 + n2):   # spread the longer pads over the tile
        at = min(step * (j + 1), len(pad))
        pad.insert(at, (int(pool[j % len(pool)]), [(1, 4, j % 9, 30 + j)] * (1 if j < n1 else 2)))
    chunk = pad + [(special_bc, [(0, 4, 0x04030201, 65535)])]
    case = _case_of_chunks([[(int(pool[0]), [(1, 4, 3, 44)])], chunk], obs, cor, rl, bc_bytes)
    case["target"] = target
    return case


def _records_tiling(total, H, rng, pool, rl):
    """python-level records (na in 0, 1, 2) whose lengths sum to exactly `total` bytes"""
    nas, left = [], total
    while left > 40 * H:
        nas.append(int(rng.choice([0, 1, 1, 1, 2])))
        left -= H + 11 * nas[-1]
    tail = next((n0, n1, n2) for n2 in range(40) for n1 in range(40) for n0 in range(41) if n0 * H + n1 * (H + 11) + n2 * (H + 22) == left)
    nas += [0] * tail[0] + [2] * tail[2] + [1] * tail[1]
    assert sum(H + 11 * na for na in nas) == total
    return [(int(pool[rng.integers(0, len(pool))]), [(0, 4, int(rng.integers(0, rl[0])), int(rng.integers(20, 2500))) for _ in range(na)]) for na in nas]


EDGE_KINDS = ("tile", "tile_minus_1", "tile_plus_1", "two_tiles")


def exact_edge_case(lim, kind, bc_bytes=4):
    """Chunk 1 of two has nbytes - 8 == parse_tile, parse_tile - 1, parse_tile + 1 or 2 * parse_tile; for the whole multiples a record
    boundary lies on every tile edge, so the walk ends with q == parse_tile and p + q == nbytes."""
    tile, H = lim["parse_tile"], 4 + bc_bytes
    pool, obs, cor = _pool(bc_bytes)
    rng = np.random.default_rng(len(kind))
    rl = [1 << (lim["bin_shift"] + 1)]
    parts = {"tile": [tile], "tile_minus_1": [tile - 1], "tile_plus_1": [tile + 1], "two_tiles": [tile, tile]}[kind]
    chunk = [r for t in parts for r in _records_tiling(t, H, rng, pool, rl)]
    case = _case_of_chunks([[(int(pool[1]), [(0, 4, 5, 60)]), (int(pool[2]), [])], chunk], obs, cor, rl, bc_bytes)
    case["body"] = sum(parts)
    return case


def edge_refusals(case):
    """The malformed variants of chunk 1 of an exact-edge case that the walk is written to refuse: {name: bytes}.  nrec one more,
    nrec one fewer, and the na of the chunk's last record pointing past the chunk's end."""
    data, o1 = case["data"], int(case["off"][1])
    nrec = int.from_bytes(data[o1 + 4:o1 + 8], "little")
    H = 4 + case["bc_bytes"]
    last = case["chunks"][1][-1]
    at_last = len(data) - (H + 11 * len(last[1]))

    def patched(at, value):
        b = bytearray(data)
        b[at:at + 4] = int(value).to_bytes(4, "little")
        return bytes(b)

    assert int.from_bytes(data[at_last:at_last + 4], "little") == len(last[1])
    return {"nrec one more": patched(o1 + 4, nrec + 1), "nrec one fewer": patched(o1 + 4, nrec - 1),
            "the last na past the end": patched(at_last, len(last[1]) + 1)}


# -------------------------------------------------------------------------------------------------- the correction table
def table_slots(keys, n_corr, slot_fn):
    """WITNESS.  Linear probing as k_sort_table_insert does it, for the keys in the given order (the set of taken slots does not
    depend on the order): {key: (home, slot)} and the capacity.  The all-ones barcode is not in the table (the host carries it)."""
    taken, where, cap = set(), {}, slot_fn(0, n_corr)[1]
    for k in keys:
        k = int(k)
        if k in where or k == (1 << 64) - 1:
            continue
        home = slot_fn(k, n_corr)[0]
        s = home
        while s in taken:
            s = (s + 1) & (cap - 1)
        taken.add(s)
        where[k] = (home, s)
    return where, cap


def _with_home(slot_fn, n_corr, homes, n, start):
    """the first n integers from `start` up whose home slot is one of `homes`, and where the scan stopped"""
    out, x = [], start
    while len(out) < n:
        if slot_fn(x, n_corr)[0] in homes:
            out.append(x)
        x += 1
    return out, x


_chain_memo = {}


def chain_case(lim, n_corr, slot_fn, n_chain=300, n_wrap=40, n_absent=20):
    """A correction map of n_corr pairs over 8-byte barcodes: 1 << 63, up to n_chain observed barcodes with ONE home slot, up to n_wrap
    whose home slots are the table's last three (their chain wraps to slot 0), and random ones.  n_corr a power of two: n_corr
    distinct observed barcodes, every one of them a key of the table, whose load is then EXACTLY one half (capacity == 2 n_corr).
    Any other n_corr: the all-ones barcode (which the host carries, not the table) is one of them and a few pairs are there a second
    time.  Every observed barcode maps to a corrected barcode of its own (a neighbour's rank would change the row).  The records
    carry every observed barcode, and n_absent barcodes that share the crowded home slot but are not in the map."""
    if n_corr in _chain_memo:
        return _chain_memo[n_corr]
    cap = slot_fn(0, n_corr)[1]
    plain = n_corr & (n_corr - 1) == 0
    n_dup = 0 if plain else max(1, n_corr // 200)
    n_own = n_corr - n_dup
    specials = [1 << 63] if plain else [(1 << 64) - 1, 1 << 63][:n_own]
    crowded_home = slot_fn(12345, n_corr)[0]
    n_chain = min(n_chain, max(n_own - len(specials), 0) * 3 // 4 if n_own < 400 else n_chain)
    found, nxt = _with_home(slot_fn, n_corr, {crowded_home}, n_chain + n_absent, 1 << 40)
    chain, absent = found[:n_chain], found[n_chain:]
    n_wrap = min(n_wrap, max(n_own - len(specials) - n_chain, 0))
    wrap, _ = _with_home(slot_fn, n_corr, {cap - 1, cap - 2, cap - 3}, n_wrap, 1 << 41)
    rng = np.random.default_rng(n_corr)
    used = set(specials + chain + wrap + absent)
    rnd = [int(x) for x in distinct(rng, n_own + 8, 63) if int(x) not in used][: n_own - len(specials) - n_chain - n_wrap]
    obs = np.asarray(specials + chain + wrap + rnd, np.uint64)
    assert len(obs) == n_own and len(set(obs.tolist())) == n_own
    cor = distinct(rng, n_own, 64)
    if n_dup:
        again = np.minimum(np.arange(n_dup) * 3 + 2, n_own - 1)   # (chain members where there are any)
        obs, cor = np.append(obs, obs[again]), np.append(cor, cor[again])
    p = rng.permutation(n_corr)
    obs, cor = obs[p], cor[p]
    bc = np.concatenate((obs, np.asarray(absent, np.uint64), obs[: len(obs) // 2]))
    n = len(bc)
    B = 1 << lim["bin_shift"]
    case = _case_of_columns(bc, np.zeros(n, np.uint32), rng.integers(0, 2 * B, size=n), rng.integers(20, 60, size=n), obs, cor, [2 * B], 8,
                            per_chunk=700, shuffle_seed=n_corr)
    case.update(chain=chain, wrap=wrap, absent=absent, rnd=rnd, crowded_home=crowded_home, cap=cap, n_dup=n_dup, plain=plain)
    _chain_memo[n_corr] = case
    return case


# ---------------------------------------------------------------------------------------------- witness: the level model
def level_model(case, lim):
    """WITNESS ONLY - never the judge of a result.  DESIGN 3.4b's levelling rule restated in numpy on the kept records of a case:
    bin = first bin of the reference + (start >> bin_shift), key = start_low << 47 | frag_len << 31 | rank of the corrected barcode;
    a bin above repartition_above is a segment; per level, every segment's AND and OR are taken in one launch, an all-equal segment
    is a one-run leaf where it lies, the others are split in one launch by the 8 bits that end at their highest differing bit
    (from bit 0 if that is below bit 7), into the OTHER buffer; parts above repartition_above are the next level's segments.
    Returns {"bits": launches of the AND/OR kernel, "parts": partition launches above level 0, "leaves": {(level, buffer)} -
    level 0 = a position bin, level k = a part of the k-th split, a one-run leaf has the level of the segment it is; buffer 0 / 1 =
    first / second key buffer - "shifts": the shifts used, "mixed": a level had both one-run and splitting segments,
    "repartitioned": bins above the threshold}."""
    S, above = lim["bin_shift"], lim["repartition_above"]
    bc, ref, start, fl = (np.asarray(x) for x in case["cols"])
    obs, cor = case["obs"], case["cor"]
    o = np.argsort(obs)
    i = np.minimum(np.searchsorted(obs[o], bc.astype(np.uint64)), len(obs) - 1)
    hit = obs[o][i] == bc
    rank = np.searchsorted(np.unique(cor), cor[o][i][hit]).astype(np.uint64)
    ref, start, fl = ref[hit].astype(np.int64), start[hit].astype(np.uint64), fl[hit].astype(np.uint64)
    nbins = (case["ref_lengths"].astype(np.int64) + (1 << S) - 1) >> S
    base = np.concatenate(([0], np.cumsum(nbins)))[:-1]
    bins = base[ref] + (start >> np.uint64(S)).astype(np.int64)
    key = ((start & np.uint64((1 << S) - 1)) << np.uint64(47)) | (fl << np.uint64(31)) | rank
    order = np.argsort(bins, kind="stable")
    bins, key = bins[order], key[order]
    cuts = np.flatnonzero(np.diff(bins)) + 1
    segs, leaves = [], set()
    for seg in np.split(key, cuts):
        if len(seg) > above:
            segs.append(seg)
        else:
            leaves.add((0, 0))
    out = {"bits": 0, "parts": 0, "leaves": leaves, "shifts": [], "mixed": False, "repartitioned": len(segs)}
    level = 0   # (the segments of level k lie in buffer k & 1: every split writes to the other one)
    while segs:
        out["bits"] += 1
        split = []
        for seg in segs:
            diff = int(np.bitwise_and.reduce(seg)) ^ int(np.bitwise_or.reduce(seg))
            if not diff:
                leaves.add((level, level & 1))   # (a one-run leaf stays where it lies)
            else:
                split.append((seg, max(diff.bit_length() - 1 - 7, 0)))
        out["mixed"] |= bool(split) and len(split) < len(segs)
        segs = []
        if not split:
            break
        out["parts"] += 1
        level += 1
        for seg, shift in split:
            out["shifts"].append(shift)
            d = (seg >> np.uint64(shift)) & np.uint64(255)
            for v in np.unique(d):
                part = seg[d == v]
                if len(part) > above:
                    segs.append(part)
                else:
                    leaves.add((level, level & 1))
    return out


# ------------------------------------------------------------------------------------------------------------ level cases
def deep_case(lim, extra_bins=30, seed=1):
    """One reference, three oversize bins: (a) 8 key values, each repartition_above + 1 + (a few) times, that differ from a base in
    exactly one of start-low bit 16 / 8 / 0, frag_len bit 8 / 0, rank bit 15 / 7 - every level peels one value off, seven
    splitting levels and a last one of one-run leaves; (b) 4 * leaf_cap keys that differ only in the low 8 bits of the rank
    (shift == 0); (c) 3 * leaf_cap identical keys.  Between them a bin of leaf_cap - 1 distinct keys, and 2 000 random fragments over
    all other bins.  The map is the identity on 2^15 + 400 barcodes, so the rank of a barcode is the barcode."""
    S, cap, above = lim["bin_shift"], lim["leaf_cap"], lim["repartition_above"]
    assert S >= 17 and cap - 1 <= (1 << S)
    B = 1 << S
    rng = np.random.default_rng(seed)
    n_bc = (1 << 15) + 400
    ident = np.arange(n_bc, dtype=np.uint64)
    s0, f0, r0 = 0x0A1A1, 0x0421, 0x0155   # the base: the flipped bits are 0 in it or 1, both occur
    flips = [(0, 0, 0), (1 << 16, 0, 0), (1 << 8, 0, 0), (1, 0, 0), (0, 1 << 8, 0), (0, 1, 0), (0, 0, 1 << 15), (0, 0, 1 << 7)]
    cols = []
    for ds, df, dr in flips:   # (a), bin 1
        n = above + 1 + int(rng.integers(0, 9))
        cols.append((np.full(n, r0 ^ dr), np.full(n, B + (s0 ^ ds)), np.full(n, f0 ^ df)))
    cols.append((rng.integers(0, 30000, size=cap - 1), 2 * B + rng.permutation(B)[:cap - 1], rng.integers(20, 900, size=cap - 1)))   # distinct starts
    nb = 4 * cap
    cols.append((0x4200 | rng.integers(0, 256, size=nb), np.full(nb, 3 * B + 99), np.full(nb, 777)))   # (b), bin 3
    cols.append((np.full(3 * cap, 21), np.full(3 * cap, 5 * B + 17), np.full(3 * cap, 150)))   # (c), bin 5
    other = np.asarray([0, 1, 3, 4, 5, 6])[rng.integers(0, 6, size=2000)]   # (every bin but the one of leaf_cap - 1 keys, which stays a leaf)
    cols.append((rng.integers(0, n_bc, size=2000), other * B + rng.integers(0, B, size=2000), rng.integers(20, 2500, size=2000)))
    bc, start, fl = (np.concatenate([c[k] for c in cols]) for k in range(3))
    assert len(bc) <= 300000
    return _case_of_columns(bc, np.zeros(len(bc), np.uint32), start, fl, ident, ident, [(7 + extra_bins) * B - 5], 4, shuffle_seed=seed)


def mixed_case(lim):
    """Five oversize bins in bin order: one run | split by start bits | one run | split by frag_len only | one run.  In both
    splitting bins one value alone is above repartition_above, so a second level (of one-run segments) follows: the split segments'
    histogram rows are 0 and 1 while their positions in the level's segment list are 1 and 3."""
    S, above = lim["bin_shift"], lim["repartition_above"]
    B = 1 << S
    rng = np.random.default_rng(2)
    cols = []
    for b in (0, 2, 4):
        n = above + 1 + b
        cols.append((np.full(n, 3 + b), np.full(n, 2 * b * B + 1000 + b), np.full(n, 200 + b)))
    cols.append((np.full(above + 5, 7), np.full(above + 5, 2 * B + 0x111), np.full(above + 5, 300)))
    cols.append((rng.integers(0, 40, size=300), np.full(300, 2 * B + 0x1F111), rng.integers(20, 900, size=300)))
    cols.append((np.full(above + 9, 9), np.full(above + 9, 6 * B + 5), np.full(above + 9, 0x0100)))
    cols.append((np.full(500, 9), np.full(500, 6 * B + 5), np.full(500, 0x0101)))
    bc, start, fl = (np.concatenate([c[k] for c in cols]) for k in range(3))
    ident = np.arange(40, dtype=np.uint64)
    return _case_of_columns(bc, np.zeros(len(bc), np.uint32), start, fl, ident, ident, [9 * B], 4, shuffle_seed=2)


# ------------------------------------------------------------------------------------------------------------- leaf cases
def leaf_class_sizes(lim):
    """2^k - 1, 2^k, 2^k + 1 for k = 6..14, as far as the leaf cap allows"""
    return [n for k in range(6, 15) for n in ((1 << k) - 1, 1 << k, (1 << k) + 1) if n <= min(lim["leaf_cap"], lim["repartition_above"])]


def leaf_class_case(lim, repeated):
    """A bin per size of leaf_class_sizes, an empty bin between two of them.  repeated = False: that many distinct keys.
    repeated = True: that many RECORDS, the keys present 1, 2, 3, 1, 2, 3, ... times (the last one as often as is left)."""
    S = lim["bin_shift"]
    B = 1 << S
    sizes = leaf_class_sizes(lim)
    rng = np.random.default_rng(40 + repeated)
    starts, reps = [], []
    for i, n in enumerate(sizes):
        if repeated:
            m = np.tile([1, 2, 3], n // 6 + 1)
            m = m[: np.searchsorted(np.cumsum(m), n) + 1].copy()
            m[-1] -= m.sum() - n
        else:
            m = np.ones(n, np.int64)
        assert m.sum() == n and m.min() >= 1
        starts.append(2 * i * B + rng.permutation(B)[: len(m)])
        reps.append(m)
    start, reps = np.concatenate(starts), np.concatenate(reps)
    fl, bc = rng.integers(20, 900, size=len(start)), rng.integers(0, 30, size=len(start))
    ident = np.arange(30, dtype=np.uint64)
    return _case_of_columns(np.repeat(bc, reps), np.zeros(reps.sum(), np.uint32), np.repeat(start, reps), np.repeat(fl, reps), ident, ident,
                            [2 * len(sizes) * B], 4, shuffle_seed=41)


def run_heads(lim):
    """numbers of distinct keys of a leaf: one below, at and one above each leaf workgroup's thread count (255 ... 1 025)"""
    return sorted({nt + d for nt in (lim["small_leaf_threads"], lim["leaf_threads"]) for d in (-1, 0, 1)})


def run_lengths(nh, total, at, straddle):
    """nh run lengths that sum to `total`, the first and the last 1; straddle = False: a run BEGINS at sorted position `at`;
    True: a run of three begins at `at - 1` and ends at `at + 1`."""
    first = at - 1 if straddle else at          # sorted position at which the special run begins
    special = 3 if straddle else 2
    t = min(nh - 3, first)                      # index of the special run: t runs (the first of length 1) cover [0, first)
    assert t >= 2 and first - 1 >= t - 1
    L = [1] + [(first - 1) // (t - 1) + (1 if j < (first - 1) % (t - 1) else 0) for j in range(t - 1)] + [special]
    rest_runs = nh - len(L) - 1                 # runs between the special one and the last (of length 1)
    rest = total - sum(L) - 1
    assert rest_runs >= 1 and rest >= rest_runs
    L += [rest // rest_runs + (1 if j < rest % rest_runs else 0) for j in range(rest_runs)] + [1]
    assert len(L) == nh and sum(L) == total and L[0] == 1 and L[-1] == 1 and min(L) >= 1
    assert sum(L[:t]) == first and L[t] == special
    return L


def run_head_leaves(lim):
    """[(records, nh, slice, straddle, run lengths)] of the run-head case's bins: for both leaf classes (records at most small_leaf,
    and above), nh in run_heads(lim), a run that begins at the class's slice width and one that straddles it."""
    out = []
    for small in (True, False):
        at = lim["small_leaf_threads"] if small else lim["leaf_threads"]
        for nh in run_heads(lim):
            for straddle in (False, True):
                total = min(lim["small_leaf"], nh + at + 200) if small else lim["small_leaf"] + 1 + nh
                assert (total <= lim["small_leaf"]) == small and total <= min(lim["leaf_cap"], lim["repartition_above"])
                out.append((total, nh, at, straddle, run_lengths(nh, total, at, straddle)))
    return out


def run_head_case(lim):
    S = lim["bin_shift"]
    B = 1 << S
    leaves = run_head_leaves(lim)
    rng = np.random.default_rng(50)
    start, fl, bc = [], [], []
    for i, (total, nh, at, straddle, L) in enumerate(leaves):
        L = np.asarray(L)
        base = i * B + int(rng.integers(0, B - nh))
        # ascending keys in run order: (start, frag_len, barcode) ascend lexicographically with the run index
        start.append(np.repeat(base + np.arange(nh) // 3, L))
        fl.append(np.repeat(100 + np.arange(nh) % 3, L))
        bc.append(np.repeat(np.full(nh, 5), L))
    ident = np.arange(8, dtype=np.uint64)
    n = sum(len(x) for x in start)
    return _case_of_columns(np.concatenate(bc), np.zeros(n, np.uint32), np.concatenate(start), np.concatenate(fl), ident, ident, [len(leaves) * B], 1,
                            shuffle_seed=51)


# -------------------------------------------------------------------------------------------------------------- emit cases
def emit_cases(lim):
    """{name: case}: references without a bin first, last and several in a row; ref_count == 1 with starts up to 2^32 - 2; a
    reference that ends on a bin edge, with a fragment on its last base and one on base 0 of the next."""
    S = lim["bin_shift"]
    B = 1 << S
    out = {}
    rl = [0, 0, 5, 0, 0, B, 0, B + 1, 0]
    recs = [(b, [(r, 4, s, 40 + r)]) for r in (2, 5, 7) for s in (0, rl[r] - 1) for b in (1, 2)] + [(1, [(7, 4, B - 1, 47)]), (1, [(7, 4, 0, 47)])]
    out["zero_length_references"] = _case_of_chunks([recs[::-1]], [1, 2], [2, 1], rl, 2)
    starts = [0, B - 1, B, (1 << 31) - 1, 1 << 31, (1 << 32) - 2]
    recs = [(b, [(0, 4, s, 60)]) for s in starts for b in (6, 4)] + [(4, [(0, 4, s, 60)]) for s in starts[::2]] + [(6, [(0, 4, (1 << 32) - 2, 61)])]
    rng = np.random.default_rng(60)
    recs = [recs[i] for i in rng.permutation(len(recs))]
    out["one_reference_of_2^32-1"] = _case_of_chunks([recs[:7], recs[7:]], [4, 6], [4, 6], [(1 << 32) - 1], 1)
    rl = [3, 2 * B, 9, 0, B]
    recs = [(1, [(1, 4, 2 * B - 1, 50)]), (1, [(2, 4, 0, 50)]), (1, [(1, 4, 2 * B - 1, 50)]), (1, [(4, 4, B - 1, 50)]), (1, [(4, 4, 0, 50)]), (1, [(0, 4, 2, 50)])]
    out["reference_ends_on_a_bin_edge"] = _case_of_chunks([recs], [1], [1], rl, 4)
    return out


# ----------------------------------------------------------------------------------------------------------- context cases
def eleven_record_case():
    recs = [(b, [(r, 4, s, f)]) for b, r, s, f in ((1, 0, 5, 30), (2, 2, 0, 30), (1, 1, 8, 2000), (1, 0, 5, 30), (3, 1, 8, 31), (2, 0, 99, 30), (1, 2, 6, 30))]
    recs += [(1, []), (2, [(0, 4, 1, 30), (1, 4, 1, 30)]), (9, [(0, 4, 1, 30)]), (2, [(1, 4, 0, 65535)])]
    return _case_of_chunks([recs[:4], recs[4:]], [1, 2, 3], [3, 3, 1], [100, 9, 7], 4)


def many_references_case(n_ref=70000):
    """the reference ids above 65 535 of tests/test_gpu_atac_sort.py::test_reference_ids_above_65535"""
    rng = np.random.default_rng(8)
    ref = np.concatenate((rng.integers(0, n_ref, size=5000), [65535, 65536, 65536, n_ref - 1, 0])).astype(np.uint32)
    n = len(ref)
    start, fl, bc = rng.integers(0, 100, size=n), rng.integers(30, 33, size=n), rng.integers(0, 4, size=n).astype(np.uint64)
    return _case_of_columns(bc, ref, start, fl, [0, 1, 2, 3], [3, 2, 1, 0], np.full(n_ref, 100, np.uint32), 2, per_chunk=700)
