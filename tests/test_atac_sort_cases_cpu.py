"""The builders of tests/atac_sort_cases.py without a device: each input reaches the edge it names.  The witnesses are a few lines
that walk the na chain as k_sort_parse tiles it (atac_sort_cases.tile_walk), the level model of DESIGN 3.4b and linear probing over
afq_atac_sort_table_slot; every size comes from atac_sort_limits().  tests/test_gpu_atac_sort_edges.py re-asserts the cheap ones."""
import numpy as np
import pytest

import atac_sort_cases as A
from util import pkg


@pytest.fixture(scope="module")
def lim():
    return pkg.atac_sort_limits()


WIDTHS = [1, 2, 4, 8]


def test_table_capacity_is_the_smallest_power_of_two_at_least_twice_the_entries():
    for n in list(range(0, 70)) + [1023, 1024, 1025, 5000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 30) - 1]:
        home, cap = pkg.atac_sort_table_slot(0x0123456789ABCDEF, n)
        want = 2
        while want < max(2, 2 * n):
            want *= 2
        assert cap == want and 0 <= home < cap, (n, cap, home)
    # the home slot of a barcode in a larger table extends its home slot in a smaller one (one hash, masked by the capacity)
    for bc in (0, 1, (1 << 64) - 1, 1 << 63, 0xDEADBEEF):
        assert pkg.atac_sort_table_slot(bc, 1 << 20)[0] & 2047 == pkg.atac_sort_table_slot(bc, 1024)[0]
    assert len({pkg.atac_sort_table_slot(b, 1024)[0] for b in range(4000)}) > 1500   # (it spreads)


@pytest.mark.parametrize("bc_bytes", WIDTHS)
def test_tile_full_case_fills_a_tile_with_record_starts(lim, bc_bytes):
    tile, H = lim["parse_tile"], 4 + bc_bytes
    c = A.tile_full_case(lim, bc_bytes)
    n = 3 * (tile // H) + 7
    assert c["counts"][0] == 2 * n and c["counts"][1] > n and c["counts"][2] == 0
    tiles, end = A.tile_walk(c["data"], c["off"][0], bc_bytes, lim)
    assert end == 8 + n * H and len(tiles) >= 3
    first = tiles[0][1]
    assert len(first) == -(-tile // H) and all(na == 0 for _, na in first)
    if H == 5:
        assert len(first) == tile // 5 + 1 and first[-1][0] == tile - 1
    # the second chunk: its kept records are the 64th and 65th of every 64 records - last lane of a trip, first lane of the next
    kept = [i for i, (_, a) in enumerate(c["chunks"][1]) if len(a) == 1]
    assert kept[:4] == [63, 64, 127, 128] and len(kept) == 2 * ((n - 1) // 64) + ((n - 1) % 64 == 63)
    t1 = A.tile_walk(c["data"], c["off"][1], bc_bytes, lim)[0][0][1]
    assert len(t1) > 128 and [i for i, (_, na) in enumerate(t1) if na == 1][:4] == [63, 64, 127, 128]


@pytest.mark.parametrize("bc_bytes", WIDTHS)
def test_long_record_case_has_records_beyond_tile_and_halo(lim, bc_bytes):
    tile, H = lim["parse_tile"], 4 + bc_bytes
    nas = A.long_record_nas(lim)
    assert 8 + 11 * nas[2] <= tile + lim["parse_halo"] < 8 + 11 * nas[3] and nas[1] + 2 == nas[3] and nas[0] == 2 and max(nas) == 5000
    c = A.long_records_case(lim, bc_bytes)
    seen = set()
    for ci, chunk in enumerate(c["chunks"]):
        tiles, end = A.tile_walk(c["data"], c["off"][ci], bc_bytes, lim)
        assert end == int.from_bytes(c["data"][int(c["off"][ci]):int(c["off"][ci]) + 4], "little")
        for p, recs in tiles:
            seen |= {na for _, na in recs}
            q, na = recs[-1]
            if H + 11 * na > tile + lim["parse_halo"]:   # the next tile begins beyond everything this one staged
                assert q + H + 11 * na > tile + lim["parse_halo"]
    assert set(nas) <= seen and sum(H + 11 * na > tile + lim["parse_halo"] for na in nas) >= 3 and sum(tile < H + 11 * na <= tile + lim["parse_halo"] for na in nas) >= 2
    assert [len(a) for _, a in c["chunks"][1]] == [5000] and len(c["chunks"][2][-1][1]) == nas[3] and len(c["chunks"][3][0][1]) == nas[2]
    assert c["counts"][2] == len(nas) + 4 and len(c["cols"][0]) > 15


@pytest.mark.parametrize("bc_bytes", WIDTHS)
@pytest.mark.parametrize("position", A.HALO_POSITIONS)
def test_halo_case_puts_its_record_where_it_says(lim, bc_bytes, position):
    tile, H = lim["parse_tile"], 4 + bc_bytes
    c = A.halo_case(lim, bc_bytes, position)
    want_q = {"last_byte": tile - 1, "head_fits": tile - H, "record_fits": tile - H - 11, "next_tile": tile}[position]
    assert c["target"] == want_q
    tiles, end = A.tile_walk(c["data"], c["off"][1], bc_bytes, lim)
    assert end == 8 + want_q + H + 11 and len(c["data"]) == int(c["off"][1]) + end      # the record ends the chunk and the buffer
    if position == "next_tile":
        assert len(tiles) == 2 and tiles[1] == (8 + tile, [(0, 1)])
    else:
        assert len(tiles) == 1 and tiles[0][1][-1] == (want_q, 1)
    if position == "record_fits":
        assert want_q + H + 11 == tile
    bc, ref, start, fl = c["cols"]
    assert (ref[-1], start[-1], fl[-1]) == (0, 0x04030201, 65535) and len(set(int(start[-1]).to_bytes(4, "little"))) == 4
    assert len(set(int(bc[-1]).to_bytes(bc_bytes, "little"))) == bc_bytes
    w = A.want_of(c)
    assert w["frag_len"].max() == 65535 and w["n_kept"] >= 2


@pytest.mark.parametrize("kind", A.EDGE_KINDS)
def test_exact_edge_chunk_is_a_whole_number_of_tile_advances(lim, kind):
    tile = lim["parse_tile"]
    c = A.exact_edge_case(lim, kind)
    o1 = int(c["off"][1])
    nb = int.from_bytes(c["data"][o1:o1 + 4], "little")
    assert nb - 8 == c["body"] == {"tile": tile, "tile_minus_1": tile - 1, "tile_plus_1": tile + 1, "two_tiles": 2 * tile}[kind]
    tiles, end = A.tile_walk(c["data"], o1, c["bc_bytes"], lim)
    assert end == nb
    if kind in ("tile", "two_tiles"):   # every advance is exactly one tile: q == parse_tile and, at the end, p + q == nbytes
        assert [p for p, _ in tiles] == [8 + tile * i for i in range(c["body"] // tile)]
    if kind in ("tile_minus_1", "tile_plus_1"):   # ONE tile: its last record starts below parse_tile and ends one byte before / behind the tile's end
        q, na = tiles[0][1][-1]
        assert len(tiles) == 1 and q < tile and q + 4 + c["bc_bytes"] + 11 * na == c["body"]
    assert {na for _, recs in tiles for _, na in recs} == {0, 1, 2}
    bad = A.edge_refusals(c)
    assert len(bad) == 3 and all(len(b) == len(c["data"]) and b != c["data"] for b in bad.values())
    if kind == "two_tiles":   # the last record, whose na the third variant patches, lies in the second tile
        assert len(tiles) == 2 and len(tiles[1][1]) > 10


@pytest.mark.parametrize("n_corr", [1, 2, 3, 4, 1024, 1025])
def test_chain_case_has_its_chains_and_wraps(lim, n_corr):
    slot = pkg.atac_sort_table_slot
    c = A.chain_case(lim, n_corr, slot)
    assert len(c["obs"]) == len(c["cor"]) == n_corr and c["cap"] == slot(0, n_corr)[1]
    pairs = set(zip(c["obs"].tolist(), c["cor"].tolist()))
    plain = n_corr & (n_corr - 1) == 0
    assert c["plain"] == plain and c["n_dup"] == (0 if plain else max(1, n_corr // 200))
    assert len(pairs) == len(set(c["obs"].tolist())) == n_corr - c["n_dup"]   # the same pair twice, never two corrections
    assert ((1 << 64) - 1 in c["obs"].tolist()) == (not plain) and 1 << 63 in c["obs"].tolist()
    where, cap = A.table_slots(c["obs"], n_corr, slot)
    if plain:   # n_corr distinct keys, all of them in the table: a load of exactly one half; n_corr + 1 entries take the next capacity
        assert len(where) == n_corr and 2 * len(where) == cap and slot(0, n_corr + 1)[1] == (2 * cap if n_corr > 1 else 4)
    else:
        assert len(where) == n_corr - c["n_dup"] - 1 and 2 * len(where) < cap
    assert all(slot(k, n_corr)[0] == c["crowded_home"] for k in c["chain"] + c["absent"]) and len(c["absent"]) == 20
    assert not set(c["absent"]) & set(c["obs"].tolist())
    if n_corr >= 1024:
        assert len(c["chain"]) == 300 and len(c["wrap"]) == 40
        d = sorted((where[k][1] - where[k][0]) % cap for k in c["chain"])
        assert d[-1] >= 299                                               # one home slot: the chain's last member lies 299 slots or more from it
        assert all(where[k][0] >= cap - 3 for k in c["wrap"])
        wrapped = [k for k in c["wrap"] if where[k][1] < where[k][0]]
        assert len(wrapped) >= 37, len(wrapped)                           # 40 keys on three home slots: all but three wrap past the last slot
        # an absent barcode's probe walks the whole crowded chain before it meets a free slot
        taken = {s for _, s in where.values()}
        s, steps = c["crowded_home"], 0
        while s in taken:
            s, steps = (s + 1) & (cap - 1), steps + 1
        assert steps >= 300
    w = A.want_of(c)
    assert w["n_uncorrected"] == 20 and w["n_kept"] == n_corr + n_corr // 2 and not set(c["rnd"]) & set(c["chain"] + c["wrap"])


def test_deep_case_reaches_every_level(lim):
    c = A.deep_case(lim)
    m = A.level_model(c, lim)
    assert len(c["cols"][0]) <= 300000
    assert m["repartitioned"] == 3, m
    assert (m["parts"], m["bits"]) == (7, 8), m                       # seven splitting levels and a last one of one-run leaves
    assert 0 in m["shifts"] and 56 in m["shifts"] and len(set(m["shifts"])) >= 7, m
    assert {b for _, b in m["leaves"]} == {0, 1} and {lv for lv, _ in m["leaves"]} >= set(range(0, 8)), m
    assert m["mixed"]
    assert m["bits"] - 1 <= 64 // 8                                    # at the ceiling's side that a key can reach
    shrunk = A.deep_case(lim, extra_bins=0)
    assert shrunk["cols"][2].tolist() == c["cols"][2].tolist() and int(shrunk["ref_lengths"][0]) < int(c["ref_lengths"][0])
    assert A.level_model(shrunk, lim) == m


def test_mixed_case_splits_the_second_and_fourth_of_five_segments(lim):
    c = A.mixed_case(lim)
    m = A.level_model(c, lim)
    assert m["repartitioned"] == 5 and m["mixed"] and (m["bits"], m["parts"]) == (2, 1), m
    assert len(set(m["shifts"])) == 2 and min(m["shifts"]) < 31 + 16 - 7 < 47 <= max(m["shifts"]) + 7, m   # one by frag_len bits only, one by start bits
    S, above = lim["bin_shift"], lim["repartition_above"]
    bins, n = np.unique(np.asarray(c["cols"][2]) >> S, return_counts=True)
    assert bins.tolist() == [0, 2, 4, 6, 8] and (n > above).all()
    per_bin = [len(np.unique(np.stack([np.asarray(x)[(np.asarray(c["cols"][2]) >> S) == b] for x in c["cols"]]), axis=1).T) for b in bins]
    assert [k == 1 for k in per_bin] == [True, False, True, False, True]


def test_leaf_cases_have_the_sizes_they_name(lim):
    sizes = A.leaf_class_sizes(lim)
    assert sizes[:3] == [63, 64, 65] and max(sizes) <= lim["leaf_cap"] and len(sizes) >= 26 and any(s > lim["small_leaf"] for s in sizes) and lim["small_leaf"] + 1 in sizes
    S = lim["bin_shift"]
    for repeated in (False, True):
        c = A.leaf_class_case(lim, repeated)
        bins, n = np.unique(np.asarray(c["cols"][2]) >> S, return_counts=True)
        assert n.tolist() == sizes and (np.diff(bins) == 2).all() and n.max() <= lim["repartition_above"]
        w = A.want_of(c)
        if repeated:
            assert set(np.unique(w["count"]).tolist()) == {1, 2, 3} and len(w["count"]) < len(c["cols"][0]) * 0.6
        else:
            assert (w["count"] == 1).all()
    leaves = A.run_head_leaves(lim)
    assert sorted({(t <= lim["small_leaf"], nh) for t, nh, *_ in leaves}) == sorted((s, nh) for s in (False, True) for nh in A.run_heads(lim))
    for total, nh, at, straddle, L in leaves:
        heads = np.concatenate(([0], np.cumsum(L)))[:-1]
        assert len(L) == nh and sum(L) == total and L[0] == 1 and L[-1] == 1
        assert at == (lim["small_leaf_threads"] if total <= lim["small_leaf"] else lim["leaf_threads"])
        if straddle:
            i = heads.tolist().index(at - 1)
            assert L[i] == 3 and at not in heads
        else:
            assert at in heads
        assert max(L) > 1
    c = A.run_head_case(lim)
    bins, n = np.unique(np.asarray(c["cols"][2]) >> S, return_counts=True)
    assert n.tolist() == [t for t, *_ in leaves]
    w = A.want_of(c)
    pos = 0
    for total, nh, at, straddle, L in leaves:   # the judge sees the runs the builder meant
        assert w["count"][pos:pos + nh].tolist() == L
        pos += nh
    assert pos == len(w["count"])


def test_emit_and_context_cases(lim):
    B = 1 << lim["bin_shift"]
    e = A.emit_cases(lim)
    z = e["zero_length_references"]
    assert z["ref_lengths"].tolist() == [0, 0, 5, 0, 0, B, 0, B + 1, 0]
    w = A.want_of(z)
    assert sorted(set(zip(w["ref"].tolist(), w["start"].tolist()))) == [(2, 0), (2, 4), (5, 0), (5, B - 1), (7, 0), (7, B - 1), (7, B)]
    o = e["one_reference_of_2^32-1"]
    w = A.want_of(o)
    assert o["ref_lengths"].tolist() == [(1 << 32) - 1] and w["start"].max() == (1 << 32) - 2 and (1 << 31) in w["start"].tolist() and w["count"].max() == 2
    assert (w["start"] >> lim["bin_shift"]).max() == 32767 if lim["bin_shift"] == 17 else True
    r = e["reference_ends_on_a_bin_edge"]
    w = A.want_of(r)
    assert int(r["ref_lengths"][1]) % B == 0 and list(zip(w["ref"].tolist(), w["start"].tolist()))[1:3] == [(1, 2 * B - 1), (2, 0)]
    c = A.eleven_record_case()
    assert c["counts"] == (11, 1, 1) and A.want_of(c)["n_uncorrected"] == 1 and len(c["ref_lengths"]) == 3
    assert len(A.many_references_case()["ref_lengths"]) == 70000
