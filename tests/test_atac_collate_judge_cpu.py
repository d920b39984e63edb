"""CPU tests of tests/atac_collate_judge.py and tests/atac_collate_cases.py: the judge on hand-written vectors with the expected bytes
spelled out; every case builder reaches what it claims to reach; and conservation - the judge's output, re-read with rad's decoder,
holds exactly the (corrected barcode, alignment bytes) of the kept input records, which does not go through the judge's layout code."""
from collections import Counter

import pytest

import atac_collate_cases as C
import atac_collate_judge as J
from util import pkg

rad = pkg.rad


@pytest.fixture(scope="module")
def lim():
    return pkg.atac_collate_limits()


def le(v, n):
    return int(v).to_bytes(n, "little")


def aln(ref, ty, start, fl):
    return le(ref, 4) + bytes([ty]) + le(start, 4) + le(fl, 2)


# ------------------------------------------------------------------------------------------------------------- hand-written
def test_hand_written_vector_two_byte_barcodes():
    """two input chunks; cells [0xBBBB, 0xCCCC, 0xAAAA]; 0xAAA1 is corrected onto 0xAAAA, 0xDDDD is not in the map; 0xCCCC's only
    reads are unmapped and multi-mapped, so it has no chunk"""
    a1, a2, a3, a4 = (7, 4, 100, 50), (0x80000001, 1, 0xFFFFFFFF, 0xFFFF), (9, 2, 5, 6), (1, 3, 2, 3)
    chunks = [[(0xAAAA, [a1]), (0xCCCC, []), (0xBBBB, [a2]), (0xDDDD, [a3])], [(0xAAA1, [a3]), (0xCCCC, [a1, a2]), (0xAAAA, [a4])]]
    data, off = rad.encode_atac_chunks(chunks, bc_bytes=2)
    got = J.collate(data, off, 2, {0xAAAA: 0xAAAA, 0xBBBB: 0xBBBB, 0xCCCC: 0xCCCC, 0xAAA1: 0xAAAA}, [0xBBBB, 0xCCCC, 0xAAAA])
    R = 17
    want = (le(8 + R, 4) + le(1, 4) + le(1, 4) + le(0xBBBB, 2) + aln(*a2) +
            le(8 + 3 * R, 4) + le(3, 4) + le(1, 4) + le(0xAAAA, 2) + aln(*a1) + le(1, 4) + le(0xAAAA, 2) + aln(*a3) + le(1, 4) + le(0xAAAA, 2) + aln(*a4))
    assert got["bytes"] == want
    assert got["chunk_off"] == [0, 8 + R, 16 + 4 * R] and got["nrec"] == [1, 3] and got["cell"] == [0, 2]
    assert got["stats"] == dict(n_records=7, n_unmapped=1, n_multimapped=1, n_uncorrected=1, n_kept=4, n_cells_out=2, n_cells_empty=1, out_bytes=16 + 4 * R)


def test_hand_written_vector_nothing_kept_and_nothing_in():
    data, off = rad.encode_atac_chunks([[(1, []), (2, [(0, 4, 1, 2), (0, 4, 3, 4)])], []], bc_bytes=1)
    got = J.collate(data, off, 1, {1: 1, 2: 2}, [2, 1])
    assert got["bytes"] == b"" and got["chunk_off"] == [0] and got["nrec"] == [] and got["cell"] == []
    assert got["stats"] == dict(n_records=2, n_unmapped=1, n_multimapped=1, n_uncorrected=0, n_kept=0, n_cells_out=0, n_cells_empty=2, out_bytes=0)
    got = J.collate(b"", [], 8, {}, [])
    assert got["bytes"] == b"" and got["chunk_off"] == [0] and got["stats"]["n_records"] == 0 and got["stats"]["n_cells_empty"] == 0


def test_hand_written_vector_eight_byte_all_ones():
    a1 = (3, 4, 10, 20)
    data, off = rad.encode_atac_chunks([[(C.ONES, [a1])]], bc_bytes=8)
    got = J.collate(data, off, 8, {C.ONES: 5}, [5])
    assert got["bytes"] == le(8 + 23, 4) + le(1, 4) + le(1, 4) + le(5, 8) + aln(*a1)
    got = J.collate(data, off, 8, {C.ONES: C.ONES}, [4, C.ONES])
    assert got["bytes"] == le(8 + 23, 4) + le(1, 4) + le(1, 4) + b"\xFF" * 8 + aln(*a1) and got["cell"] == [1]


def test_cell_order_is_count_descending_then_barcode_ascending():
    assert J.cell_order({5: 2, 3: 9, 8: 2, 1: 2}) == [3, 1, 5, 8]


# ------------------------------------------------------------------------------------------------------------- conservation
def decode(out, chunk_off, bc_bytes):
    """the judge's output re-read: rad.chunk_offsets walks the chunk headers, the record size cuts the chunks; the barcode and the
    alignment bytes of every record"""
    R = 4 + bc_bytes + 11
    offs = rad.chunk_offsets(out) if len(out) else []
    assert [int(o) for o in offs] == [int(o) for o in chunk_off[:-1]]
    recs = []
    for o in offs:
        o = int(o)
        nbytes, nrec = int.from_bytes(out[o:o + 4], "little"), int.from_bytes(out[o + 4:o + 8], "little")
        assert nbytes == 8 + R * nrec and nrec > 0
        for k in range(nrec):
            p = o + 8 + R * k
            assert out[p:p + 4] == le(1, 4)
            recs.append((int.from_bytes(out[p + 4:p + 4 + bc_bytes], "little"), out[p + 4 + bc_bytes:p + R]))
    return recs


def conserved(c, w):
    got = decode(w["bytes"], w["chunk_off"], c["bc_bytes"])
    assert Counter(got) == Counter(C.kept_input(c)) and len(got) == w["stats"]["n_kept"] == sum(w["nrec"])
    st = w["stats"]
    assert st["n_records"] == st["n_unmapped"] + st["n_multimapped"] + st["n_uncorrected"] + st["n_kept"] == sum(len(r) for r in c["chunks"])
    assert st["n_cells_out"] + st["n_cells_empty"] == len(c["cells"]) and st["out_bytes"] == len(w["bytes"]) == w["chunk_off"][-1]
    # a chunk carries one barcode, its cell's; the chunks follow the order of the cells
    assert w["cell"] == sorted(w["cell"])
    for o, n, ci in zip(w["chunk_off"], w["nrec"], w["cell"]):
        R = 4 + c["bc_bytes"] + 11
        assert all(int.from_bytes(w["bytes"][o + 8 + R * k + 4:o + 8 + R * k + 4 + c["bc_bytes"]], "little") == c["cells"][ci] for k in range(n))
    return w


def nas(c):
    return {len(a) for recs in c["chunks"] for _, a in recs}


# ------------------------------------------------------------------------------------------------------------- the builders
def test_width_cases_reach_every_output_residue():
    starts, ends = set(), set()
    for b in C.WIDTHS:
        c = C.widths_case(b)
        w = conserved(c, C.want(c))
        assert w["stats"]["n_kept"] > 20 and w["stats"]["n_uncorrected"] > 0 and w["stats"]["n_unmapped"] > 0 and w["stats"]["n_multimapped"] > 0
        top = (1 << (8 * b)) - 1
        assert {0, top} <= {r[0] for recs in c["chunks"] for r in recs} and [] in c["chunks"]
        for s, e in C.record_spans(w["bytes"], w["chunk_off"], b):
            assert e - s == 4 + b + 11
            starts.add(s % 4)
            ends.add(e % 4)
    assert starts == {0, 1, 2, 3} and ends == {0, 1, 2, 3}


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_alignment_cases_start_their_chunks_off_a_dword(pad):
    c = C.alignment_case(pad)
    assert int(c["off"][0]) == pad and {int(o) % 4 for o in c["off"]} != {0}
    conserved(c, C.want(c))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_edge_cases_end_a_kept_head_at_the_tile_edge(lim, delta):
    c, q = C.tile_edge_case(lim, delta)
    H = 4 + c["bc_bytes"]
    assert q + H == lim["parse_tile"] + delta
    # a record of the first chunk starts at payload offset q, has one alignment and a barcode of the map
    p, hit = 0, None
    for bc, a in c["chunks"][0]:
        if p == q:
            hit = (bc, len(a))
        p += H + 11 * len(a)
    assert hit == (3, 1) and 3 in c["corrections"] and p > lim["parse_tile"] + lim["parse_halo"]
    conserved(c, C.want(c))


def test_halo_case_puts_a_kept_record_on_the_tiles_last_byte(lim):
    c, q = C.halo_case(lim)
    p, hit = 0, None
    for bc, a in c["chunks"][0]:
        if p == q:
            hit = (bc, len(a))
        p += 12 + 11 * len(a)
    assert q == lim["parse_tile"] - 1 and hit == (C.ONES, 1)
    conserved(c, C.want(c))


@pytest.mark.parametrize("extra", [0, 1])
def test_one_tile_chunk_cases(lim, extra):
    c = C.one_tile_chunk_case(lim, extra)
    assert int(c["off"][1]) - int(c["off"][0]) == 8 + lim["parse_tile"] + extra and c["chunks"][1] == []
    conserved(c, C.want(c))


@pytest.mark.parametrize("tiles", [1, 2])
def test_long_record_cases(lim, tiles):
    c, na = C.long_record_case(lim, tiles)
    assert 11 * na > tiles * lim["parse_tile"] and 11 * (na - 1) <= tiles * lim["parse_tile"]
    i = next(k for k, r in enumerate(c["chunks"][0]) if len(r[1]) == na)
    assert 0 < i and len(c["chunks"][0][i + 1][1]) == 1 and c["chunks"][0][i + 1][0] in c["corrections"]   # a kept record follows
    assert (4 + c["bc_bytes"] + 11) * i % lim["parse_tile"] != 0 and len(c["chunks"][1][0][1]) == na                     # mid-tile; and one at a chunk's start
    w = conserved(c, C.want(c))
    assert w["stats"]["n_multimapped"] == 3


def test_na_case_holds_zero_one_and_two():
    c = C.na_case()
    assert nas(c) == {0, 1, 2}
    w = conserved(c, C.want(c))
    assert (w["stats"]["n_unmapped"], w["stats"]["n_kept"], w["stats"]["n_multimapped"]) == (2, 2, 1)


@pytest.mark.parametrize("n_cells", [1, 255, 256, 257, 65535, 65536, 65537])
def test_many_cells_cases(n_cells):
    c = C.many_cells_case(n_cells)
    w = C.want(c)
    assert w["nrec"] == [1] * n_cells and w["cell"] == list(range(n_cells)) and w["stats"]["n_uncorrected"] == 1
    if n_cells <= 257:
        conserved(c, w)


@pytest.mark.parametrize("which", C.EMPTY)
def test_empty_cell_cases(which):
    c, idle = C.empty_cells_case(which)
    w = conserved(c, C.want(c))
    assert w["cell"] == [i for i in range(9) if i not in idle] and w["stats"]["n_cells_empty"] == len(idle)
    assert w["stats"]["n_unmapped"] == len(idle) and w["stats"]["n_multimapped"] == 2 * len(idle)


def test_barcode_case():
    c = C.barcode_case()
    w = conserved(c, C.want(c))
    corr = c["corrections"]
    assert corr[C.ONES] != C.ONES and C.ONES in corr.values() and C.ONES in c["cells"]
    assert sum(1 for o, t in corr.items() if o == t) >= 2 and sum(1 for t in corr.values() if t == 0x1111111111111111) >= 31
    assert w["stats"]["n_uncorrected"] == 1 and w["cell"] == [0, 1, 2] and w["nrec"][1] == 31


def test_chain_case_has_a_probe_chain_of_the_stated_length():
    c, chain, where = C.chain_case(16, 12, 4)
    homes = {where[b][0] for b in chain}
    cap = pkg.atac_sort_table_slot(0, 16)[1]
    assert len(homes) == 1 and cap == 32
    assert sorted((where[b][1] - where[b][0]) % cap for b in chain) == list(range(12))   # probe distances 0 .. 11
    w = conserved(c, C.want(c))
    assert w["stats"]["n_uncorrected"] == 4 and w["stats"]["n_kept"] == 16 + 12


def test_skew_case(lim):
    c = C.skew_case(lim)
    w = conserved(c, C.want(c))
    assert w["cell"] == [2] and w["nrec"][0] > lim["radix_block"] and w["stats"]["n_cells_empty"] == 4


@pytest.mark.parametrize("kind", ["head_cut", "alns_cut", "junk", "nrec_low", "nrec_high"])
def test_malformed_cases_break_chunk_two_only(kind):
    data, off = C.malformed_case(kind)
    with pytest.raises(AssertionError) as e:
        J.collate(data, off, 4, {1: 1}, [1])
    assert e.value.args[0][:2] == ("chunk", 2)
    assert J.collate(data, off[:2], 4, {1: 1}, [1])["stats"]["n_records"] == 3
