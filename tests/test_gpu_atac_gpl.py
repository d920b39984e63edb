"""GPU tests of the `atac generate-permit-list` record pass (afq_atac_gpl_hist_rad, csrc/afq_atac_gpl.hip): the chunks of an uncollated
scATAC RAD in; the count of every observed barcode over ALL records, the largest na, and the position-bin histogram of the records
with one alignment out.  Every expected value is tests/atac_gpl_judge.py on the python-level records (exact integer equality, array
for array); the shapes come from atac_gpl_limits() and gpl_table_slot(), not from copied constants."""
import numpy as np
import pytest

import atac_gpl_cases as G
import atac_gpl_judge as J
from util import pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
BAD_INPUT, INVALID_ARG = pkg._abi.AFQ_ERR_BAD_INPUT, pkg._abi.AFQ_ERR_INVALID_ARG
A = lambda ref, start: (ref, 4, start, 50)


@pytest.fixture(scope="module")
def q():
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    qq = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    yield qq
    qq.close()


@pytest.fixture(scope="module")
def lim():
    L = pkg.atac_gpl_limits()
    assert L["parse_tile"] >= 64 and L["parse_halo"] >= 4 + 8 + 9
    return L


def run(q, chunks, blens, bc_bytes=4, bin_size=J.SIZE_RANGE, al=0):
    data, off = rad.encode_atac_chunks(chunks, bc_bytes=bc_bytes)
    return q.atac_gpl_hist_rad(b"\xEE" * al + data, off + np.uint64(al), blens, bc_bytes=bc_bytes, bin_size=bin_size)


def refused(q, code, sentence, *a, **kw):
    with pytest.raises(pkg.AfqError) as e:
        q.atac_gpl_hist_rad(*a, **kw)
    assert e.value.code == code and sentence in str(e.value), (e.value.code, str(e.value))


# ------------------------------------------------------------------------------------------------------------------ the walk
@pytest.mark.parametrize("bc_bytes", [1, 2, 4, 8])
def test_every_width_alignment_na_and_chunk_shape(q, lim, bc_bytes):
    """na = 0, 1, 2 and 400 (longer than tile + halo) all count their barcode, only na == 1 is binned, max_ambig is 400; a header-only
    chunk, an na == 0 record and the long record as the last of a chunk; at each of the four byte alignments of the chunk starts"""
    rl = [250001, 900, 99993]
    chunks = G.mixed_chunks(lim, bc_bytes, rl)
    blens = G.blens_of(rl)
    want = G.want_of(chunks, blens)
    s = want["stats"]
    assert s["max_ambig"] == 400 and s["n_unmapped"] > 100 and s["n_multimapped"] > 100 and s["n_binned"] > 300 and any(len(c) == 0 for c in chunks)
    assert any(len(c[-1][1]) == 0 for c in chunks if c) and any(len(c[-1][1]) == 400 for c in chunks if c)
    for al in range(4):
        G.same(run(q, chunks, blens, bc_bytes, al=al), want, f"alignment {al}")


@pytest.mark.parametrize("bc_bytes", [1, 8])
def test_records_at_the_tile_edges_and_in_the_halo(q, lim, bc_bytes):
    for name, (chunks, rl) in G.walk_cases(lim, bc_bytes).items():
        blens = G.blens_of(rl)
        G.same(run(q, chunks, blens, bc_bytes), G.want_of(chunks, blens), name)
    # the witness: in the `last_byte` case the last record does start on the tile's last byte
    import atac_sort_cases as S
    c = S.halo_case(G.sort_lim(lim), bc_bytes, "last_byte")
    tiles, end = S.tile_walk(c["data"], c["off"][1], bc_bytes, G.sort_lim(lim))
    assert tiles[0][1][-1] == (lim["parse_tile"] - 1, 1) and len(tiles) == 1


def test_long_records_between_short_ones(q, lim):
    import atac_sort_cases as S
    c = S.long_records_case(G.sort_lim(lim), 4)
    blens = G.blens_of(c["ref_lengths"])
    want = G.want_of(c["chunks"], blens)
    assert want["stats"]["max_ambig"] == 5000
    G.same(run(q, c["chunks"], blens), want)


def test_nothing_in_nothing_out(q):
    bc, count, bins, st = q.atac_gpl_hist_rad(b"", np.zeros(0, np.uint64), [0, 3])
    assert len(bc) == 0 and len(count) == 0 and bins.tolist() == [0, 0, 0] and st == dict(n_records=0, n_unmapped=0, n_multimapped=0, n_binned=0, max_ambig=0, max_bin=0)
    chunks = [[], [(5, [])], []]
    G.same(run(q, chunks, [0, 3]), G.want_of(chunks, [0, 3]))
    # no reference, no bin: records without an alignment are still counted
    bc, count, bins, st = run(q, [[(5, []), (5, [A(0, 1)] * 2)]], [0])
    assert bc.tolist() == [5] and count.tolist() == [2] and len(bins) == 0 and st["max_bin"] == 0 and st["max_ambig"] == 2


def test_70000_records_of_one_barcode_in_one_bin(q):
    import atac_sort_cases as S
    n = 70000
    data, off = S.na1_chunks(np.full(n, 77), np.zeros(n, np.uint32), np.full(n, 123456), np.full(n, 40), 9000, bc_bytes=2)
    bc, count, bins, st = q.atac_gpl_hist_rad(data, off, [0, 3], bc_bytes=2)
    assert bc.tolist() == [77] and count.tolist() == [n] and bins.tolist() == [0, n, 0] and st["max_bin"] == n and st["n_binned"] == n and st["max_ambig"] == 1


# ------------------------------------------------------------------------------------------------------------------ the table
def test_the_all_ones_barcode_and_the_top_bit(q):
    ones = G.ONES
    chunks = [[(ones, [A(0, 5)]), (1 << 63, []), (ones, []), (ones - 1, [A(0, 5)] * 2), (0, [A(0, 100000)])], [(ones, [A(0, 5)])]]
    got = run(q, chunks, [0, 2], bc_bytes=8)
    G.same(got, G.want_of(chunks, [0, 2]))
    assert got[0].tolist() == [0, 1 << 63, ones - 1, ones] and got[1].tolist() == [1, 1, 1, 3]
    # all-ones of the narrower widths are ordinary keys of the table
    for w in (1, 2, 4):
        m = (1 << (8 * w)) - 1
        chunks = [[(m, []), (m, [A(0, 5)]), (m - 1, [])]]
        G.same(run(q, chunks, [0, 2], bc_bytes=w), G.want_of(chunks, [0, 2]), f"width {w}")


def test_probe_chains_and_a_wrap_around_the_tables_end(q):
    chunks, info = G.chain_chunks()
    n = sum(len(c) for c in chunks)
    assert n == info["n"]
    slot = lambda x: pkg.gpl_table_slot(x, n, 8)
    assert all(slot(b) == (info["home"], info["cap"]) for b in info["chain"]) and len(info["chain"]) == 60
    assert {slot(b)[0] for b in info["wrap"]} <= {info["cap"] - 1, info["cap"] - 2, info["cap"] - 3} and len(info["wrap"]) > 3   # more keys than slots to the end
    want = G.want_of(chunks, [0, 1])
    assert set(want["count"].tolist()) == {3}
    G.same(run(q, chunks, [0, 1], bc_bytes=8), want)


@pytest.mark.parametrize("n_bc", [64, 65])
def test_a_fill_on_a_capacity_step(q, n_bc):
    chunks = G.capacity_step_chunks(n_bc)
    assert pkg.gpl_table_slot(0, n_bc, 8)[1] == (128 if n_bc == 64 else 256)
    want = G.want_of(chunks, [0, 1])
    assert len(want["bc"]) == n_bc
    G.same(run(q, chunks, [0, 1], bc_bytes=8), want)


# -------------------------------------------------------------------------------------------------------------------- the bins
def test_bin_edges_the_last_bin_and_the_next_references_bins(q):
    rl = [250000, 100000, 150001]
    blens = G.blens_of(rl)
    assert blens == [0, 3, 4, 6]
    chunks = [[(1, [A(0, 99999)]), (1, [A(0, 100000)]), (1, [A(0, 100001)]), (2, [A(2, 150000)]), (2, [A(2, 199999)]),   # ... the last bin of the last reference
               (3, [A(0, 300000)]),        # past reference 0: the first bin of reference 1
               (3, [A(1, 100000)]),        # past reference 1: the first bin of reference 2
               (4, [A(1, 0)]), (4, [A(0, 0)])]]
    want = G.want_of(chunks, blens)
    assert want["bins"].tolist() == [2, 2, 0, 2, 1, 2]
    G.same(run(q, chunks, blens), want)
    # another bin size
    want = G.want_of(chunks, [0, 40, 60, 90], 7000)
    G.same(run(q, chunks, [0, 40, 60, 90], bin_size=7000), want)
    assert want["bins"][14] == 3 and want["bins"][42] == 1 and want["bins"][88] == 1


def test_a_bin_past_the_end_and_a_reference_id_out_of_range_are_refused(q):
    blens = [0, 3, 4, 6]
    good = [(1, [A(0, 5)])]
    with pytest.raises(J.ReferencePanics):
        J.record_pass([good, [(1, [A(2, 200000)])]], blens)
    data, off = rad.encode_atac_chunks([good, good, [(1, [A(2, 199999)]), (1, [A(2, 200000)])]])
    refused(q, BAD_INPUT, "chunk 2:", data, off, blens)
    data, off = rad.encode_atac_chunks([good, [(1, [A(0, 600000)])], good])       # reference 0, but six bins on: past all of them
    refused(q, BAD_INPUT, "chunk 1:", data, off, blens)
    with pytest.raises(J.ReferencePanics):
        J.record_pass([[(1, [A(3, 0)])]], blens)
    data, off = rad.encode_atac_chunks([good, good, good, [(1, [A(3, 0)])]])      # ref == ref_count
    refused(q, BAD_INPUT, "chunk 3: a reference id", data, off, blens)
    data, off = rad.encode_atac_chunks([[(1, [A(0xFFFFFFFF, 0)])]])
    refused(q, BAD_INPUT, "chunk 0: a reference id", data, off, blens)
    # a record with two alignments is not binned: its fields are not looked at
    chunks = [[(1, [A(9, 0), A(0, 4000000000)])], good]
    G.same(q.atac_gpl_hist_rad(*rad.encode_atac_chunks(chunks), blens), G.want_of(chunks, blens))
    # both kinds in one chunk: the message does not depend on the lane (the smaller code, the reference id, wins)
    data, off = rad.encode_atac_chunks([[(1, [A(0, 600000)]), (1, [A(3, 0)]), (1, [A(0, 600000)])]])
    refused(q, BAD_INPUT, "chunk 0: a reference id", data, off, blens)


def test_three_references_of_2_32_minus_1_bases(q, lim):
    rl = [4294967295] * 3
    blens = G.blens_of(rl)
    assert blens[-1] == 128850
    rng = np.random.default_rng(3)
    recs = [(int(rng.integers(0, 50)), [A(int(r), int(s))]) for r, s in zip(rng.integers(0, 3, size=3000), rng.integers(0, 1 << 32, size=3000))]
    recs += [(7, [A(0, 0)]), (7, [A(2, 4294967295)]), (7, [A(2, 4294967294)]), (7, [A(1, 4294900000)]), (7, [A(0, 4294967295)])]
    chunks = [recs[i::4] for i in range(4)]
    want = G.want_of(chunks, blens)
    assert want["bins"][0] >= 1 and want["bins"][-1] >= 2 and want["bins"][42949] >= 1
    G.same(run(q, chunks, blens), want)
    P = lim["private_bins"]
    for n_bins in ([P - 1, P, P + 1] if P else []):   # around a workgroup's private capacity: a hit in the first and in the last bin
        chunks = [[(1, [A(0, 0)]), (2, [A(0, (n_bins - 1) * 100000 + 99999)]), (2, [A(0, (n_bins - 1) * 100000)])]]
        G.same(run(q, chunks, [0, n_bins]), G.want_of(chunks, [0, n_bins]), f"{n_bins} bins")


def test_bin_base_must_ascend_from_zero(q):
    data, off = rad.encode_atac_chunks([[(1, [A(0, 5)])]])
    refused(q, INVALID_ARG, "ascend", data, off, [0, 5, 4])
    refused(q, INVALID_ARG, "bin_base[0]", data, off, [1, 5])
    refused(q, INVALID_ARG, "bin_size", data, off, [0, 5], bin_size=0)
    refused(q, INVALID_ARG, "bc_bytes", data, off, [0, 5], bc_bytes=3)
    G.same(q.atac_gpl_hist_rad(data, off, [0, 5, 5, 5]), G.want_of([[(1, [A(0, 5)])]], [0, 5, 5, 5]))   # references without a bin share a base


# --------------------------------------------------------------------------------------------------------------- malformed chunks
def test_malformed_chunks_are_refused_with_their_index_and_the_context_stays_usable(q, lim):
    bad, (data, off, chunks) = G.malformed(lim)
    want = G.want_of(chunks, [0, 1])
    assert set(bad) == {"head cut", "alignments cut", "junk tail", "nrec low", "nrec high"}
    for kind, (b, o, idx) in bad.items():
        refused(q, BAD_INPUT, f"chunk {idx}:", b, o, [0, 1])
        G.same(q.atac_gpl_hist_rad(data, off, [0, 1]), want, "after " + kind)
    # a chunk outside the buffer
    refused(q, BAD_INPUT, "chunk 2", data[:-1], off, [0, 1])
    G.same(q.atac_gpl_hist_rad(data, off, [0, 1]), want, "after a chunk outside the buffer")


def test_a_record_count_one_too_high_is_refused_by_sentence(q):
    data, off = rad.encode_atac_chunks([[(1, [A(0, 5)]), (2, [])], [(1, [A(0, 7)]), (2, [A(0, 9)])]])
    o1 = int(off[1])
    bad = data[:o1 + 4] + (3).to_bytes(4, "little") + data[o1 + 8:]   # chunk 1 holds two records and says three
    refused(q, BAD_INPUT, "chunk 1: the records do not tile the chunk", bad, off, [0, 1])


# ------------------------------------------------------------------------------------------------------------------- the context
def test_two_calls_merged_by_hand_equal_one_call(q, lim):
    rl = [250001, 900, 99993]
    chunks = G.mixed_chunks(lim, 4, rl)[:40]
    blens = G.blens_of(rl)
    whole = run(q, chunks, blens)
    a, b = run(q, chunks[:17], blens), run(q, chunks[17:], blens)
    hist = {}
    for bc, cnt, _, _ in (a, b):
        for k, v in zip(bc.tolist(), cnt.tolist()):
            hist[k] = hist.get(k, 0) + v
    keys = sorted(hist)
    assert whole[0].tolist() == keys and whole[1].tolist() == [hist[k] for k in keys]
    assert np.array_equal(whole[2], a[2] + b[2])
    for k in ("n_records", "n_unmapped", "n_multimapped", "n_binned"):
        assert whole[3][k] == a[3][k] + b[3][k]
    assert whole[3]["max_ambig"] == max(a[3]["max_ambig"], b[3]["max_ambig"]) and whole[3]["max_bin"] == int((a[2] + b[2]).max())
    G.same(whole, G.want_of(chunks, blens))
    again = run(q, chunks, blens)                       # run to run: a function of the input alone
    assert all(np.array_equal(x, y) for x, y in zip(whole[:3], again[:3])) and whole[3] == again[3]


def test_device_resident_input_equals_host_input(q, lim):
    import torch

    rl = [250001, 900, 99993]
    chunks = G.mixed_chunks(lim, 2, rl)[:30]
    blens = G.blens_of(rl)
    data, off = rad.encode_atac_chunks(chunks, bc_bytes=2)
    want = G.want_of(chunks, blens)
    G.same(q.atac_gpl_hist_rad(data, off, blens, bc_bytes=2), want, "host bytes")
    for al in (0, 3):   # (a device buffer that starts off a dword boundary: nothing in front of it is read)
        t = torch.from_numpy(np.frombuffer(b"\0" * al + data, np.uint8).copy()).cuda()
        G.same(q.atac_gpl_hist_rad(None, off, blens, bc_bytes=2, d_ptr=t.data_ptr() + al, n_bytes=len(data)), want, f"device bytes + {al}")


def test_kernel_times_name_the_record_pass(lim):
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, profile=True)
    qq = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    try:
        run(qq, [[(1, [A(0, 5)]), (2, [])]], [0, 1])
        t = qq.kernel_times()
    finally:
        qq.close()
    assert t["k_atac_gpl_parse"][1] == 1 and t["k_gpl_count"][1] == 1 and t["k_gpl_compact"][1] == 1
