"""GPU tests of `atac sort` at the parse, table, level, leaf and emit edges; the inputs are the builders of tests/atac_sort_cases.py,
whose reach tests/test_atac_sort_cases_cpu.py shows without a device (the cheap witnesses are asserted again here, so that a changed
constant makes a test say "no longer covers").

Every result is judged by `atac_sort_cases.expected`: np.lexsort + unique-with-counts on the decoded records, exact integer equality array for array
through `same`, plus the stats.  The level model and the probe-chain walk are witnesses that the deep paths RAN (launch counts of a
profiled context against the model's); they never decide whether a row is right."""
import numpy as np
import pytest

import atac_sort_cases as A
from atac_sort_cases import same, want_of
from util import assert_same_result, cfg_for, pkg

pytestmark = pytest.mark.gpu
BAD_INPUT = pkg._abi.AFQ_ERR_BAD_INPUT
WIDTHS = [1, 2, 4, 8]


def _quantifier(**kw):
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, **kw)
    return pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)


@pytest.fixture(scope="module")
def q():
    qq = _quantifier()
    yield qq
    qq.close()


@pytest.fixture(scope="module")
def qp():
    """a context that times its launches: kernel_times() counts them per kernel group"""
    qq = _quantifier(profile=True)
    yield qq
    qq.close()


@pytest.fixture(scope="module")
def lim():
    L = pkg.atac_sort_limits()
    assert L["repartition_above"] >= L["leaf_cap"] > 1025 and L["parse_tile"] >= 64
    return L


@pytest.fixture(scope="module")
def deep(lim):
    c = A.deep_case(lim)
    return c, want_of(c), A.level_model(c, lim)


def run(q, c, data=None, off=None, **kw):
    return q.atac_sort_rad(c["data"] if data is None else data, c["off"] if off is None else off, c["obs"], c["cor"], c["ref_lengths"], bc_bytes=c["bc_bytes"], **kw)


def check(q, c, what="", **kw):
    got = run(q, c, **kw)
    same(got, want_of(c), what)
    st = got["stats"]
    assert (st["n_records"], st["n_unmapped"], st["n_multimapped"]) == c["counts"], (what, st)
    return got


def partition_launches(qp):
    return qp.kernel_times()["k_sort_partition"][1]


# ------------------------------------------------------------------------------------------------------------------ parse
@pytest.mark.parametrize("bc_bytes", WIDTHS)
def test_a_tile_full_of_record_starts(q, lim, bc_bytes):
    tile, H = lim["parse_tile"], 4 + bc_bytes
    c = A.tile_full_case(lim, bc_bytes)
    first = A.tile_walk(c["data"], c["off"][0], bc_bytes, lim)[0][0][1]
    assert len(first) == -(-tile // H) and (H != 5 or (len(first) == tile // 5 + 1 and first[-1][0] == tile - 1)), "no longer covers a full tile"
    got = check(q, c)   # (n_unmapped and n_kept among what it compares)
    n = 3 * (tile // H) + 7
    assert c["counts"] == (2 * n, 2 * n - 2 * ((n - 1) // 64) - ((n - 1) % 64 == 63), 0) and got["stats"]["n_kept"] > 0 and got["stats"]["n_uncorrected"] > 0


@pytest.mark.parametrize("bc_bytes", WIDTHS)
def test_records_longer_than_a_tile(q, lim, bc_bytes):
    tile, H = lim["parse_tile"], 4 + bc_bytes
    c = A.long_records_case(lim, bc_bytes)
    nas = A.long_record_nas(lim)
    assert 8 + 11 * nas[2] <= tile + lim["parse_halo"] < 8 + 11 * nas[3] and H + 11 * nas[-1] > 10 * tile, "no longer covers the crossing"
    for al in range(4):
        got = check(q, c, f"alignment {al}", data=b"\xEE" * al + c["data"], off=c["off"] + np.uint64(al))
        assert got["stats"]["n_multimapped"] == len(nas) + 4


@pytest.mark.parametrize("bc_bytes", WIDTHS)
@pytest.mark.parametrize("position", A.HALO_POSITIONS)
def test_heads_in_the_halo(q, lim, bc_bytes, position):
    """the chunk with the record is the last of the buffer: once with nothing behind it, once with 0xEE bytes behind it, and once as
    device bytes with n_bytes == the buffer's length - the kernel must not depend on what follows the buffer"""
    import torch

    tile, H = lim["parse_tile"], 4 + bc_bytes
    c = A.halo_case(lim, bc_bytes, position)
    tiles, end = A.tile_walk(c["data"], c["off"][1], bc_bytes, lim)
    assert tiles[-1][1][-1] == ((0, 1) if position == "next_tile" else (c["target"], 1)) and int(c["off"][1]) + end == len(c["data"]), "no longer covers"
    assert c["target"] in (tile - 1, tile - H, tile - H - 11, tile)
    bare = check(q, c, "nothing behind")
    tail = check(q, c, "0xEE behind", data=c["data"] + b"\xEE" * 64)
    t = torch.from_numpy(np.frombuffer(c["data"], np.uint8).copy()).cuda()
    dev = check(q, c, "device bytes", data=None, d_ptr=t.data_ptr(), n_bytes=len(c["data"]))
    for other in (tail, dev):
        assert all(np.array_equal(bare[k], other[k]) for k in ("ref", "start", "frag_len", "bc", "count")) and other["stats"] == bare["stats"]
    i = int(np.flatnonzero(bare["frag_len"] == 65535)[0])
    assert (int(bare["ref"][i]), int(bare["start"][i]), int(bare["count"][i])) == (0, 0x04030201, 1)
    assert int(bare["bc"][i]) == (0x0807060504030201 & ((1 << (8 * bc_bytes)) - 1)) ^ 0x80


@pytest.mark.parametrize("kind", A.EDGE_KINDS)
def test_chunk_ends_on_a_tile_edge(q, lim, kind):
    tile = lim["parse_tile"]
    c = A.exact_edge_case(lim, kind)
    tiles, end = A.tile_walk(c["data"], c["off"][1], c["bc_bytes"], lim)
    assert end - 8 == c["body"] and (kind not in ("tile", "two_tiles") or [p for p, _ in tiles] == [8 + tile * i for i in range(c["body"] // tile)]), "no longer covers"
    check(q, c)
    for what, blob in A.edge_refusals(c).items():
        with pytest.raises(pkg.AfqError) as e:
            run(q, c, data=blob)
        assert e.value.code == BAD_INPUT and "chunk 1:" in str(e.value) and "do not tile" in str(e.value), (what, str(e.value))
        check(q, c, "after " + what)


# ------------------------------------------------------------------------------------------------------------- correction
@pytest.mark.parametrize("n_corr", [1, 2, 3, 4, 1024, 1025])
def test_probe_chains_and_wrap(q, lim, n_corr):
    slot = pkg.atac_sort_table_slot
    c = A.chain_case(lim, n_corr, slot)
    assert len(c["obs"]) == n_corr and all(slot(k, n_corr)[0] == c["crowded_home"] for k in c["chain"][:5] + c["absent"])
    where, cap = A.table_slots(c["obs"], n_corr, slot)
    if n_corr & (n_corr - 1) == 0:
        assert 2 * len(where) == cap == 2 * n_corr, "no longer covers a load of exactly one half"
    if n_corr >= 1024:
        assert len(c["chain"]) == 300 and len(c["wrap"]) == 40 and sum(where[k][1] < where[k][0] for k in c["wrap"]) >= 37, "no longer covers"
    got = check(q, c)
    assert got["stats"]["n_uncorrected"] == len(c["absent"]) == 20   # absent barcodes on the crowded home slot: never a neighbour's rank
    if n_corr >= 1024:   # a chain member with two corrections is refused with the chain in place
        obs, cor = c["obs"].copy(), c["cor"]   # (an entry outside the chain becomes a second entry of a chain member, under its own correction: n_corr stays)
        obs[np.flatnonzero(obs == np.uint64(c["rnd"][0]))[0]] = np.uint64(c["chain"][150])
        assert (obs == np.uint64(c["chain"][150])).sum() == 2 and len(obs) == n_corr
        with pytest.raises(pkg.AfqError) as e:
            q.atac_sort_rad(c["data"], c["off"], obs, cor, c["ref_lengths"], bc_bytes=8)
        assert e.value.code == BAD_INPUT and "two different corrected" in str(e.value)
        check(q, c, "after the refusal")


# ----------------------------------------------------------------------------------------------------------------- levels
def test_deep_repartition(qp, lim, deep):
    c, want, m = deep
    assert (m["parts"], m["bits"], m["repartitioned"]) == (7, 8, 3) and 0 in m["shifts"], "no longer covers seven splitting levels and shift == 0"
    assert {b for _, b in m["leaves"]} == {0, 1} and len({lv for lv, _ in m["leaves"]}) >= 8, "no longer covers leaves in both buffers"
    got = run(qp, c)
    launches = partition_launches(qp)
    same(got, want)
    assert got["stats"]["n_repartitioned_bins"] == 3
    assert launches == 1 + m["bits"] + m["parts"], (launches, m)
    again = run(qp, c)
    same(again, want)
    assert again["stats"] == got["stats"] and all(np.array_equal(again[k], got[k]) for k in ("ref", "start", "frag_len", "bc", "count"))


def test_mixed_segment_list(qp, lim):
    c = A.mixed_case(lim)
    m = A.level_model(c, lim)
    assert m["mixed"] and (m["bits"], m["parts"], m["repartitioned"]) == (2, 1, 5) and len(set(m["shifts"])) == 2, "no longer covers"
    got = check(qp, c)
    assert partition_launches(qp) == 1 + m["bits"] + m["parts"] and got["stats"]["n_repartitioned_bins"] == 5


# ----------------------------------------------------------------------------------------------------------------- leaves
@pytest.mark.parametrize("repeated", [False, True])
def test_leaf_classes(q, lim, repeated):
    """bins of 2^k - 1, 2^k, 2^k + 1 records for k = 6..14 (63 .. 16 384; 16 385 is above the leaf cap and left out), as distinct
    keys and with every key present 1, 2, 3, 1, 2, 3, ... times"""
    sizes = A.leaf_class_sizes(lim)
    assert sizes[0] == 63 and max(sizes) >= 1 << 14 and max(sizes) <= lim["repartition_above"]
    got = check(q, A.leaf_class_case(lim, repeated))
    assert got["stats"]["n_repartitioned_bins"] == 0 and int(got["count"].max()) == (3 if repeated else 1)


def test_run_head_slices(q, lim):
    leaves = A.run_head_leaves(lim)
    assert len(leaves) == 24 and all(L[0] == 1 and L[-1] == 1 for *_, L in leaves)
    c = A.run_head_case(lim)
    got = check(q, c)
    assert got["stats"]["n_repartitioned_bins"] == 0 and got["count"].tolist() == [n for *_, L in leaves for n in L]


# ------------------------------------------------------------------------------------------------------------------- emit
def test_bisection_and_high_starts(q, lim):
    for name, c in A.emit_cases(lim).items():
        got = check(q, c, name)
        if name == "one_reference_of_2^32-1":
            assert int(got["start"].max()) == (1 << 32) - 2 and (got["ref"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- context
def test_call_sequence_on_one_context(lim, deep):
    c, want, _ = deep
    qq = _quantifier()
    try:
        same(run(qq, c), want, "deep")
        check(qq, A.eleven_record_case(), "11 records on 3 references")
        check(qq, A.many_references_case(), "70 000 references")
        shrunk = A.deep_case(lim, extra_bins=0)
        assert len(shrunk["ref_lengths"]) == 1 and int(shrunk["ref_lengths"][0]) < int(c["ref_lengths"][0])
        got = run(qq, shrunk)
        same(got, want_of(shrunk), "deep, fewer bins")
        assert got["stats"]["n_repartitioned_bins"] == 3
        check(qq, A.eleven_record_case(), "11 records again")
    finally:
        qq.close()


def test_quant_before_and_after_a_sort(oracle, lim):
    import torch

    s = pkg.synth.synth(1, [50] * 300 + [900, 5, 2500], num_genes=1000)
    b, off = s.encode()
    cfg = cfg_for(s)
    want = oracle.quant(cfg, s.tid_to_gid, b, off)
    halo = A.halo_case(lim, 8, "last_byte")
    other = A.exact_edge_case(lim, "two_tiles")
    qq = pkg.Quantifier(cfg, s.tid_to_gid, device=0)
    try:
        assert_same_result(qq.quant_chunks(b, off), want, what="quant before")
        check(qq, halo, "sort between two quant batches")
        assert_same_result(qq.quant_chunks(b, off), want, what="quant after")
        check(qq, other, "host bytes")
        t = torch.from_numpy(np.frombuffer(b"\0" + halo["data"], np.uint8).copy()).cuda()
        check(qq, halo, "device bytes right after host bytes", data=None, d_ptr=t.data_ptr() + 1, n_bytes=len(halo["data"]))
        assert_same_result(qq.quant_chunks(b, off), want, what="quant at the end")
    finally:
        qq.close()
