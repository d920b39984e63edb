"""GPU tests of the multi-barcode generate-permit-list record pass: Quantifier.gpl_multi_hist_rad against tests/gpl_multi_judge.py on
the cases of tests/gpl_multi_cases.py (whose reach tests/test_gpl_multi_cases_cpu.py shows without a device).  Everything is exact:
array for array, plus the stats.  `n_long_records` and the launch counts of a profiled context are witnesses that a route RAN; they
never decide whether a result is right."""
import numpy as np
import pytest

import gpl_multi_cases as MC
from util import pkg

pytestmark = pytest.mark.gpu
BAD_INPUT, INVALID_ARG = pkg._abi.AFQ_ERR_BAD_INPUT, pkg._abi.AFQ_ERR_INVALID_ARG


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
    return pkg.gpl_multi_limits()


def run(q, c, ori):
    q.set_aln_extra_bytes(c["pos_bytes"])
    try:
        return q.gpl_multi_hist_rad(c["data"], c["off"], np.asarray(c["entries"], np.uint64), b0_bytes=c["b0_bytes"], b1_bytes=c["b1_bytes"],
                                    umi_bytes=c["umi_bytes"], expected_ori=ori)
    finally:
        q.set_aln_extra_bytes(0)


def check(q, c, oris=MC.ORIS, what=""):
    out = {}
    for ori in oris:
        out[ori] = run(q, c, ori)
        MC.same_pairs(out[ori], MC.want_pairs(c, ori), f"{what} {ori}")
    return out


# ------------------------------------------------------------------------------------------------------------------ parse
@pytest.mark.parametrize("b1_bytes", MC.B_WIDTHS)
@pytest.mark.parametrize("b0_bytes", MC.B_WIDTHS)
def test_every_width_pair_with_every_umi_width(q, b0_bytes, b1_bytes):
    """the smallest and the largest b0 of the width as entries and as misses; the all-ones pair at every width pair (4 + 4 included)"""
    for ub in MC.U_WIDTHS:
        for edges in ("entries", "misses"):
            check(q, MC.widths_case(b0_bytes, b1_bytes, ub, edges), what=f"b0 {b0_bytes} b1 {b1_bytes} umi {ub} {edges}")
    check(q, MC.widths_case(b0_bytes, b1_bytes, 4, "entries", pos_bytes=4), what=f"b0 {b0_bytes} b1 {b1_bytes} positions")


@pytest.mark.parametrize("pad", range(4))
def test_chunks_at_every_byte_alignment(q, pad):
    check(q, MC.alignment_case(pad), what=f"pad {pad}")


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_records_ending_at_the_tile_edge(q, lim, delta):
    check(q, MC.tile_edge_case(lim, delta)[0], what=f"tile end {delta:+d}")


def test_the_halo_holds_lane_alns_of_the_widest_alignments(q, lim):
    under, over = (check(q, MC.halo_case(lim, lim["lane_alns"] + d)[0], oris=["fw", "rc", "both"]) for d in (0, 1))
    assert under["fw"]["stats"]["n_long_records"] == 0 and over["fw"]["stats"]["n_long_records"] == 1   # witness: the route changed
    assert over["both"]["stats"]["n_long_records"] == 0   # `both` reads no alignment word


@pytest.mark.parametrize("where", ["first", "last", "absent"])
def test_long_records_are_tested_over_every_alignment(q, where):
    got = check(q, MC.long_case(where), what=where)
    assert got["fw"]["stats"]["n_long_records"] == 5 == got["rc"]["stats"]["n_long_records"]   # witness: 3 x 2500, 3000 and 40


def test_records_without_an_alignment_count_only_under_both(q):
    got = check(q, MC.no_alignment_case())
    assert got["both"]["stats"]["n_compatible"] == 7 and got["fw"]["stats"]["n_compatible"] == 1 == got["rc"]["stats"]["n_compatible"]


@pytest.mark.parametrize("kind", ["head_cut", "alns_cut", "junk", "nrec_low", "nrec_high"])
def test_malformed_chunks_are_refused_with_their_index(q, kind):
    data, off = MC.malformed_case(kind)
    for ori in ("both", "fw"):
        with pytest.raises(pkg.AfqError) as e:   # (raised: no arrays come back)
            q.gpl_multi_hist_rad(data, off, np.asarray([1, 2], np.uint64), b0_bytes=2, b1_bytes=2, umi_bytes=4, expected_ori=ori)
        assert e.value.code == BAD_INPUT and "chunk 2:" in str(e.value), str(e.value)
    # the context serves again afterwards
    a, _ = MC.two_fill_cases()
    check(q, a, oris=["both"])


def test_a_record_count_one_too_high_is_refused_by_sentence(q):
    data, off = pkg.rad.encode_multi_bc_chunks([[(1, 7, 1, [(0, True)]), (2, 8, 2, [(1, False)])], [(1, 7, 3, [(0, True), (1, True)]), (3, 8, 4, [(0, False), (1, True)])]])
    o1 = int(off[1])
    bad = data[:o1 + 4] + (3).to_bytes(4, "little") + data[o1 + 8:]   # chunk 1 holds two records and says three (three heads would fit it)
    with pytest.raises(pkg.AfqError) as e:
        q.gpl_multi_hist_rad(bad, off, np.asarray([1, 2], np.uint64), b0_bytes=2, b1_bytes=4, umi_bytes=4)
    assert e.value.code == BAD_INPUT and "chunk 1:" in str(e.value) and "the records do not tile the chunk" in str(e.value), str(e.value)


def test_chunk_table_and_argument_refusals(q):
    c = MC.widths_case(2, 4, 4)
    ent = np.asarray(c["entries"], np.uint64)
    off = c["off"].copy()
    off[1] = len(c["data"]) - 4
    with pytest.raises(pkg.AfqError) as e:
        q.gpl_multi_hist_rad(c["data"], off, ent)
    assert e.value.code == BAD_INPUT and "chunk 1" in str(e.value)
    got = q.gpl_multi_hist_rad(b"", np.zeros(0, np.uint64), ent)
    assert len(got["entry"]) == 0 and got["stats"]["n_records"] == 0


def test_the_same_case_twice_gives_identical_arrays(q):
    c = MC.widths_case(2, 4, 4)
    a, b = run(q, c, "fw"), run(q, c, "fw")
    assert all(np.array_equal(a[k], b[k]) for k in ("entry", "cell", "count")) and a["stats"] == b["stats"]


# ------------------------------------------------------------------------------------------------------------ entry table
@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_entry_counts_and_a_capacity_step(q, n):
    got = check(q, MC.n_entries_case(n), oris=["both"])["both"]
    assert (got["stats"]["n_routed"] == 0) == (n == 0)


@pytest.mark.parametrize("wrap", [False, True])
def test_entry_probe_chains(q, wrap):
    c, chain, misses, cap, slot = MC.entry_chain_case(wrap)
    got = check(q, c, oris=["both"])["both"]
    assert {c["entries"].index(b) for b in chain} <= set(got["entry"].tolist())


# --------------------------------------------------------------------------------------------------------- counting table
def test_one_pair_on_70000_records(qp):
    got = check(qp, MC.hot_case())
    assert got["both"]["count"].tolist() == [70, 70000, 70]
    t = qp.kernel_times()
    assert t["k_gpl_multi_table"][1] == 1 and t["k_gpl_multi_parse"][1] == 1 and t["k_gpl_count"][1] == 1 and t["k_gpl_compact"][1] == 1


def test_keys_homing_at_the_last_slot(q):
    c, pairs, cap = MC.count_chain_case()
    got = check(q, c, oris=["both"])["both"]
    assert set(pairs) <= set(zip(got["entry"].tolist(), got["cell"].tolist()))


def test_two_fills_of_one_context_merge(q):
    a, b = MC.two_fill_cases()
    ga, gb = run(q, a, "both"), run(q, b, "both")
    want = MC.want_pairs(MC.multi_case(a["chunks"] + b["chunks"], a["entries"]), "both")
    m = MC.merge_pairs(ga, gb)
    assert sorted(m) == list(zip(want["entry"].tolist(), want["cell"].tolist())) and [m[k] for k in sorted(m)] == want["count"].tolist()
    for k in ("n_records", "n_compatible", "n_routed", "n_unrouted"):
        assert ga["stats"][k] + gb["stats"][k] == want["stats"][k]
