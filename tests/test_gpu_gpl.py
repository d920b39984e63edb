"""GPU tests of the generate-permit-list kernels: Quantifier.gpl_hist_rad and Quantifier.gpl_correct against tests/gpl_judge.py on
the cases of tests/gpl_cases.py (whose reach tests/test_gpl_cases_cpu.py shows without a device).  Everything is exact: array for
array, plus the stats.  `n_long_records` and the launch counts of a profiled context are witnesses that a route RAN; they never
decide whether a result is right."""
import numpy as np
import pytest

import gpl_cases as G
import gpl_judge as J
from util import pkg

pytestmark = pytest.mark.gpu
BAD_INPUT, INVALID_ARG, UNSUPPORTED = pkg._abi.AFQ_ERR_BAD_INPUT, pkg._abi.AFQ_ERR_INVALID_ARG, pkg._abi.AFQ_ERR_UNSUPPORTED


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
    return pkg.gpl_limits()


def hist(q, c, ori):
    q.set_aln_extra_bytes(c["pos_bytes"])
    try:
        return q.gpl_hist_rad(c["data"], c["off"], bc_bytes=c["bc_bytes"], umi_bytes=c["umi_bytes"], expected_ori=ori)
    finally:
        q.set_aln_extra_bytes(0)


def check_hist(q, c, oris=G.ORIS, what=""):
    out = {}
    for ori in oris:
        out[ori] = hist(q, c, ori)
        G.same_hist(out[ori], G.want_hist(c, ori), f"{what} {ori}")
    return out


# ------------------------------------------------------------------------------------------------------------------ parse
@pytest.mark.parametrize("bc_bytes", G.WIDTHS)
def test_every_field_width_with_and_without_positions(q, bc_bytes):
    for ub in G.WIDTHS:
        for pb in (0, 4):
            check_hist(q, G.widths_case(bc_bytes, ub, pb), what=f"bc {bc_bytes} umi {ub} pos {pb}")


@pytest.mark.parametrize("pad", range(4))
def test_chunks_at_every_byte_alignment(q, pad):
    check_hist(q, G.alignment_case(pad), what=f"pad {pad}")


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_records_ending_at_the_tile_edge(q, lim, delta):
    check_hist(q, G.tile_edge_case(lim, delta)[0], what=f"tile end {delta:+d}")


def test_the_halo_holds_lane_alns_of_the_widest_alignments(q, lim):
    under, over = (check_hist(q, G.halo_case(lim, lim["lane_alns"] + d)[0], oris=["fw", "rc", "both"]) for d in (0, 1))
    assert under["fw"]["stats"]["n_long_records"] == 0 and over["fw"]["stats"]["n_long_records"] == 1   # witness: the route changed
    assert over["both"]["stats"]["n_long_records"] == 0   # `both` reads no alignment word


@pytest.mark.parametrize("where", ["first", "last", "absent"])
def test_long_records_are_tested_over_every_alignment(q, where):
    got = check_hist(q, G.long_case(where), what=where)
    assert got["fw"]["stats"]["n_long_records"] == 4 == got["rc"]["stats"]["n_long_records"]   # witness: 2 x 2500, 3000 and 40
    assert got["fw"]["stats"]["max_ambig"] == 2500 and got["both"]["stats"]["max_ambig"] == 3000


@pytest.mark.parametrize("kind", ["head_cut", "alns_cut", "junk", "nrec_low", "nrec_high"])
def test_malformed_chunks_are_refused_with_their_index(q, kind):
    data, off = G.malformed_case(kind)
    for ori in ("both", "fw"):
        with pytest.raises(pkg.AfqError) as e:
            q.gpl_hist_rad(data, off, bc_bytes=4, umi_bytes=4, expected_ori=ori)
        assert e.value.code == BAD_INPUT and "chunk 2:" in str(e.value), str(e.value)
    # the context serves again afterwards
    a, _ = G.two_fill_cases()
    check_hist(q, a, oris=["both"])


def test_a_record_count_one_too_high_is_refused_by_sentence(q):
    data, off = pkg.rad.encode_chunks([[(7, 1, [(0, True)]), (8, 2, [(1, False)])], [(7, 3, [(0, True), (1, True)]), (8, 4, [(0, False), (1, True)])]])
    o1 = int(off[1])
    bad = data[:o1 + 4] + (3).to_bytes(4, "little") + data[o1 + 8:]   # chunk 1 holds two records and says three (three heads would fit it)
    with pytest.raises(pkg.AfqError) as e:
        q.gpl_hist_rad(bad, off, bc_bytes=4, umi_bytes=4)
    assert e.value.code == BAD_INPUT and "chunk 1:" in str(e.value) and "the records do not tile the chunk" in str(e.value), str(e.value)


def test_chunk_table_refusals(q):
    c = G.widths_case(4, 4, 0)
    off = c["off"].copy()
    off[1] = len(c["data"]) - 4
    with pytest.raises(pkg.AfqError) as e:
        q.gpl_hist_rad(c["data"], off)
    assert e.value.code == BAD_INPUT and "chunk 1" in str(e.value)
    with pytest.raises(pkg.AfqError) as e:
        q.gpl_hist_rad(c["data"], c["off"], bc_bytes=3)
    assert e.value.code == INVALID_ARG
    with pytest.raises(pkg.AfqError) as e:
        q.gpl_hist_rad(c["data"], c["off"], expected_ori=3)
    assert e.value.code == INVALID_ARG
    got = q.gpl_hist_rad(b"", np.zeros(0, np.uint64))
    assert len(got["bc"]) == 0 and got["stats"]["n_records"] == 0


# ------------------------------------------------------------------------------------------------------------------ count
def test_one_barcode_on_70000_records(qp):
    got = check_hist(qp, G.hot_case())
    assert got["both"]["count"].tolist() == [70, 70000, 70]
    t = qp.kernel_times()
    assert t["k_gpl_parse"][1] == 1 and t["k_gpl_count"][1] == 1 and t["k_gpl_compact"][1] == 1


@pytest.mark.parametrize("wrap", [False, True])
def test_probe_chains(q, wrap):
    c, bcs, cap, slot = G.chain_case(wrap)
    got = check_hist(q, c, oris=["both"])["both"]
    assert set(bcs) <= set(got["bc"].tolist())


@pytest.mark.parametrize("n", [64, 65])
def test_fill_on_a_capacity_step(q, n):
    check_hist(q, G.capacity_step_case(n), oris=["both"])


def test_two_fills_of_one_context_merge(q):
    a, b = G.two_fill_cases()
    ga, gb = hist(q, a, "both"), hist(q, b, "both")
    bc, cnt = G.merge_hists(ga, gb)
    want = G.want_hist(G.parse_case(a["chunks"] + b["chunks"], 4, 4), "both")
    assert np.array_equal(bc, want["bc"]) and np.array_equal(cnt, want["count"])
    assert ga["stats"]["n_records"] + gb["stats"]["n_records"] == want["n_records"]
    assert max(ga["stats"]["max_ambig"], gb["stats"]["max_ambig"]) == want["max_ambig"]


# ---------------------------------------------------------------------------------------------------------------- correct
def correct(q, c):
    w = G.want_correct(c)
    obs = np.asarray([b for b, _ in c["observed"]], np.uint64)
    cnt = np.asarray([n for _, n in c["observed"]], np.uint64)
    res = c["resolution"]
    kw = {} if res == "unique" else {"confidence": res[1], "pseudocount": res[2]}
    got = q.gpl_correct(obs, cnt, w["retained"], w["retained_count"], c["L"], neighborhood=c["neighborhood"],
                        resolution="unique" if res == "unique" else "frequency", **kw)
    return got, w


def check_correct(q, c, what=""):
    got, w = correct(q, c)
    G.same_correct(got, w, what)
    return got, w


@pytest.mark.parametrize("nbh", [J.HAMMING, J.SHIFT])
@pytest.mark.parametrize("res", ["unique", G.RNA], ids=["unique", "frequency"])
def test_l4_exhaustive(q, nbh, res):
    for k in range(len(G.L4_RETAINED)):
        check_correct(q, G.l4_case(k, nbh, res), what=f"retained set {k}")


@pytest.mark.parametrize("L", [16, 32])
@pytest.mark.parametrize("nbh", [J.HAMMING, J.SHIFT])
@pytest.mark.parametrize("res", ["unique", G.RNA], ids=["unique", "frequency"])
def test_random_barcodes(q, L, nbh, res):
    check_correct(q, G.random_case(L, nbh, res, top_bit=(L == 32)))


@pytest.mark.parametrize("res", ["unique", G.RNA], ids=["unique", "frequency"])
def test_l32_shift_masks_at_both_ends(q, res):
    check_correct(q, G.boundary_case_l32(res))


def test_frequency_thresholds_ties_and_single_weighing(q):
    code = {J.EXACT: 0, J.CORRECTED: 1, J.AMBIGUOUS: 2, J.NOT_FOUND: 3}
    for name, (c, x, dec, tgt) in G.frequency_cases().items():
        got, w = check_correct(q, c, what=name)
        i = [b for b, _ in c["observed"]].index(x)
        assert got["decision"][i] == code[dec], name
        assert got["target"][i] == (0xFFFFFFFF if tgt is None else sorted(c["retained"]).index(tgt)), name


def test_never_observed_retained_barcode(q):
    c = G.never_observed_case()
    got, w = check_correct(q, c)
    assert got["target_count"].tolist() == [0, 7] and got["stats"]["exact_distinct"] == 1


def test_full_neighbourhood_route(qp):
    """permit_map.bin's theoretical neighbourhood: every retained barcode and all its neighbours as the observed list, counts 0"""
    ret = G.L4_RETAINED[3]
    for res in ("unique", G.RNA):
        idx = J.identity_index(4, J.SHIFT, res, ret)
        obs = idx.theoretical_observations()
        got, w = check_correct(qp, G.correct_case(4, J.SHIFT, res, ret, {b: 0 for b in obs}))
        entries, st = idx.compile_full_neighborhood()
        srt = sorted(ret)
        mine = [(b, srt[t]) for b, t in zip(obs, got["target"].tolist()) if t != 0xFFFFFFFF]
        assert mine == entries and got["stats"] == st and not got["target_count"].any()
        t = qp.kernel_times()
        assert t["k_gpl_table"][1] == 1 and t["k_gpl_correct"][1] == 1


def test_correct_refusals(q):
    one = np.asarray([1], np.uint64)
    def call(obs, ret, L=4, **kw):
        return q.gpl_correct(np.asarray(obs, np.uint64), np.ones(len(obs), np.uint64), np.asarray(ret, np.uint64), np.ones(len(ret), np.uint64), L, **kw)
    for obs, ret in (([2, 1], [3]), ([1, 1], [3]), ([1], [3, 3]), ([1], [4, 3])):
        with pytest.raises(pkg.AfqError) as e:
            call(obs, ret)
        assert e.value.code == INVALID_ARG, (obs, ret)
    for obs, ret in (([256], [3]), ([1], [256])):
        with pytest.raises(pkg.AfqError) as e:
            call(obs, ret)
        assert e.value.code == BAD_INPUT and "does not fit declared length 4" in str(e.value)
    for kw in ({"confidence": (3, 0)}, {"confidence": (3, 2)}, {"pseudocount": 0}):
        with pytest.raises(pkg.AfqError) as e:
            call([1], [3], resolution="frequency", **kw)
        assert e.value.code == INVALID_ARG, kw
    with pytest.raises(pkg.AfqError) as e:
        call([1], [3], L=33)
    assert e.value.code == INVALID_ARG
    with pytest.raises(pkg.AfqError) as e:
        q.gpl_correct(one, one, one * 3, one << np.uint64(55), 4, resolution="frequency")
    assert e.value.code == UNSUPPORTED
    got = call([], [])
    assert len(got["decision"]) == 0 and not any(got["stats"].values())
