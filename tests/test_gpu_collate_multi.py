"""GPU tests of the multi-barcode collate kernels: Quantifier.collate_multi_rad against tests/collate_multi_judge.py on the cases of
tests/collate_multi_cases.py (whose reach tests/test_collate_multi_cases_cpu.py shows).  Everything is exact: the output bytes, the
chunk offsets, the per-cell record counts and every stat.  Shapes derive from collate_multi_limits()."""
import numpy as np
import pytest

import collate_multi_cases as C
from util import pkg

pytestmark = pytest.mark.gpu
BAD_INPUT, INVALID_ARG = pkg._abi.AFQ_ERR_BAD_INPUT, pkg._abi.AFQ_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def q():
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    qq = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    yield qq
    qq.close()


@pytest.fixture(scope="module")
def lim():
    return pkg.collate_multi_limits()


def run(q, c, ori, **kw):
    q.set_aln_extra_bytes(c["pos_bytes"])
    try:
        return q.collate_multi_rad(kw.pop("data", c["data"]), c["off"], *C.args(c), b0_bytes=c["b0_bytes"], b1_bytes=c["b1_bytes"], umi_bytes=c["umi_bytes"],
                                   expected_ori=ori, **kw)
    finally:
        q.set_aln_extra_bytes(0)


def same(got, want, what=""):
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert got["nrec"].tolist() == want["nrec"], (what, "nrec")
    assert got["chunk_off"].tolist() == want["chunk_off"], (what, "chunk_off")
    gb = got["bytes"].tobytes()
    if gb != want["bytes"]:
        at = next(i for i, (x, y) in enumerate(zip(gb, want["bytes"])) if x != y)
        raise AssertionError((what, "bytes differ first at", at, gb[max(0, at - 8):at + 24].hex(), want["bytes"][max(0, at - 8):at + 24].hex()))


def check(q, lim, c, oris=C.ORIS, what=""):
    out = {}
    for ori in oris:
        w = C.want(c, ori, lim["lane_alns"])
        out[ori] = (run(q, c, ori), w)
        same(out[ori][0], w, f"{what} {ori}")
    return out


# ------------------------------------------------------------------------------------------------------------------ widths
@pytest.mark.parametrize("b0", C.B_WIDTHS)
@pytest.mark.parametrize("b1", C.B_WIDTHS)
def test_every_width_pair_and_umi_width_under_every_orientation(q, lim, b0, b1):
    for uw in C.U_WIDTHS:
        check(q, lim, C.widths_case(b0, b1, uw), what=f"b0 {b0} b1 {b1} umi {uw}")


# ------------------------------------------------------------------------------------------------------------------ tile edges
@pytest.mark.parametrize("pad", [0, 1, 2, 3])
def test_chunks_and_output_records_at_every_alignment(q, lim, pad):
    check(q, lim, C.alignment_case(pad), what=f"pad {pad}")


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_records_at_the_tile_edge(q, lim, delta):
    check(q, lim, C.tile_edge_case(lim, delta)[0], what=f"tile end {delta:+d}")


def test_a_chunk_of_exactly_one_tile(q, lim):
    check(q, lim, C.one_tile_chunk_case(lim), what="one tile")


@pytest.mark.parametrize("d", [0, 1])
def test_an_alignment_list_in_the_halo_and_one_alignment_more(q, lim, d):
    out = check(q, lim, C.halo_case(lim, lim["lane_alns"] + d)[0], what=f"halo {d}")
    assert out["fw"][0]["stats"]["n_long_records"] == d


@pytest.mark.parametrize("where", ["first", "last", "absent"])
def test_long_records_kept_dropped_unrouted_and_uncorrected(q, lim, where):
    check(q, lim, C.long_case(where), what=f"long {where}")


@pytest.mark.parametrize("pos_bytes", [4, 8])
def test_every_route_with_position_bytes_and_every_fate(q, lim, pos_bytes):
    """records of up to 129 alignments WITH position bytes, fitting words before and beyond the first 64-lane trip, kept, corrected,
    unrouted and uncorrected in turn (tests/test_collate_multi_cases_cpu.py shows the reach)"""
    out = check(q, lim, C.route_case(lim, pos_bytes), what=f"routes pos {pos_bytes}")
    assert set(out) == set(C.ORIS) and out["fw"][0]["stats"]["n_long_records"] > 0


def test_records_without_alignments(q, lim):
    check(q, lim, C.no_alignment_case(), what="na 0")


# ------------------------------------------------------------------------------------------------------------------ the lookup
def test_the_two_level_lookup(q, lim):
    check(q, lim, C.lookup_case(), what="lookup")


def test_probe_chains_that_wrap_both_tables(q, lim):
    check(q, lim, C.chain_case()[0], what="chains")


# ------------------------------------------------------------------------------------------------------------------ placement
@pytest.mark.parametrize("n_cells", [255, 256, 257, 65537])
def test_one_two_and_three_radix_digits(q, lim, n_cells):
    check(q, lim, C.many_cells_case(n_cells)[0], oris=["both"], what=f"{n_cells} cells")


def test_a_cell_interleaved_over_the_input_chunks_keeps_the_input_order(q, lim):
    check(q, lim, C.interleave_case(), what="interleave")


def test_one_cell_takes_more_records_than_a_radix_block_twice_the_same(q, lim):
    c = C.big_cell_case(lim)
    a = check(q, lim, c, oris=["fw"])["fw"][0]
    b = run(q, c, "fw")
    assert a["bytes"].tobytes() == b["bytes"].tobytes() and np.array_equal(a["chunk_off"], b["chunk_off"]) and np.array_equal(a["nrec"], b["nrec"])
    check(q, lim, c, oris=["both"])


# ------------------------------------------------------------------------------------------------------------------ errors, edges
@pytest.mark.parametrize("kind", C.MALFORMED_KINDS)
def test_malformed_chunks_are_refused_with_their_index(q, lim, kind):
    data, off = C.malformed_case(kind)
    for ori in ("both", "fw"):
        with pytest.raises(pkg.AfqError) as e:
            q.collate_multi_rad(data, off, [1], [0], [0], [1], [1], [0], [1], [0], b0_bytes=2, b1_bytes=2, umi_bytes=4, expected_ori=ori)
        assert e.value.code == BAD_INPUT and "chunk 2:" in str(e.value), str(e.value)
    check(q, lim, C.interleave_case(), oris=["both"])   # the context serves again afterwards


def test_no_chunks_no_cells_no_corrections(q, lim):
    got = q.collate_multi_rad(b"", np.zeros(0, np.uint64), [3], [0], [0], [1], [2], [0, 0], [2, 9], [0])
    assert got["bytes"].tobytes() == ((8).to_bytes(4, "little") + bytes(4)) * 2 and got["chunk_off"].tolist() == [0, 8, 16] and got["nrec"].tolist() == [0, 0]
    c = C.interleave_case()
    got = q.collate_multi_rad(c["data"], c["off"], [], [], [], [], [], [], [], [])
    assert len(got["bytes"]) == 0 and got["chunk_off"].tolist() == [0] and got["stats"]["n_unrouted"] == got["stats"]["n_records"] == 13
    got = q.collate_multi_rad(c["data"], c["off"], [21, 22], [1, 2], [], [], [], [1], [7], [0, 0, 1])   # routed, and no correction at all
    assert got["nrec"].tolist() == [0] and got["stats"]["n_uncorrected"] == 13 and got["stats"]["n_unrouted"] == 0 and got["stats"]["out_bytes"] == 8


def test_bad_tables_are_refused_before_the_device_runs(q):
    c = C.interleave_case()
    a = list(C.args(c))
    with pytest.raises(pkg.AfqError) as e:
        q.collate_multi_rad(c["data"], c["off"], *a, b0_bytes=3)
    assert e.value.code == INVALID_ARG
    bad = list(a)
    bad[4] = [99] * len(a[4])   # every correction into a barcode that is no cell
    with pytest.raises(pkg.AfqError) as e:
        q.collate_multi_rad(c["data"], c["off"], *bad)
    assert e.value.code == BAD_INPUT and "not a cell of that sample" in str(e.value)


@pytest.mark.parametrize("al", [0, 3])
def test_device_bytes_inside_a_larger_buffer(q, lim, al):
    """the input already on the device, starting off a dword boundary, with other bytes (all ones) in front of and behind it"""
    import torch

    c = C.long_case("last")
    t = torch.from_numpy(np.frombuffer(b"\xFF" * al + c["data"] + b"\xFF" * 9, np.uint8).copy()).cuda()
    for ori in C.ORIS:
        got = run(q, c, ori, data=None, d_ptr=t.data_ptr() + al, n_bytes=len(c["data"]))
        same(got, C.want(c, ori, lim["lane_alns"]), f"device bytes + {al} {ori}")
        same(run(q, c, ori), C.want(c, ori, lim["lane_alns"]), f"host bytes {ori}")
