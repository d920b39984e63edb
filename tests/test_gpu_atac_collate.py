"""GPU tests of the `atac collate` kernels: Quantifier.atac_collate_rad against tests/atac_collate_judge.py on the cases of
tests/atac_collate_cases.py.  Everything is exact: the output bytes, the chunk offsets, the per-chunk record counts, the chunks' cells
and every stat.  Shapes derive from atac_collate_limits()."""
import numpy as np
import pytest

import atac_collate_cases as C
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
    return pkg.atac_collate_limits()


def run(q, c, **kw):
    obs = sorted(c["corrections"])
    return q.atac_collate_rad(c["data"], c["off"], obs, [c["corrections"][b] for b in obs], c["cells"], bc_bytes=c["bc_bytes"], **kw)


def same(got, want, what=""):
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert got["nrec"].tolist() == want["nrec"], (what, "nrec")
    assert got["cell"].tolist() == want["cell"], (what, "cell")
    assert got["chunk_off"].tolist() == want["chunk_off"], (what, "chunk_off")
    gb = got["bytes"].tobytes()
    if gb != want["bytes"]:
        at = next(i for i, (x, y) in enumerate(zip(gb, want["bytes"])) if x != y)
        raise AssertionError((what, "bytes differ first at", at, gb[max(0, at - 8):at + 24].hex(), want["bytes"][max(0, at - 8):at + 24].hex()))


def check(q, c, what=""):
    w = C.want(c)
    got = run(q, c)
    same(got, w, what)
    return got, w


# ------------------------------------------------------------------------------------------------------------------ widths
@pytest.mark.parametrize("bc_bytes", C.WIDTHS)
def test_every_barcode_width(q, bc_bytes):
    got, w = check(q, C.widths_case(bc_bytes), f"bc {bc_bytes}")
    assert w["stats"]["n_kept"] > 20 and w["stats"]["n_cells_out"] > 3


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_chunks_at_unaligned_addresses(q, pad):
    check(q, C.alignment_case(pad), f"pad {pad}")


# ------------------------------------------------------------------------------------------------------------------ tile edges
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_a_kept_head_ending_at_the_tile_edge(q, lim, delta):
    check(q, C.tile_edge_case(lim, delta)[0], f"tile end {delta:+d}")


def test_a_kept_record_on_the_tiles_last_byte(q, lim):
    check(q, C.halo_case(lim)[0], "halo")


@pytest.mark.parametrize("extra", [0, 1])
def test_a_chunk_of_one_tile_and_of_one_tile_and_a_byte(q, lim, extra):
    check(q, C.one_tile_chunk_case(lim, extra), f"one tile + {extra}")


@pytest.mark.parametrize("tiles", [1, 2])
def test_a_multi_mapped_record_longer_than_tiles_is_hopped(q, lim, tiles):
    got, w = check(q, C.long_record_case(lim, tiles)[0], f"long {tiles}")
    assert w["stats"]["n_multimapped"] == 3 and w["stats"]["n_kept"] == 104


def test_na_zero_one_two(q):
    check(q, C.na_case(), "na")


def test_no_chunks_no_cells_no_map(q):
    got = q.atac_collate_rad(b"", np.zeros(0, np.uint64), [], [], [5, 6], bc_bytes=4)
    assert len(got["bytes"]) == 0 and got["chunk_off"].tolist() == [0] and len(got["nrec"]) == 0 and len(got["cell"]) == 0
    assert got["stats"] == dict(n_records=0, n_unmapped=0, n_multimapped=0, n_uncorrected=0, n_kept=0, n_cells_out=0, n_cells_empty=2, out_bytes=0)
    c = C.na_case()
    got = q.atac_collate_rad(c["data"], c["off"], [], [], [], bc_bytes=4)
    assert len(got["bytes"]) == 0 and got["chunk_off"].tolist() == [0] and got["stats"]["n_uncorrected"] == 2 and got["stats"]["n_records"] == 5


# ------------------------------------------------------------------------------------------------------------------ placement
@pytest.mark.parametrize("n_cells", [1, 255, 256, 257, 65535, 65536, 65537])
def test_cell_counts_at_the_radix_pass_boundaries(q, n_cells):
    check(q, C.many_cells_case(n_cells), f"{n_cells} cells")


@pytest.mark.parametrize("which", C.EMPTY)
def test_empty_cells_are_absent(q, which):
    c, idle = C.empty_cells_case(which)
    got, w = check(q, c, which)
    assert got["cell"].tolist() == [i for i in range(9) if i not in idle]


def test_all_ones_self_cross_and_many_to_one_corrections(q):
    check(q, C.barcode_case(), "barcodes")


def test_a_probe_chain_of_twelve(q):
    c, chain, where = C.chain_case(16, 12, 4)
    assert len({where[b][0] for b in chain}) == 1
    check(q, c, "chain")


def test_one_cell_holds_all_records(q, lim):
    got, w = check(q, C.skew_case(lim), "skew")
    assert got["nrec"].tolist() == [lim["radix_block"] + 300]


# ------------------------------------------------------------------------------------------------------------------ input routes
@pytest.mark.parametrize("al", [0, 3])
def test_device_bytes_inside_a_larger_buffer(q, lim, al):
    """the input already on the device, starting off a dword boundary, with other bytes (all ones) in front of and behind it: they
    take no part"""
    import torch

    c = C.halo_case(lim)[0]
    t = torch.from_numpy(np.frombuffer(b"\xFF" * al + c["data"] + b"\xFF" * 9, np.uint8).copy()).cuda()
    same(run(q, dict(c, data=None), d_ptr=t.data_ptr() + al, n_bytes=len(c["data"])), C.want(c), f"device bytes + {al}")
    c = C.widths_case(1)
    t = torch.from_numpy(np.frombuffer(b"\xFF" * al + c["data"] + b"\xFF" * 9, np.uint8).copy()).cuda()
    same(run(q, dict(c, data=None), d_ptr=t.data_ptr() + al, n_bytes=len(c["data"])), C.want(c), f"device bytes + {al}, width 1")


def test_two_calls_return_identical_bytes(q, lim):
    c = C.skew_case(lim)
    a, b = run(q, c), run(q, c)
    assert a["bytes"].tobytes() == b["bytes"].tobytes() and all(np.array_equal(a[k], b[k]) for k in ("chunk_off", "nrec", "cell")) and a["stats"] == b["stats"]
    c = C.many_cells_case(257)
    a, b = run(q, c), run(q, c)
    assert a["bytes"].tobytes() == b["bytes"].tobytes()


# ------------------------------------------------------------------------------------------------------------------ errors
@pytest.mark.parametrize("kind", ["head_cut", "alns_cut", "junk", "nrec_low", "nrec_high"])
def test_malformed_chunks_are_refused_with_their_index(q, kind):
    data, off = C.malformed_case(kind)
    with pytest.raises(pkg.AfqError) as e:
        q.atac_collate_rad(data, off, [1], [1], [1], bc_bytes=4)
    assert e.value.code == BAD_INPUT and "chunk 2:" in str(e.value), str(e.value)
    check(q, C.na_case(), "after " + kind)   # the context serves again afterwards


def test_a_record_count_one_too_high_is_refused_by_sentence(q):
    data, off = pkg.rad.encode_atac_chunks([[(5, [(0, 4, 10, 50)]), (8, [])], [(5, [(0, 4, 20, 50)]), (8, [(0, 4, 30, 50)])]], bc_bytes=4)
    o1 = int(off[1])
    bad = data[:o1 + 4] + (3).to_bytes(4, "little") + data[o1 + 8:]   # chunk 1 holds two records and says three
    with pytest.raises(pkg.AfqError) as e:
        q.atac_collate_rad(bad, off, [5, 8], [5, 8], [5, 8], bc_bytes=4)
    assert e.value.code == BAD_INPUT and "chunk 1:" in str(e.value) and "the records do not tile the chunk" in str(e.value), str(e.value)


def test_bad_maps_and_cell_lists_are_refused(q):
    c = C.na_case()
    with pytest.raises(pkg.AfqError) as e:
        q.atac_collate_rad(c["data"], c["off"], [5, 8], [5, 99], [5, 9], bc_bytes=4)
    assert e.value.code == BAD_INPUT and "correction entry 1" in str(e.value) and "99" in str(e.value) and "not a cell" in str(e.value)
    one, off1 = pkg.rad.encode_atac_chunks([[(5, [(0, 4, 10, 50)])]], bc_bytes=4)   # one chunk, one record; cells 1 and 2 are the same barcode
    with pytest.raises(pkg.AfqError) as e:
        q.atac_collate_rad(one, off1, [5], [5], [9, 5, 5], bc_bytes=4)
    assert e.value.code == BAD_INPUT and "cells 1 and 2 carry one barcode (5)" in str(e.value), str(e.value)
    with pytest.raises(pkg.AfqError) as e:
        q.atac_collate_rad(c["data"], c["off"], [5, 8, 5], [5, 8, 8], [5, 8], bc_bytes=4)
    assert e.value.code == BAD_INPUT and "two different corrected barcodes" in str(e.value)
    with pytest.raises(pkg.AfqError) as e:
        q.atac_collate_rad(c["data"], c["off"], [C.ONES, C.ONES], [5, 8], [5, 8], bc_bytes=8)
    assert e.value.code == BAD_INPUT and "two different corrected barcodes" in str(e.value)
    with pytest.raises(pkg.AfqError) as e:
        q.atac_collate_rad(c["data"], c["off"], [5], [5], [5, 5], bc_bytes=4)
    assert e.value.code == BAD_INPUT and "one barcode" in str(e.value)
    with pytest.raises(pkg.AfqError) as e:
        q.atac_collate_rad(c["data"], c["off"], [5], [5], [5], bc_bytes=3)
    assert e.value.code == INVALID_ARG
    off = c["off"].copy()
    off[0] = len(c["data"]) - 4
    with pytest.raises(pkg.AfqError) as e:
        q.atac_collate_rad(c["data"], off, [5], [5], [5], bc_bytes=4)
    assert e.value.code == BAD_INPUT and "chunk 0" in str(e.value)
    q.atac_collate_rad(c["data"], c["off"], [5, 5], [5, 5], [5], bc_bytes=4)   # the same pair twice is no conflict
    check(q, c, "after the refusals")
