"""GPU tests of afq_set_collate_compress: collate_rad, collate_multi_rad and atac_collate_rad with the setter on hand "bytes" out as
the snappy frame stream of exactly the bytes they hand out with it off; offsets, counts, cells and every stat stay in uncompressed
coordinates.  The plain call is the reference here (the collate judges hold IT to account in the suites beside this one); the
stream goes before tests/snappy_judge.py and the library's decoder.  Cases come from the collates' own case modules."""

import numpy as np
import pytest

import atac_collate_cases as AC
import collate_cases as CC
import collate_multi_cases as MC
import snappy_judge as sj
from test_gpu_snappy import lib_decode
from util import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def q():
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    qq = pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)
    yield qq
    qq.close()


@pytest.fixture(scope="module")
def B():
    return pkg.afquant.snappy_limits()["block"]


def run_collate(q, c, ori="both"):
    obs = sorted(c["corrections"])
    q.set_aln_extra_bytes(c["pos_bytes"])
    try:
        return q.collate_rad(c["data"], c["off"], obs, [c["corrections"][b] for b in obs], c["cells"], bc_bytes=c["bc_bytes"], umi_bytes=c["umi_bytes"], expected_ori=ori)
    finally:
        q.set_aln_extra_bytes(0)


def run_multi(q, c, ori="both"):
    q.set_aln_extra_bytes(c["pos_bytes"])
    try:
        return q.collate_multi_rad(c["data"], c["off"], *MC.args(c), b0_bytes=c["b0_bytes"], b1_bytes=c["b1_bytes"], umi_bytes=c["umi_bytes"], expected_ori=ori)
    finally:
        q.set_aln_extra_bytes(0)


def run_atac(q, c):
    obs = sorted(c["corrections"])
    return q.atac_collate_rad(c["data"], c["off"], obs, [c["corrections"][b] for b in obs], c["cells"], bc_bytes=c["bc_bytes"])


def off_on_off(q, B, run, what):
    """setter off, on, off again on one context -> the plain result"""
    plain = run()
    q.set_collate_compress(True)
    try:
        sz = run()
    finally:
        q.set_collate_compress(False)
    again = run()
    want = plain["bytes"].tobytes()
    stream = sz["bytes"].tobytes()
    s = sj.decode(stream)
    assert s.data == want, (what, "the judge decodes other bytes than the plain call's")
    assert lib_decode(stream, len(want)) == want, (what, "the library decodes other bytes than the plain call's")
    assert stream[:10] == sj.STREAM_ID and s.n_chunks == -(-len(want) // B) and len(stream) <= 10 + len(want) + 8 * s.n_chunks, what
    for k in plain:
        if k == "bytes":
            continue
        if k == "stats":
            assert sz[k] == plain[k] and again[k] == plain[k], (what, k, sz[k], plain[k])
            assert plain[k]["out_bytes"] == len(want), what
        else:
            assert np.array_equal(sz[k], plain[k]) and np.array_equal(again[k], plain[k]), (what, k)
    assert again["bytes"].tobytes() == want, (what, "setter off again: not the plain bytes")
    return plain, s


# ------------------------------------------------------------------------------------------------------------------ collate
def collate_cases(lim):
    big = CC.big_cell_case(lim)
    return {
        "widths 4 4 4": CC.widths_case(4, 4, 4), "widths 1 8 0": CC.widths_case(1, 8, 0), "unaligned 3": CC.alignment_case(3),
        "tile edge -1": CC.tile_edge_case(lim, -1), "tile edge 0": CC.tile_edge_case(lim, 0), "tile edge +1": CC.tile_edge_case(lim, 1),
        "one tile + 1": CC.one_tile_chunk_case(lim, 1), "interleave": CC.interleave_case(), "corrected": CC.corrected_case(),
        "257 cells": CC.many_cells_case(257), "radix block + 100": big,
        "no cell": CC.case(big["chunks"][:1], {}, [], 4, 4, 0),
        "cells, none kept": CC.case(CC.interleave_case()["chunks"], {100: 100, 101: 101}, [101, 100], 4, 4, 0),
        "one kept record": CC.case([[(7, 1, [(3, True)]), (8, 2, [(4, False)])]], {7: 7, 9: 9}, [9, 7], 4, 4, 0),
    }


def test_collate(q, B):
    lim = pkg.collate_limits()
    spans = set()
    for what, c in collate_cases(lim).items():
        for ori in (("both", "fw") if what.startswith("widths") else ("both",)):
            plain, s = off_on_off(q, B, lambda: run_collate(q, c, ori), f"collate {what} {ori}")
            spans.add(s.n_chunks)
            if what == "no cell":
                assert len(plain["bytes"]) == 0 and s.n_chunks == 0
            if what == "cells, none kept":
                assert plain["stats"]["n_kept"] == 0 and len(plain["bytes"]) == 16 and plain["nrec"].tolist() == [0, 0]
            if what == "one kept record":
                assert plain["stats"]["n_kept"] == 1 and plain["nrec"].tolist() == [0, 1]
            if what == "radix block + 100":
                assert s.n_chunks > 2 and s.n_stored == 0
    assert {0, 1} <= spans and max(spans) > 2


# ------------------------------------------------------------------------------------------------------------------ multi-barcode collate
def multi_cases(lim):
    n = 2 * lim["radix_block"] + 100
    recs = [(5, i % 7, i, [(i, True)] * (i % 3)) for i in range(n)]
    cut = lim["radix_block"] - 7
    inter = MC.interleave_case()
    return {
        "widths 2 4 4": MC.widths_case(2, 4, 4), "unaligned 1": MC.alignment_case(1), "tile edge 0": MC.tile_edge_case(lim, 0)[0],
        "tile edge +1": MC.tile_edge_case(lim, 1)[0], "one tile": MC.one_tile_chunk_case(lim), "interleave": inter, "257 cells": MC.many_cells_case(257)[0],
        "radix block + 100": MC.big_cell_case(lim),
        "two radix blocks": MC.case([recs[:cut], recs[cut:]], {5: 1}, {(1, b): 3 for b in range(7)}, [(1, 3), (1, 4)], 2, 1, 1, 4),
        "no cell": MC.case(inter["chunks"], {21: 1, 22: 2}, {}, [], 3),
        "cells, none kept": MC.case(inter["chunks"], {21: 1, 22: 2}, {(1, 100): 100}, [(1, 100), (2, 100)], 3),
        "one kept record": MC.case([[(21, 7, 1, [(3, True)]), (21, 8, 2, [(4, False)])]], {21: 1}, {(1, 7): 7}, [(1, 9), (1, 7)], 2),
    }


def test_collate_multi(q, B):
    lim = pkg.collate_multi_limits()
    spans = set()
    for what, c in multi_cases(lim).items():
        plain, s = off_on_off(q, B, lambda: run_multi(q, c), f"collate multi {what}")
        spans.add(s.n_chunks)
        if what == "no cell":
            assert len(plain["bytes"]) == 0 and s.n_chunks == 0
        if what == "cells, none kept":
            assert plain["stats"]["n_kept"] == 0 and len(plain["bytes"]) == 16
        if what == "one kept record":
            assert plain["stats"]["n_kept"] == 1 and plain["nrec"].tolist() == [0, 1]
        if what == "two radix blocks":
            assert s.n_chunks > 2
    assert {0, 1} <= spans and max(spans) > 2


# ------------------------------------------------------------------------------------------------------------------ atac collate
def atac_cases(lim):
    return {
        "widths 4": AC.widths_case(4), "widths 8": AC.widths_case(8), "unaligned 3": AC.alignment_case(3), "tile edge -1": AC.tile_edge_case(lim, -1)[0],
        "tile edge 0": AC.tile_edge_case(lim, 0)[0], "tile edge +1": AC.tile_edge_case(lim, 1)[0], "halo": AC.halo_case(lim)[0],
        "one tile + 1": AC.one_tile_chunk_case(lim, 1), "257 cells": AC.many_cells_case(257), "every second cell empty": AC.empty_cells_case("every second")[0],
        "radix block + 300": AC.skew_case(lim),
        "no cell": AC.case(AC.na_case()["chunks"], {}, [], 4),
        "cells, none kept": AC.empty_cells_case("all")[0],
        "one kept record": AC.case([[(5, AC.Alns(1).many(1)), (6, AC.Alns(2).many(1)), (5, AC.Alns(3).many(2))]], {5: 5, 9: 9}, [9, 5], 4),
    }


def test_atac_collate(q, B):
    lim = pkg.atac_collate_limits()
    spans = set()
    for what, c in atac_cases(lim).items():
        plain, s = off_on_off(q, B, lambda: run_atac(q, c), f"atac collate {what}")
        spans.add(s.n_chunks)
        if what in ("no cell", "cells, none kept"):   # no chunk at all: the stream is the identifier alone
            assert len(plain["bytes"]) == 0 and s.n_chunks == 0 and plain["stats"]["n_kept"] == 0 and plain["stats"]["n_records"] > 0
        if what == "one kept record":
            assert plain["stats"]["n_kept"] == 1 and plain["nrec"].tolist() == [1] and plain["cell"].tolist() == [1]
        if what == "radix block + 300":
            assert s.n_chunks > 2 and s.n_stored == 0
    assert {0, 1} <= spans and max(spans) > 2


def test_the_compressed_stream_is_the_encoders_own(q, B):
    """what the setter hands out is afq_snappy_frame_encode's stream of the plain bytes, byte for byte"""
    c = CC.big_cell_case(pkg.collate_limits())
    plain = run_collate(q, c)
    q.set_collate_compress(True)
    try:
        sz = run_collate(q, c)
    finally:
        q.set_collate_compress(False)
    stream, st = q.snappy_frame_encode(plain["bytes"])
    assert sz["bytes"].tobytes() == stream and st["n_blocks_stored"] == 0 and len(stream) < len(plain["bytes"]) // 2
