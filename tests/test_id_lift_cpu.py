"""tests/id_lift.py and the oracle, held to the relabelling identity on the CPU: quant(lifted) == relabel(quant(small)), bit for
bit, for every resolution, both EM arithmetics, USA and not, at the gene-space sizes tests/test_gpu_id_ceilings.py runs on the
device (both sides of 131 072 and 262 144 columns, and the ceiling of 2^20 gene ids / 1 572 864 columns).  The GPU tests lean on
the oracle at sizes no other test reaches and on the helper's maps; this is what says both can be leant on."""
import numpy as np
import pytest

import id_lift
from util import assert_same_result, cfg_for

RESOLUTIONS = ("trivial", "cr-like", "cr-like-em", "parsimony", "parsimony-em", "parsimony-gene", "parsimony-gene-em")
SIZES = {False: [131074, 262146, 1 << 20], True: [43692, 87382, 1 << 19]}   # genes; USA: 131 076, 262 146 and 1 572 864 columns

_small = {}


def _runs(res):
    return ("reference", "fixed") if res.endswith("-em") else ("reference",)


def _quant(ora, s, res, arith):
    b, off = _encoded(s.usa)
    return ora.quant(cfg_for(s, res), s.tid_to_gid, b, off, em_arith=arith)


_enc = {}


def _encoded(usa):
    if usa not in _enc:
        _enc[usa] = id_lift.workload(usa).encode()
    return _enc[usa]


def _small_result(ora, usa, res, arith):
    k = (usa, res, arith)
    if k not in _small:
        _small[k] = _quant(ora, id_lift.workload(usa), res, arith)
    return _small[k]


def test_the_maps_keep_order_siblings_and_sections():
    for usa in (False, True):
        s = id_lift.workload(usa)
        for G_big in SIZES[usa]:
            L = id_lift.lift_genes(s, G_big)
            G = id_lift.SMALL_GENES
            assert L.gene_map[0] < G - 1 and L.gene_map[-1] == G_big - 1   # (the offset is the remainder of the stride's division)
            assert np.all(np.diff(L.gid_map) > 0) and np.all(np.diff(L.col_map) > 0)
            assert L.s.num_rows == (3 * G_big if usa else G_big) and L.s.num_genes == (2 * G_big if usa else G_big)
            assert int(L.s.tid_to_gid.max()) == L.s.num_genes - 1 and L.col_map[-1] == L.s.num_rows - 1
            if usa:
                assert np.array_equal(L.gid_map[0::2] + 1, L.gid_map[1::2]) and np.all(L.gid_map[0::2] % 2 == 0)
                assert np.array_equal(L.col_map[G:2 * G] - L.col_map[:G], np.full(G, G_big))
                assert np.array_equal(L.col_map[2 * G:] - L.col_map[:G], np.full(G, 2 * G_big))
            assert np.array_equal(L.s.refs, s.refs) and np.array_equal(L.s.umi, s.umi)


@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_oracle_of_the_lifted_workload_is_the_relabelled_oracle_of_the_small_one(oracle_module, res, usa):
    s = id_lift.workload(usa)
    for G_big in SIZES[usa]:
        L = id_lift.lift_genes(s, G_big)
        for arith in _runs(res):
            want = L.relabel(_small_result(oracle_module, usa, res, arith), res)
            got = _quant(oracle_module, L.s, res, arith)
            assert_same_result(got, want, what=f"{res} usa={usa} G={G_big} {arith}")
            assert got.val.sum() > 0
            if G_big == SIZES[usa][-1] and res != "trivial":
                assert int(got.gene.max()) == L.s.num_rows - 1   # the workload reaches the last column


def test_lift_refs_changes_no_row(oracle_module):
    s = id_lift.workload(False)
    b, off = s.encode()
    t = id_lift.lift_refs(s, (1 << 16) + 5)
    b2, off2 = t.encode()
    assert int(t.refs.min()) >= (1 << 16) + 5 and len(t.tid_to_gid) == len(s.tid_to_gid) + (1 << 16) + 5
    for res in ("cr-like", "parsimony", "parsimony-em"):
        assert_same_result(oracle_module.quant(cfg_for(t, res), t.tid_to_gid, b2, off2), oracle_module.quant(cfg_for(s, res), s.tid_to_gid, b, off), what=res)
