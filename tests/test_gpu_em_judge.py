"""The device in front of the EM judge (tests/em_judge.py): the rows that pkg.Quantifier returns under the three -em resolutions and
from `infer`, against a float64 statement of the reference's EM that shares nothing with the oracle or the kernels.  These tests
ADD a judge; every comparison with the oracle stays where it is (tests/test_gpu_em.py, tests/test_gpu_em_edges.py).

For `quant` the judgement is end to end and without the oracle: the device's -d class table of a cell goes before
tests/quant_judge.py (reads -> classes), and its row before the EM judge on that table (classes -> row), under the project's 1e-4
and under the tight bar of 2 K units of 2^-24 (em_judge.TIGHT_BAR, valid for these batches).  tests/test_em_judge_cpu.py puts the
oracle before the same judge on the same cells."""
import numpy as np
import pytest

import em_edges as E
import em_judge as ej
import em_judge_cases as ec
from util import pkg

pytestmark = pytest.mark.gpu


def _device(cfg, t2g, data, off):
    q = pkg.Quantifier(cfg, np.asarray(t2g, np.uint32))
    try:
        return q.quant_chunks(data, off), q.em_instance_counts()
    finally:
        q.close()


def _judge_device(name, res, what, init="informative"):
    b = ec.quant_batch(name)
    got, counts = _device(b.cfg(res, dump_eq=True, em_init_uniform=init == "uniform"), b.t2g, b.data, b.off)
    ec.judge_end_to_end(b, res, got, init, what)
    return counts


@pytest.mark.parametrize("name,res", ec.QUANT_CASES)
def test_quant_rows_are_admitted_end_to_end(name, res):
    """cr-like-em, parsimony-em, parsimony-gene-em, USA and not: the fuzz batches, the `_workload` cells of tests/test_gpu_em.py
    (30 000 reads down to the tiny path), and under cr-like-em the round-control cells and the hand cells."""
    _judge_device(name, res, f"{name} {res}")


@pytest.mark.parametrize("tier", [0, 1, 2, 3, 4, "4-wide-ids"])
@pytest.mark.parametrize("name", ["workload", "workload-usa"])
def test_every_instance_of_the_rounds_kernel(monkeypatch, name, tier):
    """AFQ_TEST_EM2_MIN_TIER sends every cell to the given instance of the rounds kernel or a larger one, AFQ_TEST_EM2_WIDE_IDS
    down tier 4's 32-bit route (tests/test_gpu_em.py): the counter says where the cells went, the judge what came out."""
    if tier == "4-wide-ids":
        monkeypatch.setenv("AFQ_TEST_EM2_WIDE_IDS", "1")
        tier = 4
    monkeypatch.setenv("AFQ_TEST_EM2_MIN_TIER", str(tier))
    counts = _judge_device(name, "parsimony-em", f"{name} parsimony-em tier {tier}")
    assert sum(counts[:tier]) == 0 and sum(counts[tier:5]) > 0, counts


@pytest.mark.parametrize("name,res", [(n, r) for n, r in ec.QUANT_CASES if n not in ("base", "wide", "deep")])
def test_sequential_kernels(monkeypatch, name, res):
    """AFQ_EM_ORDER=canonical: the f32 sums in class order (csrc/afq_em.hip); no order-free instance runs."""
    monkeypatch.setenv("AFQ_EM_ORDER", "canonical")
    assert _judge_device(name, res, f"{name} {res} canonical") == [0] * 6


@pytest.mark.parametrize("name", ["usa", "workload", "workload-usa", "rounds", "rounds-usa", "hand", "hand-usa"])
def test_uniform_initialisation(name):
    """--init-uniform: every alpha of the support starts at 1 / num_alphas (em.rs:369-375, 518-523)."""
    _judge_device(name, "cr-like-em", f"{name} cr-like-em uniform", init="uniform")


@pytest.mark.parametrize("name", ec.INFER_BATCHES)
def test_infer_rows_are_admitted(name):
    """`Quantifier.infer` on class tables in EM labels: the round-control cells, the hand cells (the one that tells the dense from
    the subset loop among them, and a class of count 0) and the reference's own unit-test cells.  The judge's subset loop applies
    with USA and without (infer.rs:230)."""
    b = ec.infer_batch(name)
    num_genes = 2 * (b.num_rows // 3) if b.usa else b.num_rows
    eq_labels, cells = b.for_device()
    q = pkg.Quantifier(E.cfg("cr-like", b.usa, num_genes, b.num_rows), np.arange(num_genes, dtype=np.uint32))
    try:
        got = q.infer(eq_labels, cells, b.num_rows, usa_mode=b.usa)
    finally:
        q.close()
    assert got.n_cells == len(b.rows)
    judged = []
    for i, (cell, row) in enumerate(zip(b.names, b.rows)):
        o, u = ec.judge_table(row, b.num_rows, b.usa, "subset")
        judged.append((o, u))
        g, v = got.row(i)
        dev = list(zip(g.tolist(), v.tolist()))
        m = ej.admits(o, dev)
        assert m is True, f"infer {name} {cell} ({len(o)} outcome(s)): {m}"
        if cell == "dense-and-subset-differ":       # what tells `infer` from `quant` without USA: the dense loop's row is not this one
            dense, _ = ec.judge_table(row, b.num_rows, False, "dense")
            assert isinstance(ej.admits(dense, dev), str)
    ec.assert_the_judge_judges(judged, f"infer {name}")
