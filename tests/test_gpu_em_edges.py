"""The order-free EM (csrc/afq_em2.hip) and the bootstrap kernel (csrc/afq_em.hip k_boot) on hand-built cells at their limits:
each rounds instance's LDS word budget and register-array entries, the streamed / hot-set core limit, the 16-bit id limit,
tier 4's hot cut, the round cap and USA's floor round, and k_boot's LDS and heavy-entry limits.  The cells and the mirror of
k_em2_setup's choice are in tests/em_edges.py; afq_em_instance_counts shows where each cell went, so a change that moves a
limit fails here instead of leaving these cells off the edge they were built for."""
import os

import numpy as np
import pytest

import em_edges as E
from util import assert_same_result, pkg

pytestmark = pytest.mark.gpu
NT = min(16, os.cpu_count() or 1)


def _device(cfg, t2g, b, off):
    q = pkg.Quantifier(cfg, t2g)
    try:
        return q.quant_chunks(b, off), q.em_instance_counts()
    finally:
        q.close()


def _within_1e4(got, want, what):
    assert np.array_equal(got.cell_ptr, want.cell_ptr) and np.array_equal(got.gene, want.gene), what
    np.testing.assert_allclose(got.val, want.val, rtol=1e-4, atol=0, err_msg=what)


def _same_bootstraps(got, want, what):
    gb, wb = got.bootstraps, want.bootstraps
    for name in ("mean_ptr", "mean_col", "var_ptr", "var_col"):
        assert np.array_equal(getattr(gb, name), getattr(wb, name)), f"{what} {name}"
    assert np.array_equal(gb.mean_val.view(np.uint32), wb.mean_val.view(np.uint32)), what
    assert np.array_equal(gb.var_val.view(np.uint32), wb.var_val.view(np.uint32)), what


@pytest.mark.parametrize("limit", list(E.EXPECTED_PLACEMENT[False]))
@pytest.mark.parametrize("usa", [False, True])
def test_cells_across_each_instance_limit(oracle_module, limit, usa):
    """Three cells per limit (one unit under it, at it, one over): the counter reports the instances the mirror names, and the
    rows are the fixed-point oracle's bit for bit and within 1e-4 of the reference arithmetic."""
    G, cells = E.placement_sweeps(usa)[limit]
    shapes = [E.em2_shape(c, G, usa) for c in cells]
    assert ([s.tier for s in shapes], [s.wide for s in shapes]) == E.EXPECTED_PLACEMENT[usa][limit]
    b, off, t2g, ng, nr = E.encode(cells, G, usa)
    cfg = E.cfg("cr-like-em", usa, ng, nr)
    got, counts = _device(cfg, t2g, b, off)
    assert counts == E.instance_counts(shapes), f"{limit} usa={usa}: device {counts}, mirror {[(s.L, s.P, s.K, s.Wc, s.tier) for s in shapes]}"
    assert_same_result(got, oracle_module.quant(cfg, t2g, b, off, em_arith="fixed", n_threads=NT), what=f"{limit} usa={usa}")
    _within_1e4(got, oracle_module.quant(cfg, t2g, b, off, em_arith="reference", n_threads=NT), f"{limit} usa={usa}")


@pytest.mark.parametrize("usa", [False, True])
def test_tier4_hot_cut_inside_a_group_of_equal_degree(oracle_module, usa):
    """A natural tier 4 cell whose hot set ends inside the entries of one degree, with hub entries in more than 63 labels."""
    G = 16100
    cell = E.hot_set_cell(usa, G)
    t, extra, n_at_t, n_over_63, _ = E.hot_cut(cell, G, usa)
    assert 0 < extra < n_at_t and n_over_63 > 0
    assert E.em2_shape(cell, G, usa).tier == 4
    b, off, t2g, ng, nr = E.encode([cell], G, usa)
    cfg = E.cfg("cr-like-em", usa, ng, nr)
    got, counts = _device(cfg, t2g, b, off)
    assert counts == [0, 0, 0, 0, 1, 0]
    assert_same_result(got, oracle_module.quant(cfg, t2g, b, off, em_arith="fixed", n_threads=NT), what=f"usa={usa}")


def _round_batch(usa):
    G = 4
    cells = E.round_cells(usa, G)
    b, off, t2g, ng, nr = E.encode(cells, G, usa)
    return cells, b, off, t2g, E.cfg("cr-like-em", usa, ng, nr)


@pytest.mark.parametrize("tier", [None, 0, 1, 2, 3, 4])
@pytest.mark.parametrize("usa", [False, True])
def test_round_cap_and_floor_round_in_every_instance(oracle_module, monkeypatch, usa, tier):
    """Cells that stop at round 2 (USA: 3), at the cap of 100 without converging, and (USA) converge at round 100 and run a
    101st; USA also a cell whose floor round zeroes the sibling of a surviving entry.  By default and forced into each
    instance: bit for bit against the fixed-point oracle."""
    if tier is not None:
        monkeypatch.setenv("AFQ_TEST_EM2_MIN_TIER", str(tier))
    cells, b, off, t2g, cfg = _round_batch(usa)
    want, iters = oracle_module.quant(cfg, t2g, b, off, em_arith="fixed", want_iters=True)
    assert [int(x) for x in iters[: len(E.ROUND_CELLS[usa])]] == [r for *_, r in E.ROUND_CELLS[usa]]
    got, counts = _device(cfg, t2g, b, off)
    expect = [0] * 6
    expect[tier or 0] = len(cells)
    assert counts == expect
    assert_same_result(got, want, what=f"usa={usa} tier={tier}")


@pytest.mark.parametrize("usa", [False, True])
def test_round_cap_canonical_order(oracle_module, monkeypatch, usa):
    """AFQ_EM_ORDER=canonical (afq_em.hip k_em_rounds, the reference's f32 sums): the same cells bit for bit against the
    reference arithmetic; no order-free instance runs."""
    monkeypatch.setenv("AFQ_EM_ORDER", "canonical")
    cells, b, off, t2g, cfg = _round_batch(usa)
    got, counts = _device(cfg, t2g, b, off)
    assert counts == [0] * 6
    assert_same_result(got, oracle_module.quant(cfg, t2g, b, off, em_arith="reference"), what=f"usa={usa}")


@pytest.mark.parametrize("summary_stat", [False, True])
@pytest.mark.parametrize("usa", [False, True])
def test_round_cap_bootstraps(oracle_module, usa, summary_stat):
    """-b 4 on the round-control cells (k_boot: one EM per replicate, the same cap and floor round)."""
    cells, b, off, t2g, cfg0 = _round_batch(usa)
    cfg = E.cfg("cr-like-em", usa, cfg0.num_genes, cfg0.num_rows, num_bootstraps=4, summary_stat=summary_stat, boot_seed=0x5EED)
    got, _ = _device(cfg, t2g, b, off)
    want = oracle_module.quant(cfg, t2g, b, off, em_arith="fixed")
    assert_same_result(got, want, what=f"usa={usa}")
    _same_bootstraps(got, want, f"usa={usa} summary_stat={summary_stat}")


@pytest.mark.parametrize("usa", [False, True])
def test_round_cap_infer(oracle_module, usa):
    """`infer` (k_boot<true>) on the round-control cells' classes: the oracle's EM of some row stops at the cap; the device
    rows are the oracle's bit for bit."""
    G = 4
    cells = E.round_cells(usa, G)
    num_rows = 3 * G if usa else G
    uo = G
    ids, rows = {}, []
    for c in cells:
        row = []
        for lab, cnt in E.gene_classes(c, G, usa).items():
            cols = tuple(E.em_label(list(lab), G, usa))   # (gene ids -> output columns, as quant -d writes them)
            row.append((ids.setdefault(cols, len(ids)), cnt))
        rows.append(sorted(row))
    eq_labels = [list(l) for l, _ in sorted(ids.items(), key=lambda kv: kv[1])]
    want = [oracle_module.em([eq_labels[e] for e, _ in row], [n for _, n in row], num_rows,
                             usa_offsets=(uo, 2 * uo) if usa else None, dense=0) for row in rows]
    assert max(it for _, it in want) >= 100
    q = pkg.Quantifier(E.cfg("cr-like", usa, 2 * G if usa else G, num_rows), np.arange(2 * G if usa else G, dtype=np.uint32))
    try:
        got = q.infer(eq_labels, rows, num_rows, usa_mode=usa)
    finally:
        q.close()
    for i, (alphas, _) in enumerate(want):
        nz = np.flatnonzero(alphas > 0)
        g, v = got.row(i)
        assert np.array_equal(g, nz.astype(np.uint32)), i
        assert np.array_equal(v.view(np.uint32), alphas[nz].astype(np.float32).view(np.uint32)), i


@pytest.mark.parametrize("summary_stat", [False, True])
def test_bootstrap_kernel_limits(oracle_module, summary_stat):
    """k_boot: classes at and one past the LDS limit (11 264), a support of that many entries and one more, and an entry in
    exactly 32 and 33 classes (above 32 a wave sums it): bootstrap mean / var bit for bit."""
    G = E.BOOT_LDS + 8
    cells = [E.boot_classes_cell(E.BOOT_LDS), E.boot_classes_cell(E.BOOT_LDS + 1),
             E.boot_support_cell(E.BOOT_LDS), E.boot_support_cell(E.BOOT_LDS + 1),
             E.boot_heavy_cell(E.BOOT_HEAVY), E.boot_heavy_cell(E.BOOT_HEAVY + 1)]
    b, off, t2g, ng, nr = E.encode(cells, G, False)
    cfg = E.cfg("cr-like-em", False, ng, nr, num_bootstraps=4, summary_stat=summary_stat, boot_seed=11)
    got, _ = _device(cfg, t2g, b, off)
    want = oracle_module.quant(cfg, t2g, b, off, em_arith="fixed", n_threads=NT)
    assert_same_result(got, want)
    _same_bootstraps(got, want, f"summary_stat={summary_stat}")
