"""The builders of tests/em_edges.py without a device: the mirror of k_em2_setup puts each sweep's cells on both sides of
its limit, the oracle sees the classes the builders meant (one ambiguous molecule per multi-gene read), and the
round-control cells stop where their constants say."""
import os

import numpy as np
import pytest

import em_edges as E

NT = min(16, os.cpu_count() or 1)


@pytest.mark.parametrize("usa", [False, True])
def test_placement_sweeps_straddle_their_limits(usa):
    limits = {"t0_words": lambda s: s.all - E.T0_WORDS, "t0_entries": lambda s: s.L - E.T0_ENTRIES,
              "t1_words": lambda s: s.all - E.T1_WORDS, "t1_entries": lambda s: s.L - E.T1_ENTRIES,
              "t2_words": lambda s: s.all - E.T2_WORDS, "t3_core": lambda s: s.core - E.T2_WORDS,
              "narrow_ids": lambda s: s.L + s.P + 2 - E.NARROW_IDS}
    for name, (G, cells) in E.placement_sweeps(usa).items():
        shapes = [E.em2_shape(c, G, usa) for c in cells]
        assert ([s.tier for s in shapes], [s.wide for s in shapes]) == E.EXPECTED_PLACEMENT[usa][name], name
        d = [limits[name](s) for s in shapes]
        assert d[0] < 0 and d[-1] == 1 and max(d[:-1]) <= 0, (name, d)   # under, at (where the arithmetic allows it), one over
        if name not in ("t3_core",) or usa:
            assert d[1] == 0, (name, d)


@pytest.mark.parametrize("usa", [False, True])
def test_builders_give_the_classes_they_mean(oracle_module, usa):
    """The oracle's -d classes of a small sweep cell and the round-control cells are the builders' labels and counts."""
    G, cells = E.placement_sweeps(usa)["t0_entries"]
    for G, cells in ((G, cells[:1]), (4, E.round_cells(usa))):
        b, off, t2g, ng, nr = E.encode(cells, G, usa)
        r = oracle_module.quant(E.cfg("cr-like-em", usa, ng, nr, dump_eq=True), t2g, b, off)
        for i, c in enumerate(cells):
            assert {tuple(int(x) for x in lab): int(n) for lab, n in r.eqclasses.cell(i)} == E.gene_classes(c, G, usa)


@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("arith", ["fixed", "reference"])
def test_round_control_cells_stop_where_their_constants_say(oracle_module, usa, arith):
    G = 4
    cells = E.round_cells(usa, G)
    b, off, t2g, ng, nr = E.encode(cells, G, usa)
    r, iters = oracle_module.quant(E.cfg("cr-like-em", usa, ng, nr), t2g, b, off, want_iters=True, em_arith=arith)
    assert [int(x) for x in iters[: len(E.ROUND_CELLS[usa])]] == [it for *_, it in E.ROUND_CELLS[usa]]
    for (n, uA, uB, it), _ in zip(E.ROUND_CELLS[usa], cells):
        if it == 100:   # the cap, not a convergence at round 100: the last rounds still move by more than the tolerance
            assert min(E.two_entry_em_f64(n, uA, uB, 100)[-3:]) > 0.1
    if usa:   # the floor round zeroes S_1 (a sibling A_1 reads) while A_1 survives
        g, v = r.row(len(cells) - 1)
        assert 1 not in g.tolist() and 2 * G + 1 in g.tolist()


@pytest.mark.parametrize("usa", [False, True])
def test_hot_set_cell_cuts_inside_one_degree(usa):
    G = 16100
    cell = E.hot_set_cell(usa, G)
    t, extra, n_at_t, n_over_63, cap = E.hot_cut(cell, G, usa)
    assert E.em2_shape(cell, G, usa).tier == 4
    assert 0 < extra < n_at_t and n_over_63 > 0, (t, extra, n_at_t, n_over_63, cap)


def test_bootstrap_cells_sit_at_the_kernel_limits():
    G = E.BOOT_LDS + 8
    for k in (E.BOOT_LDS, E.BOOT_LDS + 1):
        assert len(E.gene_classes(E.boot_classes_cell(k), G, False)) == k
        assert len(set(x for l in E.gene_classes(E.boot_support_cell(k), G, False) for x in l)) == k
    for k in (E.BOOT_HEAVY, E.BOOT_HEAVY + 1):
        assert sum(0 in lab for lab in E.gene_classes(E.boot_heavy_cell(k), G, False)) == k
