"""The device in front of the bootstrap judge (tests/boot_judge.py): the means and variances that pkg.Quantifier returns under
-b, against a plain restatement of em.rs:585-757, multinomial.rs and quant.rs:157-210 over the project's Philox streams that shares
nothing with the oracle or the kernel.  These tests ADD a judge; every bit-for-bit comparison with the oracle stays where it is.

The device's -d class table of a cell is the judge's input and its two bootstrap rows are what is judged: bit for bit where no
label has two ids (the draw stream, the location rule and both summary formulas, with no tolerance at all), under em_judge's bars
and the derived variance bound elsewhere.  tests/test_boot_judge_cpu.py puts the oracle before the same judge on the same cells."""
import numpy as np
import pytest

import boot_judge_cases as bc
import em_judge_cases as ec
from util import pkg

pytestmark = pytest.mark.gpu


def _device(cfg, t2g, data, off, first):
    q = pkg.Quantifier(cfg, np.asarray(t2g, np.uint32))
    try:
        return q.quant_chunks(data, off, first_cell_index=first)
    finally:
        q.close()


@pytest.mark.parametrize("summary_stat", [False, True])
@pytest.mark.parametrize("name,res", [(n, r) for n, r in bc.CASES if n in ("base", "usa", "hand", "hand-usa", "rounds", "rounds-usa")])
def test_bootstraps_are_admitted(name, res, summary_stat):
    """-b 4 on the `base` and `usa` fuzz batches under the three -em resolutions and on the hand and round-control cells, USA and
    not: every cell's rows are the summaries of an admissible combination of the judge's replicates."""
    b = ec.quant_batch(name)
    seed = bc.SEEDS[0]
    got = _device(b.cfg(res, dump_eq=True, num_bootstraps=4, summary_stat=summary_stat, boot_seed=seed), b.t2g, b.data, b.off, bc.FIRST)
    assert got.n_cells == len(b.reads)
    what = f"{name} {res} summary_stat={summary_stat}"
    bc.assert_the_cap(name, bc.judge_result(b, got, 4, summary_stat, seed, bc.FIRST, what), what)


@pytest.mark.parametrize("name", list(bc.EDGE_RUNS))
def test_the_kernels_edges(name):
    """Hand-built cells (boot_judge_cases.edge_batch) at the bootstrap kernel's own edges:
    draws            N = 1, 2, 3, 4, 5, 7, 8 (the tail of a Philox block) and 4095, 4096, 4097, 4100 (the second pass of the
                     1024-thread draw loop); no label has two ids: bit for bit
    classes          K = 1023, 1024, 1025 classes of count 1 to 3 (the second pass of the scan over the cumulative counts): bit for bit
    support          one gene alone, and ambiguous cells of S = 2, 3, 4, 5 ids (the tail of the start stream's block)
    index-exact,     two equal cells submitted with first_cell_index 2^32 - 1: the counter's high word is 0 for one and 1 for the
    index-ambiguous  other; they differ, and neither is the other's
    replicates       B = 1 and B = 2 on one ambiguous cell
    zero-class       a gene whose every class draws 0 in one replicate stays in the support
    tiny-between     a cell on the tiny path between two others has no rows and keeps its place in the cell index
    kernel-limits    the cells of tests/test_gpu_em_edges.py::test_bootstrap_kernel_limits (11 264 / 11 265 classes and support
                     entries, an entry in 32 / 33 classes), whose comparison with the oracle stays there
    each under both summaries."""
    bc.run_edge(name, lambda cfg, b, first: _device(cfg, b.t2g, b.data, b.off, first))
