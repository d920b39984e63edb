"""The extended parsimony sweep (tests/extended_fuzz.py, run by hand for hundreds of seeds) in the suite: fixed seeds of each
of its families - big parsimony cells (0+), every resolution (1000+), the label-tail model (2000+) and the lone-vertex kernel's
per-lane route (3000+) - each under a pool pressure drawn per seed: the product's pool, 12 words per read (the range regrows),
or 12 words per read on a device with room for twice the range's pool (the range is halved).  Device rows == oracle rows, bit
for bit (EM resolutions: in the device's arithmetic)."""
import os

import pytest

from fuzz_workloads import HOOKS, with_pool_pressure, with_random_orientation, workload
from util import assert_same_result, pkg

pytestmark = pytest.mark.gpu

SEEDS = [0, 1, 3, 4, 7, 1002, 1004, 1005, 1011, 1014, 2001, 2005, 2006, 2034, 3000, 3001, 3003]
ORIENTATION_SEEDS = [9, 1008, 1013, 2009, 3005]   # one of every family; their alignment words carry random orientation bits


@pytest.mark.parametrize("seed", SEEDS)
def test_extended_parsimony_sweep(oracle, monkeypatch, seed):
    w = with_pool_pressure(workload(seed), seed)
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in w.env.items():
        monkeypatch.setenv(k, v)
    q = pkg.Quantifier(w.cfg, w.tid_to_gid)
    try:
        got = q.quant_chunks(w.data, w.chunk_off)
    finally:
        q.close()
    want = oracle.quant(w.cfg, w.tid_to_gid, w.data, w.chunk_off, n_threads=min(16, os.cpu_count() or 1))
    assert_same_result(got, want, what=w.what)


@pytest.mark.parametrize("seed", ORIENTATION_SEEDS)
def test_extended_sweep_with_random_orientation_bits(oracle, monkeypatch, seed):
    """Workloads under seeds of their own whose alignment words carry a seeded coin in bit 31: the device on those bytes against
    the oracle on the bytes as built (all bits set)."""
    w = with_pool_pressure(workload(seed), seed)
    want = oracle.quant(w.cfg, w.tid_to_gid, w.data, w.chunk_off, n_threads=min(16, os.cpu_count() or 1))
    w = with_random_orientation(w, seed)
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in w.env.items():
        monkeypatch.setenv(k, v)
    q = pkg.Quantifier(w.cfg, w.tid_to_gid)
    try:
        got = q.quant_chunks(w.data, w.chunk_off)
    finally:
        q.close()
    assert_same_result(got, want, what=w.what)
