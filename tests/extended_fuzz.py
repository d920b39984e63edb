"""One-off extended parity sweep of the parsimony phase kernels (not collected by pytest: run it on a GPU box,
`python tests/extended_fuzz.py [n_seeds] [first_seed]`).  Bigger cells than tests/test_gpu_fuzz.py (several UMI partitions,
foreign-partition probes, pool-resident class tables), skewed and short UMIs, long labels; device rows == oracle rows.
The workloads are tests/fuzz_workloads.py's; tests/test_gpu_fuzz_extended.py runs fixed seeds of each family in the suite."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fuzz_workloads import HOOKS, workload  # noqa: E402
from util import assert_same_result, pkg  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle as ora  # noqa: E402


def one(seed):
    w = workload(seed)
    for k in HOOKS:
        os.environ.pop(k, None)
    os.environ.update(w.env)
    q = pkg.Quantifier(w.cfg, w.tid_to_gid)
    try:
        got = q.quant_chunks(w.data, w.chunk_off)
        rehash = q.label_rehash_count()
        one.mono += q.mono_cell_count()
        one.regrow += q.pool_regrow_count()
    finally:
        q.close()
        for k in HOOKS:
            os.environ.pop(k, None)
    # (EM resolutions: the oracle in the device's order-free fixed-point arithmetic - bit-identical by construction)
    want = ora.quant(w.cfg, w.tid_to_gid, w.data, w.chunk_off, n_threads=os.cpu_count() or 1, em_arith="reference" if os.environ.get("AFQ_EM_ORDER") == "canonical" else "fixed")
    assert_same_result(got, want, what=w.what)
    return w.reads, rehash


one.mono = one.regrow = 0


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    bad, reads, t0 = 0, 0, time.time()
    for seed in range(first, first + n):
        try:
            r, rh = one(seed)
            reads += r
            if rh:
                print(f"seed {seed}: {rh} range(s) re-keyed", flush=True)
        except Exception as e:   # noqa: BLE001
            bad += 1
            print(f"seed {seed} FAILED: {type(e).__name__}: {str(e)[:300]}", flush=True)
    print(f"extended fuzz: {n} workloads, {reads} reads, {bad} failures, {one.mono} cells through the one-workgroup kernel, {one.regrow} pool re-grows, {time.time() - t0:.0f} s")
    sys.exit(1 if bad else 0)
