"""The workloads of the extended parsimony sweep, in one place: tests/extended_fuzz.py (the long run by hand) and
tests/test_gpu_fuzz_extended.py (fixed seeds of every family, in the suite) both draw them from here.  A workload is a batch,
its configuration and the test hooks it runs under; the caller runs the device and the oracle on it."""
import importlib
from dataclasses import dataclass, field

import numpy as np

from util import pkg

synth = pkg.synth

POOL_HOOKS = ("AFQ_TEST_POOL_WORDS", "AFQ_TEST_POOL_ROOM_WORDS")
HOOKS = ("AFQ_TEST_DECODE", "AFQ_TEST_P2_LONE_COOP", "AFQ_TEST_P2_DEFER_MIN", "AFQ_TEST_P2_GRAPH") + POOL_HOOKS


@dataclass
class Workload:
    cfg: object
    tid_to_gid: np.ndarray
    data: np.ndarray
    chunk_off: np.ndarray
    env: dict = field(default_factory=dict)   # AFQ_TEST_* -> value: the hooks the device runs under (every other one unset)
    what: str = ""
    reads: int = 0


def cell_nrec(data, chunk_off):
    """Reads per cell, out of the chunk headers (u32 nbytes, u32 nrec)."""
    b = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8)
    off = np.asarray(chunk_off, np.uint64).astype(np.int64)
    return np.array([int(b[o + 4:o + 8].view(np.uint32)[0]) for o in off], np.uint64)


def first_pool_words(nrec, cfg, words_per_read):
    """The parsimony pool run_range plans for ONE range of these cells on its first attempt (csrc/afq_api.cpp: words per read
    times the parsimony reads, plus 2^20 words under 24 per read, 2^22 from 24).  Tiny cells (winner-take-all, fewer reads than
    small_thresh) take the cr-like path and no pool."""
    nrec = np.asarray(nrec, np.uint64)
    pug = nrec[nrec >= cfg.small_thresh] if cfg.sa_model == "winner-take-all" else nrec
    return int(words_per_read) * int(pug.sum()) + (1 << 22 if words_per_read >= 24 else 1 << 20)


def room_budget(nrec, cfg, words_per_read=12):
    """An AFQ_TEST_POOL_ROOM_WORDS for a batch of one range: twice the range's first pool - no whole-range regrow (four times)
    fits - but never less than four times the pool of its largest cell alone, so that the no-room re-runs can always end in a
    cell that regrows."""
    big = int(np.max(np.asarray(nrec, np.uint64))) if len(nrec) else 0
    return max(2 * first_pool_words(nrec, cfg, words_per_read), 4 * (words_per_read * big + (1 << 20)))


def with_pool_pressure(w, seed):
    """Per seed, one of: the product's pool (24 words per read); a pool of 12 words per read, which dense graphs outgrow (the range
    runs again with four times as much); the same on a device with room for twice the range's pool only (the range is halved)."""
    kind = int(np.random.default_rng(31000 + seed).integers(0, 3))
    if kind >= 1:
        w.env["AFQ_TEST_POOL_WORDS"] = "12"
    if kind == 2:
        w.env["AFQ_TEST_POOL_ROOM_WORDS"] = str(room_budget(cell_nrec(w.data, w.chunk_off), w.cfg))
    w.what += f" pool={['plain', 'words12', 'words12+room'][kind]}"
    return w


def tailed(seed):
    """Third family (seeds from 2000; from 3000: parsimony with AFQ_TEST_P2_LONE_COOP=2): the bench's label-tail model out of the
    native generator - reads of up to 64 alignments on gene families - through a decoder picked per seed (the planner's choice,
    lane per record, lane per dword) and every resolution."""
    sn = importlib.import_module("alevin-fry_amd.synth_native")
    rng = np.random.default_rng(99000 + seed)
    res = ["cr-like", "cr-like-em", "trivial", "parsimony", "parsimony-em", "cr-like", "cr-like-em"][seed % 7]
    usa = bool(rng.integers(0, 2))
    dec = [None, "recs", "keys", "keys", "keys"][int(rng.integers(0, 5))]
    # Both draws stay, so every seed builds the workload it always did: the first picked a dedup route of the lane-per-dword decoder
    # (one is left); of the second, 0 (a lone-vertex route now gone) leaves the hook unset - the planner's pick.
    rng.integers(0, 2)
    coop = [None, "1", "2"][int(rng.integers(0, 3))]   # k_pl_lone: labels of 5..64 refs by the wave (1); 5..8 refs by the lane in registers, 9..64 by the wave (2)
    if seed >= 3000:   # fourth family: parsimony only, the lone-vertex kernel's per-lane route for labels of 5..8 refs
        res, coop = ["parsimony", "parsimony-em"][seed % 2], "2"
    env = {k: v for k, v in (("AFQ_TEST_DECODE", dec), ("AFQ_TEST_P2_LONE_COOP", coop)) if v is not None}
    d = sn.generate(seed=seed, n_cells=int(rng.choice([8, 40, 150])), median_reads=float(rng.choice([300.0, 2500.0, 9000.0])), sigma=float(rng.choice([0.5, 1.3])),
                    num_genes=int(rng.choice([40, 400, 3000])), txp_per_gene=int(rng.integers(1, 6)), usa=usa, umi_err=float(rng.choice([0.0, 0.02])),
                    tail=float(rng.choice([0.5, 0.65, 0.8, 0.9])), tail_max=int(rng.choice([8, 64])), family=int(rng.choice([4, 8, 16])))
    kw = dict(small_thresh=int(rng.choice([0, 100])))
    if usa and rng.integers(0, 2):
        kw["sa_model"] = "prefer-ambig"
    cfg = pkg.WorkerConfig.for_resolution(res, usa_mode=usa, num_genes=d.num_genes, num_rows=d.num_rows, umi_len=12, **kw)
    return Workload(cfg, d.tid_to_gid, d.data, d.chunk_off, env,
                    f"seed {seed} {res} usa={usa} decoder={dec} lone_coop={coop} {kw} cells={len(d.chunk_off)}", int(d.n_reads))


def big_cells(seed):
    """First family (seeds from 0): parsimony and parsimony-em over bigger cells than tests/test_gpu_fuzz.py - several UMI
    partitions, foreign-partition probes, pool-resident class tables - with skewed and short UMIs and long labels.  Second
    family (seeds from 1000): the same cells under every resolution (gene-level parsimony = the one-workgroup kernel, the
    cr-like routes, EM)."""
    rng = np.random.default_rng(77000 + seed)
    res = ["parsimony", "parsimony-em"][seed % 2]
    if seed >= 1000:
        res = ["trivial", "cr-like", "cr-like-em", "parsimony", "parsimony-em", "parsimony-gene", "parsimony-gene-em"][seed % 7]
    usa = bool(rng.integers(0, 2))
    sizes = [int(x) for x in rng.choice([1, 30, 300, 900, 2500, 6000, 12000], size=int(rng.integers(2, 6)))]
    sizes.append(int(rng.choice([15000, 30000, 45000, 70000])))
    if seed % 7 == 0:
        sizes.append(int(rng.integers(90000, 130000)))
    s = synth.synth(5000 + seed, sizes, num_genes=int(rng.choice([17, 300, 3000])), txp_per_gene=int(rng.integers(1, 5)), usa=usa,
                    dup=float(rng.choice([0.2, 0.5, 0.8])), cross=float(rng.choice([0.0, 0.3, 0.9])),
                    umi_err=float(rng.choice([0.0, 0.02, 0.1])), max_extra_na=int(rng.choice([0, 2, 6, 20])),
                    zipf=float(rng.choice([0.0, 0.8, 1.1])), umi_len=int(rng.choice([7, 8, 10, 12])))
    b, off = s.encode()
    kw = dict(small_thresh=int(rng.choice([0, 100])))
    env = {}
    if seed % 3 == 1:   # every third workload: tied components set aside in every cell (k_p2_tied), not only in those whose classes outgrow the LDS table
        env["AFQ_TEST_P2_DEFER_MIN"] = "0"
        env["AFQ_TEST_P2_GRAPH"] = "cell"   # ... through the per-cell graph kernel (by default: the range-wide flat build)
    if rng.integers(0, 4) == 0:
        kw["pug_exact_umi"] = True
    if rng.integers(0, 4) == 0:
        kw["large_graph_thresh"] = int(rng.choice([5, 40, 200]))
    if usa and rng.integers(0, 2):
        kw["sa_model"] = "prefer-ambig"
    if res.endswith("em") and rng.integers(0, 2):
        kw["em_init_uniform"] = True
    cfg = pkg.WorkerConfig.for_resolution(res, usa_mode=usa, num_genes=s.num_genes, num_rows=s.num_rows, umi_len=s.umi_len if rng.integers(0, 2) else 0, **kw)
    return Workload(cfg, s.tid_to_gid, b, off, env, f"seed {seed} {res} usa={usa} {kw} sizes={sizes}", sum(sizes))


def workload(seed):
    return tailed(seed) if seed >= 2000 else big_cells(seed)


def with_random_orientation(w, seed):
    """The workload with bit 31 of every alignment word drawn by a seeded coin (tests/ori_cases.py): `quant` never reads the
    orientation, so the rows are those of the bytes as built."""
    from ori_cases import reorient

    w.data = reorient(w.data, w.chunk_off, "random", 4, 4, seed=seed)
    w.what += " random orientation bits"
    return w
