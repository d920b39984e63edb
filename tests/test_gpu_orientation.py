"""Quant with the orientation bit of the alignment words clear and mixed, not only set.

An alignment word is `orientation << 31 | ref_id` and the reference's quant never reads the orientation.  The
device keeps a record's raw words in HBM and masks them where it uses them; every other quant input of this suite has the bit set
on every word, where a forgotten mask cannot show.  Here every case takes bytes that an existing builder made (the TWIN, all set),
rewrites bit 31 by one of tests/ori_cases.py's patterns and states two things:

  1. the device on the rewritten bytes is bit-identical to the device on the twin - rows, barcodes, nrec, flags, -d classes,
     bootstraps, the batch's counters, the rehash and divert counts;
  2. the rewritten run stands before tests/quant_judge.py as tests/test_gpu_quant_judge.py puts the twin there: exact where there
     is one outcome, admitted where there are several, class tables for the -em resolutions.  The judge takes ref ids.

tests/test_ori_cases_cpu.py checks on the CPU that the rewrite changes nothing else, that the cases hold the mixed pairs they are
for, and that the oracle gives the twin's result."""
import gzip
import json
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

import ori_cases as oc
import quant_judge as qj
import quant_judge_cases as qc
from pug_routes import PUG_ROUTES, set_pug_route
from util import assert_same_result, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
CLI = os.path.join(pkg.__path__[0], "csrc", "afquant")

DECODE_ROUTES = {"as-planned": {}, "decode-recs": {"AFQ_TEST_DECODE": "recs"}, "decode-keys": {"AFQ_TEST_DECODE": "keys"}}
BUCKET_ROUTES = {"slab-cap-8": {"AFQ_TEST_SLAB_CAP": "8"}, "divert-all": {"AFQ_TEST_RESOLVE_DIVERT": "all"}}
COUNTERS = ("n_records", "n_ref_words", "n_keys", "n_buckets", "n_overflow_buckets")
Run = namedtuple("Run", "got stats rehash divert ranges")
_twins = {}


def device(cfg, t2g, case, how="submit"):
    q = pkg.Quantifier(cfg, np.asarray(t2g, np.uint32), aln_extra_bytes=case.pos_bytes)
    try:
        if how == "submit":
            q.submit(case.data, case.off)
        else:
            import torch

            h = torch.from_numpy(case.data.copy())
            h = h.pin_memory() if how == "pinned" else h.cuda()
            if how == "pinned":
                q.submit_ptr(h.data_ptr(), h.numel(), case.off)
            else:
                q.submit_device(h.data_ptr(), h.numel(), case.off)
                torch.cuda.synchronize()
        got = q.collect()
        return Run(got, q.batch_stats(), q.label_rehash_count(), q.resolve_divert_count(), q.range_pipeline_counts()[0])
    finally:
        q.close()


def same_as_twin(new, twin, cfg, what, rehash=True):
    a, b = new.got, twin.got
    assert_same_result(a, b, what=what)
    if cfg.dump_eq:
        for f in ("cell_ptr", "label_ptr", "labels", "count"):
            assert np.array_equal(getattr(a.eqclasses, f), getattr(b.eqclasses, f)), f"{what}: class tables, {f}"
    if cfg.num_bootstraps:
        for f in ("mean_ptr", "mean_col", "var_ptr", "var_col"):
            assert np.array_equal(getattr(a.bootstraps, f), getattr(b.bootstraps, f)), f"{what}: bootstraps, {f}"
        for f in ("mean_val", "var_val"):
            assert np.array_equal(getattr(a.bootstraps, f).view(np.uint32), getattr(b.bootstraps, f).view(np.uint32)), f"{what}: bootstraps, {f}"
    assert {k: new.stats[k] for k in COUNTERS} == {k: twin.stats[k] for k in COUNTERS}, what
    assert new.divert == twin.divert and (new.rehash == twin.rehash or not rehash), what


def judge(got, reads, js, what, classes=False, one_outcome=False, min_judged=0.99):
    """Every judged cell is admitted, and at least min_judged of the cells are judged (a cell is left out where the judge is
    undecided or - parsimony, above oc.PARSIMONY_JUDGE_CAP reads - was not asked)."""
    assert got.n_cells == len(js) == len(reads) and [int(x) for x in got.nrec] == [len(r) for r in reads], what
    rows, tables, flags = (None, qc.classes_of(got), got.flags.tolist()) if classes else (qc.rows_of(got), None, got.flags.tolist())
    n = 0
    for i, j in enumerate(js):
        if j is None or j.undecided:
            continue
        assert not one_outcome or len(j.outcomes) == 1, what
        m = qj.admits(j, None if classes else rows[i], classes=tables[i] if classes else None, flags=flags[i])
        assert m is True, f"{what}, cell {i} ({len(j.outcomes)} outcome(s)): {m}; reads {reads[i][:40]}"
        n += 1
    assert n >= min_judged * len(js) and n > 0, (what, n, len(js))
    return n


def check(monkeypatch, name, res_case, pattern, em=False, boots=False, env=None, how="submit", seed=0, min_judged=0.99, rehash=True, **switches):
    """One case: the input `name` under RES_CASES[res_case] (em: its -em sibling with -d classes; boots: three bootstraps under a
    fixed seed) with its bits rewritten by `pattern`, against its twin and before the judge.  `switches` go to the configuration
    and to the judge alike.  The twin's run is made once per configuration and route and shared."""
    inp = oc.inputs(name)
    env = {**inp.env, **(env or {})}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    res, ckw, _ = oc.RES_CASES[res_case]
    kw = dict(ckw, **switches)
    if em:
        res = qc.EM_OF[res]
        kw.update(dump_eq=True)
        if boots:
            kw.update(num_bootstraps=3, boot_seed=41)
    cfg = inp.cfg(res, **kw)
    key = (name, res, tuple(sorted(kw.items())), tuple(sorted(env.items())))
    if key not in _twins:
        _twins[key] = device(cfg, inp.t2g, inp.twin)
    twin = _twins[key]
    new = device(cfg, inp.t2g, inp.rewritten(pattern, seed), how)
    what = f"{name} {res} {kw} {env} {how} {pattern}"
    same_as_twin(new, twin, cfg, what, rehash)
    assert new.stats["n_records"] == sum(len(r) for r in inp.reads), what
    judge(new.got, inp.reads, inp.judgements(res_case, **switches), what, classes=em, one_outcome=res_case in qc.INTEGER_EXACT, min_judged=min_judged)
    return new, twin


# ---------------------------------------------------------------------------------------------------------- integer-exact rules

@pytest.mark.parametrize("pattern", ["clear", "per-read", "random"])
@pytest.mark.parametrize("route", list(DECODE_ROUTES))
@pytest.mark.parametrize("case", ["cr-like", "prefer-ambig", "trivial"])
@pytest.mark.parametrize("name", ["base", "usa"])
def test_integer_exact_rules(monkeypatch, name, case, route, pattern):
    """cr-like, prefer-ambig and trivial on the fuzz batches, as planned and through each walk-free decoder.  Under per-read and
    random thousands of reads of one label and one UMI meet with different raw words (tests/test_ori_cases_cpu.py): a key made
    of raw words splits such a UMI's votes."""
    check(monkeypatch, name, case, pattern, env=DECODE_ROUTES[route])


@pytest.mark.parametrize("pattern", ["clear", "random"])
@pytest.mark.parametrize("route", list(BUCKET_ROUTES))
@pytest.mark.parametrize("case", ["cr-like", "prefer-ambig", "trivial"])
@pytest.mark.parametrize("name", qc.MULTI_BATCHES)
def test_multi_bucket_cells(monkeypatch, name, case, route, pattern):
    """Cells of several buckets with slabs of 8 keys (the placement fix-up runs) and with every bucket sent to the sort resolve."""
    new, _ = check(monkeypatch, name, case, pattern, env=BUCKET_ROUTES[route])
    assert new.stats["n_buckets"] >= 3 * len(oc.inputs(name).reads), new.stats
    if route == "slab-cap-8":
        assert new.stats["n_keys"] > 8 * new.stats["n_buckets"], new.stats


@pytest.mark.parametrize("pattern", ["per-read", "random"])
@pytest.mark.parametrize("name", ["base", "usa"])
def test_cells_below_small_thresh(monkeypatch, name, pattern):
    """--small-thresh 30: the cells of fewer reads take the tiny path and are flagged."""
    new, _ = check(monkeypatch, name, "cr-like-tiny-below-30", pattern)
    assert (new.got.flags & pkg._abi.CELL_TINY_PATH).any() and not (new.got.flags & pkg._abi.CELL_TINY_PATH).all()


# -------------------------------------------------------------------------------------------------------------------- parsimony

@pytest.mark.parametrize("pattern", ["per-read", "random"])
@pytest.mark.parametrize("route", list(PUG_ROUTES))
@pytest.mark.parametrize("case", ["parsimony", "parsimony-gene"])
@pytest.mark.parametrize("name", oc.FUZZ)
def test_parsimony_on_every_route(monkeypatch, name, case, route, pattern):
    """Reads of one label with different raw words are ONE vertex, and labels one base apart that share a ref are an edge however
    the shared ref is spelt: the row is one of the judge's outcomes on all seven routes, and the twin's bit for bit."""
    set_pug_route(monkeypatch, route)
    check(monkeypatch, name, case, pattern)


@pytest.mark.parametrize("pattern", ["clear", "alternate", "first-clear", "last-clear"])
@pytest.mark.parametrize("case", ["parsimony", "parsimony-gene"])
@pytest.mark.parametrize("name", oc.FUZZ)
def test_parsimony_under_the_other_patterns(monkeypatch, name, case, pattern):
    check(monkeypatch, name, case, pattern)


@pytest.mark.parametrize("pattern", ["per-read", "random"])
@pytest.mark.parametrize("case", ["umi-edit-dist-0", "large-graph-thresh-3"])
@pytest.mark.parametrize("name", oc.FUZZ)
def test_parsimony_switches(monkeypatch, name, case, pattern):
    new, _ = check(monkeypatch, name, case, pattern)
    if case == "large-graph-thresh-3":
        assert (new.got.flags & pkg._abi.CELL_ALT_RES).any()


@pytest.mark.parametrize("pattern", ["per-read", "random"])
@pytest.mark.parametrize("route", list(PUG_ROUTES))
@pytest.mark.parametrize("em", [False, True], ids=["parsimony", "parsimony-em"])
@pytest.mark.parametrize("name", ["structured", "structured-3"])
def test_structured_cells(monkeypatch, name, em, route, pattern):
    """quant_judge_cases.structured_cells: paths on both sides of the direction rule's threshold (the reads of a vertex count
    together whatever their bits), stars of 1 to 64 leaves, labels that meet in one ref or in two refs of two genes (the
    intersection is of ref ids), one UMI under twelve labels, near-misses without a shared ref, a component above
    --large-graph-thresh 3.  Each has one outcome."""
    set_pug_route(monkeypatch, route)
    check(monkeypatch, name, "parsimony", pattern, em=em, min_judged=1.0)


@pytest.mark.parametrize("thresh", [0, 60, 8])
@pytest.mark.parametrize("name,em", [("components", False), ("components-usa", True)])
def test_component_sizes_at_every_boundary_of_the_flat_build(monkeypatch, name, em, thresh):
    """test_gpu_pug.py's components of 2 to 100 vertices, under random bits: each cover kernel (pairs, a lane, eight lanes, a wave,
    the per-cell kernels, the winner-take-all fallback) holds the labels in another place.  The two cells with 9000 filler reads
    are above the judge's cap: they stand against their twin alone."""
    sw = dict(large_graph_thresh=thresh) if thresh else {}
    check(monkeypatch, name, "parsimony", "random", em=em, min_judged=0.8, **sw)


# ---------------------------------------------------------------------------------------------------------------- label lengths

@pytest.mark.parametrize("pattern", ["per-read", "random"])
@pytest.mark.parametrize("case,em", [("cr-like", False), ("cr-like", True), ("parsimony", False), ("parsimony", True)],
                         ids=["cr-like", "cr-like-em", "parsimony", "parsimony-em"])
@pytest.mark.parametrize("name", ["tailed", "tailed-usa", "wide-labels", "wide-labels-usa"])
def test_label_lengths(monkeypatch, name, case, em, pattern):
    """Each label length has its own holder of the words: the key for 1 and 2 refs, a lane's registers for 3-4 and 5-8, the wave
    for 9-64, LDS staging for 5-16, global memory beyond.  The tailed workload has mixed pairs in every class up to 17-64, the
    gene-family cells above 64 (tests/test_ori_cases_cpu.py)."""
    check(monkeypatch, name, case, pattern, em=em)


# ------------------------------------------------------------------------------------------------------------ the -em resolutions

@pytest.mark.parametrize("pattern", ["per-read", "random"])
@pytest.mark.parametrize("case", ["cr-like", "parsimony", "parsimony-gene"])
@pytest.mark.parametrize("name", ["base", "usa"])
def test_em_resolutions(monkeypatch, name, case, pattern):
    """Class tables, EM rows and three bootstraps under a fixed --boot-seed."""
    check(monkeypatch, name, case, pattern, em=True, boots=True)


@pytest.mark.parametrize("name,case", [("usa", "parsimony"), ("base", "cr-like")])
def test_em_in_canonical_order(monkeypatch, name, case):
    check(monkeypatch, name, case, "random", em=True, boots=True, env={"AFQ_EM_ORDER": "canonical"})


# ---------------------------------------------------------------------------------------------------------------------- layouts

@pytest.mark.parametrize("pattern", ["per-read", "random"])
@pytest.mark.parametrize("case,em", [("cr-like", False), ("parsimony", True)], ids=["cr-like", "parsimony-em"])
@pytest.mark.parametrize("name", list(oc.LAYOUTS) + list(oc.SPLITS) + list(oc.PADDED))
def test_layouts_that_rewrite_the_words_on_the_device(monkeypatch, name, case, em, pattern):
    """Narrow fields through k_widen, an 8-byte UMI and an 8-byte barcode, every position width through k_strip_aln, the
    split-barcode pairs with 0 to 3 bytes in front of their chunks, chunks 1 to 3 bytes off a dword; in all of them every 53rd
    record has 45 alignments and crosses the 256-byte windows (split pairs excepted)."""
    check(monkeypatch, name, case, pattern, em=em)


# ----------------------------------------------------------------------------------------------------------- around the kernels

@pytest.mark.parametrize("how", ["submit", "pinned", "device"])
@pytest.mark.parametrize("case", ["cr-like", "parsimony"])
def test_pageable_pinned_and_device_input(monkeypatch, case, how):
    """(the twin always comes the pageable way)"""
    check(monkeypatch, "wide", case, "random", how=how)


@pytest.mark.parametrize("case", ["cr-like", "parsimony"])
def test_a_batch_cut_into_a_dozen_ranges(monkeypatch, case):
    new, twin = check(monkeypatch, "base", case, "random", env={"AFQ_TEST_RANGE_BYTES": "80000"})
    assert new.ranges >= 12 and twin.ranges == new.ranges


@pytest.mark.parametrize("name", ["tailed", "tailed-cell"])
@pytest.mark.parametrize("case,em", [("parsimony", False), ("parsimony-gene", True)], ids=["parsimony", "parsimony-gene-em"])
def test_label_hash_collisions_are_rehashed(monkeypatch, case, em, name):
    """Hashes cut to 3 bits: different labels share keys, the device compares the lists (masked: equal refs under different bits
    are no collision) and decodes again under another hash.  The rehash is counted.  In a batch of ONE cell the count is 1 for
    both spellings: there is nothing to cut the range around.  In a batch of 70 cells that all collide the count is NOT a function
    of the bytes: the cell a collision names is the one whose workgroup's atomicCAS on the status word lands first (set_err,
    csrc/afq_prims.h), the range is cut around that cell, and how many re-runs that takes depends on where it lies - five runs of
    the twin alone counted 14, 13, 12, 13 and 14 on an MI355X.  There the rows, the classes and every other counter are the
    twin's, and both spellings count at least one rehash."""
    one = name == "tailed-cell"
    new, twin = check(monkeypatch, name, case, "random", em=em, env={"AFQ_TEST_LABEL_HASH_BITS": "3"}, rehash=one)
    assert new.rehash >= 1 and twin.rehash >= 1 and (not one or new.rehash == twin.rehash == 1), (new.rehash, twin.rehash)


@pytest.mark.parametrize("pattern", ["clear", "random"])
def test_a_cell_decoded_again_by_the_fix_up(monkeypatch, pattern):
    """tests/test_gpu_decode_span.py::test_cell_decoded_twice's cell: its second record claims the third as alignments of its own,
    the walk-free proof fails and k_decode's fix-up mode decodes the cell again - from raw words with mixed bits.  The bits are
    rewritten first and the count falsified afterwards, in the twin and in the rewritten bytes alike."""
    ds = __import__("test_gpu_decode_span")
    from test_gpu_decode_bins import cells_with_refs
    from util import cfg_for

    monkeypatch.setenv("AFQ_TEST_DECODE", "recs")
    hw = ds.hw_of(4)
    s = cells_with_refs(77, [3000, 200], False)
    bc = 37
    bt = ds.Batch(9)
    na = np.sort(ds.na_for_length(2 * ds.SPAN + 300, hw, bt.rng))
    bt.add(bc, na)
    bt.umi[0][2] = 50
    b, off = rad.encode_cells_np(np.concatenate((s.cell_nrec, [len(na)])), np.concatenate((s.cell_bc, [bc])).astype(np.uint64),
                                 np.concatenate((s.umi, bt.umi[0])), np.concatenate((s.na, na)), np.concatenate((s.refs, bt.refs[0])))
    cfg = cfg_for(s, "cr-like", small_thresh=0)

    def falsified(data):
        w = np.frombuffer(bytes(data), np.uint32).copy()
        c0 = int(off[-1]) // 4
        assert w[c0 + 1] == len(na) and w[c0 + 2] == 1 and w[c0 + 2 + hw + 1] == 1 and w[c0 + 3] == bc
        w[c0 + 2 + hw + 1] = 1 + hw + 1
        w[c0 + 1] = len(na) - 1
        return oc.Case(w.view(np.uint8), off)

    twin_case, new_case = falsified(b), falsified(oc.reorient(b, off, pattern, 4, 4, seed=5))
    assert twin_case.cells() == new_case.cells() and not np.array_equal(twin_case.data, new_case.data)
    twin, new = device(cfg, s.tid_to_gid, twin_case), device(cfg, s.tid_to_gid, new_case)
    same_as_twin(new, twin, cfg, f"fix-up {pattern}")
    assert new.stats["n_fallback_cells"] == 1 and twin.stats["n_fallback_cells"] == 1, (new.stats, twin.stats)
    reads = new_case.cells()
    js = [qj.judge_cell(r, s.tid_to_gid.tolist(), "cr-like", False, small_thresh=0) for r in reads]
    judge(new.got, reads, js, f"fix-up {pattern}", one_outcome=True, min_judged=1.0)


def test_a_ref_word_that_spells_the_barcode(monkeypatch):
    """With its bit clear the word of ref 37 IS the barcode 37 of its cell: the walk-free decoders take it for a record start, the
    cell's proof fails and the cell is decoded again (with the bit set that cannot happen).  The same rows either way."""
    rng = np.random.default_rng(4)
    cells = []
    for bc in (37, 90001, 5):
        reads = [(int(rng.integers(1000, 1 << 20)), sorted(int(x) for x in rng.choice(60, size=int(rng.integers(1, 5)), replace=False))) for _ in range(400)]
        reads += [(int(rng.integers(1000, 1 << 20)), [bc]) for _ in range(20) if bc < 60]
        cells.append((bc, reads))
    b, off = rad.encode_cells(cells, 4, 4)
    t2g = (np.arange(60) // 2).astype(np.uint32)
    for res in ("cr-like", "parsimony"):
        cfg = pkg.WorkerConfig.for_resolution(res, num_genes=30, num_rows=30, small_thresh=0)
        for route in ("recs", "keys"):
            monkeypatch.setenv("AFQ_TEST_DECODE", route)
            twin_case = oc.Case(b, off)
            new_case = twin_case.reoriented("clear")
            twin, new = device(cfg, t2g, twin_case), device(cfg, t2g, new_case)
            same_as_twin(new, twin, cfg, f"{res} {route}")
            print(f"\n{res} {route}: cells decoded again: twin {twin.stats['n_fallback_cells']}, clear {new.stats['n_fallback_cells']}")
            reads = new_case.cells()
            judge(new.got, reads, [qj.judge_cell(r, t2g.tolist(), res, False, small_thresh=0) for r in reads], f"{res} {route}", min_judged=1.0)


def test_a_pool_rerun(monkeypatch):
    """tests/test_gpu_pool_rerun.py's dense batch on a full device: the range is halved and its parts regrow, and every part
    decodes its records again.  The dense cells hold 15 to 40 thousand reads, beyond any quadratic judge: they stand against the
    twin; the judge has the two small cells."""
    from test_gpu_pool_rerun import dense_batch, full_device
    from util import cfg_for

    s = dense_batch(False, "middle")
    b, off = s.encode()
    cfg = cfg_for(s, "parsimony-em", small_thresh=0, dump_eq=True)
    for k, v in full_device(s.cell_nrec, cfg).items():
        monkeypatch.setenv(k, v)
    twin_case = oc.Case(b, off)
    new_case = twin_case.reoriented("random", seed=8)
    q = pkg.Quantifier(cfg, s.tid_to_gid)
    try:
        twin = Run(q.quant_chunks(twin_case.data, twin_case.off), q.batch_stats(), q.label_rehash_count(), q.resolve_divert_count(), 0)
        regrows = q.pool_regrow_count()
    finally:
        q.close()
    new = device(cfg, s.tid_to_gid, new_case)
    assert regrows > 0
    same_as_twin(new, twin, cfg, "pool re-run")
    small = [i for i, n in enumerate(s.cell_nrec.tolist()) if n <= 300]
    assert len(small) == 2
    reads = new_case.cells()
    tables, flags = qc.classes_of(new.got), new.got.flags.tolist()
    for i in small:
        j = qj.judge_cell(reads[i], s.tid_to_gid.tolist(), "parsimony-em", False, num_rows=s.num_rows, small_thresh=0)
        assert qj.admits(j, None, classes=tables[i], flags=flags[i]) is True, i


# ------------------------------------------------------------------------------------------------------------------ the command

@pytest.mark.parametrize("res,usa,extra,compressed", [("cr-like", False, ["-d"], False), ("parsimony-em", True, ["-b", "4", "--boot-seed", "9"], False),
                                                      ("cr-like", True, ["--devices", "0,0"], False), ("parsimony", False, [], True)],
                         ids=["dump", "bootstraps", "two-workers", "rad-sz"])
def test_afquant_quant_on_random_bits_and_on_the_twin(tmp_path, res, usa, extra, compressed):
    """`afquant quant` on a directory whose alignment words carry random bits and on its twin: every output file equal byte for
    byte, quant.json equal but for paths and the command line."""
    from test_gpu_positions import _strip_paths, make_dir

    s = pkg.synth.synth(188, [2500, 700, 260, 120, 60, 7], num_genes=120, txp_per_gene=2, usa=usa, dup=0.5, cross=0.3, umi_err=0.02, max_extra_na=44)
    b, off = s.encode()
    new = oc.reorient(b, off, "random", 4, 4, seed=2)
    assert oc.two_ref_bleed(oc.Case(new, off))[(0, 1)] > 0
    outs = []
    for kind in ("random", "twin"):
        d = tmp_path / kind
        tg = make_dir(d / "in", s, 0, compressed)
        if kind == "random":
            path = d / "in" / ("map.collated.rad.sz" if compressed else "map.collated.rad")
            prelude = rad.rad_prelude([f"T{t}" for t in range(len(s.tid_to_gid))], len(off), 16, s.umi_len)
            twin_file = rad.snappy_frame_encode(prelude + bytes(b)) if compressed else prelude + bytes(b)
            assert path.read_bytes() == twin_file, "the prelude is as make_dir wrote it"
            path.write_bytes(rad.snappy_frame_encode(prelude + new.tobytes()) if compressed else prelude + new.tobytes())
        out = str(d / "out")
        r = subprocess.run([CLI, "quant", "-i", str(d / "in"), "-m", tg, "-o", out, "-r", res, "-t", "2"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append((str(d), out))
    (dn, on), (dt, ot) = outs
    files = ["alevin/quants_mat.mtx", "alevin/quants_mat_rows.txt", "alevin/quants_mat_cols.txt", "featureDump.txt"]
    if "-d" in extra:
        files += ["alevin/geqc_counts.mtx"]
    if "-b" in extra:
        files += ["alevin/bootstraps_mean.mtx", "alevin/bootstraps_var.mtx"]
    for f in files:
        assert open(os.path.join(on, f), "rb").read() == open(os.path.join(ot, f), "rb").read(), f
    if "-d" in extra:
        ga = gzip.open(os.path.join(on, "alevin", "gene_eqclass.txt.gz")).read()
        assert ga == gzip.open(os.path.join(ot, "alevin", "gene_eqclass.txt.gz")).read() and len(ga) > 10
    assert len(open(os.path.join(on, "alevin", "quants_mat.mtx")).read().splitlines()) > 10
    ma = _strip_paths(json.load(open(os.path.join(on, "quant.json"))), [dn])
    mb = _strip_paths(json.load(open(os.path.join(ot, "quant.json"))), [dt])
    assert ma == mb
