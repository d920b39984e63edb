"""Multi-barcode (10x Flex) quant at every width pair, before a judge.

Library level: records whose (b0, b1) barcode pair has unequal integer widths reach the library as a split barcode field
(afq_config.bc_split), which k_widen (csrc/afq_decode.hip, "bsplit != 0") rewrites into two dwords.  For every split layout
(w0, w1, uw) and every byte offset of the chunks mod 4 the device reading the split bytes has to give, bit for bit, what the same
device gives for the TWIN - the same cells with the reported key b1 << 32 | b0 in an 8-byte barcode field - and both stand before
tests/quant_judge.py, which reads neither encoding.  The cases and their CPU-side witnesses (record starts on the edges of the
kernel's 256-byte windows, extreme field values, malformed chunks) are tests/multi_bc_cases.py's; tests/test_multi_bc_cases_cpu.py
asserts the witnesses and puts the oracle before the same judge.

CLI level: `afquant quant` on all nine width pairs - labels, featureDump, the matrix against the judge, -d, and --quant-subset,
which filters on the cell barcode b1 in every sample (src/quant.rs:1773-1781 of the reference)."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import multi_bc_cases as mb
import quant_judge as qj
import quant_judge_cases as qc
from util import assert_same_result, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
CLI = os.path.join(pkg.__path__[0], "csrc", "afquant")
INVALID_ARG, BAD_INPUT = pkg._abi.AFQ_ERR_INVALID_ARG, pkg._abi.AFQ_ERR_BAD_INPUT
# one layout of every UMI width runs all seven resolutions (and prefer-ambig); every layout runs cr-like and parsimony
FULL_LAYOUTS = [(1, 4, 1), (2, 1, 2), (4, 2, 4), (2, 4, 8)]
EVERYWHERE = ("cr-like", "parsimony")
ELSEWHERE = ("trivial", "prefer-ambig", "parsimony-gene", "cr-like-em", "parsimony-em", "parsimony-gene-em")
PLAIN_OF = {v: k for k, v in mb.EM_OF.items()}


def _id(layout):
    return "-".join(str(x) for x in layout)


class Pair:
    """A context for the split bytes and one for the twin, under one resolution case.  `run` names a result of an -em resolution
    by its plain sibling's judgement: what is judged of it is the class table (dump_eq)."""

    def __init__(self, case, run):
        self.case, self.run = case, run
        self.em = run in PLAIN_OF
        self.res_case = PLAIN_OF[run] if self.em else run
        res, ckw, _ = mb.RES_CASES[self.res_case]
        kw = dict(ckw, dump_eq=True) if self.em else ckw
        res = mb.EM_OF[res] if self.em else res
        t2g = np.asarray(case.t2g, np.uint32)
        self.cfg = {kind: case.cfg(res, kind, **kw) for kind in ("split", "twin")}
        assert self.cfg["split"].bc_split == case.w0 and self.cfg["split"].bc_bytes == case.w0 + case.w1 and self.cfg["twin"].bc_bytes == 8
        self.q = {}
        try:
            for kind in ("split", "twin"):
                self.q[kind] = pkg.Quantifier(self.cfg[kind], t2g)
        except Exception:
            self.close()
            raise

    def close(self):
        for q in self.q.values():
            q.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def quant(self, kind, pad, how="submit"):
        data, off = self.case.encode(kind, pad)
        q = self.q[kind]
        if how == "submit":
            q.submit(data, off)
        elif how == "pinned":
            import torch

            h = torch.from_numpy(data.copy()).pin_memory()
            q.submit_ptr(h.data_ptr(), h.numel(), off)
        else:
            import torch

            d = torch.from_numpy(data.copy()).cuda()
            q.submit_device(d.data_ptr(), d.numel(), off)
            torch.cuda.synchronize()
        got = q.collect()
        st = q.batch_stats()
        # witnesses that the planned route ran, no more.  (Fields of 0 and of all-ones look like record heads to the walk-free
        # decoders, which then cannot prove a cell and walk it record by record: the extremes may fall back, the fuzz cells never do.)
        assert st["n_records"] == self.case.n_records() and (st["n_fallback_cells"] == 0 or not self.case.name.startswith("fuzz")), st
        return got

    def check(self, pad, how="submit", twin_how="submit"):
        """The split bytes against the twin, bit for bit; the reported keys; every cell before the judge."""
        case = self.case
        what = f"{case.name} {_id(case.layout)} {self.run} pad {pad} {how}"
        got, twin = self.quant("split", pad, how), self.quant("twin", pad, twin_how)
        assert_same_result(got, twin, what=what)
        if self.em:
            for f in ("cell_ptr", "label_ptr", "labels", "count"):
                assert np.array_equal(getattr(got.eqclasses, f), getattr(twin.eqclasses, f)), f"{what}: class tables, {f}"
        assert [int(x) for x in got.bc] == case.keys(), what
        assert [int(x) for x in got.nrec] == [len(r) for _, r in case.cells], what
        js = case.judgements(self.res_case)
        assert len(js) == got.n_cells
        rows, tables, flags = qc.rows_of(got), qc.classes_of(got) if self.em else None, got.flags.tolist()
        for i, j in enumerate(js):
            assert not j.undecided, f"{what}: cell {i} left undecided"
            if self.res_case in mb.ONE_OUTCOME:
                assert len(j.outcomes) == 1, f"{what}: cell {i}"
            m = qj.admits(j, None if self.em else rows[i], classes=tables[i] if self.em else None, flags=flags[i])
            assert m is True, f"{what}, cell {i} ({len(j.outcomes)} outcome(s)): {m}; reads {case.cells[i][1]}"
        return got


def _runs(case, runs):
    return [r for r in runs if case.usa or r != "prefer-ambig"]     # outside USA mode the switch is ignored: that is cr-like again


# --------------------------------------------------------------------------------------------------------------- library level

@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("layout", mb.SPLIT_LAYOUTS, ids=_id)
def test_split_bytes_equal_their_twin_and_stand_before_the_judge(layout, usa):
    """cr-like and parsimony on the fuzz cells of every split layout, USA and not, with 0 to 3 bytes of padding in front of every
    chunk: bc, nrec, flags, cell_ptr, columns and value bits of the split bytes are the twin's, the key of every cell is
    b1 << 32 | b0, cr-like equals the judge's one outcome and parsimony is one of the judge's outcomes - the one, where there is
    one.  Every cell is judged."""
    case = mb.fuzz(layout, usa)
    for run in EVERYWHERE:
        with Pair(case, run) as p:
            for pad in mb.PADDINGS:
                p.check(pad)


@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("layout", FULL_LAYOUTS, ids=_id)
def test_the_other_resolutions_on_one_layout_of_every_umi_width(layout, usa):
    """trivial, prefer-ambig (USA mode), parsimony-gene, and the three -em resolutions with dump_eq: rows (the EM's value bits
    included) and class tables of the split bytes are the twin's; trivial and prefer-ambig equal the judge's outcome,
    parsimony-gene is admitted, and so are the class tables the EMs are given."""
    case = mb.fuzz(layout, usa)
    for run in _runs(case, ELSEWHERE):
        with Pair(case, run) as p:
            for pad in mb.PADDINGS:
                p.check(pad)


ROUTES = {
    "decode-recs": dict(env={"AFQ_TEST_DECODE": "recs"}),
    "decode-keys": dict(env={"AFQ_TEST_DECODE": "keys"}),
    "many-ranges": dict(env={"AFQ_TEST_RANGE_BYTES": "6000"}),
    "device": dict(how="device"),
    "pinned": dict(how="pinned"),
    "many-ranges-pinned": dict(env={"AFQ_TEST_RANGE_BYTES": "6000"}, how="pinned"),
}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("layout", [(2, 4, 2), (4, 1, 8)], ids=_id)
def test_routes(monkeypatch, layout, route):
    """The fuzz case through each walk-free decoder, cut into several ranges (each widens its own cells), from device memory and
    from pinned host memory (test_split_bytes_equal_their_twin... is the pageable route).  The twin always comes the plain way:
    a route that changed a bit shows against it and against the judge.  The range count and the batch's counters are witnesses
    that the route ran; they decide nothing."""
    r = ROUTES[route]
    for k, v in r.get("env", {}).items():
        monkeypatch.setenv(k, v)
    for usa in (False, True):
        case = mb.fuzz(layout, usa)
        for run in EVERYWHERE:
            with Pair(case, run) as p:
                for pad in mb.PADDINGS:
                    p.check(pad, how=r.get("how", "submit"))
                    if "AFQ_TEST_RANGE_BYTES" in r.get("env", {}):
                        assert p.q["split"].range_pipeline_counts()[0] >= 3, "the batch was cut into ranges"


@pytest.mark.parametrize("layout", mb.SPLIT_LAYOUTS, ids=_id)
def test_extremes(layout):
    """b0 and b1 at 0 and at all-ones in all four combinations, beside the UMI 0 and the all-ones UMI; neighbouring chunks that
    differ in b0 only or in b1 only.  A byte that bleeds from one field into its neighbour changes the reported key or the row:
    both are compared exactly, against the twin and against the judge."""
    case = mb.extremes(layout)
    for run in ("cr-like", "parsimony", "trivial", "cr-like-em"):
        with Pair(case, run) as p:
            for pad in mb.PADDINGS:
                got = p.check(pad)
                if run == "cr-like":
                    assert [dict(r)[i] for i, r in enumerate(qc.rows_of(got))] == [6.0] * 6   # (tests/multi_bc_cases.py: six UMIs on the cell's gene)


@pytest.mark.parametrize("layout", mb.SPLIT_LAYOUTS, ids=_id)
def test_record_starts_on_the_window_edges(layout):
    """The edge case: over the four paddings a record starts on each of the phases 252...255 and 0...3 of the kernel's windows, with
    and without alignments where its na field lies in two windows (asserted on the CPU side, and again here for the bytes that
    run).  Records without alignments end the parsimony resolutions (an empty label; the reference exits there too), so this case
    runs the integer-exact ones and the class table of cr-like-em."""
    case = mb.edge(layout)
    w = mb.witness(case)
    assert mb.EDGE_PHASES <= w["phases"] and 0 in w["straddling_na"] and w["straddling_na"] - {0}
    for run in ("cr-like", "trivial", "cr-like-em"):
        with Pair(case, run) as p:
            for pad in mb.PADDINGS:
                p.check(pad)


@pytest.mark.parametrize("kind", mb.MALFORMED_KINDS)
@pytest.mark.parametrize("layout", [(1, 2, 1), (2, 1, 2), (2, 4, 4), (1, 2, 4)], ids=_id)
def test_malformed_split_chunks_are_refused_by_name(layout, kind):
    """Chunk 2 of 4 with a header that no longer fits its records (record heads of 8, 9, 14 and 11 bytes: every length mod 4, so
    that the host's chunk table refuses some and the device's record walk the others): AFQ_ERR_BAD_INPUT naming cell 2, from
    host memory and from device memory, and the same context then serves the good batch."""
    import torch

    data, off, good = mb.malformed(layout, kind)
    with Pair(good, "cr-like") as p:
        q = p.q["split"]
        for how in ("submit", "device"):
            with pytest.raises(pkg.AfqError) as e:
                if how == "submit":
                    q.quant_chunks(data, off)
                else:
                    d = torch.from_numpy(data.copy()).cuda()
                    q.submit_device(d.data_ptr(), d.numel(), off)
                    q.collect()
            assert e.value.code == BAD_INPUT and "cell 2:" in str(e.value), (how, str(e.value))
            p.check(0)


def test_create_refuses_impossible_barcode_splits():
    """bc_split 5; a split that leaves b1 no byte; a b1 of more than four bytes; a UMI of three bytes."""
    lib = pkg.load_library()
    import ctypes as C

    t2g = np.zeros(4, np.uint32)
    for kw in (dict(bc_bytes=7, bc_split=5), dict(bc_bytes=2, bc_split=2), dict(bc_bytes=2, bc_split=3), dict(bc_bytes=6, bc_split=1),
               dict(bc_bytes=8, bc_split=2), dict(bc_bytes=6, bc_split=2, umi_bytes=3)):
        ccfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, **kw).to_c()
        h = C.c_void_p()
        rc = lib.afq_create(C.byref(ccfg), t2g.ctypes.data_as(C.POINTER(C.c_uint32)), len(t2g), 0, C.byref(h))
        if rc == 0:
            lib.afq_destroy(h)
        assert rc == INVALID_ARG, kw
        with pytest.raises(pkg.AfqError) as e:
            pkg.Quantifier(pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, **kw), t2g)
        assert e.value.code == INVALID_ARG
    pkg.Quantifier(pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1, bc_bytes=5, bc_split=4, umi_bytes=8), t2g).close()


# ------------------------------------------------------------------------------------------------------------------- CLI level

def _quant(tmp, name, tg, res, *extra):
    out = tmp / name
    r = subprocess.run([CLI, "quant", "-i", str(tmp / "in"), "-m", tg, "-o", str(out), "-r", res, "--small-thresh", "0", "-t", "2", *extra],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def _outputs(out):
    rows = (out / "alevin/quants_mat_rows.txt").read_text().split()
    cols = (out / "alevin/quants_mat_cols.txt").read_text().split()
    body = [l for l in (out / "alevin/quants_mat.mtx").read_text().splitlines() if not l.startswith("%")]
    size = tuple(int(x) for x in body[0].split())
    mat = [dict() for _ in rows]
    for r, c, v in (l.split() for l in body[1:]):
        assert int(c) - 1 not in mat[int(r) - 1]
        mat[int(r) - 1][int(c) - 1] = float(v)
    feat = [l.split("\t") for l in (out / "featureDump.txt").read_text().splitlines()]
    return rows, cols, size, mat, feat, json.load(open(out / "quant.json"))


def _check_cli(case, out, res_case, chunks):
    """The output of a run that kept `chunks` (indices into the case, in file order) against the labels and the judge."""
    rows, cols, size, mat, feat, meta = _outputs(out)
    labels = [mb.cli_label(case, i) for i in chunks]
    assert rows == [l for l, _ in labels], "sample_cell in chunk order; the bare cell barcode for a sample the manifest does not list"
    assert cols == [f"G{g}" for g in range(case.num_genes)]
    assert feat[0][:3] == ["CB", "sample_name", "CorrectedReads"] and len(feat[0]) == 10 and len(feat) == len(chunks) + 1
    js = case.judgements(res_case)
    for k, i in enumerate(chunks):
        cell = rad.int_to_seq(case.cells[i][0][1], 4 * case.w1)
        sample = labels[k][1]
        nrec = str(len(case.cells[i][1]))
        assert feat[1 + k][:2 if sample is None else 3] == ([cell, nrec] if sample is None else [cell, sample, nrec]), (k, feat[1 + k])
        assert len(feat[1 + k]) == (9 if sample is None else 10) and feat[1 + k][-7] == nrec
        if res_case in mb.ONE_OUTCOME:
            assert len(js[i].outcomes) == 1
        m = qj.admits(js[i], mat[k])
        assert m is True, f"{res_case}, chunk {i} ({len(js[i].outcomes)} outcome(s)): {m}"
    return size, meta


@pytest.mark.parametrize("layout", [(w0, w1, 4) for w0, w1 in mb.PAIRS] + [(2, 4, 1)], ids=_id)
def test_cli_on_every_width_pair(tmp_path, layout):
    """All nine (w0, w1) with a 4-byte UMI, and u16 + u32 with a 1-byte UMI: four samples sharing four cell barcodes, of which
    collation_manifest.bin lists three.  quants_mat_rows.txt is sample_cell in chunk order and the bare cell barcode for the
    fourth sample (quant.rs:1221-1261: `.get(si)` is None), whose featureDump lines have no sample column; quants_mat.mtx equals
    the judge's rows for cr-like and trivial and is admitted for parsimony."""
    case = mb.cli_case(layout)
    tg = mb.write_cli_dir(tmp_path / "in", case)
    for res in ("cr-like", "trivial", "parsimony"):
        size, meta = _check_cli(case, _quant(tmp_path, res, tg, res), res, range(16))
        assert size[:2] == (16, case.num_genes) and meta["num_quantified_cells"] == 16


def test_cli_dumps_the_judges_classes(tmp_path):
    """-d on a split layout: the classes written for every cell are the judge's (parsimony: admitted), and the matrix as without."""
    case = mb.cli_case((2, 4, 2))
    tg = mb.write_cli_dir(tmp_path / "in", case)
    for res in ("cr-like", "parsimony"):
        out = _quant(tmp_path, res, tg, res, "-d")
        _check_cli(case, out, res, range(16))
        lines = gzip.open(out / "alevin/gene_eqclass.txt.gz", "rt").read().split("\n")
        n_cls = int(lines[1])
        cls = {int(t[-1]): tuple(int(x) for x in t[:-1]) for t in (ln.split("\t") for ln in lines[2:2 + n_cls])}
        ent = [l.split() for l in (out / "alevin/geqc_counts.mtx").read_text().splitlines()[3:]]
        got = [dict() for _ in range(16)]
        for r, c, v in ent:
            got[int(r) - 1][cls[int(c) - 1]] = int(float(v))
        for i, j in enumerate(case.judgements(res)):
            m = qj.admits(j, classes=got[i])
            assert m is True, f"{res} -d, chunk {i}: {m}"


@pytest.mark.parametrize("pair", [(2, 2), (1, 4), (2, 4), (4, 2), (2, 1)], ids=_id)
def test_cli_quant_subset_filters_on_the_cell_barcode_in_every_sample(tmp_path, pair):
    """--quant-subset lists cell barcodes (the reference filters on collate_key(), the cell barcode, whatever the sample:
    quant.rs:1773-1781, 2012-2013): exactly the chunks whose b1 is listed survive, in every sample, in file order, and the matrix
    and num_quantified_cells are sized by the list, a barcode that is not in the file included
    (test_quant_subset_sizes_the_matrix_by_the_subset)."""
    case = mb.cli_case((pair[0], pair[1], 4))
    tg = mb.write_cli_dir(tmp_path / "in", case)
    b1s = [bc[1] for bc, _ in case.cells[:4]]
    absent = next(v for v in range(1, 256) if v not in b1s)
    keep = [b1s[2], b1s[0], absent]
    (tmp_path / "subset.txt").write_text("\n".join(rad.int_to_seq(v, 4 * case.w1) for v in keep) + "\n")
    chunks = [i for i in range(16) if case.cells[i][0][1] in keep]
    assert chunks == [0, 2, 4, 6, 8, 10, 12, 14]
    out = _quant(tmp_path, "out", tg, "cr-like", "--quant-subset", str(tmp_path / "subset.txt"))
    size, meta = _check_cli(case, out, "cr-like", chunks)
    assert size[:2] == (3, case.num_genes) and meta["num_quantified_cells"] == 3
