"""The multi-barcode cases of tests/multi_bc_cases.py before anything runs on a device: their witnesses hold for every split layout,
the twin decodes back to the cells, the split bytes are the twin but for the barcode field, the judge decides every fuzz cell and
the oracle reading the twin stands before it, and WorkerConfig carries bc_split."""
import numpy as np
import pytest

import multi_bc_cases as mb
import quant_judge as qj
import quant_judge_cases as qc
from util import pkg

rad = pkg.rad


def _id(layout):
    return "-".join(str(x) for x in layout)


def _cases(layout):
    return [mb.fuzz(layout), mb.fuzz(layout, True), mb.edge(layout), mb.extremes(layout)]


@pytest.mark.parametrize("layout", mb.SPLIT_LAYOUTS, ids=_id)
def test_window_edges_are_witnessed(layout):
    """Over the four paddings the fuzz case and the edge case put a record start on every phase 252...255 and 0...3 of the
    kernel's 256-byte windows; a record whose na field straddles two windows has alignments and another has none; chunks sit at
    every offset mod 4, one holds a single record and the last one ends the buffer."""
    f, e = mb.witness(mb.fuzz(layout)), mb.witness(mb.edge(layout))
    assert mb.EDGE_PHASES <= f["phases"] | e["phases"], sorted(mb.EDGE_PHASES - f["phases"] - e["phases"])
    assert mb.EDGE_PHASES <= e["phases"], "the edge case covers them by construction"
    assert 0 in e["straddling_na"] and any(na >= 1 for na in e["straddling_na"]), e["straddling_na"]
    for w in (f, e):
        assert w["offsets_mod_4"] == {0, 1, 2, 3} and w["last_chunk_ends_the_buffer"] and w["single_record_chunks"], w
    # the fuzz cells cross the windows several times: its longest chunk spans more than four of them
    data, off = mb.fuzz(layout).encode("split")
    assert max(np.diff(np.concatenate((off, [len(data)])).astype(np.int64))) > 4 * 256
    # and the phase is the kernel's: the chunk's window grid starts at its offset rounded down to a dword
    assert mb.phase(259, 3) == 3 and mb.phase(256 + 5, 6) == 1 and mb.phase(255, 3) == 255


@pytest.mark.parametrize("layout", mb.SPLIT_LAYOUTS, ids=_id)
def test_the_twin_decodes_to_the_cells_and_the_split_bytes_differ_in_the_barcode_field_only(layout):
    w0, w1, uw = layout
    for case in _cases(layout):
        assert case.keys() == [(b1 << 32) | b0 for (b0, b1), _ in case.cells] and len(set(case.keys())) == len(case.cells)
        for pad in mb.PADDINGS:
            twin, toff = case.encode("twin", pad)
            split, soff = case.encode("split", pad)
            for i, ((b0, b1), reads) in enumerate(case.cells):
                bc, got = rad.decode_chunk(bytes(twin), int(toff[i]), 8, uw)
                assert bc == (b1 << 32) | b0 and got == [(u, list(refs)) for u, refs in reads], (case.name, pad, i)
                field, got = rad.decode_chunk(bytes(split), int(soff[i]), w0 + w1, uw)
                assert field & mb.ones(w0) == b0 and field >> (8 * w0) == b1 and got == [(u, list(refs)) for u, refs in reads]
            # re-encoding what the split bytes decode to, with the barcode field rewritten as the twin's, gives the twin's bytes
            cells = []
            for i in range(len(case.cells)):
                field, reads = rad.decode_chunk(bytes(split), int(soff[i]), w0 + w1, uw)
                cells.append((((field >> (8 * w0)) << 32) | (field & mb.ones(w0)), reads))
            again, aoff = mb.with_padding(*rad.encode_cells(cells, 8, uw), pad)
            assert np.array_equal(again, twin) and np.array_equal(aoff, toff), (case.name, pad)
            assert len(twin) - len(split) == (8 - w0 - w1) * case.n_records()
            if pad:
                assert all((twin[int(o) - pad:int(o)] == mb.PAD_BYTE).all() and (split[int(p) - pad:int(p)] == mb.PAD_BYTE).all() for o, p in zip(toff, soff))
        # the starts the witness works from are where the records are
        for pad in (0, 3):
            data, off = case.encode("split", pad)
            for i, start, na in mb.record_starts(case, pad):
                assert int.from_bytes(bytes(data[start:start + 4]), "little") == na


@pytest.mark.parametrize("uw", mb.UMI_WIDTHS)
def test_extremes_hold_what_they_say(uw):
    for w0, w1 in mb.SPLIT_PAIRS:
        c = mb.extremes((w0, w1, uw))
        bcs = [bc for bc, _ in c.cells]
        assert set(bcs[:4]) == {(a, b) for a in (0, mb.ones(w0)) for b in (0, mb.ones(w1))}
        diff = [(a[0] != b[0], a[1] != b[1]) for a, b in zip(bcs, bcs[1:])]
        assert diff[:3] == [(True, False), (False, True), (True, False)] and diff[4] == (False, True)
        umis = {u for _, reads in c.cells for u, _ in reads}
        assert {0, mb.umi_ones(uw)} <= umis and mb.umi_ones(uw) == (mb.ones(uw) if uw < 8 else (1 << 44) - 1)
    # six UMIs on the first gene, no two of them within one base of another but 0 / 3 and ones / ones ^ 3: the judge's cr-like row
    j = c.judgements("cr-like")
    assert all(len(x.outcomes) == 1 and x.outcomes[0][0][i] == 6 for i, x in enumerate(j))


@pytest.mark.parametrize("kind", mb.MALFORMED_KINDS)
@pytest.mark.parametrize("layout", [(1, 2, 1), (2, 1, 2), (2, 4, 4), (1, 2, 4)], ids=_id)
def test_malformed_chunk_two_no_longer_decodes(layout, kind):
    data, off, good = mb.malformed(layout, kind)
    w0, w1, uw = layout
    gd, goff = good.encode("split")
    assert np.array_equal(off, goff) and len(data) == len(gd)
    differ = np.nonzero(data != gd)[0]
    assert len(differ) and differ.min() >= int(off[2]) and differ.max() < int(off[2]) + 8, "only chunk 2's header"
    for i in (0, 1, 3):
        assert rad.decode_chunk(bytes(data), int(off[i]), w0 + w1, uw)[1] == good.cells[i][1]
    with pytest.raises(AssertionError, match="does not match its records"):
        rad.decode_chunk(bytes(data), int(off[2]), w0 + w1, uw)


# ------------------------------------------------------------------------------------------- the judge, and the oracle before it

@pytest.mark.parametrize("usa", [False, True])
def test_the_judge_decides_every_fuzz_cell(usa):
    """cr-like, prefer-ambig and trivial give one outcome for all 16 cells; parsimony and parsimony-gene leave none undecided."""
    c = mb.fuzz((1, 4, 1), usa)
    assert [len(r) for _, r in c.cells] == list(mb.FUZZ_SIZES)
    assert all(0 <= u < 256 for _, reads in c.cells for u, _ in reads), "UMIs of four bases fit every UMI width"
    for rc in mb.ONE_OUTCOME:
        assert all(not j.undecided and len(j.outcomes) == 1 for j in c.judgements(rc)), rc
    for rc in ("parsimony", "parsimony-gene"):
        js = c.judgements(rc)
        several = sum(len(j.outcomes) > 1 for j in js)
        print(f"\nusa={usa} {rc}: {several} cells of several outcomes")
        assert len(js) == 16 and not any(j.undecided for j in js), rc
    # the reads, and so the judgements, are one list whatever the layout
    assert [r for _, r in mb.fuzz((4, 2, 8), usa).cells] == [r for _, r in c.cells]


def _admitted(case, js, res, what, classes=False):
    rows, tables, flags = (None, qc.classes_of(res), None) if classes else (qc.rows_of(res), None, res.flags.tolist())
    assert [int(x) for x in res.bc] == case.keys() and [int(x) for x in res.nrec] == [len(r) for _, r in case.cells], what
    for i, j in enumerate(js):
        got = qj.admits(j, None if classes else rows[i], classes=tables[i] if classes else None, flags=None if classes else flags[i])
        assert got is True, f"{what}, cell {i}: {got}; reads {case.cells[i][1]}"


@pytest.mark.parametrize("rc", ["cr-like", "trivial", "parsimony", "parsimony-gene"])
@pytest.mark.parametrize("usa", [False, True])
def test_the_oracle_on_the_twin_stands_before_the_judge(oracle, usa, rc):
    """The four plain resolutions on the fuzz cells, and cr-like / parsimony on the extremes: the oracle reading the 8-byte twin
    gives the judge's outcome (one of them, under both of its scan orders, for parsimony) and reports the key b1 << 32 | b0."""
    res, ckw, _ = mb.RES_CASES[rc]
    cases = [mb.fuzz((2, 4, 1), usa)] + ([] if usa else [mb.extremes((1, 2, uw)) for uw in mb.UMI_WIDTHS] + ([mb.edge((4, 2, 2))] if rc in mb.ONE_OUTCOME else []))
    for case in cases:
        js = case.judgements(rc)
        data, off = case.encode("twin", 0)
        t2g = np.asarray(case.t2g, np.uint32)
        for desc in ((False, True) if rc.startswith("parsimony") else (False,)):
            kw = dict(tie_break_descending=True) if desc else {}
            _admitted(case, js, oracle.quant(case.cfg(res, "twin", **ckw), t2g, data, off, **kw), f"{case.name} {rc} descending={desc}")
            if rc != "trivial":
                em = oracle.quant(case.cfg(mb.EM_OF[res], "twin", dump_eq=True, **ckw), t2g, data, off, **kw)
                _admitted(case, js, em, f"{case.name} {rc} -d descending={desc}", classes=True)


# ---------------------------------------------------------------------------------------------------------------- the binding

def test_worker_config_carries_bc_split():
    """WorkerConfig.bc_split reaches afq_config.bc_split and is 0 unless asked for.  (AfqConfig already held the field, so the
    struct's layout is untouched: tests/test_abi_cpu.py's layout check passes as before.)"""
    assert pkg.WorkerConfig().bc_split == 0 and pkg.WorkerConfig().to_c().bc_split == 0
    c = pkg.WorkerConfig.for_resolution("cr-like", bc_bytes=6, bc_split=2, umi_bytes=1).to_c()
    assert (c.bc_bytes, c.bc_split, c.umi_bytes) == (6, 2, 1)
    case = mb.fuzz((4, 1, 2))
    s, t = case.cfg("parsimony", "split").to_c(), case.cfg("parsimony", "twin").to_c()
    assert (s.bc_bytes, s.bc_split, t.bc_bytes, t.bc_split) == (5, 4, 8, 0)
    same = [f for f, _ in pkg._abi.AfqConfig._fields_ if f not in ("bc_bytes", "bc_split")]
    assert all(getattr(s, f) == getattr(t, f) for f in same)
    assert mb.cli_case((2, 2, 4)).cfg("cr-like", "split").to_c().bc_split == 0, "equal widths are one integer to the library"


@pytest.mark.parametrize("layout", [(w0, w1, 4) for w0, w1 in mb.PAIRS] + [(2, 4, 1)], ids=_id)
def test_cli_cases_lay_the_samples_out_as_collation_does(layout):
    c = mb.cli_case(layout)
    assert [bc[0] for bc, _ in c.cells] == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4
    assert [bc[1] for bc, _ in c.cells[:4]] * 4 == [bc[1] for bc, _ in c.cells] and len({bc[1] for bc, _ in c.cells}) == 4
    labels = [mb.cli_label(c, i) for i in range(16)]
    assert len(set(l for l, _ in labels[:12])) == 12 and [s for _, s in labels[12:]] == [None] * 4
    assert [l for l, _ in labels[12:]] == [l.split("_")[-1] for l, _ in labels[:4]] and all(len(l) == 4 * layout[1] for l, _ in labels[12:])
