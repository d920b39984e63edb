"""The device at the top of the id spaces it accepts: 2^20 gene ids (1 572 864 columns under USA), ref ids beyond 2^24, UMIs of
44 bits, and the sizes at which the code changes path on the way up there.

Every other module runs gene spaces of at most 36 601 genes: the top three bits of the gene field of every key, counter, label
key and EM state id are zero in all of them, and what the EM does above 131 072 and 262 144 columns, what k_cell_hist does on
its third pass and what a decoder does with a UMI of 2^44 is run by none.  Here the workload of tests/test_gpu_em.py (about
46 k reads, a few seconds a case) is lifted by tests/id_lift.py - an order-preserving relabelling of its genes, which changes no
row but the column ids (tests/test_id_lift_cpu.py) - so that each case pays for the size of the id space and for nothing else.

Two comparisons wherever both apply: the device against the oracle at the lifted size, and the device at the lifted size against
the relabelled rows of the DEVICE at the small size, which does not lean on the oracle.

The EM's arithmetic is named explicitly in every oracle call (oracle_module, not the `oracle` fixture, whose default names the
order-free arithmetic whatever the size): up to 262 144 columns the default EM is the order-free fixed-point one (afq_em2.hip,
em_arith="fixed"); above, its set-up kernel's bitmap does not fit LDS and the default EM is the canonical sequential f32 one
(afq_em.hip, em_arith="reference").  Which side ran is witnessed by em_instance_counts: cells per instance of the order-free
rounds kernel, all zero when the canonical kernels ran."""
import numpy as np
import pytest

import id_lift
from pug_routes import PUG_ROUTES, set_pug_route
from test_gpu_em import assert_within_tolerance
from util import assert_same_result, cfg_for, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad

RESOLUTIONS = ("trivial", "cr-like", "cr-like-em", "parsimony", "parsimony-em", "parsimony-gene", "parsimony-gene-em")
EM_RES = ("cr-like-em", "parsimony-em", "parsimony-gene-em")
CEILING = {False: 1 << 20, True: 1 << 19}   # genes: kGeneBits = 20 bits of gene id; under USA 2^20 gene ids are 2^19 genes
EM2_BOUND = 262144                          # em2_supported (afq_em2.hip): columns whose bitmap + ranks fit 64 KiB of LDS
# genes on both sides of the canonical set-up's LDS bitmap (131 072 columns) and of em2_supported's bound; under USA the columns
# are 3 G: 131 070 | 131 073 and 262 143 | 262 146
EM_BOUNDARY_GENES = {False: (131072, 131073, 262144, 262145), True: (43690, 43691, 87381, 87382)}

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _small(usa):
    return _once(("s", usa), lambda: id_lift.workload(usa))


def _bytes(usa):
    """The records of the small workload - and of every lift of it: lifting changes tid_to_gid alone."""
    return _once(("b", usa), lambda: _small(usa).encode())


def _lift(usa, G_big):
    return _once(("L", usa, G_big), lambda: id_lift.lift_genes(_small(usa), G_big))


def _num_alphas(s):
    return s.num_rows if s.usa else s.num_genes


def _default_arith(s):
    return "fixed" if _num_alphas(s) <= EM2_BOUND else "reference"


def _oracle(ora, s, res, arith, b=None, off=None, **cfg_kw):
    if b is None:
        b, off = _bytes(s.usa)
    key = ("o", s.usa, s.num_genes, len(s.tid_to_gid), res, arith, tuple(sorted(cfg_kw.items())), len(b))
    return _once(key, lambda: ora.quant(cfg_for(s, res, **cfg_kw), s.tid_to_gid, b, off, em_arith=arith))


def _device(s, res, b=None, off=None, counts=False, **cfg_kw):
    if b is None:
        b, off = _bytes(s.usa)
    q = pkg.Quantifier(cfg_for(s, res, **cfg_kw), s.tid_to_gid)
    try:
        got = q.quant_chunks(b, off)
        return (got, sum(q.em_instance_counts())) if counts else got
    finally:
        q.close()


def _reaches_the_last_column(got, s, res):
    """The input really is at the top: the last column of the matrix is counted (`trivial` under USA counts per gene id and
    drops the reads of the last gene's cell, which name its spliced and unspliced form: it is held to the last gene it keeps)."""
    if res == "trivial" and s.usa:
        assert int(got.gene.max()) > s.num_genes - s.num_genes // id_lift.SMALL_GENES
    else:
        assert int(got.gene.max()) == s.num_rows - 1


# ---------------------------------------------------------------------------------------------------------------------------
# a. every resolution at the ceiling, and cr-like / parsimony through each route there

@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_every_resolution_at_the_ceiling(oracle_module, monkeypatch, res, usa):
    """2^20 gene ids: 1 048 576 columns, under USA 1 572 864.  The EM resolutions take the canonical f32 kernels there by
    default; their small-size run for the relabelling check is made in the same arithmetic (AFQ_EM_ORDER=canonical)."""
    L = _lift(usa, CEILING[usa])
    assert L.s.num_genes == 1 << 20 and int(L.s.tid_to_gid.max()) == (1 << 20) - 1
    if res in EM_RES:
        got, n_em2 = _device(L.s, res, counts=True)
        assert n_em2 == 0
    else:
        got = _device(L.s, res)
    assert_same_result(got, _oracle(oracle_module, L.s, res, "reference"), what=f"{res} usa={usa} against the oracle")
    _reaches_the_last_column(got, L.s, res)
    if res in EM_RES:
        monkeypatch.setenv("AFQ_EM_ORDER", "canonical")
    small = _device(_small(usa), res)
    assert_same_result(got, L.relabel(small, res), what=f"{res} usa={usa} against the relabelled small run")


DECODE_ROUTES = {   # name: (environment, chunk shift)
    "recs": ({"AFQ_TEST_DECODE": "recs"}, 0),
    "keys": ({"AFQ_TEST_DECODE": "keys"}, 0),
    "walk": ({}, 1),   # chunks at offsets 1 mod 4
    "divert-all": ({"AFQ_TEST_RESOLVE_DIVERT": "all"}, 0),
    "slab-cap-8": ({"AFQ_TEST_SLAB_CAP": "8"}, 0),
}


def _shifted(b, off, shift):
    if not shift:
        return b, off
    return np.concatenate((np.zeros(shift, np.uint8), np.frombuffer(b, np.uint8))), np.asarray(off, np.uint64) + np.uint64(shift)


def _set_route(monkeypatch, route):
    """-> chunk shift"""
    if route in PUG_ROUTES:
        set_pug_route(monkeypatch, route)
        return 0
    env, shift = DECODE_ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return shift


@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("res", ["cr-like", "parsimony"])
@pytest.mark.parametrize("route", list(DECODE_ROUTES) + list(PUG_ROUTES))
def test_crlike_and_parsimony_through_each_route_at_the_ceiling(oracle_module, monkeypatch, route, res, usa):
    """Both decoders, the walk, every bucket down the divert list, slabs every bucket outgrows, and the parsimony routes of
    tests/test_gpu_pug.py: each packs gene ids, label keys and counters its own way."""
    shift = _set_route(monkeypatch, route)
    L = _lift(usa, CEILING[usa])
    b, off = _shifted(*_bytes(usa), shift)
    got = _device(L.s, res, b, off)
    assert_same_result(got, _oracle(oracle_module, L.s, res, "reference"), what=f"{res} usa={usa} {route}")
    _reaches_the_last_column(got, L.s, res)


# ---------------------------------------------------------------------------------------------------------------------------
# b. the EM on both sides of each num_alphas boundary

@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("res", EM_RES)
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["at-131072", "over-131072", "at-262144", "over-262144"])
def test_default_em_on_both_sides_of_each_boundary(oracle_module, res, usa, which):
    """Up to 262 144 columns the order-free EM: bit-identical to the oracle's fixed-point restatement, within 1e-4 of the
    reference's arithmetic, and the rounds kernel's instance counters say it ran (at 262 144 its set-up kernel asks for 64 KiB of
    dynamic LDS on top of its static 1.3 KiB).  Above: the canonical kernels, bit-identical to the reference's arithmetic, and
    no instance of the order-free rounds kernel ran."""
    L = _lift(usa, EM_BOUNDARY_GENES[usa][which])
    na = _num_alphas(L.s)
    assert (na <= 131072, na <= EM2_BOUND) == [(True, True), (False, True), (False, True), (False, False)][which]
    assert which != 2 or (na + 31) // 32 == 8192   # the largest bitmap the order-free set-up holds
    got, n_em2 = _device(L.s, res, counts=True)
    if na <= EM2_BOUND:
        assert_same_result(got, _oracle(oracle_module, L.s, res, "fixed"), what=f"{res} usa={usa} {na} columns, fixed")
        want = _oracle(oracle_module, L.s, res, "reference")
        assert_within_tolerance(got, want, f"{res} usa={usa} {na} columns")
        assert np.array_equal(got.flags, want.flags) and np.array_equal(got.bc, want.bc)
        assert n_em2 > 0
    else:
        assert_same_result(got, _oracle(oracle_module, L.s, res, "reference"), what=f"{res} usa={usa} {na} columns, reference")
        assert n_em2 == 0
    assert (got.val != np.round(got.val)).any()   # (an EM did run)
    assert int(got.gene.max()) == L.s.num_rows - 1


CANONICAL_SIZES = {False: (131072, 131073, CEILING[False]), True: (43690, 43691, CEILING[True])}


@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("res", EM_RES)
@pytest.mark.parametrize("which", [0, 1, 2], ids=["at-131072", "over-131072", "ceiling"])
def test_canonical_em_on_both_sides_of_its_lds_bitmap(oracle_module, monkeypatch, res, usa, which):
    """k_em's set-up builds a cell's support in an LDS bitmap up to 131 072 columns and by a tiled sort plus unique above:
    AFQ_EM_ORDER=canonical is bit-identical to the reference's arithmetic on both sides and at the ceiling."""
    monkeypatch.setenv("AFQ_EM_ORDER", "canonical")
    L = _lift(usa, CANONICAL_SIZES[usa][which])
    got, n_em2 = _device(L.s, res, counts=True)
    assert_same_result(got, _oracle(oracle_module, L.s, res, "reference"), what=f"{res} usa={usa} {_num_alphas(L.s)} columns")
    assert n_em2 == 0 and int(got.gene.max()) == L.s.num_rows - 1


def _column_label(lab, usa, uo):
    """gene ids -> output columns, as write_eqc_counts prints them (quant.rs:284-335; tests/test_gpu_crlike.py test_infer)"""
    if not usa:
        return tuple(lab)
    o, k = [], 0
    while k < len(lab):
        g = lab[k]
        if k + 1 < len(lab) and lab[k + 1] >> 1 == g >> 1:
            o.append((g >> 1) + 2 * uo); k += 2
        else:
            o.append((g >> 1) + uo if g & 1 else g >> 1); k += 1
    return tuple(o)


@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("res", EM_RES)
@pytest.mark.parametrize("which", [0, 1, 2], ids=["at-131072", "over-131072", "ceiling"])
def test_classes_and_bootstraps_on_both_sides_of_the_lds_bitmap(oracle_module, res, usa, which):
    """-d and -b read a cell's classes off the canonical set-up, which runs for them whatever EM makes the rows: classes and
    bootstrap summaries equal the oracle's (as test_bootstraps compares them); at the ceiling `infer` then runs on the dump."""
    L = _lift(usa, CANONICAL_SIZES[usa][which])
    s = L.s
    kw = dict(dump_eq=True, num_bootstraps=3, summary_stat=True, boot_seed=9)
    got = _device(s, res, **kw)
    want = _oracle(oracle_module, s, res, _default_arith(s), **kw)
    assert_same_result(got, want, what=f"{res} usa={usa} {_num_alphas(s)} columns")
    n_cls = top = 0
    for i in range(got.n_cells):
        g = got.eqclasses.cell(i)
        assert g == want.eqclasses.cell(i), (res, usa, i)
        n_cls += len(g)
        top = max([top] + [max(lab) for lab, _ in g])
    assert n_cls > 100 and top == s.num_genes - 1
    gb, wb = got.bootstraps, want.bootstraps
    for name in ("mean_ptr", "mean_col", "var_ptr", "var_col"):
        assert np.array_equal(getattr(gb, name), getattr(wb, name)), name
    assert np.array_equal(gb.mean_val.view(np.uint32), wb.mean_val.view(np.uint32))
    assert np.array_equal(gb.var_val.view(np.uint32), wb.var_val.view(np.uint32))
    assert len(gb.mean_col) > 0 and int(gb.mean_col.max()) == s.num_genes - 1   # (bootstrap columns are gene ids of the labels)
    if which != 2:
        return
    uo = s.num_rows // 3
    ids, cells = {}, []
    for i in range(got.n_cells):
        cells.append(sorted((ids.setdefault(_column_label(lab, usa, uo), len(ids)), cnt) for lab, cnt in got.eqclasses.cell(i)))
    eq_labels = [list(l) for l, _ in sorted(ids.items(), key=lambda kv: kv[1])]
    assert max(max(l) for l in eq_labels) == s.num_rows - 1
    q = pkg.Quantifier(cfg_for(s), s.tid_to_gid)
    try:
        inf = q.infer(eq_labels, cells, s.num_rows, usa_mode=usa)
    finally:
        q.close()
    assert inf.n_cells == len(cells)
    for i, row in enumerate(cells):
        alphas, _ = oracle_module.em([eq_labels[e] for e, _ in row], [c for _, c in row], s.num_rows,
                                     usa_offsets=(uo, 2 * s.num_rows // 3) if usa else None, dense=0)
        nz = np.flatnonzero(alphas > 0)
        g, v = inf.row(i)
        assert np.array_equal(g, nz.astype(np.uint32)), i
        assert np.array_equal(v.view(np.uint32), alphas[nz].astype(np.float32).view(np.uint32)), i


# ---------------------------------------------------------------------------------------------------------------------------
# c. k_cell_hist: the 16-bit / 32-bit bins at 65 535 | 65 536 molecules, columns on every pass boundary, a third pass and beyond

HIST_ROWS = 196609   # odd: four passes of 65 536 16-bit bins, seven of 32 768 32-bit bins, the last of both half a word
HIST_BOUNDARY_COLS = [0, 32767, 32768, 65535, 65536, 131071, 131072, HIST_ROWS - 1]
HIST_ODD_COL = 98305   # odd: the upper 16 bits of its word; the second bin of the fourth 32-bit pass


def _spread_counts(n):
    """n reads dealt round-robin over the eight boundary columns"""
    return [n // 8 + (1 if j < n % 8 else 0) for j in range(8)]


@pytest.mark.parametrize("n", [65535, 65536])
def test_cell_hist_bin_width_and_pass_boundaries(oracle_module, n):
    """Every read its own UMI and a single ref: a cell's resolved molecules are its reads.  One cell with all n of them on ONE
    odd column - 65 535 fills the upper half of a 16-bit pair to the brim, 65 536 takes the 32-bit bins - and beside it cells
    spread over the first and last column of the passes of both kernels: one of 4 001 molecules (16-bit bins) and one of 65 541
    (32-bit bins).  Against hand-written rows and the oracle."""
    t2g = np.asarray(HIST_BOUNDARY_COLS + [HIST_ODD_COL], np.uint32)
    sizes = [n, 4001, 65541]
    refs = np.concatenate((np.full(n, 8, np.uint32), np.arange(4001, dtype=np.uint32) % 8, np.arange(65541, dtype=np.uint32) % 8))
    umi = np.concatenate([np.arange(k, dtype=np.uint64) * np.uint64(3) + np.uint64(1) for k in sizes])
    s = pkg.synth.SynthRad(np.asarray(sizes, np.int64), np.asarray([11, 12, 13], np.uint64), umi, np.ones(len(refs), np.int64), refs, t2g,
                           HIST_ROWS, HIST_ROWS, False, 12)
    b, off = s.encode()
    q = pkg.Quantifier(cfg_for(s), t2g)
    try:
        got = q.quant_chunks(b, off)
        st = q.batch_stats()
    finally:
        q.close()
    assert st["n_buckets"] > 3   # (multi-bucket cells: the ones k_cell_hist counts)
    rows = [[(HIST_ODD_COL, float(n))],
            [(c, float(k)) for c, k in zip(HIST_BOUNDARY_COLS, _spread_counts(4001))],
            [(c, float(k)) for c, k in zip(HIST_BOUNDARY_COLS, _spread_counts(65541))]]
    assert rows[1][0] == (0, 501.0) and rows[1][7] == (196608, 500.0) and rows[2][4] == (65536, 8193.0) and rows[2][5] == (131071, 8192.0)
    for i, want in enumerate(rows):
        g, v = got.row(i)
        assert list(zip(g.tolist(), v.tolist())) == want, i
    assert_same_result(got, oracle_module.quant(cfg_for(s), t2g, b, off))


# ---------------------------------------------------------------------------------------------------------------------------
# d. UMIs of 44 bits, and one bit more

UMI_ROUTES = [("cr-like", "recs"), ("cr-like", "keys"), ("cr-like", "walk"), ("parsimony", "recs"), ("parsimony", "keys"), ("parsimony", "walk")]
UMI_TOP = (1 << 44) - 1


def _wide_umi_workload(usa):
    """The small workload with 22-base UMIs in an 8-byte field: bits 32..43 of a UMI are a function of its low bits (so the
    duplicates stay duplicates), every fifth read then has ONE of those high bits flipped - a UMI that differs from its
    molecule's in bits 32..43 alone, which a 32-bit UMI would fold back onto it - and 2^44 - 1 itself sits in the largest
    cell (several reads, two genes) and in a small one."""
    def make():
        s = _small(usa)
        low = s.umi.astype(np.uint64)
        hi = (pkg.synth.splitmix64(low) >> np.uint64(7)) & np.uint64(0xFFF)
        idx = np.arange(len(low))
        flip = np.where(idx % 5 == 0, np.uint64(1) << (idx % 12).astype(np.uint64), np.uint64(0))
        umi = low | ((hi ^ flip) << np.uint64(32))
        umi[[0, 1, 2, 7, 11]] = np.uint64(UMI_TOP)
        starts = np.concatenate([[0], np.cumsum(s.cell_nrec)]).astype(np.int64)
        umi[starts[6]:starts[6] + 3] = np.uint64(UMI_TOP)
        import dataclasses
        w = dataclasses.replace(s, umi=umi, umi_len=22)
        assert int(umi.max()) == UMI_TOP and len(np.unique(umi)) > len(np.unique(low))
        return w, rad.encode_cells_np(w.cell_nrec, w.cell_bc, w.umi, w.na, w.refs, bc_bytes=4, umi_bytes=8)
    return _once(("wide", usa), make)


@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("res,route", UMI_ROUTES)
def test_umis_up_to_44_bits_on_every_decode_route(oracle_module, monkeypatch, res, route, usa):
    shift = _set_route(monkeypatch, route)
    w, (b, off) = _wide_umi_workload(usa)
    kw = dict(umi_bytes=8, umi_len=22)
    want = _once(("wide-o", usa, res), lambda: oracle_module.quant(cfg_for(w, res, **kw), w.tid_to_gid, b, off))
    b, off = _shifted(b, off, shift)
    assert_same_result(_device(w, res, b, off, **kw), want, what=f"{res} usa={usa} {route}")
    assert want.val.sum() > 0


@pytest.mark.parametrize("res,route", UMI_ROUTES)
def test_a_umi_of_45_bits_is_refused_on_every_decode_route(oracle_module, monkeypatch, res, route):
    """One UMI of 2^44 in the largest cell (a multi-bucket cell: under cr-like / recs the scattering decoder has it): refused
    with AFQ_ERR_UNSUPPORTED, and the context then quantifies the batch without it."""
    shift = _set_route(monkeypatch, route)
    w, (b, off) = _wide_umi_workload(False)
    kw = dict(umi_bytes=8, umi_len=22)
    bad = np.frombuffer(b, np.uint8).copy()
    rec = int(off[0]) + 8   # the first record of cell 0: na u32, barcode u32, UMI u64
    assert int(bad[rec + 8:rec + 16].view(np.uint64)[0]) == UMI_TOP
    bad[rec + 8:rec + 16] = np.frombuffer(np.uint64(1 << 44).tobytes(), np.uint8)
    want = _once(("wide-o", False, res), lambda: oracle_module.quant(cfg_for(w, res, **kw), w.tid_to_gid, b, off))
    good_b, good_off = _shifted(b, off, shift)
    bad_b, bad_off = _shifted(bad, off, shift)
    q = pkg.Quantifier(cfg_for(w, res, **kw), w.tid_to_gid)
    try:
        with pytest.raises(pkg.AfqError) as e:
            q.quant_chunks(bad_b, bad_off)
        assert e.value.code == pkg._abi.AFQ_ERR_UNSUPPORTED and "UMI" in str(e.value), str(e.value)
        assert_same_result(q.quant_chunks(good_b, good_off), want, what=f"{res} {route} after the refusal")
    finally:
        q.close()


# ---------------------------------------------------------------------------------------------------------------------------
# e. ref ids beyond 2^24

@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("res", ["cr-like", "parsimony", "parsimony-em"])
def test_ref_ids_beyond_2_pow_24(oracle_module, res, usa):
    """Every ref id up by 2^24 + 5 (a 64 MiB tid_to_gid): labels of one, two and three or more refs - inline and hashed label
    keys - and not a row changes."""
    s = _small(usa)
    t = _once(("refs", usa), lambda: id_lift.lift_refs(s, (1 << 24) + 5))
    assert int(t.refs.min()) >= (1 << 24) + 5
    assert (s.na == 1).any() and (s.na == 2).any() and (s.na >= 3).any() and int(s.na.max()) >= 5
    b, off = _once(("refs-b", usa), t.encode)
    got = _device(t, res, b, off)
    assert_same_result(got, _device(s, res), what=f"{res} usa={usa} against the unlifted run")
    assert_same_result(got, _oracle(oracle_module, s, res, "fixed"), what=f"{res} usa={usa} against the oracle")
