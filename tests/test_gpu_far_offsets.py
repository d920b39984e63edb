"""GPU tests of 64-bit chunk offsets: the eight record passes and the quant decoders read chunks that lie at and across byte 2^32 of
one device buffer (tests/far_offset_cases.py places them; tests/test_far_offset_cases_cpu.py shows where byte 2^32 falls and that
the decoys at offset - 2^32 give a kernel that truncates an offset a wrong answer).  The chunks' contents are those of the families'
existing cases, so every result is compared exactly with the family's existing judge on the original case.  The same holds for the
chunk-table hop over a collated stream and for the convert walk over a BAM record stream, each with its headers or records around
byte 2^32, its decoys 2^32 lower and its existing judge (chunk_table_cases.host_hop, convert_judge.stated).

One buffer of 2^32 + 2^21 zero bytes serves the whole module; a test writes its pieces, runs, and zeroes them again."""
import contextlib
import time

import numpy as np
import pytest

import far_offset_cases as F
import gpl_cases as G
import rad_pass_calls as P
from util import pkg

pytestmark = pytest.mark.gpu
ALS = (0, 3)   # the buffer's base is 256-byte aligned; the passes are handed base + al


def _quantifier():
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=1, num_rows=1)
    return pkg.Quantifier(cfg, np.zeros(1, np.uint32), device=0)


# (first in the module: the device buffer of the other tests is not yet alive beside this pass's own 4 GiB copy)
def test_host_bytes_past_4_gib_reach_the_device_piece_by_piece():
    """gpl_hist_rad from HOST bytes of 2^32 + 2^21: the staged copy's piece arithmetic past 4 GiB.  Prints its wall time."""
    f = F.FAMILIES["gpl"]
    lim = f.limits()
    c = f.cases(lim)["widths"]
    pieces, new_off, n_bytes = F.place(c["data"], c["off"], "low-high", *f.layout(c), pad=3, aln_flip=f.aln_flip)
    host = np.zeros(n_bytes, np.uint8)
    for o, b in pieces:
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
    q = _quantifier()
    try:
        q.set_aln_extra_bytes(c["pos_bytes"])
        t0 = time.perf_counter()
        got = q.gpl_hist_rad(host, new_off, bc_bytes=c["bc_bytes"], umi_bytes=c["umi_bytes"], expected_ori="fw")
        print("host bytes past 4 GiB: %.2f s" % (time.perf_counter() - t0))
    finally:
        q.close()
    G.same_hist(got, f.want(c, "fw", lim), "host bytes, low-high")


@pytest.fixture(scope="module")
def buf():
    import torch

    holder = [torch.zeros(F.N_BYTES, dtype=torch.uint8, device="cuda")]   # (a holder: the fixture's cached value must not keep the tensor alive)
    yield holder
    holder.clear()
    torch.cuda.empty_cache()   # back to the device, not only to the allocator's cache: the module's only large allocation ends with it


@pytest.fixture(scope="module")
def q():
    qq = _quantifier()
    yield qq
    qq.close()


@contextlib.contextmanager
def placed(buf, pieces, al=0):
    """the pieces in the buffer, `al` bytes behind their offsets; zeroed again afterwards (the rest of the buffer is zero and stays so)"""
    import torch

    t = buf[0]
    for o, b in pieces:
        t[al + o:al + o + len(b)] = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    try:
        yield t.data_ptr() + al, F.N_BYTES - al
    finally:
        for o, b in pieces:
            t[al + o:al + o + len(b)] = 0
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ record passes
_placements, _wants = {}, {}


def placements(name):
    if name not in _placements:
        f = F.FAMILIES[name]
        lim = f.limits() if f.limits else None
        _placements[name] = (f, lim, F.placements(f, lim))
    return _placements[name]


@pytest.mark.parametrize("name,layout", [(n, layout) for n in sorted(F.FAMILIES) for layout in F.FAMILIES[n].layouts])
def test_a_record_pass_reads_chunks_at_and_across_byte_two_to_the_32(buf, q, name, layout):
    f, lim, pl = placements(name)
    mine = [p for p in pl if p[1] == layout]
    drawn = compared = 0
    for case_name, _, pad, c, (pieces, new_off, _) in mine:
        for al in ALS:
            with placed(buf, pieces, al) as (d_ptr, n_bytes):
                for ori in f.oris:
                    drawn += 1
                    key = (name, case_name, ori)
                    if key not in _wants:
                        _wants[key] = None if name == "atac dedup" else f.want(c, ori, lim)   # (same_as_judge judges the case itself)
                    got = P.run(name, q, c, ori, None, new_off, d_ptr=d_ptr, n_bytes=n_bytes)
                    P.same(name, got, _wants[key], c, f"{name} / {case_name} / {layout} pad {pad} / base + {al} / {ori}")
                    compared += 1
    assert mine and compared == drawn == len(mine) * len(ALS) * len(f.oris)


# ------------------------------------------------------------------------------------------------------------------ quant decoders
# submit_device reads the caller's buffer in place (4-byte aligned base) from CellMeta::chunk_off.  A cell's chunk is larger than the
# record passes' first chunks, so the far cells begin 2^20 bytes behind byte 2^32; submit_device asks for no order of the offsets, so
# `descending` runs beside the two layouts every batch runs under.
QUANT_LAYOUTS = ("low-high", "start-on", "descending")
QUANT_GAP = 1 << 20


def quant_device(cfg, t2g, d_ptr, n_bytes, off, e=0):
    q = pkg.Quantifier(cfg, np.asarray(t2g, np.uint32), aln_extra_bytes=e)
    try:
        q.submit_device(d_ptr, n_bytes, off)
        return q.collect()
    finally:
        q.close()


def compact_then_far(buf, cfg, t2g, data, off, bw, uw, e=0):
    """the batch from its compact bytes on the device, then from every layout of QUANT_LAYOUTS in the large buffer: each result bit for
    bit the compact one's (rows, barcodes, nrec, flags).  -> the compact result, the far ones"""
    import torch

    from util import assert_same_result

    data = np.asarray(data, np.uint8).tobytes() if not isinstance(data, bytes) else data
    d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    want = quant_device(cfg, t2g, d.data_ptr(), d.numel(), off, e)
    del d
    gots = []
    for layout in QUANT_LAYOUTS:
        pieces, new_off, _ = F.place(data, off, layout, [("bc", bw), ("umi", uw)], 4 + e, gap=QUANT_GAP)
        assert len(pieces) > len(new_off) and (new_off >= np.uint64(F.FAR)).any()
        with placed(buf, pieces) as (d_ptr, n_bytes):
            got = quant_device(cfg, t2g, d_ptr, n_bytes, new_off, e)
        assert_same_result(got, want, what=layout)
        gots.append(got)
    assert len(gots) == len(QUANT_LAYOUTS)
    return want, gots


@pytest.mark.parametrize("route", ["as-planned", "decode-recs", "decode-keys"])
def test_cr_like_cells_of_several_buckets_far_in_the_buffer(buf, monkeypatch, route):
    """the `multi` batch of tests/quant_judge_cases.py (24 cells, 7 to 2500 reads) as planned and through each walk-free decoder"""
    import quant_judge_cases as qc
    from test_gpu_quant_judge import DECODE_ROUTES, _judge_device

    for k, v in DECODE_ROUTES[route].items():
        monkeypatch.setenv(k, v)
    b = qc.batch("multi")
    js = [j for j, _ in qc.judgements("multi", "cr-like")]
    assert len(b.cells) == 24 and all(len(j.outcomes) == 1 for j in js)
    want, gots = compact_then_far(buf, b.cfg("cr-like"), b.t2g, b.data, b.off, 4, 4)
    for got in [want] + gots:
        _judge_device(got, b.cells, js, f"multi cr-like {route}")


@pytest.mark.parametrize("route", ["phase-kernels", "one-workgroup"])
def test_parsimony_cells_far_in_the_buffer(buf, monkeypatch, route):
    """the first 200 cells of the `base` batch under parsimony, through the phase kernels and the one-workgroup route"""
    import quant_judge as qj
    import quant_judge_cases as qc
    from pug_routes import set_pug_route
    from test_gpu_quant_judge import _judge_device

    set_pug_route(monkeypatch, route)
    b = qc.batch("base")
    n = 200
    cells = b.cells[:n]
    js = [qj.judge_cell(reads, b.t2g, "parsimony", b.usa, num_rows=b.num_rows, small_thresh=0) for _, reads in cells]
    data = np.asarray(b.data, np.uint8)[:int(b.off[n])]
    want, gots = compact_then_far(buf, b.cfg("parsimony"), b.t2g, data, b.off[:n], 4, 4)
    for got in [want] + gots:
        _judge_device(got, cells, js, f"base[:200] parsimony {route}")


@pytest.mark.parametrize("bw,uw,e,umi_len", [(1, 2, 0, 8), (4, 4, 4, 12), (1, 2, 2, 8)])
def test_widened_and_stripped_cells_far_in_the_buffer(buf, bw, uw, e, umi_len):
    """1-byte barcodes and 2-byte UMIs (k_widen rewrites the cells on the device), position bytes behind every alignment word
    (k_strip_aln), and both at once: the rewrites read the caller's far bytes"""
    import quant_judge as qj
    from test_gpu_positions import batch, long_reads
    from test_gpu_quant_judge import _judge_device
    from quant_judge_cases import cells_of

    s = long_reads(pkg.synth.synth(300 + 10 * e + bw + uw, [3000, 700, 250, 120, 99, 40, 7, 1], num_genes=150, txp_per_gene=3, umi_len=umi_len, dup=0.4, cross=0.3,
                                   umi_err=0.03, max_extra_na=6))
    bc = [3 + 5 * i for i in range(len(s.cell_nrec))] if bw == 1 else [int(x) & ((1 << (8 * bw)) - 1) for x in s.cell_bc]
    (bp, op), _ = batch(s, bw, uw, e, bc)
    cells = [(k, reads) for k, (_, reads) in zip(bc, cells_of(s))]
    cfg = pkg.WorkerConfig.for_resolution("cr-like", num_genes=s.num_genes, num_rows=s.num_rows, small_thresh=0, bc_bytes=bw, umi_bytes=uw, umi_len=umi_len)
    js = [qj.judge_cell(reads, s.tid_to_gid.tolist(), "cr-like", False, num_rows=s.num_rows, small_thresh=0) for _, reads in cells]
    want, gots = compact_then_far(buf, cfg, s.tid_to_gid, bp, op, bw, uw, e)
    for got in [want] + gots:
        _judge_device(got, cells, js, f"{bw}/{uw}/{e}")


# ------------------------------------------------------------------------------------------------------------------ the chunk table
def test_chunk_table_past_4_gib(buf, q):
    """afq_collated_chunk_table over a stream of 2^32 and some 170 KB bytes (F.chunk_table_placement): a header at each of
    F.CT_HEADERS_AT and on byte 2^32, three hundred chunks behind it, decoys 2^32 below; the table is chunk_table_cases.host_hop's
    over the sparse pieces, and so are the three refusals, whose chunks lie behind byte 2^32"""
    import chunk_table_cases as T

    tile, wants = T.hop_tile(), {}

    def hop(pl, d_ptr, n, rec_hdr, what):
        key = (pl["at"], pl["nrec"][pl["k_at"] + 2], n, rec_hdr)
        if key not in wants:
            wants[key] = T.host_hop(F.chunk_table_view(pl, n), F.CT_FIRST, rec_hdr)
        want = wants[key]
        if isinstance(want, str):
            with pytest.raises(pkg.AfqError) as e:
                q.collated_chunk_table(d_ptr, n, F.CT_FIRST, rec_hdr)
            assert e.value.code == pkg._abi.AFQ_ERR_BAD_INPUT and str(e.value).endswith(": " + want), (what, str(e.value), want)
        else:
            got = q.collated_chunk_table(d_ptr, n, F.CT_FIRST, rec_hdr)
            for g, w, name in zip(got, want, ("off", "nbytes", "nrec", "first_bc")):
                assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)
        return want

    tables = refusals = 0
    for at in F.CT_HEADERS_AT:
        pl, nr = F.chunk_table_placement(at, tile), F.chunk_table_placement(at, tile, no_record=True)
        n_chunks, K = len(pl["off"]), nr["k_at"] + 2
        assert F.chunk_table_where(pl) == F.CT_WHERE[at] and nr["off"][K] > F.FAR and sum(1 for o in pl["off"] if o >= F.FAR) > 300
        for al in ALS:
            what = f"header at 2^32 - {F.FAR - at} / base + {al}"
            with placed(buf, pl["pieces"], al) as (d_ptr, _):
                for n, rec_hdr, k in ((pl["n"], 6, n_chunks), (pl["n"], 0, n_chunks), (pl["n_whole"], 12, n_chunks - 1)):
                    w = hop(pl, d_ptr, n, rec_hdr, what)
                    assert len(w[0]) == k and int(w[0][-1]) > F.FAR
                    tables += 1
                for rec_hdr in (12, 0):
                    assert hop(pl, d_ptr, pl["n_whole"] + 5, rec_hdr, what) == "trailing bytes after the last chunk"
                    assert hop(pl, d_ptr, pl["n"] - 1, rec_hdr, what) == "corrupt chunk header"
                    refusals += 2
                assert hop(pl, d_ptr, pl["n"], 12, what) == f"chunk {n_chunks - 1} holds no record"
                refusals += 1
            with placed(buf, nr["pieces"], al) as (d_ptr, _):
                assert hop(nr, d_ptr, nr["n_whole"], 12, what) == f"chunk {K} holds no record"
                assert len(hop(nr, d_ptr, nr["n_whole"], 0, what)[0]) == n_chunks - 1
                assert len(hop(nr, d_ptr, nr["n"], 0, what)[0]) == n_chunks   # the context serves again
                refusals, tables = refusals + 1, tables + 2
    assert tables == len(F.CT_HEADERS_AT) * len(ALS) * 5 == 50 and refusals == len(F.CT_HEADERS_AT) * len(ALS) * 6 == 60


# ------------------------------------------------------------------------------------------------------------------ convert
def _convert(q, pl, fb, d_ptr):
    return q.convert_bam_rad(None, pl["span_off"], n_ref=F.BAM_N_REF, bc_bytes=F.BAM_BW, umi_bytes=F.BAM_UW, filter_best=fb, d_ptr=d_ptr, n_bytes=pl["n_bytes"])


def test_convert_reads_records_at_and_across_byte_two_to_the_32(buf, q):
    """afq_convert_bam_rad over a record stream of 2^32 and a few thousand bytes (F.bam_placement): byte 2^32 in a record's block_size,
    l_read_name, flag, name, CR, UR and AS, a record and a span on it, a run whose head lies 4 GiB in front of its other records; the
    decoys 2^32 below.  Judged by convert_judge.stated on the same records, with test_gpu_convert's `same`.  Then the two refusals
    behind byte 2^32, each naming its record, and a placement again."""
    import convert_judge as J
    from test_gpu_convert import same

    lim = pkg.convert_limits()
    compared = 0
    for where in F.BAM_PLACEMENTS:
        pl = F.bam_placement(where, lim)
        wants = {fb: J.stated(pl["records"], fb, n_ref=F.BAM_N_REF, lane_alns=lim["lane_alns"], bw=F.BAM_BW, uw=F.BAM_UW) for fb in (False, True)}
        assert wants[False]["stats"]["n_records"] == len(pl["records"]) and wants[False]["stats"]["n_dropped_by_flag"] >= 2 and pl["n_bytes"] > F.FAR
        for al in ALS:
            with placed(buf, pl["pieces"], al) as (d_ptr, _):
                for fb in (False, True):
                    same(_convert(q, pl, fb, d_ptr), wants[fb], f"convert / {where} / base + {al} / filter_best={fb}")
                    compared += 1
    assert compared == len(F.BAM_PLACEMENTS) * len(ALS) * 2 == 36
    refused = 0
    for what, pl, index in F.bam_refusals(lim):
        assert pl["offs"][index] > F.FAR
        for al in ALS:
            with placed(buf, pl["pieces"], al) as (d_ptr, _):
                with pytest.raises(pkg.AfqError) as e:
                    _convert(q, pl, False, d_ptr)
                assert e.value.code == pkg._abi.AFQ_ERR_BAD_INPUT and f"record {index}:" in str(e.value), (what, al, str(e.value))
                refused += 1
        c = _names_case()
        got = q.convert_bam_rad(c[0], c[1], n_ref=F.BAM_N_REF, bc_bytes=F.BAM_BW, umi_bytes=F.BAM_UW)   # the context serves a small case
        same(got, c[2], f"names behind {what}")
    assert refused == 2 * len(ALS)


def _names_case():
    """bam_cases' `names` case from host bytes: (stream, span table, what the judge states)"""
    import bam_cases as B
    import convert_judge as J

    c = B.name_cases()[0]
    return B.stream_of(c)[0], B.span_table(c), J.stated(c["records"], False, n_ref=F.BAM_N_REF, lane_alns=pkg.convert_limits()["lane_alns"])
