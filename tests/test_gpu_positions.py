"""GPU tests of collated RAD records that carry a position per alignment (alignment tags compressed_ori_refid:u32 then pos of
1, 2, 4 or 8 bytes; the reference's KnownRecordType::RnaShortPos, src/utils.rs:313-377).  The reference quantifies them like
plain records (src/quant.rs:1977-1990): positions never reach a count.  Here the batch is rewritten on the device without them
(k_strip_aln, afq_set_aln_extra_bytes).  Each position batch is compared with its TWIN - the same cells written without
positions - bit for bit on the device (rows, barcodes, nrec, flags, -d classes, bootstraps), and the twin with the oracle."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from util import assert_same_result, cfg_for, pkg

pytestmark = pytest.mark.gpu
rad = pkg.rad
synth = pkg.synth
CLI = os.path.join(pkg.__path__[0], "csrc", "afquant")
EM = ("cr-like-em", "parsimony-em", "parsimony-gene-em")
RESOLUTIONS = ("trivial", "cr-like", "cr-like-em", "parsimony", "parsimony-em", "parsimony-gene", "parsimony-gene-em")


def _narrow(v, width):
    return v if width == 8 else v & np.uint64((1 << (8 * width)) - 1)


def long_reads(s, step=53, na=45):
    """s with every step-th read mapping to na distinct transcripts (ascending): records that cross the walk's 256-byte windows."""
    rng = np.random.default_rng(step * 1000 + na)
    start = np.concatenate(([0], np.cumsum(s.na)[:-1]))
    nas, refs = [], []
    for r in range(len(s.na)):
        if r % step == step - 1:
            x = np.sort(rng.choice(len(s.tid_to_gid), size=na, replace=False)).astype(np.uint32)
        else:
            x = s.refs[start[r]:start[r] + s.na[r]]
        nas.append(len(x))
        refs.append(x)
    return synth.SynthRad(s.cell_nrec, s.cell_bc, s.umi, np.asarray(nas, np.int64), np.concatenate(refs).astype(np.uint32), s.tid_to_gid,
                          s.num_genes, s.num_rows, s.usa, s.umi_len)


def batch(s, bw, uw, e, bc=None):
    """(position bytes, offsets), (twin bytes, offsets) of synth batch s with bw/uw-byte barcode/UMI fields."""
    bc = _narrow(s.cell_bc, bw) if bc is None else np.asarray(bc, np.uint64)
    umi = _narrow(s.umi, uw)
    p = rad.encode_cells_np(s.cell_nrec, bc, umi, s.na, s.refs, bc_bytes=bw, umi_bytes=uw, pos_bytes=e)
    t = rad.encode_cells_np(s.cell_nrec, bc, umi, s.na, s.refs, bc_bytes=bw, umi_bytes=uw)
    return p, t


def quant(cfg, t2g, b, off, e=0, how="submit", env=None, monkeypatch=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    q = pkg.Quantifier(cfg, t2g, aln_extra_bytes=e)
    try:
        if how == "submit":
            q.submit(b, off)
        elif how == "pinned":
            import torch

            h = torch.from_numpy(np.asarray(b, np.uint8).copy()).pin_memory()
            q.submit_ptr(h.data_ptr(), h.numel(), off)
        else:
            import torch

            d = torch.from_numpy(np.asarray(b, np.uint8).copy()).cuda()
            q.submit_device(d.data_ptr(), d.numel(), off)
            torch.cuda.synchronize()
        got = q.collect()
        return got, q.batch_stats(), q.pool_regrow_count()
    finally:
        q.close()
        for k in (env or {}):
            monkeypatch.delenv(k, raising=False)


def assert_same_extras(a, b, cfg):
    if cfg.dump_eq:
        for f in ("cell_ptr", "label_ptr", "labels", "count"):
            assert np.array_equal(getattr(a.eqclasses, f), getattr(b.eqclasses, f)), f
    if cfg.num_bootstraps:
        for f in ("mean_ptr", "mean_col", "var_ptr", "var_col"):
            assert np.array_equal(getattr(a.bootstraps, f), getattr(b.bootstraps, f)), f
        for f in ("mean_val", "var_val"):
            assert np.array_equal(getattr(a.bootstraps, f).view(np.uint32), getattr(b.bootstraps, f).view(np.uint32)), f


# (bw, uw, e, umi_len): 1- and 2-byte fields (k_widen's rewrite in the same pass), an 8-byte UMI field, and each pos width
LAYOUTS = [(4, 4, 1, 12), (1, 2, 2, 8), (2, 1, 4, 4), (4, 8, 8, 12), (8, 4, 4, 12)]


@pytest.mark.parametrize("bw,uw,e,umi_len", LAYOUTS)
@pytest.mark.parametrize("usa", [False, True])
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_position_records_equal_their_twin(oracle, res, usa, bw, uw, e, umi_len):
    """Cells below small_thresh, of at most 250 reads and large; records of 1 to 49 alignments (they cross the walk's 256-byte
    windows); every resolution, USA and not, -d classes and bootstraps under a fixed seed for the -em resolutions."""
    s = synth.synth(300 + 10 * e + bw + uw, [3000, 700, 250, 120, 99, 40, 7, 1], num_genes=150, txp_per_gene=3, usa=usa, umi_len=umi_len,
                    dup=0.4, cross=0.3, umi_err=0.03, max_extra_na=6)
    s = long_reads(s)
    assert s.na.max() >= 40 and s.na.min() >= 1
    bc = [3 + 5 * i for i in range(len(s.cell_nrec))] if bw == 1 else None
    (bp, op), (bt, ot) = batch(s, bw, uw, e, bc)
    kw = dict(bc_bytes=bw, umi_bytes=uw, umi_len=umi_len)
    if res in EM:
        kw.update(dump_eq=True, num_bootstraps=3, boot_seed=41)
    cfg = cfg_for(s, res, **kw)
    got, st, _ = quant(cfg, s.tid_to_gid, bp, op, e)
    twin, st_t, _ = quant(cfg, s.tid_to_gid, bt, ot)
    assert_same_result(got, twin, what=f"{res} usa={usa} {bw}/{uw}/{e}")
    assert_same_extras(got, twin, cfg)
    assert st["n_records"] == st_t["n_records"] == int(s.cell_nrec.sum())
    assert all(st[k] == st_t[k] for k in ("n_ref_words", "n_keys", "n_buckets", "n_overflow_buckets")), (st, st_t)
    assert st["input_bytes"] == len(bp) and len(bp) == len(bt) + e * int(s.na.sum())
    want = oracle.quant(cfg, s.tid_to_gid, bt, ot)
    assert_same_result(got, want, what="oracle")
    assert got.val.sum() > 0


@pytest.mark.parametrize("how", ["submit", "pinned", "device"])
@pytest.mark.parametrize("res,e", [("cr-like", 4), ("parsimony-em", 1), ("cr-like-em", 2), ("parsimony", 8)])
def test_every_submit_path_at_odd_offsets_in_many_ranges(oracle, monkeypatch, how, res, e):
    """Pageable, pinned and device input; chunks at offsets that are not dword aligned (1-3 bytes of padding in front of each);
    a batch cut into a dozen ranges, each of which strips its own cells."""
    sizes = [1500, 900, 700, 650, 600, 500, 450, 400, 300, 250, 200, 150, 120, 110, 90, 60, 30, 8, 2, 1]
    s = long_reads(synth.synth(77 + e, sizes, num_genes=300, txp_per_gene=3, umi_len=10, dup=0.4, cross=0.3, umi_err=0.03, max_extra_na=6), 31, 41)
    (bp, op), (bt, ot) = batch(s, 4, 4, e)
    ends = list(op[1:]) + [len(bp)]
    parts, offs, pos = [], [], 0
    for i, (a, b) in enumerate(zip(op, ends)):
        pad = 1 + i % 3
        parts.append(np.full(pad, 0xEE, np.uint8)); pos += pad
        offs.append(pos)
        parts.append(np.asarray(bp[int(a):int(b)], np.uint8)); pos += int(b) - int(a)
    parts.append(np.zeros(3, np.uint8))
    b2, o2 = np.concatenate(parts), np.asarray(offs, np.uint64)
    cfg = cfg_for(s, res, umi_len=10)
    env = {"AFQ_TEST_RANGE_BYTES": str(1 << 20)}
    got, st, _ = quant(cfg, s.tid_to_gid, b2, o2, e, how, env, monkeypatch)
    twin, _, _ = quant(cfg, s.tid_to_gid, bt, ot)
    assert_same_result(got, twin, what=how)
    assert_same_result(got, oracle.quant(cfg, s.tid_to_gid, bt, ot), what="oracle")
    assert st["n_records"] == sum(sizes) and st["n_fallback_cells"] == 0, st


@pytest.mark.parametrize("how", ["submit", "device"])
def test_parsimony_reruns_strip_again(oracle, monkeypatch, how):
    """finish_range's re-runs (a pool that ran out on a full device: halvings, regrows) make the copy again for every part."""
    from test_gpu_pool_rerun import dense_batch, full_device

    s = dense_batch(False, "middle")
    cfg = cfg_for(s, "parsimony-em", small_thresh=0, dump_eq=True)
    (bp, op), (bt, ot) = batch(s, 4, 4, 4)
    env = full_device(s.cell_nrec, cfg)
    got, _, regrows = quant(cfg, s.tid_to_gid, bp, op, 4, how, env, monkeypatch)
    assert regrows > 0
    twin, _, _ = quant(cfg, s.tid_to_gid, bt, ot)
    assert_same_result(got, twin)
    assert_same_extras(got, twin, cfg)
    assert_same_result(got, oracle.quant(cfg, s.tid_to_gid, bt, ot), what="oracle")


def test_bad_position_chunks_are_refused_and_the_context_goes_on(oracle):
    s = synth.synth(61, [400, 120, 30, 5], num_genes=80, max_extra_na=10)
    cfg = cfg_for(s, "cr-like")
    (bp, op), (bt, ot) = batch(s, 4, 4, 4)
    q = pkg.Quantifier(cfg, s.tid_to_gid, aln_extra_bytes=4)
    try:
        # cell 2 four bytes longer: its alignments no longer tile it at 8 bytes each - found on the host
        b = bytearray(bp)
        o2 = int(op[2])
        nb = int.from_bytes(b[o2:o2 + 4], "little")
        b[o2:o2 + 4] = (nb + 4).to_bytes(4, "little")
        b[o2 + nb:o2 + nb] = b"\0\0\0\0"
        off = op.copy()
        off[3:] += np.uint64(4)
        with pytest.raises(pkg.AfqError) as ei:
            q.quant_chunks(bytes(b), off)
        assert ei.value.code == pkg._abi.AFQ_ERR_BAD_INPUT and "cell 2:" in str(ei.value) and "8 bytes" in str(ei.value)
        # cell 1: the total divides, but its first record claims one more alignment and its last one fewer - the chain overruns
        # the chunk; found by the walk on the device
        b = bytearray(bp)
        o1 = int(op[1])
        na0 = int.from_bytes(b[o1 + 8:o1 + 12], "little")
        b[o1 + 8:o1 + 12] = (na0 + 1).to_bytes(4, "little")
        for how in ("submit", "device"):
            with pytest.raises(pkg.AfqError) as ei:
                if how == "submit":
                    q.quant_chunks(bytes(b), op)
                else:
                    import torch

                    d = torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).cuda()
                    q.submit_device(d.data_ptr(), d.numel(), op)
                    q.collect()
            assert ei.value.code == pkg._abi.AFQ_ERR_BAD_INPUT and "cell 1:" in str(ei.value), (how, str(ei.value))
        got = q.quant_chunks(bp, op)
    finally:
        q.close()
    assert_same_result(got, oracle.quant(cfg, s.tid_to_gid, bt, ot))


def test_set_aln_extra_bytes_states(oracle):
    s = synth.synth(62, [300, 50], num_genes=40)
    (bp, op), (bt, ot) = batch(s, 4, 4, 2)
    q = pkg.Quantifier(cfg_for(s, "cr-like"), s.tid_to_gid)
    try:
        for bad in (3, 16):
            with pytest.raises(pkg.AfqError) as ei:
                q.set_aln_extra_bytes(bad)
            assert ei.value.code == pkg._abi.AFQ_ERR_INVALID_ARG
        q.set_aln_extra_bytes(2)
        q.submit(bp, op)
        with pytest.raises(pkg.AfqError) as ei:
            q.set_aln_extra_bytes(0)   # a batch is pending
        assert ei.value.code == pkg._abi.AFQ_ERR_STATE
        got = q.collect()
        q.set_aln_extra_bytes(0)
        twin = q.quant_chunks(bt, ot)
    finally:
        q.close()
    assert_same_result(got, twin)
    # multi-barcode records of unequal widths (afq_config.bc_split) with positions
    import ctypes as C

    lib = pkg.load_library()
    ccfg = cfg_for(s, "cr-like", bc_bytes=6, bc_split=2).to_c()
    assert (ccfg.bc_bytes, ccfg.bc_split) == (6, 2)
    t2g = np.ascontiguousarray(s.tid_to_gid, np.uint32)
    h = C.c_void_p()
    assert lib.afq_create(C.byref(ccfg), t2g.ctypes.data_as(C.POINTER(C.c_uint32)), len(t2g), 0, C.byref(h)) == 0
    try:
        assert lib.afq_set_aln_extra_bytes(h, 4) == pkg._abi.AFQ_ERR_UNSUPPORTED
        assert b"multi-barcode" in lib.afq_last_error(h)
        assert lib.afq_set_aln_extra_bytes(h, 0) == 0
    finally:
        lib.afq_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------------
def make_dir(tmp, s, e, compressed):
    b, off = rad.encode_cells_np(s.cell_nrec, s.cell_bc, s.umi, s.na, s.refs, pos_bytes=e)
    G = s.num_rows // 3 if s.usa else s.num_genes
    names = [f"T{t}" for t in range(len(s.tid_to_gid))]
    rows = []
    for t, gid in enumerate(s.tid_to_gid.tolist()):
        rows.append((names[t], f"G{gid >> 1}", "S" if gid % 2 == 0 else "U") if s.usa else (names[t], f"G{gid}"))
    assert len(set(r[1] for r in rows)) == G
    return rad.write_quant_input_dir(str(tmp), np.asarray(b).tobytes(), len(off), names, rows, cblen=16, ulen=s.umi_len,
                                     compressed=compressed, pos_bytes=e)


def _strip_paths(meta, dirs):
    if isinstance(meta, dict):
        return {k: _strip_paths(v, dirs) for k, v in meta.items() if k not in ("cmd", "cmdline")}
    if isinstance(meta, list):
        return [_strip_paths(v, dirs) for v in meta]
    if isinstance(meta, str):
        for d in dirs:
            meta = meta.replace(d, "<dir>")
    return meta


@pytest.mark.parametrize("res,usa,extra", [("cr-like", False, ["-d", "--quant-subset"]), ("parsimony-em", True, ["-d", "-b", "4", "--boot-seed", "9"]),
                                           ("cr-like", True, ["--devices", "0,0"]), ("parsimony-em", False, ["-b", "4", "--boot-seed", "3", "--summary-stat"])])
@pytest.mark.parametrize("compressed", [False, True])
def test_afquant_cli_on_position_records(tmp_path, res, usa, extra, compressed):
    """`afquant quant` on a directory of position records (pos of 4 bytes; of 2 in the .rad.sz form) and on its twin: the same
    output files byte for byte; quant.json equal but for paths and the command line."""
    e = 2 if compressed else 4
    s = synth.synth(88, [2500, 700, 260, 120, 60, 7], num_genes=120, txp_per_gene=2, usa=usa, dup=0.5, cross=0.3, umi_err=0.02, max_extra_na=44)
    outs = []
    for kind, ee in (("pos", e), ("twin", 0)):
        d = tmp_path / kind
        tg = make_dir(d / "in", s, ee, compressed)
        args = list(extra)
        if "--quant-subset" in args:
            sub = tmp_path / "subset.txt"
            sub.write_text("\n".join(rad.int_to_seq(int(s.cell_bc[i]), 16) for i in (0, 2, 3, 5)) + "\n")
            args[args.index("--quant-subset")] = f"--quant-subset={sub}"
            args = [a for x in args for a in (x.split("=", 1) if x.startswith("--quant-subset=") else [x])]
        out = str(d / "out")
        r = subprocess.run([CLI, "quant", "-i", str(d / "in"), "-m", tg, "-o", out, "-r", res, "-t", "2"] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append((str(d), out))
    (dp, op_), (dt, ot) = outs
    files = ["alevin/quants_mat.mtx", "alevin/quants_mat_rows.txt", "alevin/quants_mat_cols.txt", "featureDump.txt"]
    if "-d" in extra:
        files += ["alevin/geqc_counts.mtx"]
    if "-b" in extra:
        files += ["alevin/bootstraps_mean.mtx", "alevin/bootstraps_var.mtx"]
    for f in files:
        a, b = open(os.path.join(op_, f), "rb").read(), open(os.path.join(ot, f), "rb").read()
        assert a == b, f
    if "-d" in extra:
        ga = gzip.open(os.path.join(op_, "alevin", "gene_eqclass.txt.gz")).read()
        assert ga == gzip.open(os.path.join(ot, "alevin", "gene_eqclass.txt.gz")).read() and len(ga) > 10
    assert len(open(os.path.join(op_, "alevin", "quants_mat.mtx")).read().splitlines()) > 10
    ma = _strip_paths(json.load(open(os.path.join(op_, "quant.json"))), [dp])
    mb = _strip_paths(json.load(open(os.path.join(ot, "quant.json"))), [dt])
    assert ma == mb


def test_afquant_cli_infer_on_the_dump_of_position_records(tmp_path):
    """`afquant infer` on what `quant -d` wrote for position records equals infer on the twin's."""
    s = synth.synth(89, [2000, 600, 150, 20], num_genes=80, txp_per_gene=2, usa=True, dup=0.5, cross=0.4, umi_err=0.02, max_extra_na=20)
    res = []
    for kind, e in (("pos", 8), ("twin", 0)):
        d = tmp_path / kind
        tg = make_dir(d / "in", s, e, False)
        out = d / "out"
        r = subprocess.run([CLI, "quant", "-i", str(d / "in"), "-m", tg, "-o", str(out), "-r", "cr-like", "-d"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([CLI, "infer", "-c", str(out / "alevin" / "geqc_counts.mtx"), "-e", str(out / "alevin" / "gene_eqclass.txt.gz"),
                            "-o", str(d / "inf"), "--usa"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        res.append(open(d / "inf" / "quants_mat.mtx", "rb").read())
    assert res[0] == res[1] and len(res[0].splitlines()) > 5
