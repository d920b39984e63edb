"""CPU tests of collated RAD records that carry a position per alignment (alignment tags compressed_ori_refid:u32, pos;
the reference's KnownRecordType::RnaShortPos, src/utils.rs:313-377): the codec in rad.py writes and reads them and their plain
twin, `afquant quant` classifies a prelude in the reference's order and refuses the kinds it does not take before any device
work, and afq_set_aln_extra_bytes validates its width."""
import ctypes as C
import os

import numpy as np
import pytest

from util import pkg

rad = pkg.rad
synth = pkg.synth


@pytest.fixture(scope="module")
def lib():
    L = pkg.load_library()
    L.afq_host_last_error.restype = C.c_char_p
    return L


def _narrow(v, width):
    return v if width == 8 else v & np.uint64((1 << (8 * width)) - 1)


@pytest.mark.parametrize("bw,uw,e", [(4, 4, 4), (1, 2, 1), (2, 1, 2), (4, 8, 8), (8, 4, 4), (2, 2, 8), (4, 4, 1)])
def test_position_records_round_trip_with_their_twin(bw, uw, e):
    s = synth.synth(3 + e, [40, 7, 120, 1], num_genes=60, max_extra_na=45)
    bc, umi = _narrow(s.cell_bc, bw), _narrow(s.umi, uw)
    bp, op = rad.encode_cells_np(s.cell_nrec, bc, umi, s.na, s.refs, bc_bytes=bw, umi_bytes=uw, pos_bytes=e)
    bt, ot = rad.encode_cells_np(s.cell_nrec, bc, umi, s.na, s.refs, bc_bytes=bw, umi_bytes=uw)
    n_aln = int(s.na.sum())
    assert len(bp) == len(bt) + e * n_aln
    # every chunk: nbytes = 8 + nrec * header + (4 + e) * alignments
    for i in range(len(op)):
        nb = int.from_bytes(bytes(bp[int(op[i]):int(op[i]) + 4]), "little")
        nbt = int.from_bytes(bytes(bt[int(ot[i]):int(ot[i]) + 4]), "little")
        assert (nb - 8 - int(s.cell_nrec[i]) * (4 + bw + uw)) % (4 + e) == 0
        assert nb - nbt == e * ((nbt - 8 - int(s.cell_nrec[i]) * (4 + bw + uw)) // 4)
    cells = []
    r = w = 0
    for ci, n in enumerate(s.cell_nrec.tolist()):
        reads = []
        for _ in range(n):
            na = int(s.na[r])
            reads.append((int(umi[r]), [int(x) for x in s.refs[w:w + na]]))
            r += 1
            w += na
        cells.append((int(bc[ci]), reads))
    pb, po = rad.encode_cells(cells, bw, uw, pos_bytes=e)
    tb, to = rad.encode_cells(cells, bw, uw)
    assert pb == bytes(bp) and tb == bytes(bt) and np.array_equal(po, op) and np.array_equal(to, ot)
    for i in range(len(op)):
        got = rad.decode_chunk(bytes(bp), int(op[i]), bw, uw, e)
        assert got == rad.decode_chunk(bytes(bt), int(ot[i]), bw, uw) == cells[i]
        _, with_pos = rad.decode_chunk(bytes(bp), int(op[i]), bw, uw, e, with_pos=True)
        for (u, refs, pos), (_, want_refs) in zip(with_pos, cells[i][1]):
            assert refs == want_refs and len(pos) == len(refs)
            assert pos == rad.default_positions(refs, np.arange(len(refs)), e).tolist()
    # positions given by the caller are written as given, and left out of the twin
    given = [(7, [(1, [3, 9], [0xAB, 0xCD]), (2, [], [])])]
    b1, _ = rad.encode_cells(given, bw, uw, pos_bytes=e)
    assert rad.decode_chunk(b1, 0, bw, uw, e, with_pos=True) == (7, [(1, [3, 9], [0xAB, 0xCD]), (2, [], [])])
    assert rad.encode_cells(given, bw, uw)[0] == rad.encode_cells([(7, [(1, [3, 9]), (2, [])])], bw, uw)[0]


def test_prelude_with_a_pos_tag():
    names = ["t0", "t1"]
    plain = rad.rad_prelude(names, 5, 16, 12)
    for e, tid in ((1, 1), (2, 2), (4, 3), (8, 4)):
        pre = rad.rad_prelude(names, 5, 16, 12, pos_bytes=e)
        tag = (20).to_bytes(2, "little") + b"compressed_ori_refid\x03"
        assert (2).to_bytes(2, "little") + tag + (3).to_bytes(2, "little") + b"pos" + bytes([tid]) in pre
        assert len(pre) == len(plain) + 6


class _Opts(C.Structure):
    _fields_ = [("input_dir", C.c_char_p), ("tg_map", C.c_char_p), ("output_dir", C.c_char_p), ("resolution", C.c_char_p),
                ("filter_list", C.c_char_p), ("cmdline", C.c_char_p), ("num_threads", C.c_uint32), ("small_thresh", C.c_uint32),
                ("umi_edit_dist", C.c_int32), ("large_graph_thresh", C.c_int32), ("init_uniform", C.c_uint32), ("dump_eq", C.c_uint32),
                ("num_bootstraps", C.c_uint32), ("device", C.c_uint32), ("batch_bytes", C.c_uint64), ("sa_model", C.c_uint32),
                ("summary_stat", C.c_uint32), ("boot_seed", C.c_uint64), ("devices", C.POINTER(C.c_int32)), ("n_devices", C.c_uint32),
                ("reserved", C.c_uint32)]


def _quantify(lib, in_dir, tg, out_dir):
    o = _Opts(str(in_dir).encode(), str(tg).encode(), str(out_dir).encode(), b"cr-like", None, b"test", 1, 100, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0,
              None, 0, 0)
    lib.afq_quantify.argtypes = [C.POINTER(_Opts)]
    lib.afq_quantify.restype = C.c_int
    rc = lib.afq_quantify(C.byref(o))
    return rc, lib.afq_host_last_error().decode()


def _aln_section(tags):
    out = len(tags).to_bytes(2, "little")
    for name, tid in tags:
        out += len(name).to_bytes(2, "little") + name.encode() + bytes([tid])
    return out


def test_quantify_classifies_record_kinds_in_the_reference_order(lib, tmp_path):
    """Long-read (as, start, end), scATAC (type, start_pos, frag_len), multi-barcode with positions and position tags that are not
    `compressed_ori_refid:u32, pos:<int>` are refused with their own messages; all of these fail before any device work, so
    no output directory is made."""
    s = synth.synth(9, [30, 20], num_genes=5)
    names = [f"t{i}" for i in range(len(s.tid_to_gid))]
    rows = [(names[i], f"g{int(s.tid_to_gid[i])}") for i in range(len(names))]
    b, off = rad.encode_cells_np(s.cell_nrec, s.cell_bc, s.umi, s.na, s.refs, pos_bytes=4)
    plain_aln = _aln_section([("compressed_ori_refid", 3)])
    pre = rad.rad_prelude(names, len(off), 16, 12)
    assert plain_aln in pre

    def run(name, prelude):
        d = tmp_path / name
        tg = rad.write_quant_input_dir(str(d), bytes(b), len(off), names, rows, prelude=prelude)
        out = tmp_path / (name + "_out")
        rc, msg = _quantify(lib, d, tg, out)
        assert not os.path.exists(out), name
        return rc, msg

    cases = [
        ("long_read", [("compressed_ori_refid", 3), ("as", 3), ("start", 3), ("end", 3)], "long-read"),
        ("long_read_with_pos", [("compressed_ori_refid", 3), ("pos", 3), ("as", 3), ("start", 3), ("end", 3)], "long-read"),
        ("atac", [("compressed_ori_refid", 3), ("type", 1), ("start_pos", 3), ("frag_len", 2)], 'the "atac" sub-command'),
        ("pos_float", [("compressed_ori_refid", 3), ("pos", 5)], "compressed_ori_refid:u32 followed by pos"),
        ("pos_first", [("pos", 3), ("compressed_ori_refid", 3)], "compressed_ori_refid:u32 followed by pos"),
        ("pos_and_more", [("compressed_ori_refid", 3), ("pos", 3), ("x", 3)], "compressed_ori_refid:u32 followed by pos"),
        ("ref_u16_pos", [("compressed_ori_refid", 2), ("pos", 3)], "compressed_ori_refid:u32 followed by pos"),
    ]
    for name, tags, needle in cases:
        rc, msg = run(name, pre.replace(plain_aln, _aln_section(tags)))
        assert rc == pkg._abi.AFQ_ERR_UNSUPPORTED and needle in msg, (name, rc, msg)
    # the scATAC prelude as piscem writes it: refused as the reference does (quant.rs:1973-1976), not for its read tags
    rc, msg = run("atac_piscem", rad.rad_prelude_atac(names, [1000] * len(names), len(off)))
    assert rc == pkg._abi.AFQ_ERR_UNSUPPORTED and 'To process atac-seq data, you should use the "atac" sub-command' in msg
    # multi-barcode records: the multi-barcode check comes first, and positions there are refused as such
    mb = rad.rad_prelude_multi_bc(names, len(off), 8, 16, 12)
    rc, msg = run("multi_bc_pos", mb.replace(plain_aln, _aln_section([("compressed_ori_refid", 3), ("pos", 3)])))
    assert rc == pkg._abi.AFQ_ERR_UNSUPPORTED and "multi-barcode" in msg and "positions" in msg
    # a tag section that only names some of the long-read tags is not long-read: it stays refused as an unknown layout
    rc, msg = run("partial_long", pre.replace(plain_aln, _aln_section([("compressed_ori_refid", 3), ("as", 3)])))
    assert rc == pkg._abi.AFQ_ERR_UNSUPPORTED and "alignment-level tags" in msg


def test_set_aln_extra_bytes_rejects_invalid_widths(lib):
    """The width is checked before the context: on a machine without a device, a NULL context shows which check failed."""
    lib.afq_set_aln_extra_bytes.argtypes = [C.c_void_p, C.c_uint32]
    lib.afq_set_aln_extra_bytes.restype = C.c_int
    lib.afq_last_error.argtypes = [C.c_void_p]
    lib.afq_last_error.restype = C.c_char_p
    for e in (3, 5, 6, 7, 9, 16, 0xFFFFFFFF):
        assert lib.afq_set_aln_extra_bytes(None, e) == pkg._abi.AFQ_ERR_INVALID_ARG
        assert b"aln_extra_bytes must be 0, 1, 2, 4 or 8" in lib.afq_last_error(None), e
    for e in (0, 1, 2, 4, 8):
        assert lib.afq_set_aln_extra_bytes(None, e) == pkg._abi.AFQ_ERR_INVALID_ARG
        assert b"null context" in lib.afq_last_error(None), e
