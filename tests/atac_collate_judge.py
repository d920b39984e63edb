"""`atac collate` restated in plain Python on bytes, from the reference's text (src/atac/collate.rs:10-28, 158, 719-723, 869-916 and
the record layout of tests/atac_integration.rs:110-121): the judge of afq_atac_collate_rad and of `afquant atac collate`.

  record     na u32, barcode (bc_bytes), na x {ref u32, type u8, start_pos u32, frag_len u16}: an alignment is 11 bytes.
  cells      the entries of permit_freq.bin, by count descending, then barcode ascending (collate.rs:158).
  kept       a record is kept iff it has exactly ONE alignment and its barcode is an observed key of the correction map
             (collate.rs:719-723): no orientation test, no map-type test, no range test.
  written    na = 1, the CORRECTED barcode, the 11 alignment bytes untouched.
  chunks     one per cell that kept a record, in the order of the cells; a cell that kept none has NO chunk (collate.rs:869-892) and
             the header's num_chunks is the number written (:896-916).
  order      inside a chunk: input order - by input chunk, then by record.  (The reference's order depends on thread timing; this
             one is a function of the input.)

The filter itself lives in libradicl, whose sources are not at hand: this restates collate.rs's own comments.  The records are
hopped here byte by byte; nothing of the package is imported."""

ALN = 11


def u(buf, at, width):
    return int.from_bytes(buf[at:at + width], "little")


def cell_order(permit_freq):
    """permit_freq: {barcode: count} or [(barcode, count)] -> the cells in output order"""
    pairs = list(permit_freq.items()) if isinstance(permit_freq, dict) else list(permit_freq)
    return [b for b, _ in sorted(pairs, key=lambda bn: (-bn[1], bn[0]))]


def records(buf, chunk_off, bc_bytes):
    """every record of every chunk, in input order: (chunk index, na, barcode, the bytes of its alignments)"""
    H = 4 + bc_bytes
    for ci, off in enumerate(chunk_off):
        off = int(off)
        nbytes, nrec = u(buf, off, 4), u(buf, off + 4, 4)
        p, end = off + 8, off + nbytes
        for _ in range(nrec):
            na = u(buf, p, 4)
            assert p + H + ALN * na <= end, ("chunk", ci, "a record runs past the chunk")
            yield ci, na, u(buf, p + 4, bc_bytes), bytes(buf[p + H:p + H + ALN * na])
            p += H + ALN * na
        assert p == end, ("chunk", ci, "the records do not tile the chunk")


def collate(buf, chunk_off, bc_bytes, corrections, cells):
    """-> {"bytes", "chunk_off" (n_out + 1), "nrec" (per output chunk), "cell" (per output chunk: index into cells), "stats"}.
    corrections: {observed: corrected}; cells: in output order, distinct."""
    index = {b: i for i, b in enumerate(cells)}
    assert len(index) == len(cells), "cells must be distinct"
    body = [bytearray() for _ in cells]
    count = [0] * len(cells)
    st = dict(n_records=0, n_unmapped=0, n_multimapped=0, n_uncorrected=0, n_kept=0, n_cells_out=0, n_cells_empty=0, out_bytes=0)
    for _, na, bc, alns in records(buf, chunk_off, bc_bytes):
        st["n_records"] += 1
        if na == 0:
            st["n_unmapped"] += 1
        elif na > 1:
            st["n_multimapped"] += 1
        elif bc not in corrections:
            st["n_uncorrected"] += 1
        else:
            cell = index[corrections[bc]]
            st["n_kept"] += 1
            body[cell] += (1).to_bytes(4, "little") + int(cells[cell]).to_bytes(bc_bytes, "little") + alns
            count[cell] += 1
    out, offs, nrec, which = bytearray(), [], [], []
    for i, (b, n) in enumerate(zip(body, count)):
        if n == 0:
            continue
        offs.append(len(out))
        nrec.append(n)
        which.append(i)
        out += (len(b) + 8).to_bytes(4, "little") + n.to_bytes(4, "little") + b
    offs.append(len(out))
    st["n_cells_out"], st["n_cells_empty"], st["out_bytes"] = len(nrec), len(cells) - len(nrec), len(out)
    return {"bytes": bytes(out), "chunk_off": offs, "nrec": nrec, "cell": which, "stats": st}
