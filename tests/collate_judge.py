"""`collate` restated in plain Python on bytes, from the reference's text (src/collate.rs:129-289, 483-643,
docs/source/collate.rst, docs/source/generate_permit_list.rst:9-12): the judge of afq_collate_rad and of `afquant collate`.

  cells      the entries of permit_freq.bin, by count descending, then barcode ascending (collate.rs:270-274); the output has exactly
             one chunk per cell, in that order.
  kept       a record is kept iff it is compatible with expected_ori (both: always; fw: some alignment word has bit 31 set; rc:
             some has it clear; na == 0 only under both) and its barcode is an observed key of the correction map.
  written    na' (the number of kept alignments), the CORRECTED barcode, the UMI unchanged, and only the alignments that fit
             expected_ori, in input order, each word untouched (bit 31 stays) with its position bytes.
  order      inside a chunk: input order - by input chunk, then by record.
  empty      a cell that receives no record is a header-only chunk: nbytes 8, nrec 0.

The input records are hopped here, byte by byte; nothing goes through rad.decode_chunk, which strips bit 31."""

BOTH, FW, RC = "both", "fw", "rc"
ORI = {"both": BOTH, "either": BOTH, "fw": FW, "rc": RC, 0: BOTH, 1: FW, 2: RC}


def u(buf, at, width):
    return int.from_bytes(buf[at:at + width], "little")


def fits(word, ori):
    return ori == BOTH or (word >> 31 == 1) == (ori == FW)


def cell_order(permit_freq):
    """permit_freq: {barcode: count} or [(barcode, count)] -> the cells in output order"""
    pairs = list(permit_freq.items()) if isinstance(permit_freq, dict) else list(permit_freq)
    return [b for b, _ in sorted(pairs, key=lambda bn: (-bn[1], bn[0]))]


def records(buf, chunk_off, bc_bytes, umi_bytes, pos_bytes):
    """every record of every chunk, in input order: (chunk index, bc, head bytes behind na, [alignment bytes, ...])"""
    H, A = 4 + bc_bytes + umi_bytes, 4 + pos_bytes
    for ci, off in enumerate(chunk_off):
        off = int(off)
        nbytes, nrec = u(buf, off, 4), u(buf, off + 4, 4)
        p, end = off + 8, off + nbytes
        for _ in range(nrec):
            na = u(buf, p, 4)
            assert p + H + A * na <= end, ("chunk", ci, "a record runs past the chunk")
            yield ci, u(buf, p + 4, bc_bytes), bytes(buf[p + 4 + bc_bytes:p + H]), [bytes(buf[p + H + A * j:p + H + A * (j + 1)]) for j in range(na)]
            p += H + A * na
        assert p == end, ("chunk", ci, "the records do not tile the chunk")


def collate(buf, chunk_off, bc_bytes, umi_bytes, pos_bytes, expected_ori, corrections, cells, lane_alns=None):
    """-> {"bytes", "chunk_off" (n_cells + 1), "nrec" (per cell), "stats"}.  corrections: {observed: corrected}; cells: in output
    order, distinct.  lane_alns: afq_collate_limits' long-record threshold, for stats["n_long_records"] only."""
    ori = ORI[expected_ori]
    index = {b: i for i, b in enumerate(cells)}
    assert len(index) == len(cells), "cells must be distinct"
    body = [bytearray() for _ in cells]
    nrec = [0] * len(cells)
    st = dict(n_records=0, n_compatible=0, n_uncorrected=0, n_kept=0, n_alignments_in=0, n_alignments_kept=0, n_long_records=0, out_bytes=0)
    for _, bc, umi, alns in records(buf, chunk_off, bc_bytes, umi_bytes, pos_bytes):
        st["n_records"] += 1
        st["n_alignments_in"] += len(alns)
        if lane_alns is not None and len(alns) > lane_alns:
            st["n_long_records"] += 1
        keep = [a for a in alns if fits(u(a, 0, 4), ori)]
        if not (ori == BOTH or keep):
            continue
        st["n_compatible"] += 1
        if bc not in corrections:
            st["n_uncorrected"] += 1
            continue
        cell = index[corrections[bc]]
        st["n_kept"] += 1
        st["n_alignments_kept"] += len(keep)
        body[cell] += len(keep).to_bytes(4, "little") + int(cells[cell]).to_bytes(bc_bytes, "little") + umi + b"".join(keep)
        nrec[cell] += 1
    out, offs = bytearray(), []
    for b, n in zip(body, nrec):
        offs.append(len(out))
        out += (len(b) + 8).to_bytes(4, "little") + n.to_bytes(4, "little") + b
    offs.append(len(out))
    st["out_bytes"] = len(out)
    return {"bytes": bytes(out), "chunk_off": offs, "nrec": nrec, "stats": st}
