"""Collated-RAD chunk codec (host side, numpy).

Wire format as witnessed in the reference (paths relative to /root/reference):
  chunk   = nbytes:u32 (includes this 8-byte header), nrec:u32, records   src/convert.rs:473-481
  record  = na:u32, bc:<u8|u16|u32|u64>, umi:<u8|u16|u32|u64>, na x u32    src/convert.rs:124-144
            alignment word = orientation<<31 | ref_id                      src/convert.rs:443-445
  widths  = by sequence length 1-4 / 5-8 / 9-16 / 17-32 nt                 src/convert.rs:323-344
  2-bit   = A0 C1 G2 T3, first base most significant                       src/convert.rs:75-90
In a collated file one chunk holds all records of one corrected cell barcode.
Records with positions (alignment tags compressed_ori_refid:u32, pos:<1|2|4|8 bytes>; KnownRecordType::RnaShortPos,
src/utils.rs:313-377) hold `na x (u32, pos)`: the alignment tags of each alignment in prelude order.  `pos_bytes` below is
the width of that pos tag (0 = plain records); the same cells written with pos_bytes=0 are the positions' plain twin.
"""
from __future__ import annotations

import numpy as np

_NT = "ACGT"


def width_for_len(n_nt: int) -> int:
    """Bytes of the integer type the reference picks for an n_nt-long barcode/UMI."""
    if 1 <= n_nt <= 4:
        return 1
    if n_nt <= 8:
        return 2
    if n_nt <= 16:
        return 4
    if n_nt <= 32:
        return 8
    raise ValueError("cannot encode a sequence longer than 32 nt")


def seq_to_int(s: str) -> int:
    v = 0
    for ch in s:
        v = (v << 2) | (0 if ch == "N" else _NT.index(ch))
    return v


def int_to_seq(v: int, n_nt: int) -> str:
    return "".join(_NT[(v >> (2 * (n_nt - 1 - i))) & 3] for i in range(n_nt))


def default_positions(refs, within, pos_bytes: int):
    """Positions for reads that come without any: a value per alignment (ref id, index in its read) that fills the field."""
    r = np.asarray(refs, dtype=np.uint64)
    with np.errstate(over="ignore"):
        v = (r * np.uint64(0x9E3779B97F4A7C15) + np.asarray(within, dtype=np.uint64) * np.uint64(0xBF58476D1CE4E5B9)) >> np.uint64(7)
    return v & np.uint64((1 << (8 * pos_bytes)) - 1 if pos_bytes < 8 else 0xFFFFFFFFFFFFFFFF)


def encode_cells(cells, bc_bytes: int = 4, umi_bytes: int = 4, fw_bit: bool = True, pos_bytes: int = 0):
    """cells: list of (bc, [(umi, [ref, ...]) or (umi, [ref, ...], [pos, ...]), ...]).  Returns (bytes, chunk_off[u64]).

    Generic (any field width) pure-python encoder for small hand-written cases.  pos_bytes > 0: records with positions (each
    alignment word followed by its pos, default_positions when a read has none); pos_bytes = 0: the plain records (any
    positions given are left out - the twin).
    """
    out = bytearray()
    offs = []
    for bc, reads in cells:
        offs.append(len(out))
        body = bytearray()
        for read in reads:
            umi, refs = read[0], read[1]
            body += int(len(refs)).to_bytes(4, "little")
            body += int(bc).to_bytes(bc_bytes, "little")
            body += int(umi).to_bytes(umi_bytes, "little")
            if pos_bytes:
                pos = read[2] if len(read) > 2 else default_positions(refs, np.arange(len(refs)), pos_bytes)
            for j, r in enumerate(refs):
                w = int(r) | (0x80000000 if fw_bit else 0)
                body += w.to_bytes(4, "little")
                if pos_bytes:
                    body += int(pos[j]).to_bytes(pos_bytes, "little")
        out += (len(body) + 8).to_bytes(4, "little") + len(reads).to_bytes(4, "little") + body
    return bytes(out), np.asarray(offs, dtype=np.uint64)


def _put_le(out, at, vals, width):
    """out[at + k] = byte k of vals (little endian), k < width."""
    v = np.asarray(vals, dtype=np.uint64)
    for k in range(width):
        out[at + k] = ((v >> np.uint64(8 * k)) & np.uint64(0xFF)).astype(np.uint8)


def _encode_general_np(cell_nrec, cell_bc, umi, na, refs, fw_bits, bc_bytes, umi_bytes, pos_bytes, pos):
    """encode_cells_np for any field widths and pos width: byte-level scatter."""
    hdr = 4 + bc_bytes + umi_bytes
    stride = 4 + pos_bytes
    n_reads = len(na)
    n_cells = len(cell_nrec)
    cell_of_read = np.repeat(np.arange(n_cells), cell_nrec)
    rec_len = hdr + stride * na
    first_read = np.concatenate(([0], np.cumsum(cell_nrec)[:-1])).astype(np.int64)
    ends = np.cumsum(rec_len)
    starts = ends - rec_len
    cell_body = np.zeros(n_cells, np.int64)
    nz = cell_nrec > 0
    if n_reads:
        cell_body[nz] = np.add.reduceat(rec_len, first_read[nz])
    chunk_nb = cell_body + 8
    chunk_off = np.concatenate(([0], np.cumsum(chunk_nb)[:-1])).astype(np.int64)
    # record offset: its chunk's body start + the bytes of the cell's records in front of it
    cell_first_start = np.zeros(n_cells, np.int64)
    if n_reads:
        cell_first_start[nz] = starts[first_read[nz]]
    rec_off = chunk_off[cell_of_read] + 8 + (starts - cell_first_start[cell_of_read])
    out = np.zeros(int(chunk_nb.sum()), np.uint8)
    _put_le(out, chunk_off, chunk_nb, 4)
    _put_le(out, chunk_off + 4, cell_nrec, 4)
    _put_le(out, rec_off, na, 4)
    _put_le(out, rec_off + 4, np.asarray(cell_bc, dtype=np.uint64)[cell_of_read], bc_bytes)
    _put_le(out, rec_off + 4 + bc_bytes, umi, umi_bytes)
    read_of_ref = np.repeat(np.arange(n_reads), na)
    ref_start = np.concatenate(([0], np.cumsum(na)[:-1])).astype(np.int64)
    within = np.arange(len(refs)) - ref_start[read_of_ref]
    at = rec_off[read_of_ref] + hdr + stride * within
    rw = np.asarray(refs, dtype=np.uint64) & np.uint64(0x7FFFFFFF)
    rw |= (np.uint64(1) if fw_bits is None else np.asarray(fw_bits, dtype=np.uint64)) << np.uint64(31)
    _put_le(out, at, rw, 4)
    if pos_bytes:
        _put_le(out, at + 4, default_positions(refs, within, pos_bytes) if pos is None else pos, pos_bytes)
    return out, chunk_off.astype(np.uint64)


def encode_cells_np(cell_nrec, cell_bc, umi, na, refs, fw_bits=None, bc_bytes=4, umi_bytes=4, pos_bytes=0, pos=None):
    """Vectorised encoder, by default for the 10x-v3 layout (u32 barcode, u32 UMI).

    cell_nrec[n_cells], cell_bc[n_cells]; per read umi[], na[]; refs[] = concatenated,
    sorted-ascending ref ids.  Returns (uint8 array, chunk_off[u64]).  Other barcode / UMI widths and records with
    positions (pos_bytes > 0; pos[] per alignment, default_positions when None) take a byte-level path.
    """
    cell_nrec = np.asarray(cell_nrec, dtype=np.int64)
    na = np.asarray(na, dtype=np.int64)
    n_reads = int(cell_nrec.sum())
    assert n_reads == len(na) == len(umi)
    if (bc_bytes, umi_bytes, pos_bytes) != (4, 4, 0):
        return _encode_general_np(cell_nrec, cell_bc, umi, na, refs, fw_bits, bc_bytes, umi_bytes, pos_bytes, pos)
    n_cells = len(cell_nrec)
    cell_of_read = np.repeat(np.arange(n_cells), cell_nrec)
    rec_words = 3 + na
    # word offset of each record: preceding record words + 2 header words per started cell
    rec_off = np.concatenate(([0], np.cumsum(rec_words)[:-1])) + 2 * (cell_of_read + 1)
    total_words = int(rec_words.sum()) + 2 * n_cells
    w = np.zeros(total_words, dtype=np.uint32)
    # chunk headers
    first_read = np.concatenate(([0], np.cumsum(cell_nrec)[:-1]))
    cell_words = np.add.reduceat(rec_words, first_read[cell_nrec > 0]) if n_reads else np.zeros(0, np.int64)
    cw = np.zeros(n_cells, dtype=np.int64)
    cw[cell_nrec > 0] = cell_words
    chunk_word_off = np.concatenate(([0], np.cumsum(cw + 2)[:-1]))
    w[chunk_word_off] = ((cw + 2) * 4).astype(np.uint32)
    w[chunk_word_off + 1] = cell_nrec.astype(np.uint32)
    w[rec_off] = na.astype(np.uint32)
    w[rec_off + 1] = np.asarray(cell_bc, dtype=np.uint64)[cell_of_read].astype(np.uint32)
    w[rec_off + 2] = np.asarray(umi, dtype=np.uint64).astype(np.uint32)
    ref_start = np.concatenate(([0], np.cumsum(na)[:-1]))
    # position of each ref word
    read_of_ref = np.repeat(np.arange(n_reads), na)
    within = np.arange(len(refs)) - ref_start[read_of_ref]
    rw = np.asarray(refs, dtype=np.uint32).copy()
    if fw_bits is None:
        rw |= np.uint32(0x80000000)
    else:
        rw |= np.asarray(fw_bits, dtype=np.uint32) << np.uint32(31)
    w[rec_off[read_of_ref] + 3 + within] = rw
    return w.view(np.uint8), (chunk_word_off * 4).astype(np.uint64)


def decode_chunk(buf: bytes, off: int, bc_bytes: int, umi_bytes: int, pos_bytes: int = 0, with_pos: bool = False):
    """Returns (bc, [(umi, [ref...])...]) for the chunk starting at off; pos_bytes: records with positions of that width
    (with_pos: reads are (umi, [ref...], [pos...]))."""
    nbytes = int.from_bytes(buf[off : off + 4], "little")
    nrec = int.from_bytes(buf[off + 4 : off + 8], "little")
    p = off + 8
    reads = []
    bc0 = None
    st = 4 + pos_bytes
    for _ in range(nrec):
        na = int.from_bytes(buf[p : p + 4], "little")
        bc = int.from_bytes(buf[p + 4 : p + 4 + bc_bytes], "little")
        umi = int.from_bytes(buf[p + 4 + bc_bytes : p + 4 + bc_bytes + umi_bytes], "little")
        p += 4 + bc_bytes + umi_bytes
        refs = [int.from_bytes(buf[p + st * j : p + st * j + 4], "little") & 0x7FFFFFFF for j in range(na)]
        pos = [int.from_bytes(buf[p + st * j + 4 : p + st * j + st], "little") for j in range(na)]
        p += st * na
        if bc0 is None:
            bc0 = bc
        reads.append((umi, refs, pos) if with_pos else (umi, refs))
    assert p == off + nbytes, "chunk nbytes does not match its records"
    return bc0, reads


def chunk_offsets(buf, start: int = 0):
    """Hop the nbytes headers of back-to-back chunks (what the quant producer does)."""
    b = np.frombuffer(buf, dtype=np.uint8)
    offs = []
    p = start
    while p + 8 <= len(b):
        nbytes = int(b[p : p + 4].view(np.uint32)[0])
        if nbytes < 8:
            raise ValueError("corrupt chunk header")
        offs.append(p)
        p += nbytes
    if p != len(b):
        raise ValueError("trailing bytes after last chunk")
    return np.asarray(offs, dtype=np.uint64)


# ---------------------------------------------------------------------------
# whole-file writer (test fixtures / synthetic inputs for the host front-end)
_INT_TYPE_ID = {1: 1, 2: 2, 4: 3, 8: 4}  # bytes -> RadType id (U8..U64)


def rad_prelude(ref_names, num_chunks, cblen, ulen, bc_bytes=4, umi_bytes=4, is_paired=False, pos_bytes=0) -> bytes:
    """Header + the three tag sections + file-tag values of a single-barcode scRNA RAD file
    (order of writes in src/convert.rs:254-369).  pos_bytes > 0: records with positions - a second alignment tag `pos`,
    an integer of that width."""
    out = bytearray()
    out += bytes([1 if is_paired else 0])
    out += len(ref_names).to_bytes(8, "little")
    for n in ref_names:
        b = n.encode()
        out += len(b).to_bytes(2, "little") + b
    out += int(num_chunks).to_bytes(8, "little")

    def tag(name, type_id):
        b = name.encode()
        return len(b).to_bytes(2, "little") + b + bytes([type_id])

    out += (2).to_bytes(2, "little") + tag("cblen", 2) + tag("ulen", 2)  # file tags (u16, u16)
    out += (2).to_bytes(2, "little") + tag("b", _INT_TYPE_ID[bc_bytes]) + tag("u", _INT_TYPE_ID[umi_bytes])  # read tags
    if pos_bytes:
        out += (2).to_bytes(2, "little") + tag("compressed_ori_refid", 3) + tag("pos", _INT_TYPE_ID[pos_bytes])  # alignment tags
    else:
        out += (1).to_bytes(2, "little") + tag("compressed_ori_refid", 3)  # alignment tags
    out += int(cblen).to_bytes(2, "little") + int(ulen).to_bytes(2, "little")  # file tag values
    return bytes(out)


def rad_prelude_multi_bc(ref_names, num_chunks, b0len, b1len, ulen, b_bytes=4, umi_bytes=4, b0_bytes=None) -> bytes:
    """Prelude of a two-level multi-barcode (10x Flex) RAD file as the reference's tests build it
    (tests/multi_barcode_integration.rs:58-130): file tags num_barcodes, b0len, b1len, ulen (u16) and known_rad_type
    (string); read tags b0, b1, u; one u32 alignment tag."""
    out = bytearray()
    out += bytes([0])
    out += len(ref_names).to_bytes(8, "little")
    for n in ref_names:
        b = n.encode()
        out += len(b).to_bytes(2, "little") + b
    out += int(num_chunks).to_bytes(8, "little")

    def tag(name, type_id):
        b = name.encode()
        return len(b).to_bytes(2, "little") + b + bytes([type_id])

    out += (5).to_bytes(2, "little") + tag("num_barcodes", 2) + tag("b0len", 2) + tag("b1len", 2) + tag("ulen", 2) + tag("known_rad_type", 8)
    out += (3).to_bytes(2, "little") + tag("b0", _INT_TYPE_ID[b0_bytes or b_bytes]) + tag("b1", _INT_TYPE_ID[b_bytes]) + tag("u", _INT_TYPE_ID[umi_bytes])
    out += (1).to_bytes(2, "little") + tag("compressed_ori_refid", 3)
    kind = b"sc_rna_multi_bc"
    out += (2).to_bytes(2, "little") + int(b0len).to_bytes(2, "little") + int(b1len).to_bytes(2, "little") + int(ulen).to_bytes(2, "little")
    out += len(kind).to_bytes(2, "little") + kind
    return bytes(out)


def rad_prelude_atac(ref_names, ref_lengths, num_chunks, cblen=16, bc_bytes=4) -> bytes:
    """Prelude of a scATAC RAD file as piscem writes it and the reference's tests build it (tests/atac_integration.rs:75-131):
    paired flag set; file tags cblen (u16), known_rad_type (string), ref_lengths (array of u32, u32 length); read tag b;
    alignment tags ref:u32, type:u8, start_pos:u32, frag_len:u16."""
    out = bytearray()
    out += bytes([1])
    out += len(ref_names).to_bytes(8, "little")
    for n in ref_names:
        b = n.encode()
        out += len(b).to_bytes(2, "little") + b
    out += int(num_chunks).to_bytes(8, "little")

    def tag(name, type_id, extra=b""):
        b = name.encode()
        return len(b).to_bytes(2, "little") + b + bytes([type_id]) + extra

    out += (3).to_bytes(2, "little") + tag("cblen", 2) + tag("known_rad_type", 8) + tag("ref_lengths", 7, bytes([3, 3]))
    out += (1).to_bytes(2, "little") + tag("b", _INT_TYPE_ID[bc_bytes])
    out += (4).to_bytes(2, "little") + tag("ref", 3) + tag("type", 1) + tag("start_pos", 3) + tag("frag_len", 2)
    kind = b"sc_atac"
    out += int(cblen).to_bytes(2, "little") + len(kind).to_bytes(2, "little") + kind
    out += len(ref_lengths).to_bytes(4, "little") + b"".join(int(x).to_bytes(4, "little") for x in ref_lengths)
    return bytes(out)


def encode_atac_cells(cells, bc_bytes: int = 4):
    """cells: list of (bc, [[(ref, type, start, frag_len), ...] per record]).  Returns (bytes, chunk_off[u64])."""
    out = bytearray()
    offs = []
    for bc, recs in cells:
        offs.append(len(out))
        body = bytearray()
        for alns in recs:
            body += len(alns).to_bytes(4, "little") + int(bc).to_bytes(bc_bytes, "little")
            for ref, ty, start, fl in alns:
                body += int(ref).to_bytes(4, "little") + bytes([ty]) + int(start).to_bytes(4, "little") + int(fl).to_bytes(2, "little")
        out += (len(body) + 8).to_bytes(4, "little") + len(recs).to_bytes(4, "little") + body
    return bytes(out), np.asarray(offs, dtype=np.uint64)


def encode_atac_chunks(chunks, bc_bytes: int = 4):
    """chunks of an UNCOLLATED scATAC RAD: a list of chunks, each a list of records (bc, [(ref, type, start, frag_len), ...]) -
    a barcode per record.  Returns (bytes, chunk_off[u64])."""
    out = bytearray()
    offs = []
    for recs in chunks:
        offs.append(len(out))
        body = bytearray()
        for bc, alns in recs:
            body += len(alns).to_bytes(4, "little") + int(bc).to_bytes(bc_bytes, "little")
            for ref, ty, start, fl in alns:
                body += int(ref).to_bytes(4, "little") + bytes([ty]) + int(start).to_bytes(4, "little") + int(fl).to_bytes(2, "little")
        out += (len(body) + 8).to_bytes(4, "little") + len(recs).to_bytes(4, "little") + body
    return bytes(out), np.asarray(offs, dtype=np.uint64)


def encode_chunks(chunks, bc_bytes: int = 4, umi_bytes: int = 4, pos_bytes: int = 0, pad: int = 0):
    """chunks of an UNCOLLATED single-barcode RNA RAD, as the mapper writes them and generate-permit-list reads them: a list of
    chunks, each a list of records (bc, umi, [(ref, fw), ...]) - a barcode per record, the orientation in bit 31 of every
    alignment word (set = forward), pos_bytes zero bytes of position behind each.  `pad` bytes go in front of the first chunk
    (to place chunks at a chosen byte alignment).  Returns (bytes, chunk_off[u64])."""
    out = bytearray(pad)
    offs = []
    for recs in chunks:
        offs.append(len(out))
        body = bytearray()
        for bc, umi, alns in recs:
            body += len(alns).to_bytes(4, "little") + int(bc).to_bytes(bc_bytes, "little") + int(umi).to_bytes(umi_bytes, "little")
            if pos_bytes == 0 and len(alns) > 64:
                a = np.asarray(alns, dtype=np.int64).reshape(-1, 2)
                body += ((a[:, 0] & 0x7FFFFFFF) | (a[:, 1].astype(bool).astype(np.int64) << 31)).astype("<u4").tobytes()
                continue
            for ref, fw in alns:
                body += ((int(ref) & 0x7FFFFFFF) | (0x80000000 if fw else 0)).to_bytes(4, "little") + bytes(pos_bytes)
        out += (len(body) + 8).to_bytes(4, "little") + len(recs).to_bytes(4, "little") + body
    return bytes(out), np.asarray(offs, dtype=np.uint64)


def encode_multi_bc_chunks(chunks, b0_bytes: int = 2, b1_bytes: int = 4, umi_bytes: int = 4, pos_bytes: int = 0, pad: int = 0):
    """chunks of an UNCOLLATED two-barcode (10x Flex) RNA RAD, as multi-barcode generate-permit-list reads them: a list of chunks,
    each a list of records (b0, b1, umi, [(ref, fw), ...]) - the sample barcode b0 and the cell barcode b1 per record, in the order
    of the read-tag section (b0, b1, u); alignments, positions and `pad` as encode_chunks.  Returns (bytes, chunk_off[u64])."""
    out = bytearray(pad)
    offs = []
    for recs in chunks:
        offs.append(len(out))
        body = bytearray()
        for b0, b1, umi, alns in recs:
            body += len(alns).to_bytes(4, "little") + int(b0).to_bytes(b0_bytes, "little") + int(b1).to_bytes(b1_bytes, "little") + int(umi).to_bytes(umi_bytes, "little")
            if pos_bytes == 0 and len(alns) > 64:
                a = np.asarray(alns, dtype=np.int64).reshape(-1, 2)
                body += ((a[:, 0] & 0x7FFFFFFF) | (a[:, 1].astype(bool).astype(np.int64) << 31)).astype("<u4").tobytes()
                continue
            for ref, fw in alns:
                body += ((int(ref) & 0x7FFFFFFF) | (0x80000000 if fw else 0)).to_bytes(4, "little") + bytes(pos_bytes)
        out += (len(body) + 8).to_bytes(4, "little") + len(recs).to_bytes(4, "little") + body
    return bytes(out), np.asarray(offs, dtype=np.uint64)


NEIGHBORHOOD_TAGS = {"hamming-1": 0, "substitution-or-shift-1": 1}   # BarcodeNeighborhood's variants in declaration order


def _correction_spec_bytes(barcode_len, spec, neighborhood="hamming-1") -> bytes:
    """bincode of CorrectionSpec (src/barcode_correction.rs:28-37, 209-227).  spec: "unique" or
    ("frequency", (numerator, denominator), pseudocount); neighborhood: HammingOne (tag 0) or SubstitutionOrShiftOne (tag 1)."""
    out = bytes([barcode_len]) + NEIGHBORHOOD_TAGS[neighborhood].to_bytes(4, "little")
    if spec == "unique":
        return out + (0).to_bytes(4, "little")
    _, (num, den), pseudo = spec
    return out + (1).to_bytes(4, "little") + int(num).to_bytes(8, "little") + int(den).to_bytes(8, "little") + int(pseudo).to_bytes(8, "little")


def _corrections_bytes(pairs) -> bytes:
    a = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    return len(a).to_bytes(8, "little") + a.astype("<u8").tobytes()


def correction_plan_bytes(pairs, barcode_len: int = 16, spec="unique", sample_barcode_len=None, sample_scopes=(), version: int = 1,
                          magic: bytes = b"AFCORR\0\0", neighborhood="hamming-1") -> bytes:
    """correction_plan.bin (src/correction_plan.rs:20-45, 157-160): magic, u16 version, bincode of CorrectionPlan with one
    global cell scope holding `pairs` ((observed, corrected), written in observed order as write_to does).  sample_barcode_len /
    sample_scopes ((sample barcode, pairs), ...) make the sample-scoped shapes the ATAC reader refuses."""
    pairs = sorted((int(o), int(c)) for o, c in pairs)
    out = bytearray(magic) + int(version).to_bytes(2, "little")
    out += b"\x00" if sample_barcode_len is None else bytes([1, sample_barcode_len])
    out += bytes([barcode_len]) + b"\x00" + (0).to_bytes(8, "little")   # no sample spec, no sample corrections
    scopes = [(None, pairs)] + [(int(sb), sorted((int(o), int(c)) for o, c in pp)) for sb, pp in sample_scopes]
    out += len(scopes).to_bytes(8, "little")
    for sb, pp in scopes:
        out += b"\x00" if sb is None else b"\x01" + sb.to_bytes(8, "little")
        out += _correction_spec_bytes(barcode_len, spec, neighborhood) + _corrections_bytes(pp)
    return bytes(out)


def permit_map_bytes(pairs) -> bytes:
    """The legacy permit_map.bin: bincode HashMap<u64, u64> - a u64 count, then (observed, corrected) pairs."""
    return _corrections_bytes([(int(o), int(c)) for o, c in pairs])


def permit_freq_header(barcode_len: int, version: int = 1) -> bytes:
    """permit_freq.bin as far as `atac sort` reads it: u64 version, u64 barcode length, an empty bincode HashMap behind them."""
    return int(version).to_bytes(8, "little") + int(barcode_len).to_bytes(8, "little") + (0).to_bytes(8, "little")


def permit_freq_bytes(barcode_len: int, pairs, version: int = 1) -> bytes:
    """permit_freq.bin / all_freq.bin (write_permit_list_freq, src/utils.rs:431-452): u64 version, u64 barcode length, then the
    bincode HashMap<u64, u64> barcode -> count (a u64 length and the pairs, here in ascending key order)."""
    return int(version).to_bytes(8, "little") + int(barcode_len).to_bytes(8, "little") + _corrections_bytes(sorted((int(b), int(n)) for b, n in pairs))


def _read_pairs(buf, at):
    n = int.from_bytes(buf[at:at + 8], "little")
    at += 8
    if at + 16 * n > len(buf):
        raise ValueError("truncated pair list")
    a = np.frombuffer(buf, dtype="<u8", count=2 * n, offset=at).reshape(-1, 2)
    return [(int(o), int(c)) for o, c in a], at + 16 * n


def read_permit_freq(buf: bytes):
    """permit_freq.bin / all_freq.bin -> (version, barcode_len, {barcode: count}); the file must tile exactly."""
    pairs, end = _read_pairs(buf, 16)
    if end != len(buf) or len(dict(pairs)) != len(pairs):
        raise ValueError("permit frequency file: trailing data or a repeated key")
    return int.from_bytes(buf[0:8], "little"), int.from_bytes(buf[8:16], "little"), dict(pairs)


def read_permit_map(buf: bytes):
    """permit_map.bin -> {observed: corrected}; the file must tile exactly."""
    pairs, end = _read_pairs(buf, 0)
    if end != len(buf) or len(dict(pairs)) != len(pairs):
        raise ValueError("permit map: trailing data or a repeated key")
    return dict(pairs)


def read_correction_plan(buf: bytes):
    """correction_plan.bin with one global cell scope (what generate-permit-list writes for a single-barcode experiment) ->
    {"barcode_len", "neighborhood", "resolution" ("unique" or ("frequency", (num, den), pseudocount)), "corrections" [(observed,
    corrected), ...] in file order}; anything else raises."""
    if buf[:8] != b"AFCORR\0\0" or int.from_bytes(buf[8:10], "little") != 1:
        raise ValueError("correction plan: bad magic or version")
    at = 10
    if buf[at] != 0:
        raise ValueError("correction plan: sample-scoped")
    cell_len, has_sspec = buf[at + 1], buf[at + 2]
    at += 3
    if has_sspec or int.from_bytes(buf[at:at + 8], "little") != 0 or int.from_bytes(buf[at + 8:at + 16], "little") != 1 or buf[at + 16] != 0:
        raise ValueError("correction plan: not one global cell scope")
    at += 17
    spec_len, nbh, res = buf[at], int.from_bytes(buf[at + 1:at + 5], "little"), int.from_bytes(buf[at + 5:at + 9], "little")
    at += 9
    resolution = "unique"
    if res == 1:
        num, den, pseudo = (int.from_bytes(buf[at + 8 * k:at + 8 * k + 8], "little") for k in range(3))
        resolution = ("frequency", (num, den), pseudo)
        at += 24
    elif res != 0:
        raise ValueError("correction plan: unknown resolution")
    pairs, end = _read_pairs(buf, at)
    if end != len(buf) or spec_len != cell_len:
        raise ValueError("correction plan: trailing data or two barcode lengths")
    names = {v: k for k, v in NEIGHBORHOOD_TAGS.items()}
    return {"barcode_len": cell_len, "neighborhood": names[nbh], "resolution": resolution, "corrections": pairs}


def collation_manifest(groups, level_names=("sample", "cell")) -> bytes:
    """collation_manifest.bin in the layout csrc/afq_host.cpp reads (bincode of libradicl's CollationManifest - a
    restatement, libradicl's source is not in the reference tree).  groups: (key, name or None, chunk_start, num_chunks,
    num_records)."""
    out = bytearray()
    out += len(level_names).to_bytes(8, "little")
    for n in level_names:
        b = n.encode()
        out += len(b).to_bytes(8, "little") + b
    out += len(groups).to_bytes(8, "little")
    for key, name, start, nch, nrec in groups:
        out += int(key).to_bytes(8, "little")
        if name is None:
            out += b"\x00"
        else:
            b = name.encode()
            out += b"\x01" + len(b).to_bytes(8, "little") + b
        out += int(start).to_bytes(8, "little") + int(nch).to_bytes(8, "little") + int(nrec).to_bytes(8, "little")
    return bytes(out)


def _crc32c(data: bytes) -> int:
    tbl = getattr(_crc32c, "_t", None)
    if tbl is None:
        tbl = []
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
            tbl.append(c)
        _crc32c._t = tbl
    c = 0xFFFFFFFF
    for b in data:
        c = tbl[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def snappy_frame_encode(data: bytes, chunk: int = 60000, compress_literal: bool = True, real: bool = True) -> bytes:
    """Snappy *frame format* writer: stream identifier + one chunk per `chunk` bytes, alternating uncompressed
    chunks (type 0x01) and compressed chunks (type 0x00).  With `real` (and pyarrow importable) the compressed
    blocks come from Google's snappy through pyarrow - back-references and all, i.e. what
    `snap::write::FrameEncoder` (src/collate.rs:550-554) puts in a real file; otherwise they are literal-only blocks."""
    codec = None
    if real:
        try:
            import pyarrow as pa

            codec = pa.Codec("snappy") if pa.Codec.is_available("snappy") else None
        except Exception:  # noqa
            codec = None
    out = bytearray(b"\xff\x06\x00\x00sNaPpY")
    for k, i in enumerate(range(0, len(data), chunk)):
        piece = data[i : i + chunk]
        crc = _crc32c(piece)
        m = (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF
        if codec is not None and compress_literal and k % 2 == 1:
            body = m.to_bytes(4, "little") + codec.compress(bytes(piece), asbytes=True)
            out += b"\x00" + len(body).to_bytes(3, "little") + body
        elif compress_literal and k % 2 == 1:
            n = len(piece)
            blk = bytearray()
            v = n
            while True:  # uvarint of the uncompressed length
                if v < 0x80:
                    blk.append(v)
                    break
                blk.append((v & 0x7F) | 0x80)
                v >>= 7
            ln = n - 1
            if ln < 60:
                blk.append(ln << 2)
            elif ln < 256:
                blk += bytes([60 << 2, ln])
            elif ln < 65536:
                blk += bytes([61 << 2]) + ln.to_bytes(2, "little")
            else:
                blk += bytes([62 << 2]) + ln.to_bytes(3, "little")
            blk += piece
            body = m.to_bytes(4, "little") + bytes(blk)
            out += b"\x00" + len(body).to_bytes(3, "little") + body
        else:
            body = m.to_bytes(4, "little") + piece
            out += b"\x01" + len(body).to_bytes(3, "little") + body
    return bytes(out)


def write_quant_input_dir(path, chunk_bytes, n_chunks, ref_names, t2g_rows, cblen=16, ulen=12, bc_bytes=4, umi_bytes=4,
                          compressed=False, prelude=None, pos_bytes=0):
    """Lay out what `alevin-fry quant -i` expects: generate_permit_list.json, collate.json,
    map.collated.rad[.sz], plus the tg-map next to it.  t2g_rows: list of tab-separated row tuples.
    pos_bytes: the chunks hold records with positions of that width (the prelude says so)."""
    import json
    import os

    os.makedirs(path, exist_ok=True)
    if prelude is None:
        prelude = rad_prelude(ref_names, n_chunks, cblen, ulen, bc_bytes, umi_bytes, pos_bytes=pos_bytes)
    with open(os.path.join(path, "generate_permit_list.json"), "w") as f:
        json.dump({"velo_mode": False, "expected_ori": "fw"}, f)
    with open(os.path.join(path, "collate.json"), "w") as f:
        json.dump({"cmd": "synthetic", "version_str": "0.18.0", "compressed_output": bool(compressed)}, f)
    if compressed:
        with open(os.path.join(path, "map.collated.rad.sz"), "wb") as f:
            f.write(snappy_frame_encode(prelude + bytes(chunk_bytes)))
    else:
        with open(os.path.join(path, "map.collated.rad"), "wb") as f:   # (no concatenated copy: inputs run to gigabytes)
            f.write(prelude)
            f.write(memoryview(chunk_bytes))
    tg = os.path.join(path, "t2g.tsv")
    with open(tg, "w") as f:
        for row in t2g_rows:
            f.write("\t".join(row) + "\n")
    return tg
