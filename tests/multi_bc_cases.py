"""Multi-barcode (10x Flex) inputs for tests/test_multi_bc_cases_cpu.py and tests/test_gpu_multi_bc.py, each with a witness
computed on the CPU.

A record of a multi-barcode file holds `na, b0, b1, u, na x u32` with b0 (the sample index after collation) and b1 (the cell
barcode) integers of w0 and w1 bytes.  A layout is (w0, w1, uw).  Unequal widths are a SPLIT barcode field to the library
(afq_config.bc_split = w0, bc_bytes = w0 + w1), which csrc/afq_decode.hip's k_widen rewrites into two dwords; it reports the key
b1 << 32 | b0.  Equal widths are an ordinary integer of 2 w0 bytes to the library and matter for the CLI only.

A case is a list of ((b0, b1), reads) cells.  It is encoded twice: as SPLIT bytes (barcode field b1 << (8 w0) | b0 in w0 + w1
bytes) and as its TWIN (an 8-byte barcode field holding b1 << 32 | b0 - the key the library reports for the split bytes), and
both with 0 to 3 bytes of padding in front of every chunk, so that chunks sit at every byte offset mod 4.  The device has to give
the same bits for both; the judge (tests/quant_judge.py) reads neither, only the reads."""
import functools

import numpy as np

import quant_judge as qj
import quant_judge_cases as qc
from util import pkg

rad = pkg.rad

WIDTHS = (1, 2, 4)
UMI_WIDTHS = (1, 2, 4, 8)
PAIRS = [(w0, w1) for w0 in WIDTHS for w1 in WIDTHS]
SPLIT_PAIRS = [p for p in PAIRS if p[0] != p[1]]
EQUAL_PAIRS = [p for p in PAIRS if p[0] == p[1]]
SPLIT_LAYOUTS = [(w0, w1, uw) for w0, w1 in SPLIT_PAIRS for uw in UMI_WIDTHS]
PADDINGS = (0, 1, 2, 3)
PAD_BYTE = 0xEE                      # what lies in front of the chunks: not zero, so that padding read as a field shows
EDGE_PHASES = frozenset((252, 253, 254, 255, 0, 1, 2, 3))
STRADDLING = frozenset((253, 254, 255))     # the record's na field lies in two of k_widen's 256-byte windows
UMI_KEY_BITS = 44                    # the widest UMI the device keys hold (22 bases; csrc/afq_common.h kUmiBits)

FUZZ_SEED = 21
FUZZ_SIZES = (1, 2, 3, 7, 13, 14, 15, 16, 17, 40, 64, 65, 120, 300, 37, 5)
FUZZ_KW = dict(num_genes=12, txp_per_gene=3, dup=0.4, cross=0.5, umi_err=0.05, umi_len=4)

# name: (resolution, WorkerConfig switches, the same switches as judge_cell takes them); small_thresh is 0 throughout
RES_CASES = {**{k: qc.INTEGER_EXACT[k] for k in ("cr-like", "prefer-ambig", "trivial")},
             **{k: qc.PARSIMONY[k] for k in ("parsimony", "parsimony-gene")}}
ONE_OUTCOME = ("cr-like", "prefer-ambig", "trivial")
EM_OF = qc.EM_OF                     # the -em sibling whose class table (dump_eq) is the plain resolution's


def ones(width):
    return (1 << (8 * width)) - 1


def reported_key(b0, b1):
    return (b1 << 32) | b0


def with_padding(data, off, pad):
    """`pad` bytes of PAD_BYTE in front of every chunk; the last chunk still ends the buffer.  Returns (uint8 array, offsets)."""
    b = np.frombuffer(bytes(data), np.uint8)
    if pad == 0:
        return b.copy(), np.asarray(off, np.uint64).copy()
    ends = [int(x) for x in off[1:]] + [len(b)]
    parts, offs, pos = [], [], 0
    for a, e in zip((int(x) for x in off), ends):
        parts.append(np.full(pad, PAD_BYTE, np.uint8))
        pos += pad
        offs.append(pos)
        parts.append(b[a:e])
        pos += e - a
    return np.concatenate(parts), np.asarray(offs, np.uint64)


class Case:
    """cells: [((b0, b1), [(umi, [ref ids])])].  reads_id names the reads (not the barcodes): cases that share it share their
    judgements."""

    def __init__(self, name, layout, cells, t2g, usa, num_genes, num_rows, umi_len, reads_id):
        self.name, self.layout, self.cells, self.reads_id = name, tuple(layout), cells, reads_id
        self.w0, self.w1, self.uw = layout
        self.t2g = [int(g) for g in t2g]
        self.usa, self.num_genes, self.num_rows, self.umi_len = usa, num_genes, num_rows, umi_len
        for (b0, b1), reads in cells:
            assert 0 <= b0 <= ones(self.w0) and 0 <= b1 <= ones(self.w1) and reads
            assert all(0 <= u <= ones(self.uw) and u >> UMI_KEY_BITS == 0 for u, _ in reads)
        self._enc = {}

    @property
    def split(self):
        return self.w0 != self.w1

    def keys(self):
        """What the library reports for the split bytes and for the twin: b1 << 32 | b0."""
        return [reported_key(b0, b1) for (b0, b1), _ in self.cells]

    def field_cells(self):
        """The cells as the file holds them: barcode field b1 << (8 w0) | b0 in w0 + w1 bytes."""
        return [((b1 << (8 * self.w0)) | b0, reads) for (b0, b1), reads in self.cells]

    def twin_cells(self):
        return [(reported_key(b0, b1), reads) for (b0, b1), reads in self.cells]

    def bc_bytes(self, kind):
        return 8 if kind == "twin" else self.w0 + self.w1

    def encode(self, kind, pad=0):
        """kind "split" (the file's bytes; for equal widths the ordinary 2 w0-byte field) or "twin"; computed once, never changed."""
        if (kind, pad) not in self._enc:
            cells = self.twin_cells() if kind == "twin" else self.field_cells()
            data, off = with_padding(*rad.encode_cells(cells, self.bc_bytes(kind), self.uw), pad)
            data.flags.writeable = False
            off.flags.writeable = False
            self._enc[kind, pad] = (data, off)
        return self._enc[kind, pad]

    def cfg(self, resolution, kind, **kw):
        kw.setdefault("small_thresh", 0)
        split = self.w0 if kind == "split" and self.split else 0
        return pkg.WorkerConfig.for_resolution(resolution, usa_mode=self.usa, num_genes=self.num_genes, num_rows=self.num_rows,
                                               bc_bytes=self.bc_bytes(kind), bc_split=split, umi_bytes=self.uw, umi_len=self.umi_len, **kw)

    def judged_reads(self):
        """The reads the judge is given, a list per cell.  A record without alignments names no gene and no vertex: the judge,
        like the reference's rules, is stated over reads that map somewhere (a mapper writes no others), and the integer-exact
        resolutions count votes per gene, of which such a record has none (tests/test_gpu_crlike.py::test_degenerate_records pins
        that on the device).  Such records stay in nrec."""
        return [[r for r in reads if r[1]] for _, reads in self.cells]

    def judgements(self, res_case):
        return _judgements(self.reads_id, res_case, self)

    def n_records(self):
        return sum(len(reads) for _, reads in self.cells)


_JUDGED = {}


def _judgements(reads_id, res_case, case):
    """The judgement of every cell, computed once per (reads, resolution case), shared, never changed."""
    key = (reads_id, res_case)
    if key not in _JUDGED:
        res, _, jkw = RES_CASES[res_case]
        kw = dict(dict(small_thresh=0), **jkw)
        _JUDGED[key] = tuple(qj.judge_cell(reads, case.t2g, res, case.usa, num_rows=case.num_rows, **kw) for reads in case.judged_reads())
    return _JUDGED[key]


# ----------------------------------------------------------------------------------------------------------------------- fuzz

@functools.lru_cache(maxsize=None)
def _fuzz_synth(usa):
    return pkg.synth.synth(FUZZ_SEED, list(FUZZ_SIZES), usa=usa, **FUZZ_KW)


def _fuzz_barcodes(w0, w1, n):
    """n distinct (b0, b1): four samples' worth of b0 values with the high and the low byte of the field in use, b1 spread over
    its width."""
    b0s = [(0x9E3779B1 * (k + 1)) & ones(w0) for k in range(4)]
    out = [(b0s[i % 4], (0x85EBCA6B * (i // 4 + 1) + 0x3D) & ones(w1)) for i in range(n)]
    assert len(set(out)) == n and len(set(b0s)) == 4
    return out


@functools.lru_cache(maxsize=None)
def fuzz(layout, usa=False):
    """16 synthetic cells of 1 to 300 reads, UMIs of four bases (they fit every UMI width)."""
    s = _fuzz_synth(usa)
    reads = [r for _, r in qc.cells_of(s)]
    bcs = _fuzz_barcodes(layout[0], layout[1], len(reads))
    return Case(f"fuzz{'-usa' if usa else ''}", layout, list(zip(bcs, reads)), s.tid_to_gid.tolist(), usa, s.num_genes, s.num_rows,
                FUZZ_KW["umi_len"], ("fuzz", usa))


# ----------------------------------------------------------------------------------------------------------------------- edge

E_T2G = [t // 3 for t in range(36)]


def _e_refs(i, na):
    return sorted((5 * i + 7 * k) % 36 for k in range(na))      # 7 and 36 are coprime: na <= 36 distinct refs


def _fill(nbytes, H, first):
    """Records of 1 to 8 alignments (H + 4 na bytes each) that fill exactly nbytes; reads numbered from `first`."""
    for n in range(1, nbytes // (H + 4) + 1):
        extra = nbytes - n * (H + 4)
        if extra >= 0 and extra % 4 == 0 and extra // 4 <= 7 * n:
            words = extra // 4
            nas = [1 + words // n + (1 if k < words % n else 0) for k in range(n)]
            return [((37 * (first + k)) & 0xFF, _e_refs(first + k, na)) for k, na in enumerate(nas)]
    raise AssertionError(f"no records of {H} + 4 na bytes fill {nbytes} bytes")


@functools.lru_cache(maxsize=None)
def edge(layout):
    """Record starts ON the edges of k_widen's 256-byte windows.  Chunk 0 sits at byte offset `pad`, so its record at byte r of
    the chunk has phase pad + r: a record of two alignments at byte 252, one WITHOUT alignments at byte 508 and one of one
    alignment at byte 768 take the phases 252...255 and 0...3 over the four paddings, and on 253...255 the first two have their na
    field in two windows - lane 63's dword and the next window's lane 0.  Chunk 1 holds a single record, chunk 2 a record
    without alignments between two others, chunk 3 ends the buffer."""
    w0, w1, uw = layout
    H = 4 + w0 + w1 + uw
    reads = _fill(252 - 8, H, 0)
    reads.append((0xA1, _e_refs(100, 2)))                     # at byte 252
    reads += _fill(508 - (252 + H + 8), H, 200)
    reads.append((0xA2, []))                                  # at byte 508
    reads += _fill(768 - (508 + H), H, 300)
    reads.append((0xA3, _e_refs(101, 1)))                     # at byte 768
    reads += _fill(3 * (H + 4) + 8, H, 400)
    cells = [reads, [(0x17, [4])], [(5, [1, 2]), (6, []), (7, [3])], [(9 + k, _e_refs(500 + k, 1 + k % 3)) for k in range(5)]]
    bcs = [((0x5A5A5A5A + i) & ones(w0), (0xC3C3C3C3 - 0x01010101 * i) & ones(w1)) for i in range(len(cells))]
    assert len(set(bcs)) == len(bcs)
    return Case("edge", layout, list(zip(bcs, cells)), E_T2G, False, 12, 12, 4, ("edge", layout))


def record_starts(case, pad, kind="split"):
    """[(chunk, byte offset in the buffer, na)] of every record of the encoding, from the cells and the chunk offsets."""
    _, off = case.encode(kind, pad)
    H = 4 + case.bc_bytes(kind) + case.uw
    out = []
    for i, (_, reads) in enumerate(case.cells):
        p = int(off[i]) + 8
        for _, refs in reads:
            out.append((i, p, len(refs)))
            p += H + 4 * len(refs)
    return out


def phase(start, chunk_off):
    """Where a record starts in k_widen's windows: they are 256 bytes wide and begin at the chunk's offset rounded down to a dword."""
    return (int(start) - (int(chunk_off) & ~3)) % 256


def witness(case, pads=PADDINGS):
    """What the split encodings of `case` put in front of k_widen over the paddings: the phases on which a record starts, the na
    of the records whose na field straddles two windows, the chunk offsets mod 4, the chunks of one record, and whether the last
    chunk ends the buffer in every padding."""
    phases, straddling_na, mis, single, ends = set(), set(), set(), set(), True
    for pad in pads:
        data, off = case.encode("split", pad)
        for i, start, na in record_starts(case, pad):
            ph = phase(start, off[i])
            phases.add(ph)
            if ph in STRADDLING:
                straddling_na.add(na)
        mis.update(int(o) & 3 for o in off)
        single.update(i for i, (_, reads) in enumerate(case.cells) if len(reads) == 1)
        last = int(off[-1])
        ends = ends and last + int.from_bytes(bytes(data[last:last + 4]), "little") == len(data)
    return dict(phases=phases, straddling_na=straddling_na, offsets_mod_4=mis, single_record_chunks=single, last_chunk_ends_the_buffer=ends)


# ------------------------------------------------------------------------------------------------------------------- extremes

def umi_ones(uw):
    """The all-ones UMI of the field; of the 44 bits a device key holds where the field is wider (an 8-byte field of 22 bases)."""
    return (1 << min(8 * uw, UMI_KEY_BITS)) - 1


@functools.lru_cache(maxsize=None)
def extremes(layout):
    """b0 and b1 each at 0 and at all-ones, in all four combinations and in an order in which neighbouring chunks differ in b0
    only (one cell barcode in two samples), then in b1 only, then in b0 only; a fifth and a sixth chunk repeat that with values in
    between.  Every cell holds the UMI 0 and the all-ones UMI next to UMIs that differ from them in the field's top bit and in its
    lowest base, all on one gene: six molecules to cr-like, and fewer if any byte of the UMI were lost or taken from a neighbour;
    a second gene holds 0 and all-ones again, under labels of two refs."""
    w0, w1, uw = layout
    top = 1 << (min(8 * uw, UMI_KEY_BITS) - 1)
    u1 = umi_ones(uw)
    m0, m1 = ones(w0), ones(w1)
    bcs = [(0, 0), (m0, 0), (m0, m1), (0, m1), (0x5A & m0, m1), (0x5A & m0, 0xC3C3C3C3 & m1)]
    assert all(a[1] == b[1] for a, b in (bcs[0:2], bcs[2:4])) and bcs[1][0] == bcs[2][0] and bcs[4][0] == bcs[5][0] and len(set(bcs)) == 6
    cells = []
    for i, bc in enumerate(bcs):
        g = 3 * (i % 11)
        reads = [(0, [g]), (u1, [g]), (top, [g]), (u1 ^ top, [g]), (3, [g]), (u1 ^ 3, [g]), (0, [g]), (u1, [g]), (u1, [g, g + 1]),
                 (0, [g + 3, g + 4]), (u1, [g + 3, g + 4]), (u1, [g + 3])]
        cells.append((bc, reads))
    return Case("extremes", layout, cells, E_T2G, False, 12, 12, min(4 * uw, UMI_KEY_BITS // 2), ("extremes", uw))


# ------------------------------------------------------------------------------------------------------------------ malformed

MALFORMED_KINDS = ("head_cut", "alns_cut", "nrec_low", "nrec_high")


def malformed(layout, kind, pad=0):
    """Four chunks of split bytes of which chunk 2 is malformed, only in its header: (data, off, the good case).  head_cut: nbytes
    ends seven bytes into the last record's head; alns_cut: nbytes ends one word short, inside the last record's alignment list (a
    cut that is no whole word never passes the host's chunk table; this one is the record walk's to find); nrec_low / nrec_high:
    the header's count is one off.  Whether the chunk table on the host or the walk on the device refuses the chunk depends on
    the record head's length mod 4; both name cell 2."""
    f = fuzz(layout)
    pick = [f.cells[i] for i in (2, 3, 9, 1)]
    pick[2] = (pick[2][0], pick[2][1] + [(0x3C, [1, 5, 9])])
    good = Case("malformed-good", layout, pick, f.t2g, False, f.num_genes, f.num_rows, f.umi_len, ("malformed", layout))
    data, off = good.encode("split", pad)
    data = data.copy()
    o2 = int(off[2])
    nb = int.from_bytes(bytes(data[o2:o2 + 4]), "little")
    nrec = int.from_bytes(bytes(data[o2 + 4:o2 + 8]), "little")
    H = 4 + layout[0] + layout[1] + layout[2]
    last = H + 4 * 3
    nb2, nrec2 = {"head_cut": (nb - last + 7, nrec), "alns_cut": (nb - 4, nrec), "nrec_low": (nb, nrec - 1), "nrec_high": (nb, nrec + 1)}[kind]
    data[o2:o2 + 4] = np.frombuffer(int(nb2).to_bytes(4, "little"), np.uint8)
    data[o2 + 4:o2 + 8] = np.frombuffer(int(nrec2).to_bytes(4, "little"), np.uint8)
    return data, off.copy(), good


# ------------------------------------------------------------------------------------------------------------------------ CLI

CLI_SAMPLES = 3                                   # samples with an entry in collation_manifest.bin; a fourth has none
CLI_SAMPLE_NAMES = ("sample_a", None, "sample_c")  # an unnamed sample goes by its key in hex
CLI_SAMPLE_KEYS = (0xAA, 0xAB, 0xAC)
CLI_CELL_BARCODES = (0x00000000, 0x9E3779B1, 0xFFFFFFFF, 0x2545F491)


@functools.lru_cache(maxsize=None)
def cli_case(layout):
    """The fuzz cells as a collated file of four samples x four cell barcodes, every sample with the same four (the samples are
    contiguous and b0 is the sample's ordinal, as collation leaves them).  The manifest names three samples."""
    w0, w1, uw = layout
    f = fuzz((1, 2, uw))                            # (the reads do not depend on the widths)
    b1s = [b & ones(w1) for b in CLI_CELL_BARCODES]
    assert len(set(b1s)) == 4 and len(f.cells) == 16
    cells = [((i // 4, b1s[i % 4]), reads) for i, (_, reads) in enumerate(f.cells)]
    return Case("cli", layout, cells, f.t2g, False, f.num_genes, f.num_rows, f.umi_len, ("fuzz", False))


def cli_label(case, i):
    """(row label, sample column or None) of chunk i: sample_cell, or the bare cell barcode where the manifest has no such sample."""
    b0, b1 = case.cells[i][0]
    cell = rad.int_to_seq(b1, 4 * case.w1)
    if b0 >= CLI_SAMPLES:
        return cell, None
    name = CLI_SAMPLE_NAMES[b0] or f"{CLI_SAMPLE_KEYS[b0]:x}"
    return f"{name}_{cell}", name


def write_cli_dir(path, case):
    """The input directory of `afquant quant` for a case: map.collated.rad with the multi-barcode prelude (b0len, b1len and ulen
    are the base counts the widths hold), the tg-map and collation_manifest.bin.  Returns the tg-map's path."""
    names = [f"T{t}" for t in range(len(case.t2g))]
    data, off = case.encode("split")
    pre = rad.rad_prelude_multi_bc(names, len(off), 4 * case.w0, 4 * case.w1, case.umi_len, b_bytes=case.w1, umi_bytes=case.uw, b0_bytes=case.w0)
    tg = rad.write_quant_input_dir(str(path), data.tobytes(), len(off), names, [(names[t], f"G{g}") for t, g in enumerate(case.t2g)], prelude=pre)
    groups = [(CLI_SAMPLE_KEYS[s], CLI_SAMPLE_NAMES[s], 4 * s, 4, 0) for s in range(CLI_SAMPLES)]
    with open(f"{path}/collation_manifest.bin", "wb") as fh:
        fh.write(rad.collation_manifest(groups))
    return tg
