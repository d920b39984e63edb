"""Orientation bits for the quant tests: the rewrite of a batch's alignment words, its patterns, and CPU-side witnesses.

An alignment word of a collated record is `orientation << 31 | ref_id` (convert.rs:443-445 of the reference), and the reference's
`quant` never reads the orientation: two reads with the same ref list are the same label, vertex and class whatever their bits
say.  Every builder of this suite sets the bit on every word.  `reorient` takes the bytes any of them made - the TWIN - and
returns a copy in which bit 31 of every alignment word follows a rule and nothing else has changed; the device has to give the
twin's bits for it (tests/test_gpu_orientation.py), the oracle too (tests/test_ori_cases_cpu.py).

The witnesses count what a rewritten case puts in front of the kernels: pairs of records of one label whose raw words differ (a
site that compares, hashes or sorts raw words sees two labels there), two-ref records whose first or second word lacks the bit
(a `t0 << 31 | t1` key that lets t1's bit 31 run into t0's field), records whose raw words are not ascending (a binary search
over raw words).  They say that a case holds what it is for; they never decide a result."""
import functools
import importlib
from collections import Counter, namedtuple
from struct import unpack_from

import numpy as np

import quant_judge as qj
import quant_judge_cases as qc
from util import pkg

PATTERNS = ("clear", "alternate", "first-clear", "last-clear", "per-read", "random")
LENGTH_CLASSES = ("1", "2", "3-4", "5-8", "9-16", "17-64", ">64")
BIT = 0x80000000

# one entry a record: its cell, its index in the cell, its alignment count, the byte offset of its first alignment word
Records = namedtuple("Records", "cell rec na first")


def length_class(n):
    for name, top in zip(LENGTH_CLASSES, (1, 2, 4, 8, 16, 64)):
        if n <= top:
            return name
    return LENGTH_CLASSES[-1]


def walk(data, off, bc_bytes, umi_bytes, pos_bytes=0):
    """The records of the chunks at `off`, by their own headers: chunk = nbytes:u32, nrec:u32, records; record = na:u32, barcode,
    UMI, na x (u32 [+ pos]).  Chunks may sit at any byte offset, with anything between them."""
    buf = bytes(data)
    head, stride = 4 + bc_bytes + umi_bytes, 4 + pos_bytes
    cell, rec, nas, first = [], [], [], []
    for c, o in enumerate(int(x) for x in off):
        nbytes, nrec = unpack_from("<II", buf, o)
        p = o + 8
        for r in range(nrec):
            na = unpack_from("<I", buf, p)[0]
            cell.append(c); rec.append(r); nas.append(na); first.append(p + head)
            p += head + stride * na
        assert p == o + nbytes, f"chunk {c}: its records do not tile it"
    return Records(*(np.asarray(x, np.int64) for x in (cell, rec, nas, first)))


def _word_positions(recs, pos_bytes):
    """(byte offset, record, index in its record) of every alignment word, in file order."""
    rec_of = np.repeat(np.arange(len(recs.na)), recs.na)
    start = np.concatenate(([0], np.cumsum(recs.na)[:-1])).astype(np.int64)
    j = np.arange(int(recs.na.sum()), dtype=np.int64) - start[rec_of]
    return recs.first[rec_of] + (4 + pos_bytes) * j, rec_of, j


def _gather_le(d, at, width):
    v = np.zeros(len(at), np.uint64)
    for k in range(width):
        v |= d[at + k].astype(np.uint64) << np.uint64(8 * k)
    return v


def pattern_bits(pattern, recs, rec_of, j, seed=0):
    """Bit 31 of every alignment word under `pattern`: c, r, j are the cell, the record in the cell, the word in the record."""
    na, r = recs.na[rec_of], recs.rec[rec_of]
    if pattern == "clear":
        return np.zeros(len(j), np.uint8)
    if pattern == "alternate":
        return (j & 1).astype(np.uint8)
    if pattern == "first-clear":
        return (j != 0).astype(np.uint8)
    if pattern == "last-clear":
        return (j != na - 1).astype(np.uint8)
    if pattern == "per-read":          # a record is of one strand: odd records forward, even ones reverse
        return (r & 1).astype(np.uint8)
    if pattern == "random":
        return np.random.default_rng(seed).integers(0, 2, len(j)).astype(np.uint8)
    raise KeyError(pattern)


def reorient(data, off, pattern, bc_bytes, umi_bytes, pos_bytes=0, seed=0):
    """A copy of the chunk bytes (uint8 array) with bit 31 of every alignment word set by `pattern` and nothing else changed.
    bc_bytes is the whole barcode field (w0 + w1 for a split barcode).  The refs keep their order - ascending by id - so the raw
    words are in general no longer ascending; a record holds a ref twice only if it did before."""
    out = np.frombuffer(bytes(data), np.uint8).copy()
    recs = walk(out, off, bc_bytes, umi_bytes, pos_bytes)
    at, rec_of, j = _word_positions(recs, pos_bytes)
    top = at + 3                       # little endian: bit 31 is bit 7 of the word's fourth byte
    out[top] = (out[top] & 0x7F) | (pattern_bits(pattern, recs, rec_of, j, seed) << 7)
    return out


class Case:
    """Chunk bytes with their layout: what a witness reads.  `pattern` is None for the twin."""

    def __init__(self, data, off, bc_bytes=4, umi_bytes=4, pos_bytes=0, pattern=None):
        self.data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8)
        self.off = np.asarray(off, np.uint64)
        self.bc_bytes, self.umi_bytes, self.pos_bytes, self.pattern = bc_bytes, umi_bytes, pos_bytes, pattern

    def reoriented(self, pattern, seed=0):
        return Case(reorient(self.data, self.off, pattern, self.bc_bytes, self.umi_bytes, self.pos_bytes, seed), self.off,
                    self.bc_bytes, self.umi_bytes, self.pos_bytes, pattern)

    def words(self):
        """(records, raw word of every alignment, its record, its index in the record)."""
        recs = walk(self.data, self.off, self.bc_bytes, self.umi_bytes, self.pos_bytes)
        at, rec_of, j = _word_positions(recs, self.pos_bytes)
        return recs, _gather_le(self.data, at, 4).astype(np.uint32), rec_of, j

    def records(self):
        """[(cell, umi, (raw words))] in file order."""
        recs, w, _, _ = self.words()
        umi = _gather_le(self.data, recs.first - self.umi_bytes, self.umi_bytes).tolist()
        w, end = w.tolist(), np.cumsum(recs.na).tolist()
        return [(c, umi[i], tuple(w[end[i] - n:end[i]])) for i, (c, n) in enumerate(zip(recs.cell.tolist(), recs.na.tolist()))]

    def cells(self):
        """[[(umi, [ref ids])]] a cell, the orientation bit taken off: what a judge reads."""
        out = [[] for _ in self.off]
        for c, umi, raw in self.records():
            out[c].append((umi, [x & 0x7FFFFFFF for x in raw]))
        return out


def _one_base_apart(u, v):
    x = u ^ v
    x = (x | (x >> 1)) & 0x5555555555555555
    return x != 0 and x & (x - 1) == 0


def _pairs(n):
    return n * (n - 1) // 2


def mixed_label_pairs(case):
    """Pairs of records of one cell with equal masked ref lists and different raw words, by label length:
    {length class: {"pairs", "same_umi" (of them, those with one UMI), "one_base" (those with UMIs one base apart)}}."""
    groups = {}
    for c, umi, raw in case.records():
        groups.setdefault((c, tuple(x & 0x7FFFFFFF for x in raw)), Counter())[(umi, raw)] += 1
    out = {k: {"pairs": 0, "same_umi": 0, "one_base": 0} for k in LENGTH_CLASSES}
    n_bases = 4 * case.umi_bytes
    for (_, label), g in groups.items():
        if not label or len({raw for _, raw in g}) == 1:
            continue
        t = out[length_class(len(label))]
        by_raw, by_umi = Counter(), {}
        for (umi, raw), n in g.items():
            by_raw[raw] += n
            by_umi.setdefault(umi, Counter())[raw] += n
        t["pairs"] += _pairs(sum(by_raw.values())) - sum(_pairs(n) for n in by_raw.values())
        t["same_umi"] += sum(_pairs(sum(r.values())) - sum(_pairs(n) for n in r.values()) for r in by_umi.values())
        umis = sorted(by_umi)
        if len(umis) <= 3 * n_bases:
            near = [(u, v) for i, u in enumerate(umis) for v in umis[i + 1:] if _one_base_apart(u, v)]
        else:
            near = [(u, u ^ (d << (2 * p))) for u in umis for p in range(n_bases) for d in (1, 2, 3)]
            near = [(u, v) for u, v in near if u < v and v in by_umi]
        for u, v in near:
            a, b = by_umi[u], by_umi[v]
            t["one_base"] += sum(a.values()) * sum(b.values()) - sum(n * b[raw] for raw, n in a.items())
    return out


def two_ref_bleed(case):
    """Two-ref records by (bit(t0), bit(t1)) where a bit is clear: {(0, 0): n, (0, 1): n, (1, 0): n}."""
    out = {(0, 0): 0, (0, 1): 0, (1, 0): 0}
    for _, _, raw in case.records():
        if len(raw) == 2:
            k = (raw[0] >> 31, raw[1] >> 31)
            if k in out:
                out[k] += 1
    return out


def unsorted_raw(case):
    """Records whose raw words are not ascending although their refs are."""
    n = 0
    for _, _, raw in case.records():
        refs = [x & 0x7FFFFFFF for x in raw]
        if all(a < b for a, b in zip(refs, refs[1:])) and not all(a < b for a, b in zip(raw, raw[1:])):
            n += 1
    return n


def classes_reached(pairs):
    """The label-length classes with at least one mixed pair."""
    return {k for k, t in pairs.items() if t["pairs"] > 0}


# ------------------------------------------------------------------------------------------------------------------------ inputs
# The twins that tests/test_gpu_orientation.py rewrites, each made by a builder the suite already has.  An Input knows its layout,
# how to configure a context for it, and the reads of its cells for the judge.

RES_CASES = {**qc.INTEGER_EXACT, **qc.PARSIMONY}     # name: (resolution, WorkerConfig switches, judge_cell's switches)
FUZZ_FLOOR = 100                                     # mixed pairs with one UMI, and one base apart, that a fuzz batch must hold
PARSIMONY_JUDGE_CAP = 1500                           # reads of the largest cell the judge's quadratic graph build is asked for


class Input:
    def __init__(self, name, twin, t2g, usa, num_genes, num_rows, cfg_kw=None, judge_kw=None, cfg_fn=None, judged=None, env=None):
        self.name, self.twin, self.usa, self.num_genes, self.num_rows = name, twin, usa, num_genes, num_rows
        self.t2g = [int(g) for g in t2g]
        self.cfg_kw, self.judge_kw, self._cfg_fn, self._judged, self.env = cfg_kw or {}, judge_kw or {}, cfg_fn, judged, env or {}
        self._rewritten, self._js, self._reads = {}, {}, None
        self.twin.data.flags.writeable = False

    @property
    def e(self):
        return self.twin.pos_bytes

    def cfg(self, resolution, **kw):
        kw.setdefault("small_thresh", 0)
        if self._cfg_fn is not None:
            return self._cfg_fn(resolution, **kw)
        return pkg.WorkerConfig.for_resolution(resolution, usa_mode=self.usa, num_genes=self.num_genes, num_rows=self.num_rows,
                                               bc_bytes=self.twin.bc_bytes, umi_bytes=self.twin.umi_bytes, **{**self.cfg_kw, **kw})

    def rewritten(self, pattern, seed=0):
        """The twin under `pattern`: made once, shared, never changed."""
        if (pattern, seed) not in self._rewritten:
            c = self.twin.reoriented(pattern, seed)
            c.data.flags.writeable = False
            self._rewritten[pattern, seed] = c
        return self._rewritten[pattern, seed]

    @property
    def reads(self):
        if self._reads is None:
            self._reads = self.twin.cells()
        return self._reads

    def judgements(self, res_case, **switches):
        """The judgement of every cell under RES_CASES[res_case] (and further judge_cell switches), or None for a cell that a
        parsimony judge is not asked for (more than PARSIMONY_JUDGE_CAP reads: its graph build is quadratic).  The judge takes ref
        ids: it is given the masked reads of the twin.  Computed once, shared, never changed."""
        key = (res_case, tuple(sorted(switches.items())))
        if key not in self._js:
            if self._judged is not None and not switches:
                self._js[key] = self._judged(res_case)
            else:
                res, _, jkw = RES_CASES[res_case]
                kw = {**dict(small_thresh=0), **self.judge_kw, **jkw, **switches}
                cap = PARSIMONY_JUDGE_CAP if res.startswith("parsimony") else None
                self._js[key] = tuple(None if cap and len(r) > cap else qj.judge_cell(r, self.t2g, res, self.usa, num_rows=self.num_rows, **kw)
                                      for r in self.reads)
        return self._js[key]


def _layout_synth(umi_len, usa=False):
    """120 cells of 5 to 59 reads, every 53rd read with 45 alignments (a record of 200 bytes and more: it crosses the decoders' and
    k_widen's 256-byte windows)."""
    tpos = importlib.import_module("test_gpu_positions")
    sizes = np.random.default_rng(17).integers(5, 60, 120)
    s = pkg.synth.synth(400 + umi_len, sizes, num_genes=40, txp_per_gene=3, usa=usa, umi_len=umi_len, dup=0.4, cross=0.5, umi_err=0.05, max_extra_na=6)
    return tpos.long_reads(s)


# name: (barcode bytes, UMI bytes, position bytes, UMI bases)
LAYOUTS = {"narrow-1-2": (1, 2, 0, 8), "narrow-2-1": (2, 1, 0, 4), "narrow-2-2": (2, 2, 0, 8), "umi-8": (4, 8, 0, 12), "bc-8": (8, 4, 0, 12),
           "pos-1": (4, 4, 1, 12), "pos-2": (4, 4, 2, 12), "pos-4": (4, 4, 4, 12), "pos-8": (4, 4, 8, 12), "narrow-pos": (1, 2, 2, 8),
           "long-reads": (4, 4, 0, 12)}
SPLITS = {"split-1-4": (1, 4, 2), "split-2-2": (2, 2, 4), "split-4-2": (4, 2, 8)}     # (w0, w1, UMI bytes); chunk i has i % 4 bytes in front
PADDED = ("pad-1", "pad-2", "pad-3")
FUZZ = qc.BATCHES
NAMES = (FUZZ + qc.MULTI_BATCHES + ("structured", "structured-3", "components", "components-usa", "wide-labels", "wide-labels-usa",
                                    "tailed", "tailed-usa", "tailed-cell") + tuple(LAYOUTS) + tuple(SPLITS) + PADDED)


@functools.lru_cache(maxsize=None)
def inputs(name):
    rad = pkg.rad
    if name in FUZZ + qc.MULTI_BATCHES:
        b = qc.batch(name)
        judged = (lambda rc: tuple(j for j, _ in qc.judgements(name, rc))) if name in FUZZ else None
        return Input(name, Case(b.data, b.off), b.t2g, b.usa, b.num_genes, b.num_rows, judged=judged)
    if name in ("structured", "structured-3"):
        s = qc.structured(3 if name.endswith("3") else None)
        lg = {} if s.thresh is None else dict(large_graph_thresh=s.thresh)
        return Input(name, Case(s.data, s.off, 4, 8), s.t2g, False, 13, 13, cfg_kw=dict(umi_len=qc.S_UMI_LEN, **lg), judge_kw=lg)
    if name.startswith("components"):
        usa = name.endswith("usa")
        cells, t2g, G = importlib.import_module("test_gpu_pug").component_size_cells(usa)
        return Input(name, Case(*rad.encode_cells(cells, 4, 4)), t2g, usa, 2 * G if usa else G, 3 * G if usa else G)
    if name.startswith("wide-labels"):
        usa = name.endswith("usa")
        cells, t2g, ng, nr = importlib.import_module("test_gpu_pug").wide_label_cells(usa)
        return Input(name, Case(*rad.encode_cells(cells, 4, 4)), t2g, usa, ng, nr)
    if name == "tailed-cell":          # the largest cell of `tailed`, alone in its batch
        t = inputs("tailed")
        k = int(np.argmax([len(r) for r in t.reads]))
        return Input(name, Case(t.twin.data, t.twin.off[k:k + 1]), t.t2g, t.usa, t.num_genes, t.num_rows, cfg_kw=t.cfg_kw)
    if name.startswith("tailed"):
        usa = name.endswith("usa")
        sn = importlib.import_module("alevin-fry_amd.synth_native")
        sizes = np.random.default_rng(23).integers(20, 600, 70).astype(np.uint32)
        d = sn.generate(seed=63 + usa, n_cells=70, sizes=sizes, num_genes=300, txp_per_gene=4, usa=usa, umi_err=0.02, tail=0.75, tail_max=64, family=8)
        return Input(name, Case(d.data, d.chunk_off), d.tid_to_gid, usa, d.num_genes, d.num_rows, cfg_kw=dict(umi_len=12))
    if name in LAYOUTS:
        bw, uw, e, umi_len = LAYOUTS[name]
        s = _layout_synth(umi_len)
        (b, off), _ = importlib.import_module("test_gpu_positions").batch(s, bw, uw, e, [3 + 5 * i for i in range(len(s.cell_nrec))] if bw < 4 else None)
        return Input(name, Case(b, off, bw, uw, e), s.tid_to_gid, s.usa, s.num_genes, s.num_rows, cfg_kw=dict(umi_len=umi_len))
    if name in SPLITS:
        mb = importlib.import_module("multi_bc_cases")
        w0, w1, uw = SPLITS[name]
        c = mb.fuzz((w0, w1, uw))
        parts = [mb.with_padding(*rad.encode_cells([cell], w0 + w1, uw), i % 4) for i, cell in enumerate(c.field_cells())]
        off = np.cumsum([0] + [len(p) for p, _ in parts[:-1]]) + np.asarray([int(o[0]) for _, o in parts])
        return Input(name, Case(np.concatenate([p for p, _ in parts]), off.astype(np.uint64), w0 + w1, uw), c.t2g, False, c.num_genes, c.num_rows,
                     cfg_fn=lambda res, **kw: c.cfg(res, "split", **kw))
    if name in PADDED:
        mb = importlib.import_module("multi_bc_cases")
        base = inputs("long-reads")
        b, off = mb.with_padding(base.twin.data, base.twin.off, int(name[-1]))
        return Input(name, Case(b, off), base.t2g, base.usa, base.num_genes, base.num_rows, cfg_kw=base.cfg_kw)
    raise KeyError(name)
