"""The cells that tests/test_quant_judge_cpu.py puts before the judge with the oracle, and tests/test_gpu_quant_judge.py with the
device: four fuzz batches of small cells (a misread rule shows at ten reads as well as at ten thousand), the resolutions and
switches each runs under, and structured cells whose one outcome is written down by hand next to them."""
import functools

import numpy as np

import quant_judge as qj
from util import pkg

N_FUZZ = 2000


def cells_of(s):
    """A SynthRad as the `cells` lists that rad.encode_cells takes: [(barcode, [(umi, [ref ids])])]."""
    out, r, a = [], 0, 0
    umi, na, refs = s.umi.tolist(), s.na.tolist(), s.refs.tolist()
    for n, bc in zip(s.cell_nrec.tolist(), s.cell_bc.tolist()):
        reads = []
        for i in range(r, r + n):
            reads.append((umi[i], refs[a:a + na[i]]))
            a += na[i]
        r += n
        out.append((bc, reads))
    return out


class Batch:
    def __init__(self, name, s):
        self.name, self.s = name, s
        self.cells = cells_of(s)
        self.t2g = s.tid_to_gid.tolist()
        self.data, self.off = s.encode()
        self.usa, self.num_genes, self.num_rows = s.usa, s.num_genes, s.num_rows

    def cfg(self, resolution, **kw):
        kw.setdefault("small_thresh", 0)
        return pkg.WorkerConfig.for_resolution(resolution, usa_mode=self.usa, num_genes=self.num_genes, num_rows=self.num_rows, **kw)


BATCHES = ("base", "usa", "wide", "deep")
# Cells of the fuzz batches hold at most 96 alignment words: one bucket each, no slab, and the cr-like resolve sorts such a cell
# without its UMI table.  These two batches hold cells of 280 to 2500 reads next to a few small ones - several buckets a cell, 100
# to 250 keys a bucket - for the resolutions whose rule is linear in the reads; they average under two alignments a read, so the
# table is what resolves them.
MULTI_BATCHES = ("multi", "multi-usa")
MULTI_SIZES = (2500, 1800, 1200, 900, 700, 600, 500, 450, 400, 350, 300, 280, 2000, 1000, 800, 650, 60, 20, 1500, 320, 290, 7, 1100, 550)


@functools.lru_cache(maxsize=None)
def batch(name):
    sizes = np.random.default_rng(11).integers(5, 60, N_FUZZ)
    kw = dict(num_genes=12, txp_per_gene=3, dup=0.4, cross=0.5, umi_err=0.05, umi_len=6)
    if name == "base":
        return Batch(name, pkg.synth.synth(9, sizes, **kw))
    if name == "usa":
        return Batch(name, pkg.synth.synth(9, sizes, **dict(kw, usa=True, umi_len=5, umi_err=0.08)))
    if name == "wide":
        return Batch(name, pkg.synth.synth(9, sizes, **dict(kw, num_genes=40, umi_len=12, max_extra_na=6)))
    if name == "deep":
        # few molecules with many reads each and a UMI error in three reads of ten: vertices with 2, 4, 8 reads beside ones with
        # 1, 2, 4, which is where the direction rule's threshold lies.  The three batches above never put a vertex pair ON it in a
        # place that matters at transcript level: an oracle with `x > 2 y` for `x > 2 y - 1` gives the same 2000 rows there.
        return Batch(name, pkg.synth.synth(9, sizes, **dict(kw, num_genes=6, txp_per_gene=2, dup=0.9, umi_err=0.3, cross=0.2,
                                                            p_na=(0.9, 0.08, 0.02))))
    if name in MULTI_BATCHES:
        return Batch(name, pkg.synth.synth(9, MULTI_SIZES, num_genes=30, txp_per_gene=3, usa=name == "multi-usa", dup=0.5, cross=0.5,
                                           umi_err=0.03, umi_len=8, max_extra_na=4))
    raise KeyError(name)


# name: (resolution, WorkerConfig switches, the same switches as judge_cell takes them)
INTEGER_EXACT = {
    "cr-like": ("cr-like", {}, {}),
    "cr-like-tiny-below-30": ("cr-like", dict(small_thresh=30), dict(small_thresh=30)),
    "prefer-ambig": ("cr-like", dict(sa_model="prefer-ambig"), dict(sa_model="prefer-ambig")),
    "trivial": ("trivial", {}, {}),
}
PARSIMONY = {
    "parsimony": ("parsimony", {}, {}),
    "parsimony-gene": ("parsimony-gene", {}, {}),
    "umi-edit-dist-0": ("parsimony", dict(pug_exact_umi=True), dict(umi_edit_dist=0)),
    "large-graph-thresh-3": ("parsimony", dict(large_graph_thresh=3), dict(large_graph_thresh=3)),
}
EM_OF = {"cr-like": "cr-like-em", "parsimony": "parsimony-em", "parsimony-gene": "parsimony-gene-em"}


@functools.lru_cache(maxsize=None)
def judgements(batch_name, case):
    """(judgement, size of the largest component) of every cell of a batch; computed once, shared, never changed."""
    b = batch(batch_name)
    res, _, jkw = {**INTEGER_EXACT, **PARSIMONY}[case]
    out = []
    for _, reads in b.cells:
        st = {}
        kw = dict(dict(small_thresh=0), **jkw)
        out.append((qj.judge_cell(reads, b.t2g, res, b.usa, num_rows=b.num_rows, stats=st, **kw), st.get("largest_component", 0)))
    return tuple(out)


def rows_of(res):
    """A QuantResult's rows as [(column, value)] lists, one a cell."""
    ptr, g, v = res.cell_ptr.tolist(), res.gene.tolist(), res.val.tolist()
    return [list(zip(g[a:b], v[a:b])) for a, b in zip(ptr, ptr[1:])]


def classes_of(res):
    """A QuantResult's -d class tables as [(label, molecules)] lists, one a cell."""
    ec = res.eqclasses
    cp, lp, lab, n = ec.cell_ptr.tolist(), ec.label_ptr.tolist(), ec.labels.tolist(), ec.count.tolist()
    return [[(tuple(lab[lp[k]:lp[k + 1]]), n[k]) for k in range(a, b)] for a, b in zip(cp, cp[1:])]


# --------------------------------------------------------------------------------------------------------------- structured cells
# 26 refs, ref t belongs to gene t // 2; UMIs of 22 bases in an 8-byte field, so that a vertex can have 64 neighbours one base off.

S_T2G = [t // 2 for t in range(26)]
S_UMI_LEN = 22
HUB = 0x2E4A9C31B57         # 42 bits


def one_off(umi, i):
    """The i-th UMI one base from `umi`: positions first, so that the first 22 are two bases from each other."""
    pos, delta = i % S_UMI_LEN, 1 + i // S_UMI_LEN
    return umi ^ (delta << (2 * pos))


def path(m, big, t=0):
    """a - b - c one base apart in a row, reads (big, m, big): ends on ref t, the middle on refs t and t + 1 (one gene)."""
    b = HUB
    return [(b ^ 1, [t])] * big + [(b, [t, t + 1])] * m + [(b ^ (1 << 2), [t])] * big


def star(n, labels, hub_label, hub_reads=4, hub=HUB):
    """A hub of hub_reads reads and n single-read leaves one base from it: 4 >= 2 * 1, so every edge points at the leaf
    (pugutils.rs:88-97), the hub reaches all of them and no leaf reaches the hub."""
    return [(hub, hub_label)] * hub_reads + [(one_off(hub, i), labels[i % len(labels)]) for i in range(n)]


def structured_cells():
    """[(name, reads, classes written down by hand, large_graph_thresh)]; every cell has exactly one outcome."""
    out = []
    for m in (63, 64, 126, 127, 128):
        out.append((f"path-{2 * m}-{m}-{2 * m}", path(m, 2 * m), {(0,): 2}, None))              # the middle reaches neither end
        out.append((f"path-{2 * m - 1}-{m}-{2 * m - 1}", path(m, 2 * m - 1), {(0,): 1}, None))  # every edge goes both ways
    for n in (1, 3, 7, 8, 63, 64):
        out.append((f"star-{n}", star(n, [[0]], [0]), {(0,): 1}, None))
    every = []
    for k, n in enumerate((1, 3, 7, 8, 63, 64)):     # the six stars in one cell, on refs of six genes: no label overlaps another
        every += star(n, [[2 * k]], [2 * k], hub=HUB ^ (k << 30))
    out.append(("stars-together", every, {(k,): 1 for k in range(6)}, None))
    # two labels that share ref 1 only: the hub covers all leaves through ref 1, the molecule is ref 1's gene
    out.append(("star-common-ref", star(7, [[0, 1], [1, 2]], [0, 1]), {(0,): 1}, None))
    # two labels that share refs 1 and 2, of genes 0 and 1: a two-gene molecule, no count without an EM
    out.append(("star-common-two-genes", star(7, [[1, 2], [1, 2, 3]], [1, 2]), {(0, 1): 1}, None))
    # one UMI under twelve labels {i, 12}: all edges at distance 0, every vertex reaches all others through ref 12 (gene 6)
    out.append(("twelve-labels", [(HUB, [i, 12]) for i in range(12) for _ in range(1 + i % 3)], {(6,): 1}, None))
    # UMIs equal or one base apart under labels that share no ref (refs 19 apart among them): no edge, five lone molecules
    out.append(("no-shared-ref", [(HUB, [0]), (HUB, [2]), (HUB ^ 1, [4]), (HUB, [1]), (HUB ^ 2, [20]), (HUB ^ 2, [20])],
                {(0,): 2, (1,): 1, (2,): 1, (10,): 1}, None))
    # large_graph_thresh 3.  Four UMIs in a row on ref 0 are a component of 4: cr-like inside it, four molecules where the cover
    # gives one.  UMIs p, q on refs 4 / 6 / both: four vertices; p has 3 reads of gene 2 and 1 of gene 3, q has 2 of gene 3
    # and 1 of gene 2.  Three UMIs in a row on ref 8 stay with the cover: one molecule.
    p = HUB ^ (3 << 20)
    q = p ^ 1
    r = HUB ^ (3 << 30)
    big = [(HUB, [0]), (HUB ^ 1, [0]), (HUB ^ 2, [0]), (HUB ^ 3, [0]),
           (p, [4]), (p, [4]), (p, [4, 6]), (q, [6]), (q, [4, 6]),
           (r, [8]), (r ^ 1, [8]), (r ^ (1 | 1 << 2), [8])]
    out.append(("above-large-graph-thresh", big, {(0,): 4, (2,): 1, (3,): 1, (4,): 1}, 3))
    return out


class Structured:
    """The structured cells as two batches: those under the default large_graph_thresh and those under 3."""

    def __init__(self, thresh):
        self.thresh = thresh
        self.items = [c for c in structured_cells() if c[3] == thresh]
        self.cells = [(900 + i, c[1]) for i, c in enumerate(self.items)]
        self.t2g = S_T2G
        self.data, self.off = pkg.rad.encode_cells(self.cells, 4, 8)

    def cfg(self, resolution, **kw):
        if self.thresh is not None:
            kw["large_graph_thresh"] = self.thresh
        return pkg.WorkerConfig.for_resolution(resolution, num_genes=13, num_rows=13, small_thresh=0, umi_bytes=8, umi_len=S_UMI_LEN, **kw)

    def judge(self, i, resolution):
        kw = {} if self.thresh is None else dict(large_graph_thresh=self.thresh)
        return qj.judge_cell(self.items[i][1], self.t2g, resolution, False, small_thresh=0, **kw)


@functools.lru_cache(maxsize=None)
def structured(thresh):
    return Structured(thresh)
