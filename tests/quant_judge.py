"""A judge for the quant rows: what alevin-fry's `quant` computes for ONE cell, stated as definitions in plain Python.

Written from the reference's text (COMBINE-lab/alevin-fry, src/; cited `file:line` below) and SURVEY.md appendix B, and from
nothing else: not from oracle/afq_oracle.cpp, not from the kernels.  The oracle follows the reference's control flow (EqMap,
vertex ids, BFS, first-maximum scans); this file says what the result IS - multisets of reads, sets of vertices, intersections of
labels - so that a rule misread there is not repeated here.  Only ints, tuples, dicts, sets and Counters; no numpy, no ctypes.

What it covers: the tiny-cell path, cr-like (winner-take-all and prefer-ambig), trivial, parsimony and parsimony-gene with the
large-component fall-back, the step from a cell's gene-level classes to its row (non-USA and USA), and the class table that the
-em resolutions hand to their EM (what -d dumps).  The EM's numbers are judged from that table on by tests/em_judge.py, the
bootstrap means and variances by tests/boot_judge.py.  What is left out: the decoding of bytes.

The parsimony cover's tie-break.  The reference walks a HashSet of the uncovered vertices and keeps the first largest
arborescence (pugutils.rs:1110-1146); which one is first depends on the hash order.  The judge therefore does not replay a scan:
in every round it takes EVERY largest candidate set as an admissible choice and returns the set of outcomes that some scan order
could produce.  A cell with one outcome is decided exactly; a row from any scan order has to be one of the outcomes.

    judge_cell(reads, t2g, resolution, usa, **cfg) -> Judgement(outcomes, undecided, flags)
    admits(judgement, row, classes=None, flags=None) -> True, or a message naming the first difference
"""
from collections import Counter, namedtuple

FLAG_TINY, FLAG_ALT, FLAG_EMPTY = 0x1, 0x2, 0x4     # quant.json's tiny_cell / alt_resolved / empty_resolved cell lists
BOUND = 4096                                          # partial outcomes kept per cell before it is reported undecided

PLAIN = ("cr-like", "trivial", "parsimony", "parsimony-gene")
WITH_EM = ("cr-like-em", "parsimony-em", "parsimony-gene-em")

# outcomes: list of (row, classes); row = {column: molecules} or None where an EM makes it; classes = {gene label: molecules} or
# None where the reference keeps none (trivial, the tiny path).  flags: the bits that no scan order changes (tiny, alt-resolved).
Judgement = namedtuple("Judgement", "outcomes undecided flags")


class _Undecided(Exception):
    pass


# ---------------------------------------------------------------------------------------------------------------- reads -> genes

def genes_of(refs, t2g):
    """The distinct genes of one read, ascending (pugutils.rs:774-781).  A read counts each of them once."""
    return sorted({t2g[t] for t in refs})


def is_spliced(g):
    return g & 1 == 0                       # utils.rs:419-422


def same_gene(a, b):
    return a >> 1 == b >> 1                 # utils.rs:409-416, with_unspliced = true


# --------------------------------------------------------------------------------------------------------------------- cr-like

def winners(gene_reads, prefer_ambig=False):
    """One UMI's gene label from {gene id: reads} (pugutils.rs:644-749): the gene ids with the most reads, ascending.
    prefer-ambig (pugutils.rs:505-641) tallies the spliced and unspliced id of a gene together and answers with every id
    that was seen of the genes with the most reads."""
    if not prefer_ambig:
        top = max(gene_reads.values())
        return tuple(sorted(g for g, n in gene_reads.items() if n == top))
    per_gene = Counter()
    for g, n in gene_reads.items():
        per_gene[g >> 1] += n
    top = max(per_gene.values())
    return tuple(sorted(g for g in gene_reads if per_gene[g >> 1] == top))


def crlike_classes(umi_gene_reads, prefer_ambig=False):
    """{UMI: {gene: reads}} -> {label: molecules}: every UMI is one molecule of its winners' label."""
    return Counter(winners(gr, prefer_ambig) for gr in umi_gene_reads.values())


def tally_reads(reads, t2g):
    """{UMI: {gene: reads}} of a cell's reads (pugutils.rs:769-785, 811-838; quant.rs:486-520)."""
    out = {}
    for umi, refs in reads:
        c = out.setdefault(umi, Counter())
        for g in genes_of(refs, t2g):
            c[g] += 1
    return out


# ------------------------------------------------------------------------------------------------------------- classes -> a row

def usa_slot(label, num_rows):
    """The USA column of a molecule with gene label `label`, or None if it is dropped (utils.rs:688-753)."""
    u_off = num_rows // 3
    a_off = 2 * u_off
    n = len(label)
    if n == 1:
        g = label[0]
        return g >> 1 if is_spliced(g) else u_off + (g >> 1)
    if n == 2:
        g1, g2 = label
        if same_gene(g1, g2):
            return a_off + (g1 >> 1)
        if is_spliced(g1) != is_spliced(g2):                 # exactly one of two different genes is spliced: report it
            return (g1 if is_spliced(g1) else g2) >> 1
        return None
    if 3 <= n <= 10:
        at = [i for i, g in enumerate(label) if is_spliced(g)]
        if len(at) != 1:                                     # none, or gene-ambiguous among spliced ones
            return None
        i = at[0]
        if i + 1 < n and same_gene(label[i], label[i + 1]):  # its own unspliced id follows it
            return a_off + (label[i] >> 1)
        return label[i] >> 1
    return None                                              # labels of more than ten ids are cut


def row_of_classes(classes, usa, num_rows):
    """only_unique extraction: non-USA keeps the single-gene classes (em.rs:499-514), USA applies the slot rules."""
    row = Counter()
    for label, n in classes.items():
        col = usa_slot(label, num_rows) if usa else (label[0] if len(label) == 1 else None)
        if col is not None:
            row[col] += n
    return dict(row)


# --------------------------------------------------------------------------------------------------------------------- trivial

def trivial_row(reads, t2g):
    """pugutils.rs:852-911: a gene's count is the number of distinct UMIs among the reads whose refs all lie in that gene."""
    umis = {}
    for umi, refs in reads:
        g = {t2g[t] for t in refs}
        if len(g) == 1:
            umis.setdefault(g.pop(), set()).add(umi)
    return {g: len(s) for g, s in umis.items()}


# ------------------------------------------------------------------------------------------------------------------- parsimony

def umi_distance(a, b):
    x = a ^ b
    return bin((x | (x >> 1)) & 0x5555555555555555).count("1")      # utils.rs:389-393: bases that differ, two bits a base


def arcs(xu, xn, yu, yn, exact):
    """(x -> y, y -> x) for two vertices with overlapping labels, from their UMIs and read counts (pugutils.rs:76-99)."""
    d = (0 if xu == yu else 2) if exact else umi_distance(xu, yu)
    if d == 0:
        return True, True
    if d >= 2:
        return False, False
    if xn > 2 * yn - 1:
        return True, False
    if yn > 2 * xn - 1:
        return False, True
    return True, True


def vertices_of(reads, t2g, gene_level):
    """(label, UMI) -> reads.  The label is the read's ref list (eq_class.rs:859-903) or, at gene level, its distinct genes
    ascending (eq_class.rs:740-746)."""
    v = Counter()
    for umi, refs in reads:
        label = tuple(genes_of(refs, t2g)) if gene_level else tuple(refs)
        assert all(a < b for a, b in zip(label, label[1:])), "labels are searched as ascending lists (pugutils.rs:375)"
        v[(label, umi)] += 1
    return v


def graph_of(vertex_reads, exact):
    """Vertices as a list of (label, UMI, reads), successor sets, and the weakly connected components (pugutils.rs:65-301)."""
    vs = [(lab, umi, n) for (lab, umi), n in vertex_reads.items()]
    sets = [frozenset(lab) for lab, _, _ in vs]
    out = [set() for _ in vs]
    comp = list(range(len(vs)))

    def find(i):
        while comp[i] != i:
            comp[i] = comp[comp[i]]
            i = comp[i]
        return i

    umis = [umi for _, umi, _ in vs]
    for i, ui in enumerate(umis):
        for j in range(i + 1, len(vs)):
            x = ui ^ umis[j]
            x = (x | (x >> 1)) & 0x5555555555555555
            if x & (x - 1):                                                    # two or more bases differ: no edge either way
                continue
            fwd, back = arcs(vs[i][1], vs[i][2], vs[j][1], vs[j][2], exact)
            if (fwd or back) and not sets[i].isdisjoint(sets[j]):          # an edge needs a shared ref (pugutils.rs:187-204)
                if fwd:
                    out[i].add(j)
                if back:
                    out[j].add(i)
                comp[find(i)] = find(j)
    comps = {}
    for i in range(len(vs)):
        comps.setdefault(find(i), []).append(i)
    return vs, sets, out, list(comps.values())


def candidate(v, uncovered, vs, sets, out):
    """cand(v): the closure from v over outgoing edges through uncovered vertices whose label holds t, for the first t of v's
    label, in label order, that gives the largest closure (pugutils.rs:331-387)."""
    best = ()
    for t in vs[v][0]:
        seen = {v}
        todo = [v]
        while todo:
            for n in out[todo.pop()]:
                if n in uncovered and n not in seen and t in sets[n]:
                    seen.add(n)
                    todo.append(n)
        if len(seen) > len(best):
            best = seen
    return frozenset(best)


def molecule_label(chosen, vs, sets, t2g, gene_level):
    """The genes of the refs common to ALL vertices of the chosen set, ascending and distinct (pugutils.rs:1161-1225)."""
    common = frozenset.intersection(*(sets[v] for v in chosen))
    assert common, "an arborescence is covered by at least one ref"
    return tuple(sorted(common)) if gene_level else tuple(genes_of(common, t2g))


def cover_outcomes(comp, vs, sets, out, t2g, gene_level, budget):
    """Every {label: molecules} that covering the component can give, branching over each round's admissible choices: the
    distinct vertex sets among the largest cand(v) (pugutils.rs:1097-1146, 1256-1260).  Outcomes are frozensets of items."""
    memo = {}

    def rest(uncovered):
        if not uncovered:
            return {frozenset()}
        if uncovered in memo:
            return memo[uncovered]
        cands = {candidate(v, uncovered, vs, sets, out) for v in uncovered}
        top = max(len(c) for c in cands)
        got = set()
        for chosen in cands:
            if len(chosen) == top:
                label = molecule_label(chosen, vs, sets, t2g, gene_level)
                for o in rest(uncovered - chosen):
                    c = Counter(dict(o))
                    c[label] += 1
                    got.add(frozenset(c.items()))
        budget[0] -= len(got)
        if budget[0] < 0:
            raise _Undecided
        memo[uncovered] = got
        return got

    return rest(frozenset(comp))


def parsimony_class_outcomes(reads, t2g, gene_level, exact, large_graph_thresh):
    """The set of admissible class tables of a cell, and whether a component took the fall-back (pugutils.rs:989-1331)."""
    vs, sets, out, comps = graph_of(vertices_of(reads, t2g, gene_level), exact)
    fixed = Counter()           # what no scan order changes
    open_comps = []
    alt = False
    budget = [BOUND]
    for comp in comps:
        if len(comp) == 1:                                                  # pugutils.rs:1262-1322
            fixed[molecule_label(comp, vs, sets, t2g, gene_level)] += 1
        elif len(comp) > large_graph_thresh:                                # pugutils.rs:1055-1072, 916-982: always winner-take-all
            alt = True
            tally = {}
            for v in comp:
                lab, umi, n = vs[v]
                c = tally.setdefault(umi, Counter())
                for g in (lab if gene_level else genes_of(lab, t2g)):
                    c[g] += n
            fixed.update(crlike_classes(tally))
        else:
            o = cover_outcomes(comp, vs, sets, out, t2g, gene_level, budget)
            if len(o) == 1:
                fixed.update(dict(next(iter(o))))
            else:
                open_comps.append(o)
    sums = {frozenset(fixed.items())}
    for o in open_comps:                                                    # a running set of partial sums, never a full product
        nxt = set()
        for a in sums:
            for b in o:
                c = Counter(dict(a))
                c.update(dict(b))
                nxt.add(frozenset(c.items()))
        if len(nxt) > BOUND:
            raise _Undecided
        sums = nxt
    return [dict(s) for s in sums], alt, max((len(c) for c in comps), default=0)


# ----------------------------------------------------------------------------------------------------------------------- a cell

def judge_cell(reads, t2g, resolution, usa, num_rows=None, small_thresh=100, sa_model="winner-take-all", umi_edit_dist=None,
               large_graph_thresh=None, stats=None):
    """reads: [(umi, [ref ids])] of one cell; t2g: ref id -> gene id (USA: spliced 2g, unspliced 2g + 1); num_rows: the USA
    row's width (3 G).  The defaults are the CLI's (main.rs:320-341, 652-703): parsimony* join UMIs one base apart and fall
    back above 1000 vertices.  stats, if a dict, receives the size of the cell's largest component."""
    assert resolution in PLAIN + WITH_EM
    pars = resolution.startswith("parsimony")
    if umi_edit_dist is None:
        umi_edit_dist = 1 if pars else 0
    if large_graph_thresh is None:
        large_graph_thresh = 1000 if pars else 0
    prefer_ambig = usa and sa_model == "prefer-ambig"                       # quant.rs:1456-1469: ignored outside USA mode
    reads = [(int(u), [int(t) for t in refs]) for u, refs in reads]
    with_em = resolution in WITH_EM

    def plain_row(classes):
        return row_of_classes(classes, usa, num_rows)

    if not prefer_ambig and len(reads) < small_thresh:                      # quant.rs:794-846: cr-like whatever -r says, no classes
        return Judgement([(plain_row(crlike_classes(tally_reads(reads, t2g))), None)], False, FLAG_TINY)
    if resolution == "trivial":
        return Judgement([(trivial_row(reads, t2g), None)], False, 0)
    if not pars:
        classes = dict(crlike_classes(tally_reads(reads, t2g), prefer_ambig))
        return Judgement([(None if with_em else plain_row(classes), classes)], False, 0)
    try:
        tables, alt, biggest = parsimony_class_outcomes(reads, t2g, "gene" in resolution, umi_edit_dist == 0, large_graph_thresh)
    except _Undecided:
        return Judgement([], True, 0)
    if stats is not None:
        stats["largest_component"] = biggest
    return Judgement([(None if with_em else plain_row(c), c) for c in tables], False, FLAG_ALT if alt else 0)


def _as_row(row):
    return {int(c): float(v) for c, v in (row.items() if isinstance(row, dict) else row)}


def _as_classes(classes):
    return {tuple(int(g) for g in lab): int(n) for lab, n in (classes.items() if isinstance(classes, dict) else classes)}


def _first_difference(want, got, what):
    for k in sorted(set(want) | set(got)):
        if want.get(k, 0) != got.get(k, 0):
            return f"{what} {k}: judge {want.get(k, 0)}, got {got.get(k, 0)}"
    return None


def admits(judgement, row=None, classes=None, flags=None):
    """Is (row, classes, flags) one of the judgement's outcomes?  True, or a message naming the first difference from the
    first outcome.  row: {column: count} or [(column, count)]; classes: {label: count} or [(label, count)] (what -d dumps);
    flags: the cell's flag bits; the empty-cell bit is judged against the row itself.  What is None is not judged."""
    if judgement.undecided:
        return "the judge left this cell undecided"
    if flags is not None:
        fixed = int(flags) & (FLAG_TINY | FLAG_ALT)
        if fixed != judgement.flags:
            return f"flags: judge {judgement.flags:#x}, got {fixed:#x}"
        if row is not None and bool(int(flags) & FLAG_EMPTY) != (len(_as_row(row)) == 0):
            return f"empty-cell flag {bool(int(flags) & FLAG_EMPTY)} on a row of {len(_as_row(row))} entries"
    row = None if row is None else _as_row(row)
    classes = None if classes is None else _as_classes(classes)
    first = None
    for want_row, want_classes in judgement.outcomes:
        msg = None
        if row is not None and want_row is not None:
            msg = _first_difference(_as_row(want_row), row, "column")
        if msg is None and classes is not None:
            msg = _first_difference(want_classes or {}, classes, "class")
        if msg is None:
            return True
        first = first or msg
    return f"{first} (against the first of {len(judgement.outcomes)} outcomes; none fits)" if len(judgement.outcomes) > 1 else first
