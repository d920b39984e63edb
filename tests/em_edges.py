"""Hand-built cells at the limits of the order-free EM (csrc/afq_em2.hip) and of the bootstrap kernel (csrc/afq_em.hip k_boot),
shared by tests/test_em_edges_cpu.py (builders and mirror, no device) and tests/test_gpu_em_edges.py (the device against them).

Every cell is cr-like-em input spelled out molecule by molecule: one read per molecule, each under a UMI of its own, with the
ids of tid_to_gid as the ref ids (identity).  A molecule of one gene is a single-label count; a molecule of several genes is
an ambiguous molecule whose gene-level label is exactly those genes (cr-like ties every gene of a one-read UMI,
oracle/afq_oracle.cpp crlike_walk).  USA: gene g has the spliced id 2g and the unspliced id 2g + 1 (num_genes = 2G,
num_rows = 3G); a unique molecule on column c is a read of 2c (S, c < G), of 2(c - G) + 1 (U), or of both ids of the gene (A).

`Em2Shape` restates how k_em2_setup sizes a cell and picks its rounds instance; the line numbers are those of afq_em2.hip."""
from dataclasses import dataclass, field

import numpy as np

from util import pkg

rad = pkg.rad

# afq_em2.hip:106, 116
T0_WORDS, T1_WORDS, T2_WORDS = 9728, 19968, 40192
# afq_em2.hip:325-327: the register arrays of the all-in-LDS instances (EPT x threads)
T0_ENTRIES, T1_ENTRIES, T2_ENTRIES = 256 * 8, 512 * 8, 1024 * 16
NARROW_IDS = 65536   # afq_em2.hip:320: L + P + 2 state ids must fit 16 bits
# afq_em.hip:895-896
BOOT_LDS, BOOT_HEAVY = 11264, 32


def lds_core_words(L, P, usa):
    """em2_lds_core_words, afq_em2.hip:114: acc u64[L] | ab f32[L] (USA) | v f32[L + P + 2]."""
    return 2 * L + (L if usa else 0) + (L + P + 2)


def lds_all_words(L, P, K, Wc, usa):
    """em2_lds_all_words, afq_em2.hip:117-119: the core, coff u16[K + 1] and cw u16[Wc], each rounded up to words."""
    return lds_core_words(L, P, usa) + (K + 2) // 2 + (Wc + 1) // 2 + 2


@dataclass
class Cell:
    """uniq: output column -> single-label count; amb: gene-level labels (ascending gene ids, two or more), one molecule each."""
    uniq: dict = field(default_factory=dict)
    amb: list = field(default_factory=list)


@dataclass
class Em2Shape:
    L: int      # live entries: distinct EM label words
    P: int      # passive siblings (USA): single-label columns outside every label that a live entry reads
    K: int      # classes: ambiguous molecules (the device does not merge equal labels, afq_em2.hip:14-16)
    Wc: int     # label words
    all: int    # lds_all_words
    core: int   # lds_core_words
    tier: int   # the rounds instance
    wide: bool  # tier 4 on the 32-bit route


def em_label(lab, G, usa):
    """k_em2_setup's em_label, afq_em2.hip:168-184 (extract_usa_eqmap): S alone -> g, U alone -> G + g, an adjacent S, U pair
    of one gene -> 2G + g."""
    if not usa:
        return list(lab)
    out, i = [], 0
    while i < len(lab):
        gn = lab[i]
        if gn & 1 == 0 and i + 1 < len(lab) and lab[i + 1] >> 1 == gn >> 1:
            out.append(2 * G + (gn >> 1)); i += 2
        else:
            out.append((G if gn & 1 else 0) + (gn >> 1)); i += 1
    return out


def em2_shape(cell, G, usa, min_tier=0):
    """What k_em2_setup counts for a cell and which instance it picks (afq_em2.hip:157-331, 340)."""
    labels = [em_label(l, G, usa) for l in cell.amb]
    K = len(labels)                                    # :319 K = M
    Wc = sum(len(l) for l in labels)                   # :194-207 every label word, in runs by length
    live = set(x for l in labels for x in l)           # :180 the live bitmap
    L = len(live)                                      # :244-258 popcount ranks
    P = 0
    if usa:                                            # :289-303 a column outside every label that a live entry reads
        uo, ao = G, 2 * G
        for col in cell.uniq:
            if col in live:
                continue
            if col >= ao:
                n = (col - ao, col - uo)
            elif col >= uo:
                n = (col + uo,)
            else:
                n = (col + ao,)
            P += any(x in live for x in n)
    return shape_of_counts(L, P, K, Wc, usa, min_tier)


def shape_of_counts(L, P, K, Wc, usa, min_tier=0):
    """The instance k_em2_setup picks from what it has counted (afq_em2.hip:319-331, 340)."""
    narrow = L + P + 2 <= NARROW_IDS                   # :320
    ids16 = narrow and K < 65535 and Wc <= 65535       # :323
    a, core = lds_all_words(L, P, K, Wc, usa), lds_core_words(L, P, usa)
    if ids16 and a <= T0_WORDS and L <= T0_ENTRIES:    # :325-329
        tier = 0
    elif ids16 and a <= T1_WORDS and L <= T1_ENTRIES:
        tier = 1
    elif ids16 and a <= T2_WORDS and L <= T2_ENTRIES:
        tier = 2
    elif core <= T2_WORDS:
        tier = 3
    else:
        tier = 4
    tier = max(tier, min_tier)                         # :330 AFQ_TEST_EM2_MIN_TIER
    return Em2Shape(L, P, K, Wc, a, core, tier, tier == 4 and not narrow)   # :340 narrow4


def covering_labels(L, K, n_triples=0, label_len=2):
    """K labels over entries 0..L-1 that use every entry: the first ceil(L / label_len) cover them in order, the rest are
    pairs spread over the entries; the first n_triples labels take one more entry (one more label word each)."""
    n_cover = -(-L // label_len)
    assert K >= n_cover and n_triples <= K
    out = []
    for j in range(K):
        if j < n_cover:
            lab = {(j * label_len + t) % L for t in range(label_len)}
        else:
            a = (j * 7919) % L
            lab = {a, (a + 1 + j % (L - 1)) % L}
        t = 1
        while j < n_triples and len(lab) < (label_len if j < n_cover else 2) + 1:
            lab.add((max(lab) + t) % L); t += 1
        out.append(sorted(lab))
    return out


def entry_cell(L, K, usa, G=0, n_triples=0, label_len=2, passive=0, uniq_of=lambda g: 1 + g % 3):
    """A cell whose live entries are genes 0..L-1 (S columns in USA), K labels over them (covering_labels) and single-label
    counts on the live entries; USA: `passive` of those genes also have a single-label count on their A column, which is in
    no label - a passive sibling of the gene's S entry (afq_em2.hip:294)."""
    labels = covering_labels(L, K, n_triples, label_len)
    cell = Cell(uniq={g: uniq_of(g) for g in range(L) if uniq_of(g)}, amb=[[2 * g for g in lab] for lab in labels] if usa else labels)
    for g in range(passive if usa else 0):
        cell.uniq[2 * G + g] = 2 + g % 5
    return cell


def words_cell(L, target_all, usa, G=0, passive=0):
    """A cell of L live entries (pair labels, entry_cell) whose lds_all_words is exactly target_all: the fewest pairs, none,
    one or two of them triples, that make it so.  (Pairs over live entries leave L and P alone: K pairs and n3 triples are
    K classes of 2K + n3 words.)"""
    core = lds_core_words(L, passive if usa else 0, usa)
    for K in range(-(-L // 2), target_all):
        if core + (K + 2) // 2 + (2 * K + 1) // 2 + 2 > target_all:
            break
        for n3 in range(3):
            if core + (K + 2) // 2 + (2 * K + n3 + 1) // 2 + 2 == target_all:
                c = entry_cell(L, K, usa, G, n_triples=n3, passive=passive)
                assert em2_shape(c, G, usa).all == target_all
                return c
    raise ValueError(f"no cell of {L} entries has exactly {target_all} LDS words")


def encode(cells, G, usa, bc0=1000):
    """The cells as collated chunks: (bytes, chunk_off, tid_to_gid, num_genes, num_rows)."""
    nrec, umi, na, refs = [], [], [], []
    for c in cells:
        n = 0
        for col, cnt in sorted(c.uniq.items()):
            if usa:
                ids = [2 * col] if col < G else ([2 * (col - G) + 1] if col < 2 * G else [2 * (col - 2 * G), 2 * (col - 2 * G) + 1])
            else:
                ids = [col]
            for _ in range(cnt):
                na.append(len(ids)); refs.extend(ids); n += 1
        for lab in c.amb:
            na.append(len(lab)); refs.extend(lab); n += 1
        umi.extend(range(n))
        nrec.append(n)
    num_genes = 2 * G if usa else G
    b, off = rad.encode_cells_np(nrec, [bc0 + i for i in range(len(cells))], umi, na, refs)
    return b, off, np.arange(num_genes, dtype=np.uint32), num_genes, (3 * G if usa else G)


def cfg(res, usa, num_genes, num_rows, **kw):
    return pkg.WorkerConfig.for_resolution(res, usa_mode=usa, num_genes=num_genes, num_rows=num_rows, **kw)


# --- placement sweeps: for each limit, cells one below, at and one above it (non-USA / USA); expected (tier, wide) by the mirror
def placement_sweeps(usa):
    """name -> (G, cells).  The cells of a sweep go into one batch."""
    if not usa:
        return {
            "t0_words": (2100, [words_cell(2000, T0_WORDS + d, False) for d in (-1, 0, 1)]),
            "t0_entries": (2100, [entry_cell(T0_ENTRIES + d, -(-(T0_ENTRIES + d) // 64), False, label_len=64) for d in (-1, 0, 1)]),
            "t1_words": (4100, [words_cell(4000, T1_WORDS + d, False) for d in (-1, 0, 1)]),
            "t1_entries": (4100, [entry_cell(T1_ENTRIES + d, -(-(T1_ENTRIES + d) // 64), False, label_len=64) for d in (-1, 0, 1)]),
            "t2_words": (10100, [words_cell(10000, T2_WORDS + d, False) for d in (-1, 0, 1)]),
            # core = 3L + 2: 40187, 40190 (the last L at or under the limit), 40193
            "t3_core": (13400, [entry_cell(L, -(-L // 2), False) for L in (13395, 13396, 13397)]),
            # L + 2 = 65535, 65536, 65537
            "narrow_ids": (65600, [entry_cell(L, -(-L // 2), False, uniq_of=lambda g: g % 2) for L in (65533, 65534, 65535)]),
        }
    return {
        "t0_words": (2000, [words_cell(1500, T0_WORDS + d, True, 2000, passive=100) for d in (-1, 0, 1)]),
        "t0_entries": (2100, [entry_cell(T0_ENTRIES + d, -(-(T0_ENTRIES + d) // 64), True, 2100, label_len=64, passive=20) for d in (-1, 0, 1)]),
        "t1_words": (3600, [words_cell(3500, T1_WORDS + d, True, 3600, passive=50) for d in (-1, 0, 1)]),
        "t1_entries": (4100, [entry_cell(T1_ENTRIES + d, -(-(T1_ENTRIES + d) // 64), True, 4100, label_len=64, passive=20) for d in (-1, 0, 1)]),
        "t2_words": (8100, [words_cell(8000, T2_WORDS + d, True, 8100, passive=50) for d in (-1, 0, 1)]),
        # core = 4L + P + 2 = 40191, 40192, 40193
        "t3_core": (10100, [entry_cell(10000, 5000, True, 10100, passive=P) for P in (189, 190, 191)]),
        # L + P + 2 = 65535, 65536, 65537
        "narrow_ids": (65100, [entry_cell(65000, 32500, True, 65100, passive=P, uniq_of=lambda g: g % 2) for P in (533, 534, 535)]),
    }


# what the mirror must say of each sweep (one below / at / one above the limit): the tiers, and tier 4 on 32-bit ids
EXPECTED_PLACEMENT = {
    False: {"t0_words": ([0, 0, 1], [False] * 3), "t0_entries": ([0, 0, 1], [False] * 3), "t1_words": ([1, 1, 2], [False] * 3),
            "t1_entries": ([1, 1, 2], [False] * 3), "t2_words": ([2, 2, 3], [False] * 3), "t3_core": ([3, 3, 4], [False] * 3),
            "narrow_ids": ([4, 4, 4], [False, False, True])},
    True: {"t0_words": ([0, 0, 1], [False] * 3), "t0_entries": ([0, 0, 1], [False] * 3), "t1_words": ([1, 1, 2], [False] * 3),
           "t1_entries": ([1, 1, 2], [False] * 3), "t2_words": ([2, 2, 3], [False] * 3), "t3_core": ([3, 3, 4], [False] * 3),
           "narrow_ids": ([4, 4, 4], [False, False, True])},
}


def instance_counts(shapes):
    """The six numbers afq_em_instance_counts reports for a batch of these cells."""
    out = [0] * 6
    for s in shapes:
        out[s.tier] += 1
        out[5] += s.wide
    return out


# --- tier 4's hot set (afq_em2.hip:341-376)
def hot_cut(cell, G, usa):
    """k_em2_setup step 7: an entry's degree is its label words (clamped at 63); every degree above t is hot, plus the first
    `extra` entries (column order) of degree t, where t is the largest degree at which the hot cap is not yet full.
    Returns (t, extra, entries of degree t, entries in more than 63 labels, hot cap)."""
    labels = [em_label(l, G, usa) for l in cell.amb]
    deg = {}
    for l in labels:
        for x in l:
            deg[x] = deg.get(x, 0) + 1
    hist = [0] * 64
    for d in deg.values():
        hist[min(d, 63)] += 1
    cap = T2_WORDS // (4 if usa else 3)                 # em2_hot_cap, :116
    t, n = 63, 0
    while t > 0 and n + hist[t] <= cap:                 # :357
        n += hist[t]; t -= 1
    extra = min(cap - n, hist[t]) if t > 0 else 0       # :358
    return t, extra, hist[t], sum(d > 63 for d in deg.values()), cap


def hot_set_cell(usa, G):
    """A cell past the core limit whose hot cut falls inside a group of equal degree: 60 hub entries in 70 labels each (more
    than 63), the others in two labels, a few in three (the hubs' partners)."""
    L = 16000 if not usa else 12000
    amb = []
    hubs = 60
    for h in range(hubs):
        for k in range(70):
            amb.append([h, hubs + (h * 70 + k) % (L - hubs)])
    for rep in range(2):
        for j in range(hubs, L, 2):
            amb.append([j, j + 1] if j + 1 < L else [hubs, j])
    if usa:
        amb = [[2 * g for g in lab] for lab in amb]
    uniq = {g: 1 + g % 4 for g in range(0, L, 3)}
    return Cell(uniq=uniq, amb=amb)


# --- round control: cells whose EM stops at a given round (oracle want_iters), found by a seeded sweep of {A, B} cells
# (n molecules of label {A, B}, uA and uB single-label counts; numpy default_rng(2024), n in 200..3000, uA in 0..12, uB in 0..60)
ROUND_CELLS = {
    # usa: [(n, uA, uB, oracle rounds)]
    False: [(300, 3, 3, 2), (300, 0, 3, 100)],
    True: [(300, 3, 3, 3), (300, 0, 3, 100), (1027, 5, 41, 101)],
}


def ab_cell(n, uA, uB, usa):
    return Cell(uniq={k: v for k, v in ((0, uA), (1, uB)) if v}, amb=[[0, 2] if usa else [0, 1]] * n)


def sibling_zero_cell(G):
    """USA: S_1 is in one label, next to S_0 with 2000 molecules, and leans on a live A_1 (em.rs:167-187); it converges to ~0.005
    and is zeroed after the first converged round, while A_1 (gene 1's reads of both statuses, in labels with S_2) survives: the
    last round runs with a sibling of a surviving entry at 0."""
    uniq = {0: 2000, 2 * G + 1: 10, 2: 50}
    return Cell(uniq=uniq, amb=[[0, 2]] + [[2, 3, 4]] * 50)


def round_cells(usa, G=4):
    cells = [ab_cell(n, a, b, usa) for n, a, b, _ in ROUND_CELLS[usa]]
    if usa:
        cells.append(sibling_zero_cell(G))
    return cells


def two_entry_em_f64(n, uA, uB, rounds):
    """The {A, B} cell's EM in float64 (em.rs:458-485 without the f32 rounding): the largest change of an entry above the
    0.01 cutoff in each round - a capped cell's last rounds still move by far more than the 0.01 tolerance."""
    a, b = (uA + 0.5) * 1e-3, (uB + 0.5) * 1e-3
    out = []
    for _ in range(rounds):
        a2, b2 = uA + n * a / (a + b), uB + n * b / (a + b)
        out.append(max(abs(a2 - a) if a2 > 0.01 else 0.0, abs(b2 - b) if b2 > 0.01 else 0.0))
        a, b = a2, b2
    return out


def two_entry_em_row_f64(n, uA, uB, rounds):
    """The same rounds' values: (A, B) after `rounds` rounds."""
    a, b = (uA + 0.5) * 1e-3, (uB + 0.5) * 1e-3
    for _ in range(rounds):
        a, b = uA + n * a / (a + b), uB + n * b / (a + b)
    return a, b


# --- k_boot (afq_em.hip:895-896, 1026, 1111): classes / support entries in LDS up to BOOT_LDS; an entry in more than BOOT_HEAVY
# classes is summed by a whole wave
def boot_classes_cell(K, S=3000):
    """K gene-level classes over S genes: each gene's single-label class, and K - S distinct pairs."""
    pairs, seen = [], set()
    a = 0
    while len(pairs) < K - S:
        x, y = a % S, (a * 31 + 7 + a // S) % S
        a += 1
        if x != y and (min(x, y), max(x, y)) not in seen:
            seen.add((min(x, y), max(x, y))); pairs.append([min(x, y), max(x, y)])
    return Cell(uniq={g: 1 + g % 2 for g in range(S)}, amb=pairs)


def boot_support_cell(S):
    """S genes in pair labels only (no single-label class): a support of S entries over ceil(S / 2) classes."""
    return Cell(uniq={}, amb=[[j, j + 1] if j + 1 < S else [0, j] for j in range(0, S, 2)])


def boot_heavy_cell(n_classes):
    """Gene 0 in exactly n_classes classes: its single-label class and n_classes - 1 pairs {0, j}, next to 200 others."""
    amb = [[0, j] for j in range(1, n_classes)] * 3
    return Cell(uniq={g: 2 + g % 3 for g in range(200)}, amb=amb)


def gene_classes(cell, G, usa):
    """The cell's gene-level classes as the oracle's -d reports them: {label tuple: count}."""
    out = {}
    for col, c in cell.uniq.items():
        if usa:
            lab = (2 * col,) if col < G else ((2 * (col - G) + 1,) if col < 2 * G else (2 * (col - 2 * G), 2 * (col - 2 * G) + 1))
        else:
            lab = (col,)
        out[lab] = out.get(lab, 0) + c
    for l in cell.amb:
        out[tuple(l)] = out.get(tuple(l), 0) + 1
    return out
