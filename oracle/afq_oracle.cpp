// afq_oracle.cpp — CPU restatement of the `alevin-fry quant` per-cell hot path.
//
// TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the product: only
// tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this
// library, and only as the checker / the timed CPU baseline.
//
// It restates, single-threaded and deliberately following the reference's
// control flow, the Rust code of COMBINE-lab/alevin-fry v0.18.0 (paths relative
// to /root/reference):
//   strategy dispatch            src/quant.rs:794-1026
//   tiny-cell sparse path        src/quant.rs:469-657, 808-845
//   cr-like from reads / eqmap   src/pugutils.rs:751-850, 644-749; --sa-model prefer-ambig 505-641
//   EqMap (txp / gene level)     src/eq_class.rs:723-1036
//   PUG construction             src/pugutils.rs:65-267, src/utils.rs:389-393
//   WCC                          src/pugutils.rs:278-301
//   monochromatic arborescence   src/pugutils.rs:308-391
//   parsimony cover              src/pugutils.rs:989-1331, 916-982
//   trivial                      src/pugutils.rs:852-911
//   USA extraction               src/utils.rs:673-756, 842-926
//   EM (dense / sparse+USA)      src/em.rs:28-34, 167-582   (ora_em over a row of classes = the per-cell work of src/infer.rs:213-224)
//   bootstraps (-b)              src/em.rs:585-757, src/multinomial.rs:9-49, src/quant.rs:157-210
//   gene_eqc as -d sees it       src/quant.rs:1282-1307
//   ATAC fragment dedup          src/atac/deduplicate.rs:199-237, src/atac/sort.rs:37-64
//
// PARITY PINNING.  The reference is Rust and cannot be built here (no cargo /
// rustc, crates not vendored), and its own tests hold no literal count vectors
// for this path.  What pins this restatement: the reference's
// structural known-answers (tests/multi_barcode_integration.rs:1350-1556,
// 163-199; src/em.rs:1035-1215 "sparse == dense") and hand-derived fixtures in
// tests/golden/.  Two behaviours of the reference depend on ahash/hashbrown
// iteration order, which is not reproducible without those crates, so for them
// this oracle fixes a canonical order and is "parity unpinned" there:
//   (1) the scan order of `uncovered_vertices` in the parsimony cover
//       (src/pugutils.rs:1090-1110): ascending vertex id here;
//   (2) the f32 accumulation order of em_update (src/em.rs:464): gene-level
//       classes in lexicographic label order here.
//   (3) bootstraps: the reference draws from an unseeded ThreadRng - no run of it can be reproduced, parity with it
//       is statistical by construction; the draws are restated here on Philox4x32-10 (pinned on the published
//       Random123 known-answer vectors in tests/) with a canonical class / support order, see bootstrap_cell.
// cr-like (both --sa-model's) / trivial / USA extraction are integer-exact and order-independent.

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../include/afquant.h"

namespace {

using u8 = uint8_t;
using u16 = uint16_t;
using u32 = uint32_t;
using u64 = uint64_t;

// gene-level eq classes of one cell: sorted gene-id set -> UMI count
// (`gene_eqc`, src/quant.rs:719-720).  std::map = canonical (lexicographic) order.
using GeneEqc = std::map<std::vector<u32>, u32>;

struct Cell {
    u64 bc = 0;
    u32 nrec = 0;
    std::vector<u64> umi;        // per read
    std::vector<u32> ref_start;  // per read, CSR into refs (nrec+1)
    std::vector<u32> refs;       // orientation bit stripped (libradicl refs())
    u32 na(u32 r) const { return ref_start[r + 1] - ref_start[r]; }
    const u32* rp(u32 r) const { return refs.data() + ref_start[r]; }
};

static inline u64 load_le(const u8* p, u32 w) {
    u64 v = 0;
    for (u32 i = 0; i < w; ++i) v |= (u64)p[i] << (8 * i);
    return v;
}

// Chunk = nbytes:u32 (incl. 8-byte header), nrec:u32, then records
// na:u32, bc, umi, na x u32 (src/convert.rs:124-144, 473-481).
static int parse_chunk(const u8* p, size_t avail, u32 bw, u32 uw, Cell& c, std::string& err) {
    if (avail < 8) { err = "chunk header truncated"; return AFQ_ERR_BAD_INPUT; }
    u32 nbytes = (u32)load_le(p, 4), nrec = (u32)load_le(p + 4, 4);
    if (nbytes < 8 || nbytes > avail) { err = "chunk nbytes out of range"; return AFQ_ERR_BAD_INPUT; }
    c.nrec = nrec;
    c.umi.clear(); c.ref_start.clear(); c.refs.clear();
    c.umi.reserve(nrec); c.ref_start.reserve(nrec + 1);
    c.ref_start.push_back(0);
    size_t pos = 8;
    for (u32 r = 0; r < nrec; ++r) {
        if (pos + 4 + bw + uw > nbytes) { err = "record header overruns chunk"; return AFQ_ERR_BAD_INPUT; }
        u32 na = (u32)load_le(p + pos, 4);
        u64 bc = load_le(p + pos + 4, bw);
        u64 um = load_le(p + pos + 4 + bw, uw);
        pos += 4 + bw + uw;
        if (pos + 4ull * na > nbytes) { err = "record refs overrun chunk"; return AFQ_ERR_BAD_INPUT; }
        if (r == 0) c.bc = bc;
        c.umi.push_back(um);
        for (u32 j = 0; j < na; ++j) c.refs.push_back((u32)load_le(p + pos + 4 * j, 4) & 0x7FFFFFFFu);
        pos += 4ull * na;
        c.ref_start.push_back((u32)c.refs.size());
    }
    if (pos != nbytes) { err = "chunk nbytes does not match its records"; return AFQ_ERR_BAD_INPUT; }
    return 0;
}

// ---------------------------------------------------------------------------
// USA helpers, src/utils.rs:396-428
static inline bool is_spliced(u32 g) { return (g & 1u) == 0; }
static inline bool same_gene(u32 a, u32 b) { return (a & ~1u) == (b & ~1u); }

struct Triplet { u64 umi; u32 gene; u32 ct; };
static inline bool trip_less(const Triplet& a, const Triplet& b) {
    if (a.umi != b.umi) return a.umi < b.umi;
    if (a.gene != b.gene) return a.gene < b.gene;
    return a.ct < b.ct;
}

static void gene_set_of(const u32* refs, u32 na, const u32* t2g, std::vector<u32>& g) {
    g.clear();
    for (u32 j = 0; j < na; ++j) g.push_back(t2g[refs[j]]);
    std::sort(g.begin(), g.end());
    g.erase(std::unique(g.begin(), g.end()), g.end());
}

// resolve_num_molecules_crlike_from_vec, src/pugutils.rs:644-749.
// `F(best_genes, umi)` is called once per UMI with the ascending tie set.
template <class F>
static void crlike_walk(std::vector<Triplet>& v, F&& commit) {
    if (v.empty()) return;
    std::sort(v.begin(), v.end(), trip_less);
    u64 curr_umi = v[0].umi;
    u32 curr_gn = v[0].gene;
    u32 max_count = 0, count_aggr = 0;
    std::vector<u32> best;
    // NB the reference starts with an empty best set and count 0 and lets the
    // first triplet fall into the "same umi" branch; the tiny path
    // (quant.rs:547-552) seeds best with the first gene.  Both give the same
    // tie sets; this follows pugutils.rs.
    for (size_t i = 0; i < v.size(); ++i) {
        const Triplet& t = v[i];
        if (t.umi != curr_umi) {
            commit(best, curr_umi);
            curr_umi = t.umi; curr_gn = t.gene;
            best.clear(); best.push_back(t.gene);
            count_aggr = t.ct; max_count = t.ct;
        } else {
            if (t.gene == curr_gn) count_aggr += t.ct;
            else { count_aggr = t.ct; curr_gn = t.gene; }
            if (count_aggr > max_count) {
                max_count = count_aggr;
                if (!(best.size() == 1 && best[0] == t.gene)) { best.clear(); best.push_back(t.gene); }
            } else if (count_aggr == max_count) {
                best.push_back(t.gene);
            }
        }
        if (i + 1 == v.size()) commit(best, curr_umi);
    }
}

// resolve_num_molecules_crlike_from_vec_prefer_ambig, src/pugutils.rs:505-641 (hidden `--sa-model prefer-ambig`,
// USA mode only): the same walk, but the reads of a UMI are tallied per gene with both splicing states together
// (same_gene(.., true), utils.rs:414-416); `curr` holds the ids of the gene seen so far - [S], [U] or [S, U] - and
// it is `curr`, not the single id, that replaces or joins the best set.
template <class F>
static void crlike_walk_prefer_ambig(std::vector<Triplet>& v, F&& commit) {
    if (v.empty()) return;
    std::sort(v.begin(), v.end(), trip_less);
    u64 curr_umi = v[0].umi;
    std::vector<u32> curr{v[0].gene};          // ArrayVec<u32, 2> in the reference
    u32 max_count = 0, count_aggr = 0;
    std::vector<u32> best;
    for (size_t i = 0; i < v.size(); ++i) {
        const Triplet& t = v[i];
        if (t.umi != curr_umi) {               // pugutils.rs:544-563
            commit(best, curr_umi);
            curr_umi = t.umi;
            curr.assign(1, t.gene);
            best.assign(1, t.gene);
            count_aggr = t.ct; max_count = t.ct;
        } else {                               // pugutils.rs:564-629
            const u32 prev = curr.back();
            if (prev == t.gene || (prev >> 1) == (t.gene >> 1)) {
                if (prev != t.gene) curr.push_back(t.gene);   // spliced -> unspliced transition of one gene
                count_aggr += t.ct;
            } else {
                count_aggr = t.ct;
                curr.assign(1, t.gene);
            }
            if (count_aggr > max_count) { max_count = count_aggr; best = curr; }
            else if (count_aggr == max_count) best.insert(best.end(), curr.begin(), curr.end());
        }
        if (i + 1 == v.size()) commit(best, curr_umi);   // pugutils.rs:633-638
    }
}

static void crlike_into_eqc(std::vector<Triplet>& v, GeneEqc& eqc, bool prefer_ambig = false) {
    if (prefer_ambig) crlike_walk_prefer_ambig(v, [&](const std::vector<u32>& best, u64) { eqc[best] += 1; });
    else crlike_walk(v, [&](const std::vector<u32>& best, u64) { eqc[best] += 1; });
}

// get_num_molecules_cell_ranger_like_small, src/pugutils.rs:751-797
static void crlike_from_reads(const Cell& c, const u32* t2g, GeneEqc& eqc, bool prefer_ambig = false) {
    std::vector<Triplet> v;
    std::vector<u32> g;
    for (u32 r = 0; r < c.nrec; ++r) {
        gene_set_of(c.rp(r), c.na(r), t2g, g);
        for (u32 x : g) v.push_back({c.umi[r], x, 1});
    }
    crlike_into_eqc(v, eqc, prefer_ambig);   // sa_model switch, pugutils.rs:786-797
}

// ---------------------------------------------------------------------------
// EqMap, src/eq_class.rs:314-344, 723-1036
struct EqMap {
    std::vector<u32> labels, label_start;                 // CSR of class labels
    std::vector<std::vector<std::pair<u64, u32>>> umis;   // per class sorted (umi,count)
    u32 n() const { return (u32)umis.size(); }
    const u32* lab(u32 e) const { return labels.data() + label_start[e]; }
    u32 lab_len(u32 e) const { return label_start[e + 1] - label_start[e]; }
};

static void eqmap_build(const Cell& c, const u32* t2g, bool gene_level, EqMap& m) {
    m.labels.clear(); m.label_start.clear(); m.umis.clear();
    struct VH {
        size_t operator()(const std::vector<u32>& v) const {
            u64 h = 0x9E3779B97F4A7C15ull ^ v.size();
            for (u32 x : v) { h ^= x; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 29; }
            return (size_t)h;
        }
    };
    std::unordered_map<std::vector<u32>, u32, VH> ids;  // class id = first-appearance order (eq_class.rs:890)
    std::vector<u32> key;
    for (u32 r = 0; r < c.nrec; ++r) {
        if (gene_level) gene_set_of(c.rp(r), c.na(r), t2g, key);  // eq_class.rs:740-746
        else key.assign(c.rp(r), c.rp(r) + c.na(r));
        auto it = ids.find(key);
        u32 e;
        if (it == ids.end()) {
            e = (u32)m.umis.size();
            ids.emplace(key, e);
            m.label_start.push_back((u32)m.labels.size());
            m.labels.insert(m.labels.end(), key.begin(), key.end());
            m.umis.emplace_back();
        } else e = it->second;
        m.umis[e].push_back({c.umi[r], 1});
    }
    m.label_start.push_back((u32)m.labels.size());
    for (auto& u : m.umis) {  // sort + run-length, eq_class.rs:964-1034
        std::sort(u.begin(), u.end());
        size_t w = 0;
        for (size_t i = 0; i < u.size(); ++i) {
            if (w > 0 && u[w - 1].first == u[i].first) u[w - 1].second += 1;
            else u[w++] = {u[i].first, 1};
        }
        u.resize(w);
    }
}

// get_num_molecules_cell_ranger_like, src/pugutils.rs:799-850
static void crlike_from_eqmap(const EqMap& m, const u32* t2g, GeneEqc& eqc, bool prefer_ambig = false) {
    std::vector<Triplet> v;
    std::vector<u32> g;
    for (u32 e = 0; e < m.n(); ++e) {
        gene_set_of(m.lab(e), m.lab_len(e), t2g, g);
        for (auto& uc : m.umis[e])
            for (u32 x : g) v.push_back({uc.first, x, uc.second});
    }
    crlike_into_eqc(v, eqc, prefer_ambig);   // sa_model switch, pugutils.rs:839-850
}

// ---------------------------------------------------------------------------
// PUG, src/pugutils.rs:65-267
static inline u32 hamming2bit(u64 a, u64 b) {  // src/utils.rs:389-393
    u64 d = a ^ b;
    u64 t = (d | (d >> 1)) & 0x5555555555555555ull;
    return (u32)__builtin_popcountll(t);
}

struct Pug {
    std::vector<u32> v_eq, v_rank;          // vertex -> (class, umi rank)
    std::vector<u32> eq_first;              // class -> first vertex id
    std::vector<std::vector<u32>> out;      // outgoing adjacency
};

static void pug_build(const EqMap& m, bool exact, u32 n_targets, Pug& g) {
    g.v_eq.clear(); g.v_rank.clear(); g.eq_first.clear(); g.out.clear();
    for (u32 e = 0; e < m.n(); ++e) {  // node index = insertion order, pugutils.rs:110-117
        g.eq_first.push_back((u32)g.v_eq.size());
        for (u32 i = 0; i < m.umis[e].size(); ++i) { g.v_eq.push_back(e); g.v_rank.push_back(i); }
    }
    g.out.assign(g.v_eq.size(), {});
    auto edge = [&](u32 vx, const std::pair<u64, u32>& x, u32 vy, const std::pair<u64, u32>& y) {
        u32 d = exact ? (x.first == y.first ? 0u : 99u) : hamming2bit(x.first, y.first);
        if (d == 0) { g.out[vx].push_back(vy); g.out[vy].push_back(vx); return; }
        if (d < 2) {  // pugutils.rs:88-97
            if (x.second > 2 * y.second - 1) g.out[vx].push_back(vy);
            else if (y.second > 2 * x.second - 1) g.out[vy].push_back(vx);
            else { g.out[vx].push_back(vy); g.out[vy].push_back(vx); }
        }
    };
    // inverted index ref -> classes (eq_class.rs:950-959)
    std::unordered_map<u32, std::vector<u32>> containing;
    (void)n_targets;
    for (u32 e = 0; e < m.n(); ++e)
        for (u32 j = 0; j < m.lab_len(e); ++j) containing[m.lab(e)[j]].push_back(e);
    std::vector<u8> seen(m.n(), 0);
    std::vector<u32> touched;
    for (u32 e = 0; e < m.n(); ++e) {
        const auto& u1 = m.umis[e];
        for (u32 a = 0; a < u1.size(); ++a)
            for (u32 b = a + 1; b < u1.size(); ++b) edge(g.eq_first[e] + a, u1[a], g.eq_first[e] + b, u1[b]);
        for (u32 t : touched) seen[t] = 0;
        touched.clear();
        for (u32 j = 0; j < m.lab_len(e); ++j) {
            for (u32 e2 : containing[m.lab(e)[j]]) {
                if (e2 <= e || seen[e2]) continue;
                seen[e2] = 1; touched.push_back(e2);
                const auto& u2 = m.umis[e2];
                for (u32 a = 0; a < u1.size(); ++a)
                    for (u32 b = 0; b < u2.size(); ++b) edge(g.eq_first[e] + a, u1[a], g.eq_first[e2] + b, u2[b]);
            }
        }
    }
}

struct UF {
    std::vector<u32> p;
    explicit UF(u32 n) : p(n) { std::iota(p.begin(), p.end(), 0u); }
    u32 find(u32 x) { while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; } return x; }
    void unite(u32 a, u32 b) { a = find(a); b = find(b); if (a != b) p[std::max(a, b)] = std::min(a, b); }
};

// collapse_vertices, src/pugutils.rs:308-391
static void collapse_vertices(u32 v, const std::vector<u8>& uncovered, const Pug& g, const EqMap& m,
                              std::vector<u32>& largest, u32& chosen, std::vector<u32>& visit_stamp,
                              u32& stamp) {
    largest.clear(); chosen = 0;
    u32 e = g.v_eq[v];
    std::vector<u32> cur, queue;
    for (u32 j = 0; j < m.lab_len(e); ++j) {
        u32 txp = m.lab(e)[j];
        ++stamp;
        cur.clear(); queue.clear();
        queue.push_back(v); visit_stamp[v] = stamp;
        for (size_t h = 0; h < queue.size(); ++h) {
            u32 cv = queue[h];
            cur.push_back(cv);
            for (u32 n : g.out[cv]) {
                if (!uncovered[n] || visit_stamp[n] == stamp) continue;
                visit_stamp[n] = stamp;
                u32 ne = g.v_eq[n];
                if (std::binary_search(m.lab(ne), m.lab(ne) + m.lab_len(ne), txp)) queue.push_back(n);
            }
        }
        if (largest.size() < cur.size()) { largest = cur; chosen = txp; }
    }
}

struct PugStats {
    bool alt = false; u64 total = 0, ambiguous = 0, trivial = 0;
    // How much of the cell hangs on the cover's tie-break (the reference scans a HashSet, pugutils.rs:1090-1110, so WHICH of
    // several equally large monochromatic arborescences is taken first is hash order there and ascending vertex id here):
    // tie_events = cover rounds that met two maximal candidates with different vertex sets; tie_molecules = molecules
    // of the components in which that happened (everything resolved after a tie may depend on it).
    u64 tie_events = 0, tie_components = 0, tie_molecules = 0;
    // ora_set_tie_break(2): every component is also covered with the scan reversed; tie_free_differing counts components in
    // which NO tie event was met and whose molecules nevertheless differ between the two scans (must stay 0: what the
    // tie-break can change is confined to the components that report a tie)
    u64 tie_free_differing = 0;
};
// 0: ascending vertex id (the canonical order the device reproduces); 1: descending - the other extreme, used only to
// measure how many counts depend on the choice (ora_set_tie_break); 2: ascending, and every component checked against its
// descending cover (PugStats::tie_free_differing)
static int g_tie_desc = 0;

// get_num_molecules, src/pugutils.rs:989-1331 (HAS_PROBS == false)
static int parsimony(const Pug& g, const EqMap& m, const u32* t2g, bool gene_level, u32 large_thresh,
                     GeneEqc& eqc, PugStats& st, std::string& err) {
    u32 nv = (u32)g.v_eq.size();
    UF uf(nv);
    for (u32 v = 0; v < nv; ++v) for (u32 w : g.out[v]) uf.unite(v, w);
    std::map<u32, std::vector<u32>> comps;  // root(min id) -> ascending vertex ids
    for (u32 v = 0; v < nv; ++v) comps[uf.find(v)].push_back(v);

    std::vector<u8> uncovered(nv, 0);
    std::vector<u32> visit_stamp(nv, 0);
    u32 stamp = 0;
    std::vector<u32> genes, cand, best, gtx;
    auto label_genes = [&](const u32* lab, u32 n, std::vector<u32>& out) {
        if (gene_level) out.assign(lab, lab + n);
        else gene_set_of(lab, n, t2g, out);
    };
    for (auto& kv : comps) {
        const std::vector<u32>& cv = kv.second;
        if (cv.size() == 1) {  // pugutils.rs:1262-1322
            u32 e = g.v_eq[cv[0]];
            label_genes(m.lab(e), m.lab_len(e), genes);
            st.total++; st.trivial++;
            if (genes.size() > 1) st.ambiguous++;
            eqc[genes] += 1;
            continue;
        }
        if (cv.size() > large_thresh) {  // get_num_molecules_large_component, pugutils.rs:916-982
            std::vector<Triplet> trip;
            for (u32 v : cv) {
                u32 e = g.v_eq[v];
                label_genes(m.lab(e), m.lab_len(e), genes);
                const auto& uc = m.umis[e][g.v_rank[v]];
                for (u32 x : genes) trip.push_back({uc.first, x, uc.second});
            }
            crlike_into_eqc(trip, eqc);
            st.alt = true;
            continue;
        }
        // one cover of the component: molecules (gene labels) in emission order; desc = scan the candidates in descending vertex id
        auto cover = [&](bool desc, std::vector<std::vector<u32>>& mols, bool& comp_tie, u64& ties) -> int {
            for (u32 v : cv) uncovered[v] = 1;
            size_t remaining = cv.size();
            std::vector<u32> best_sorted, cand_sorted;
            while (remaining > 0) {
                best.clear();
                u32 best_txp = UINT32_MAX;
                bool tie_here = false;
                for (size_t vi = 0; vi < cv.size(); ++vi) {  // canonical scan order: ascending vertex id (reference: hash order)
                    const u32 v = desc ? cv[cv.size() - 1 - vi] : cv[vi];
                    if (!uncovered[v]) continue;
                    u32 txp;
                    collapse_vertices(v, uncovered, g, m, cand, txp, visit_stamp, stamp);
                    size_t len = cand.size();
                    if (best.size() < len) { best = cand; best_txp = txp; tie_here = false; best_sorted = cand; std::sort(best_sorted.begin(), best_sorted.end()); }
                    else if (best.size() == len && !tie_here) {
                        cand_sorted = cand; std::sort(cand_sorted.begin(), cand_sorted.end());
                        if (cand_sorted != best_sorted) tie_here = true;   // same vertex set = same molecule whatever the start / transcript
                    }
                    if (len == remaining) break;
                }
                if (tie_here) { ++ties; comp_tie = true; }
                if (best_txp == UINT32_MAX) { err = "could not find a covering transcript"; return AFQ_ERR_BAD_INPUT; }
                // intersection of labels over the mcc, pugutils.rs:1161-1188
                gtx.clear();
                for (size_t i = 0; i < best.size(); ++i) {
                    u32 e = g.v_eq[best[i]];
                    const u32* lb = m.lab(e); u32 ln = m.lab_len(e);
                    if (i == 0) gtx.assign(lb, lb + ln);
                    else {
                        size_t w = 0;
                        for (u32 t : gtx) if (std::binary_search(lb, lb + ln, t)) gtx[w++] = t;
                        gtx.resize(w);
                    }
                }
                label_genes(gtx.data(), (u32)gtx.size(), genes);
                if (gene_level) { std::sort(genes.begin(), genes.end()); genes.erase(std::unique(genes.begin(), genes.end()), genes.end()); }
                if (genes.empty()) { err = "no representative gene for a molecule"; return AFQ_ERR_BAD_INPUT; }
                mols.push_back(genes);
                for (u32 v : best) { uncovered[v] = 0; }
                remaining -= best.size();
            }
            return 0;
        };
        std::vector<std::vector<u32>> mols;
        bool comp_tie = false;
        u64 ties = 0;
        if (int rc = cover(g_tie_desc == 1, mols, comp_tie, ties)) return rc;
        st.tie_events += ties;
        const u64 comp_mols = mols.size();
        for (auto& gs : mols) { st.total++; if (gs.size() > 1) st.ambiguous++; eqc[gs] += 1; }
        if (g_tie_desc == 2 && !comp_tie) {
            std::vector<std::vector<u32>> other;
            bool t2 = false; u64 n2 = 0;
            if (int rc = cover(true, other, t2, n2)) return rc;
            std::sort(mols.begin(), mols.end()); std::sort(other.begin(), other.end());
            if (mols != other) st.tie_free_differing++;
        }
        if (comp_tie) { st.tie_components++; st.tie_molecules += comp_mols; }
    }
    return 0;
}

// ---------------------------------------------------------------------------
// get_num_molecules_trivial_discard_all_ambig, src/pugutils.rs:852-911
static void trivial_counts(const EqMap& m, const u32* t2g, u32 num_genes, std::vector<float>& counts,
                           double& mmrate) {
    counts.assign(num_genes, 0.0f);
    std::map<u32, std::vector<u64>> gene_map;
    u64 total = 0, multi = 0;
    for (u32 e = 0; e < m.n(); ++e) {
        u32 prev = UINT32_MAX; bool multi_gene = false;
        for (u32 j = 0; j < m.lab_len(e); ++j) {
            u32 gid = t2g[m.lab(e)[j]];
            if (gid != prev && prev < UINT32_MAX) { multi_gene = true; break; }
            prev = gid;
        }
        total += m.umis[e].size();
        if (multi_gene) multi += m.umis[e].size();
        else if (prev != UINT32_MAX) { auto& v = gene_map[prev]; for (auto& uc : m.umis[e]) v.push_back(uc.first); }
        // (an alignment-free record would index counts[u32::MAX] in the reference and panic, pugutils.rs:891-907;
        //  mappers do not emit such records - the oracle and the device path leave them out)
    }
    for (auto& kv : gene_map) {
        auto& v = kv.second;
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        counts[kv.first] += (float)v.size();
    }
    mmrate = (double)multi / (double)total;
}

// ---------------------------------------------------------------------------
// USA slot decision shared by extract_counts (utils.rs:688-753) and the tiny
// path's commit_umi (quant.rs:557-605).  Returns the output slot or -1.
static int64_t usa_slot(const std::vector<u32>& lab, u32 unspliced_off, u32 ambig_off) {
    size_t n = lab.size();
    if (n == 1) return is_spliced(lab[0]) ? (lab[0] >> 1) : unspliced_off + (lab[0] >> 1);
    if (n == 2) {
        u32 g1 = lab[0], g2 = lab[1];
        if (same_gene(g1, g2)) return ambig_off + (g1 >> 1);
        bool s1 = is_spliced(g1), s2 = is_spliced(g2);
        if (s1 && !s2) return g1 >> 1;
        if (!s1 && s2) return g2 >> 1;
        return -1;
    }
    if (n >= 3 && n <= 10) {
        int64_t sidx = -1; int ns = 0;
        for (size_t i = 0; i < n; ++i) if (is_spliced(lab[i])) { if (ns == 0) sidx = (int64_t)i; ++ns; }
        if (ns != 1) return -1;
        u32 sg = lab[(size_t)sidx];
        if ((size_t)sidx + 1 < n && same_gene(sg, lab[(size_t)sidx + 1])) return ambig_off + (sg >> 1);
        return sg >> 1;
    }
    return -1;
}

// extract_counts, src/utils.rs:673-756
static void extract_counts(const GeneEqc& eqc, u32 num_rows, std::vector<float>& counts) {
    u32 uo = num_rows / 3, ao = 2 * uo;
    counts.assign(num_rows, 0.0f);
    for (auto& kv : eqc) {
        int64_t s = usa_slot(kv.first, uo, ao);
        if (s >= 0) counts[(size_t)s] += (float)kv.second;
    }
}

// IndexedEqList + (eq_id,count) as built by extract_usa_eqmap, src/utils.rs:842-926
struct IdxEq { std::vector<u32> labels, start; std::vector<u32> count; };
static void extract_usa_eqmap(const GeneEqc& eqc, u32 num_rows, IdxEq& q) {
    u32 uo = num_rows / 3, ao = 2 * uo;
    q.labels.clear(); q.start.assign(1, 0); q.count.clear();
    for (auto& kv : eqc) {
        const auto& lab = kv.first;
        if (lab.size() == 1) {
            q.labels.push_back(is_spliced(lab[0]) ? (lab[0] >> 1) : uo + (lab[0] >> 1));
        } else {
            for (size_t i = 0; i < lab.size(); ++i) {
                u32 gn = lab[i], idx = gn >> 1;
                if (is_spliced(gn)) {
                    if (i + 1 < lab.size() && same_gene(gn, lab[i + 1])) { idx += ao; ++i; }
                } else idx += uo;
                q.labels.push_back(idx);
            }
        }
        q.start.push_back((u32)q.labels.size());
        q.count.push_back(kv.second);
    }
}
static void eqc_to_idx(const GeneEqc& eqc, IdxEq& q) {
    q.labels.clear(); q.start.assign(1, 0); q.count.clear();
    for (auto& kv : eqc) {
        q.labels.insert(q.labels.end(), kv.first.begin(), kv.first.end());
        q.start.push_back((u32)q.labels.size());
        q.count.push_back(kv.second);
    }
}

// Canonical class order for the EM's f32 accumulation.  The reference walks a HashMap
// (em.rs:464; cell_data is filled in hash order, utils.rs:865) so its order is unpinnable;
// this restatement fixes: every single-label class first (ascending label), then the
// multi-label classes in lexicographic order of their gene-level labels (the order the
// caller built them in).  Integer adds first, fractional ones after, per output index.
// g_em_perm != 0 (ora_set_em_order): the canonical order is then shuffled with that seed - what the reference's HashMap does
// to it run by run (em.rs:464, ahash seeded per process) - to measure how much of an EM count hangs on the f32 summation
// order.  Measurement only: parity tests compare against the canonical order.
static uint64_t g_em_perm = 0;
static void canonical_em_order(IdxEq& q) {
    const size_t K = q.count.size();
    std::vector<u32> ord;
    for (u32 c = 0; c < K; ++c) if (q.start[c + 1] - q.start[c] == 1) ord.push_back(c);
    std::stable_sort(ord.begin(), ord.end(), [&](u32 a, u32 b) { return q.labels[q.start[a]] < q.labels[q.start[b]]; });
    for (u32 c = 0; c < K; ++c) if (q.start[c + 1] - q.start[c] != 1) ord.push_back(c);
    if (g_em_perm) {   // Fisher-Yates under splitmix64(seed, number of classes, first label): any order, the same one for a given cell and seed
        uint64_t x = g_em_perm ^ (0x9E3779B97F4A7C15ull * (K + 1)) ^ (q.labels.empty() ? 0 : q.labels[0]);
        auto next = [&]() { x += 0x9E3779B97F4A7C15ull; uint64_t z = x; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); };
        for (size_t i = ord.size(); i > 1; --i) std::swap(ord[i - 1], ord[next() % i]);
    }
    IdxEq r; r.start.push_back(0);
    for (u32 c : ord) {
        r.labels.insert(r.labels.end(), q.labels.begin() + q.start[c], q.labels.begin() + q.start[c + 1]);
        r.start.push_back((u32)r.labels.size());
        r.count.push_back(q.count[c]);
    }
    q = std::move(r);
}

// ---------------------------------------------------------------------------
// EM, src/em.rs
constexpr float MIN_OUTPUT_ALPHA = 0.01f, ALPHA_CHECK_CUTOFF = 1e-2f, REL_DIFF_TOLERANCE = 1e-2f;
constexpr u32 MIN_ITER = 2, MAX_ITER = 100;

static inline float abundance_for(u32 idx, const float* a, u32 uo, u32 ao) {  // em.rs:167-187
    if (idx >= ao) return a[idx - uo] + a[idx - ao] + a[idx];
    if (idx >= uo) return a[idx + uo] + a[idx];
    return a[idx + ao] + a[idx];
}

// g_em_arith (ora_set_em_arith).  0: the reference's arithmetic - f32 additions into alphas_out, in this oracle's canonical
// class order (the reference's own order is a HashMap walk, em.rs:464: unpinnable).  1: ORDER-FREE arithmetic, what the
// device EM computes by default (alevin-fry_amd/csrc/afq_em2.hip): a class's share to an entry is taken as
//     q = (u64)((abundance * (1.0f / denom)) * 2^F)   truncated fixed point, F = min(40, 62 - bitlen(nrec))
// and count * q is added to the entry's 64-bit accumulator, which starts at (sum of its single-label counts) << F; the new
// abundance is (float)acc * 2^-F.  Integer sums do not depend on the order of the classes (so the HashMap question does
// not arise), nor on whether equal labels were merged (count * q is linear in count).  It is NOT the reference's f32
// sequence: tests require it within north_star's 1e-4 of mode 0, and the device bit-identical to it.
static int g_em_arith = 0;
static inline u32 em_fbits(u32 nrec) {
    u32 bl = 0; for (u32 x = nrec | 1u; x; x >>= 1) ++bl;
    const u32 f = 62u - bl;
    return f < 40u ? f : 40u;
}
static void em_update_fixed(const IdxEq& q, const float* ain, u64* acc, bool usa, u32 uo, u32 ao, u32 F) {
    const float scale = std::ldexp(1.0f, (int)F);
    for (size_t c = 0; c + 1 < q.start.size(); ++c) {
        const u32* lab = q.labels.data() + q.start[c];
        const u32 n = q.start[c + 1] - q.start[c];
        if (n > 1) {
            float denom = 0.0f;
            for (u32 j = 0; j < n; ++j) denom += usa ? abundance_for(lab[j], ain, uo, ao) : ain[lab[j]];
            if (denom > 0.0f) {
                const float r = 1.0f / denom;
                for (u32 j = 0; j < n; ++j) {
                    const float ab = usa ? abundance_for(lab[j], ain, uo, ao) : ain[lab[j]];
                    const float u = ab * r;
                    acc[lab[j]] += (u64)q.count[c] * (u64)(u * scale);
                }
            }
        } else acc[lab[0]] += (u64)q.count[c] << F;
    }
}

// one EM round: em_update (em.rs:458-485), em_update_subset[_usa] (em.rs:189-248)
static void em_update(const IdxEq& q, const float* ain, float* aout, bool usa, u32 uo, u32 ao) {
    for (size_t c = 0; c + 1 < q.start.size(); ++c) {
        const u32* lab = q.labels.data() + q.start[c];
        u32 n = q.start[c + 1] - q.start[c];
        float count = (float)q.count[c];
        if (n > 1) {
            float denom = 0.0f;
            for (u32 j = 0; j < n; ++j) denom += usa ? abundance_for(lab[j], ain, uo, ao) : ain[lab[j]];
            if (denom > 0.0f) {
                float inv = count / denom;
                for (u32 j = 0; j < n; ++j) {
                    float x = (usa ? abundance_for(lab[j], ain, uo, ao) : ain[lab[j]]) * inv;
                    aout[lab[j]] += x;
                }
            }
        } else aout[lab[0]] += count;
    }
}

// em_optimize, src/em.rs:487-582 (dense over num_alphas)
static void em_optimize_dense(const GeneEqc& eqc, u32 num_alphas, bool only_unique, bool init_uniform,
                              std::vector<float>& alphas, u32* iters_out, bool canon = false, u32 fixed_bits = 0) {
    IdxEq q; eqc_to_idx(eqc, q);
    if (canon) canonical_em_order(q);
    std::vector<float> ain(num_alphas, 0.0f), aout(num_alphas, 0.0f);
    for (size_t c = 0; c + 1 < q.start.size(); ++c)
        if (q.start[c + 1] - q.start[c] == 1) ain[q.labels[q.start[c]]] += (float)q.count[c];
    if (iters_out) *iters_out = 0;
    if (only_unique) { alphas.swap(ain); return; }
    float uni = 1.0f / (float)num_alphas;
    for (u32 i = 0; i < num_alphas; ++i) ain[i] = init_uniform ? uni : (ain[i] + 0.5f) * 1e-3f;
    u32 it = 0; bool conv = true;
    std::vector<u64> acc(fixed_bits ? num_alphas : 0, 0);
    const float inv_scale = std::ldexp(1.0f, -(int)fixed_bits);
    while (it < MIN_ITER || (it < MAX_ITER && !conv)) {
        if (fixed_bits) {
            em_update_fixed(q, ain.data(), acc.data(), false, 0, 0, fixed_bits);
            for (u32 i = 0; i < num_alphas; ++i) { aout[i] = (float)acc[i] * inv_scale; acc[i] = 0; }
        } else em_update(q, ain.data(), aout.data(), false, 0, 0);
        conv = true;
        for (u32 i = 0; i < num_alphas; ++i) {
            if (aout[i] > ALPHA_CHECK_CUTOFF) {
                float d = std::fabs(ain[i] - aout[i]);
                if (d > REL_DIFF_TOLERANCE) conv = false;
            }
            ain[i] = aout[i]; aout[i] = 0.0f;
        }
        ++it;
    }
    for (auto& a : ain) if (a < MIN_OUTPUT_ALPHA) a = 0.0f;
    if (iters_out) *iters_out = it;
    alphas.swap(ain);
}

// em_optimize_subset_impl, src/em.rs:306-456 (sparse support; optional USA coupling)
// `full_support` walks every alpha instead of the cell's support: that is the
// `dense_reference` of the reference's own unit tests (em.rs:1049-1133), which
// must agree bit for bit with the sparse-support variant.
static void em_optimize_subset(const IdxEq& q, u32 num_alphas, bool only_unique, bool init_uniform,
                               bool usa, u32 uo, u32 ao, std::vector<float>& alphas, u32* iters_out,
                               bool full_support = false, u32 fixed_bits = 0) {
    std::vector<float> ain(num_alphas, 0.0f), aout(num_alphas, 0.0f);
    bool needs_em = false;
    for (size_t c = 0; c + 1 < q.start.size(); ++c) {
        if (q.start[c + 1] - q.start[c] == 1) ain[q.labels[q.start[c]]] += (float)q.count[c];
        else needs_em = true;
    }
    if (iters_out) *iters_out = 0;
    if (only_unique || !needs_em) { alphas.swap(ain); return; }
    // prepare_support, em.rs:87-113
    std::vector<u32> support; std::vector<u8> member(num_alphas, 0);
    auto mark = [&](u32 i) { if (!member[i]) { member[i] = 1; support.push_back(i); } };
    if (full_support) for (u32 i = 0; i < num_alphas; ++i) mark(i);
    for (size_t c = 0; c + 1 < q.start.size() && !full_support; ++c)
        for (u32 j = q.start[c]; j < q.start[c + 1]; ++j) {
            u32 idx = q.labels[j];
            mark(idx);
            if (usa) {
                if (idx >= ao) { mark(idx - uo); mark(idx - ao); }
                else if (idx >= uo) mark(idx + uo);
                else mark(idx + ao);
            }
        }
    float uni = 1.0f / (float)num_alphas;
    for (u32 i : support) ain[i] = init_uniform ? uni : (ain[i] + 0.5f) * 1e-3f;
    u32 it = 0; bool conv = true, last_round = false;
    std::vector<u64> acc(fixed_bits ? num_alphas : 0, 0);
    const float inv_scale = std::ldexp(1.0f, -(int)fixed_bits);
    while (it < MIN_ITER || (it < MAX_ITER && !conv) || last_round) {
        if (fixed_bits) {
            em_update_fixed(q, ain.data(), acc.data(), usa, uo, ao, fixed_bits);
            for (u32 i : support) { aout[i] = (float)acc[i] * inv_scale; acc[i] = 0; }
        } else em_update(q, ain.data(), aout.data(), usa, uo, ao);
        conv = true;
        for (u32 i : support) {
            if (aout[i] > ALPHA_CHECK_CUTOFF) {
                float d = std::fabs(ain[i] - aout[i]);
                if (d > REL_DIFF_TOLERANCE) conv = false;
            }
            ain[i] = aout[i]; aout[i] = 0.0f;
        }
        ++it;
        if (last_round) break;
        if (it >= MIN_ITER && conv) {
            for (u32 i : support) if (ain[i] < MIN_OUTPUT_ALPHA) ain[i] = 0.0f;
            last_round = true;
        }
    }
    for (u32 i : support) if (ain[i] < MIN_OUTPUT_ALPHA) ain[i] = 0.0f;
    if (iters_out) *iters_out = it;
    alphas.swap(ain);
}

// ---------------------------------------------------------------------------
// Bootstraps, src/em.rs:585-757 (run_bootstrap_with_scratch -> run_bootstrap_subset_with_scratch), the multinomial of
// src/multinomial.rs:9-49 (nsamp draws from a WeightedIndex = uniform integer below the total, binary search in the
// cumulative weights) and the summaries of src/quant.rs:157-210.
// The reference's generator is `rand::rng()` (unseeded ThreadRng): its numbers are not reproducible and no run of it can
// be matched - parity here is statistical by construction.  To make the oracle and the device comparable bit for bit the
// draws are restated on a counter-based generator both sides implement independently from the published algorithm
// (Philox4x32-10, Salmon et al., SC'11; known-answer vectors of the Random123 distribution in tests/):
//   draw j of replicate b of cell c   = word j&3 of philox(ctr = (j>>2, b, c_lo, c_hi), key = (seed_lo, seed_hi))
//   start value of support entry s    = word s&3 of philox(ctr = (s>>2, b | 2^31, c_lo, c_hi), same key)
// Hash-order dependent pieces get a canonical order (parity unpinned, as everywhere else): classes = first the labels that
// are one output column (by column), then the rest lexicographically - the order the device keeps them in; support = gene
// ids ascending (the reference's is first-touch order, which only decides which entry gets which random start).
static inline void philox4x32_10(const u32 ctr[4], const u32 key[2], u32 out[4]) {
    u32 c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n1 = (u32)p1, n2 = (u32)(p0 >> 32) ^ c3 ^ k1, n3 = (u32)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct BootOut { std::vector<u32> mean_col, var_col; std::vector<float> mean_val, var_val; };

static int64_t single_column_of(const std::vector<u32>& lab, bool usa, u32 uo, u32 ao) {
    if (lab.size() == 1) return !usa ? (int64_t)lab[0] : (is_spliced(lab[0]) ? (int64_t)(lab[0] >> 1) : (int64_t)uo + (lab[0] >> 1));
    if (usa && lab.size() == 2 && same_gene(lab[0], lab[1])) return (int64_t)ao + (lab[0] >> 1);
    return -1;
}

static void bootstrap_cell(const GeneEqc& eqc, bool usa, u32 num_rows, u32 num_alphas, u32 B, bool summary_stat, u64 seed,
                           u64 cell_index, BootOut& o) {
    o = BootOut();
    if (eqc.empty() || B == 0) return;
    const u32 uo = num_rows / 3, ao = 2 * uo;
    // cell_data in the canonical class order
    std::vector<std::pair<int64_t, const std::vector<u32>*>> single;
    std::vector<const std::vector<u32>*> order;
    for (auto& kv : eqc) { int64_t c = single_column_of(kv.first, usa, uo, ao); if (c >= 0) single.push_back({c, &kv.first}); }
    std::sort(single.begin(), single.end(), [](auto& a, auto& b) { return a.first < b.first; });
    for (auto& x : single) order.push_back(x.second);
    for (auto& kv : eqc) if (single_column_of(kv.first, usa, uo, ao) < 0) order.push_back(&kv.first);
    const size_t K = order.size();
    std::vector<u32> base(K);
    std::vector<u64> cum(K);
    u64 N = 0;
    bool needs_em = false;
    for (size_t k = 0; k < K; ++k) { base[k] = eqc.at(*order[k]); N += base[k]; cum[k] = N; if (order[k]->size() > 1) needs_em = true; }
    // possible support (prepare_support, em.rs:87-113, no USA siblings: usa_offsets is None for the bootstrap, em.rs:632)
    std::vector<u32> support;
    for (auto* l : order) support.insert(support.end(), l->begin(), l->end());
    std::sort(support.begin(), support.end());
    support.erase(std::unique(support.begin(), support.end()), support.end());
    for (u32 g : support) if (g >= num_alphas) return;   // the reference asserts (em.rs:72-75); cannot happen: ids < num_genes <= num_alphas
    const size_t S = support.size();
    std::vector<float> ain(num_alphas, 0.0f), aout(num_alphas, 0.0f), sum(S, 0.0f), sq(S, 0.0f), reps;
    if (!summary_stat) reps.assign((size_t)B * S, 0.0f);
    const u32 key[2] = {(u32)seed, (u32)(seed >> 32)};
    std::vector<u32> cnt(K);
    for (u32 b = 0; b < B; ++b) {
        // Multinomial::sample_u32, multinomial.rs:37-48
        std::fill(cnt.begin(), cnt.end(), 0u);
        u32 w[4];
        for (u64 j = 0; j < N; ++j) {
            if ((j & 3) == 0) { const u32 ctr[4] = {(u32)(j >> 2), b, (u32)cell_index, (u32)(cell_index >> 32)}; philox4x32_10(ctr, key, w); }
            const u64 x = ((u64)w[j & 3] * N) >> 32;   // uniform below the total weight
            const size_t k = (size_t)(std::upper_bound(cum.begin(), cum.end(), x) - cum.begin());
            cnt[k] += 1;
        }
        // em_optimize_subset_impl(.., EmInitType::Random, .., only_unique = false, usa_offsets = None, ..), em.rs:306-456
        for (u32 g : support) { ain[g] = 0.0f; aout[g] = 0.0f; }
        for (size_t k = 0; k < K; ++k) if (order[k]->size() == 1) ain[(*order[k])[0]] += (float)cnt[k];
        if (needs_em) {
            for (size_t si = 0; si < S; ++si) {
                if ((si & 3) == 0) { const u32 ctr[4] = {(u32)(si >> 2), b | 0x80000000u, (u32)cell_index, (u32)(cell_index >> 32)}; philox4x32_10(ctr, key, w); }
                ain[support[si]] = (float)(w[si & 3] >> 8) * (1.0f / 16777216.0f) + 1e-5f;   // rng.random::<f32>() + 1e-5, em.rs:379-381
            }
            u32 it = 0; bool conv = true, last_round = false;
            while (it < MIN_ITER || (it < MAX_ITER && !conv) || last_round) {
                for (size_t k = 0; k < K; ++k) {   // em_update_subset, em.rs:189-218
                    const std::vector<u32>& lab = *order[k];
                    if (lab.size() > 1) {
                        float den = 0.0f;
                        for (u32 l : lab) den += ain[l];
                        if (den > 0.0f) {
                            const float inv = (float)cnt[k] / den;
                            for (u32 l : lab) { const float c = ain[l] * inv; aout[l] += c; }
                        }
                    } else aout[lab[0]] += (float)cnt[k];
                }
                conv = true;
                for (u32 i : support) {
                    if (aout[i] > ALPHA_CHECK_CUTOFF) { if (std::fabs(ain[i] - aout[i]) > REL_DIFF_TOLERANCE) conv = false; }
                    ain[i] = aout[i]; aout[i] = 0.0f;
                }
                ++it;
                if (last_round) break;
                if (it >= MIN_ITER && conv) { for (u32 i : support) if (ain[i] < MIN_OUTPUT_ALPHA) ain[i] = 0.0f; last_round = true; }
            }
            for (u32 i : support) if (ain[i] < MIN_OUTPUT_ALPHA) ain[i] = 0.0f;
        }
        for (size_t si = 0; si < S; ++si) {
            const float a = ain[support[si]];
            if (summary_stat) { sum[si] += a; sq[si] += a * a; }   // em.rs:662-666
            else reps[(size_t)b * S + si] = a;
        }
    }
    for (size_t si = 0; si < S; ++si) {
        float mean, var;
        if (summary_stat) {   // em.rs:673-683, then record_cell keeps the non-zero entries of each (quant.rs:159-182)
            mean = sum[si] / (float)B;
            var = (sq[si] / (float)B) - (mean * mean);
            if (mean != 0.0f) { o.mean_col.push_back(support[si]); o.mean_val.push_back(mean); }
            if (var != 0.0f) { o.var_col.push_back(support[si]); o.var_val.push_back(var); }
        } else {              // record_cell_from_replicates, quant.rs:185-210
            const float n = (float)B;
            float s1 = 0.0f;
            for (u32 b = 0; b < B; ++b) s1 += reps[(size_t)b * S + si];
            mean = s1 / n;
            if (mean != 0.0f) {
                o.mean_col.push_back(support[si]); o.mean_val.push_back(mean);
                float s2 = 0.0f;
                for (u32 b = 0; b < B; ++b) { const float d = reps[(size_t)b * S + si] - mean; s2 += d * d; }
                var = s2 / std::max(n - 1.0f, 1.0f);
                if (var != 0.0f) { o.var_col.push_back(support[si]); o.var_val.push_back(var); }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// tiny-cell sparse path, src/quant.rs:469-657 + caller RLE 808-845
static void tiny_cell(const Cell& c, const u32* t2g, bool usa, u32 num_rows,
                      std::vector<u32>& ind, std::vector<float>& val) {
    ind.clear(); val.clear();
    std::vector<Triplet> trip; std::vector<u32> g;
    for (u32 r = 0; r < c.nrec; ++r) {
        if (c.na(r) == 0) continue;  // quant.rs:495-497
        gene_set_of(c.rp(r), c.na(r), t2g, g);
        for (u32 x : g) trip.push_back({c.umi[r], x, 1});
    }
    if (trip.empty()) return;
    u32 uo = usa ? num_rows / 3 : 0, ao = 2 * uo;
    std::vector<std::pair<u32, u64>> buf;
    crlike_walk(trip, [&](const std::vector<u32>& best, u64 umi) {
        if (best.empty()) return;
        if (!usa) { if (best.size() == 1) buf.push_back({best[0], umi}); return; }
        int64_t s = usa_slot(best, uo, ao);
        if (s >= 0) buf.push_back({(u32)s, umi});
    });
    std::sort(buf.begin(), buf.end());
    for (size_t i = 0; i < buf.size();) {
        size_t j = i;
        while (j < buf.size() && buf[j].first == buf[i].first) ++j;
        ind.push_back(buf[i].first); val.push_back((float)(j - i));
        i = j;
    }
}

struct CellOut {
    std::vector<u32> ind; std::vector<float> val; u8 flags = 0; double mmrate = 0.0; u32 em_iters = 0;
    u32 pug[5] = {0, 0, 0, 0, 0};   // parsimony: molecules, tie events, components with a tie, molecules of those components, tie-free components whose reversed cover differs (mode 2)
    // cfg.dump_eq: gene_eqc as the -d block sees it (quant.rs:1282-1307), in lexicographic label order
    std::vector<u32> eq_labels, eq_len, eq_count;
    BootOut boot;
};

static bool is_parsimony(u32 r) {
    return r == AFQ_RES_PARSIMONY || r == AFQ_RES_PARSIMONY_EM || r == AFQ_RES_PARSIMONY_GENE || r == AFQ_RES_PARSIMONY_GENE_EM;
}

// body of the per-cell loop of run_worker_thread, src/quant.rs:794-1179
static int quant_cell(const afq_config& cfg, const u32* t2g, u32 ref_count, const Cell& c, int force_route,
                      CellOut& o, std::string& err, u64 cell_index = 0) {
    o = CellOut();
    bool usa = cfg.usa_mode != 0;
    u32 sa = usa ? cfg.sa_model : (u32)AFQ_SA_WINNER_TAKE_ALL;  // quant.rs:1456-1469
    if (sa > AFQ_SA_PREFER_AMBIG) { err = "bad sa_model"; return AFQ_ERR_INVALID_ARG; }
    if (cfg.num_bootstraps > 0 && !(cfg.resolution == AFQ_RES_CR_LIKE_EM || cfg.resolution == AFQ_RES_PARSIMONY_EM || cfg.resolution == AFQ_RES_PARSIMONY_GENE_EM)) {
        err = "bootstrapping can only be used with the cr-like-em, parsimony-em, or parsimony-gene-em resolution strategies";   // main.rs:713-728
        return AFQ_ERR_INVALID_ARG;
    }
    const bool pa = sa == AFQ_SA_PREFER_AMBIG;
    for (u32 x : c.refs) if (x >= ref_count) { err = "ref id out of range"; return AFQ_ERR_BAD_INPUT; }
    if (c.nrec == 0) { err = "chunk with no reads"; return AFQ_ERR_BAD_INPUT; }  // quant.rs:756 panics
    if (sa == AFQ_SA_WINNER_TAKE_ALL && c.nrec < cfg.small_thresh && force_route == 0) {
        tiny_cell(c, t2g, usa, cfg.num_rows, o.ind, o.val);
        o.flags |= AFQ_CELL_TINY_PATH;
        if (o.ind.empty()) o.flags |= AFQ_CELL_EMPTY;
        return 0;
    }
    std::vector<float> counts;
    GeneEqc eqc;
    EqMap m;
    u32 uo = cfg.num_rows / 3, ao = 2 * cfg.num_rows / 3;  // usa_offsets, quant.rs:1647-1651
    bool init_uni = cfg.em_init_uniform != 0;
    auto finish = [&](bool only_unique) {
        if (usa && only_unique) extract_counts(eqc, cfg.num_rows, counts);
        else if (usa) {
            IdxEq q; extract_usa_eqmap(eqc, cfg.num_rows, q);
            canonical_em_order(q);
            em_optimize_subset(q, cfg.num_rows, false, init_uni, true, uo, ao, counts, &o.em_iters, false, g_em_arith ? em_fbits(c.nrec) : 0u);
        } else em_optimize_dense(eqc, cfg.num_genes, only_unique, init_uni, counts, &o.em_iters, true, g_em_arith ? em_fbits(c.nrec) : 0u);
    };
    u32 res = cfg.resolution;
    if (res == AFQ_RES_CR_LIKE || res == AFQ_RES_CR_LIKE_EM) {
        bool small_cell = c.nrec <= 250;  // quant.rs:853
        if (force_route == 1) small_cell = true;
        if (force_route == 2) small_cell = false;
        if (small_cell) crlike_from_reads(c, t2g, eqc, pa);
        else { eqmap_build(c, t2g, false, m); crlike_from_eqmap(m, t2g, eqc, pa); }
        finish(res == AFQ_RES_CR_LIKE);
    } else if (res == AFQ_RES_TRIVIAL) {
        eqmap_build(c, t2g, false, m);
        trivial_counts(m, t2g, cfg.num_genes, counts, o.mmrate);
    } else if (is_parsimony(res)) {
        bool gl = (res == AFQ_RES_PARSIMONY_GENE || res == AFQ_RES_PARSIMONY_GENE_EM);
        eqmap_build(c, t2g, gl, m);
        Pug g; pug_build(m, cfg.pug_exact_umi != 0, gl ? cfg.num_genes : ref_count, g);
        PugStats st;
        int rc = parsimony(g, m, t2g, gl, cfg.large_graph_thresh, eqc, st, err);
        if (rc) return rc;
        if (st.alt) o.flags |= AFQ_CELL_ALT_RES;
        o.pug[0] = (u32)st.total; o.pug[1] = (u32)st.tie_events; o.pug[2] = (u32)st.tie_components; o.pug[3] = (u32)st.tie_molecules; o.pug[4] = (u32)st.tie_free_differing;
        finish(res == AFQ_RES_PARSIMONY || res == AFQ_RES_PARSIMONY_GENE);
    } else { err = "bad resolution"; return AFQ_ERR_INVALID_ARG; }
    for (u32 gidx = 0; gidx < counts.size(); ++gidx)  // quant.rs:1156-1168
        if (counts[gidx] > 0.0f) { o.ind.push_back(gidx); o.val.push_back(counts[gidx]); }
    if (o.ind.empty()) o.flags |= AFQ_CELL_EMPTY;
    if (cfg.num_bootstraps > 0 && (res == AFQ_RES_CR_LIKE_EM || res == AFQ_RES_PARSIMONY_EM || res == AFQ_RES_PARSIMONY_GENE_EM))
        // quant.rs:1028-1038: gene_eqc as is, num_alphas = counts.len() (main.rs:713-724 admits the -em resolutions only)
        bootstrap_cell(eqc, usa, cfg.num_rows, (u32)counts.size(), cfg.num_bootstraps, cfg.summary_stat != 0, cfg.boot_seed, cell_index, o.boot);
    if (cfg.dump_eq)   // quant.rs:1282-1307 (`trivial` and tiny-path cells leave gene_eqc empty)
        for (auto& kv : eqc) {
            o.eq_labels.insert(o.eq_labels.end(), kv.first.begin(), kv.first.end());
            o.eq_len.push_back((u32)kv.first.size()); o.eq_count.push_back(kv.second);
        }
    return 0;
}

struct Result {
    std::vector<u64> cell_ptr, bc; std::vector<u32> gene, nrec; std::vector<float> val;
    std::vector<u8> flags; std::vector<double> mmrate; std::vector<u32> em_iters, pug;
    std::vector<u64> eq_cell_ptr{0}, eq_label_ptr{0}; std::vector<u32> eq_labels, eq_count;
    std::vector<u64> bm_ptr{0}, bv_ptr{0}; std::vector<u32> bm_col, bv_col; std::vector<float> bm_val, bv_val;
    void add_eq(const CellOut& o) {
        eq_labels.insert(eq_labels.end(), o.eq_labels.begin(), o.eq_labels.end());
        eq_count.insert(eq_count.end(), o.eq_count.begin(), o.eq_count.end());
        for (u32 l : o.eq_len) eq_label_ptr.push_back(eq_label_ptr.back() + l);
        eq_cell_ptr.push_back(eq_count.size());
        bm_col.insert(bm_col.end(), o.boot.mean_col.begin(), o.boot.mean_col.end());
        bm_val.insert(bm_val.end(), o.boot.mean_val.begin(), o.boot.mean_val.end());
        bv_col.insert(bv_col.end(), o.boot.var_col.begin(), o.boot.var_col.end());
        bv_val.insert(bv_val.end(), o.boot.var_val.begin(), o.boot.var_val.end());
        bm_ptr.push_back(bm_col.size()); bv_ptr.push_back(bv_col.size());
    }
};

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* ora_last_error(void) { return g_err.c_str(); }

// Quantify n_cells chunks.  `force_route`: 0 = reference dispatch; 1 = force the
// from-reads cr-like route; 2 = force the EqMap cr-like route (both skip the
// tiny path) — used by tests to show the three cr-like routes agree.
int ora_quant(const afq_config* cfg, const uint32_t* t2g, uint32_t ref_count, const uint8_t* bytes,
              size_t n_bytes, const uint64_t* chunk_off, uint32_t n_cells, uint64_t first_cell_index,
              int force_route, afq_result* out) {
    if (!cfg || !t2g || !bytes || !chunk_off || !out) { g_err = "null argument"; return AFQ_ERR_INVALID_ARG; }
    auto* R = new Result();
    R->cell_ptr.push_back(0);
    Cell c; CellOut o; std::string err;
    for (uint32_t i = 0; i < n_cells; ++i) {
        if (chunk_off[i] > n_bytes) { delete R; g_err = "chunk offset out of range"; return AFQ_ERR_BAD_INPUT; }
        int rc = parse_chunk(bytes + chunk_off[i], n_bytes - chunk_off[i], cfg->bc_bytes, cfg->umi_bytes, c, err);
        if (!rc) rc = quant_cell(*cfg, t2g, ref_count, c, force_route, o, err, first_cell_index + i);
        if (rc) { delete R; g_err = "cell " + std::to_string(i) + ": " + err; return rc; }
        R->gene.insert(R->gene.end(), o.ind.begin(), o.ind.end());
        R->val.insert(R->val.end(), o.val.begin(), o.val.end());
        R->cell_ptr.push_back(R->gene.size());
        R->bc.push_back(c.bc); R->nrec.push_back(c.nrec); R->flags.push_back(o.flags);
        R->mmrate.push_back(o.mmrate); R->em_iters.push_back(o.em_iters); R->pug.insert(R->pug.end(), o.pug, o.pug + 5); R->add_eq(o);
    }
    out->n_cells = n_cells; out->first_cell_index = first_cell_index; out->nnz = R->gene.size();
    out->cell_ptr = R->cell_ptr.data(); out->gene = R->gene.data(); out->val = R->val.data();
    out->bc = R->bc.data(); out->nrec = R->nrec.data(); out->flags = R->flags.data();
    out->opaque = R;   // (R->mmrate: `trivial`'s multi-mapping rate, kept for ora_result_mmrate; the reference never reads its own, quant.rs:936)
    return 0;
}

// Same, with the cells spread over n_threads worker threads (the reference runs
// t-1 workers over a chunk queue, src/quant.rs:1567-1571).  Used for the CPU baseline.
int ora_quant_mt(const afq_config* cfg, const uint32_t* t2g, uint32_t ref_count, const uint8_t* bytes,
                 size_t n_bytes, const uint64_t* chunk_off, uint32_t n_cells, uint64_t first_cell_index,
                 uint32_t n_threads, afq_result* out) {
    if (!cfg || !t2g || !bytes || !chunk_off || !out) { g_err = "null argument"; return AFQ_ERR_INVALID_ARG; }
    if (n_threads < 1) n_threads = 1;
    std::vector<CellOut> outs(n_cells);
    std::vector<u64> bcs(n_cells);
    std::vector<u32> nrecs(n_cells);
    std::vector<int> rcs(n_threads, 0);
    std::vector<std::string> errs(n_threads);
    std::vector<std::thread> th;
    std::atomic<uint32_t> next{0};   // a shared queue of cells, as the reference's workers pop chunks (quant.rs:733-757)
    for (uint32_t t = 0; t < n_threads; ++t)
        th.emplace_back([&, t]() {
            Cell c; std::string err;
            for (uint32_t i; (i = next.fetch_add(1)) < n_cells && rcs[t] == 0;) {
                int rc = chunk_off[i] > n_bytes ? AFQ_ERR_BAD_INPUT
                                                : parse_chunk(bytes + chunk_off[i], n_bytes - chunk_off[i], cfg->bc_bytes, cfg->umi_bytes, c, err);
                if (!rc) rc = quant_cell(*cfg, t2g, ref_count, c, 0, outs[i], err, first_cell_index + i);
                if (rc) { rcs[t] = rc; errs[t] = "cell " + std::to_string(i) + ": " + err; }
                bcs[i] = c.bc; nrecs[i] = c.nrec;
            }
        });
    for (auto& x : th) x.join();
    for (uint32_t t = 0; t < n_threads; ++t) if (rcs[t]) { g_err = errs[t]; return rcs[t]; }
    auto* R = new Result();
    R->cell_ptr.push_back(0);
    for (uint32_t i = 0; i < n_cells; ++i) {
        R->gene.insert(R->gene.end(), outs[i].ind.begin(), outs[i].ind.end());
        R->val.insert(R->val.end(), outs[i].val.begin(), outs[i].val.end());
        R->cell_ptr.push_back(R->gene.size());
        R->bc.push_back(bcs[i]); R->nrec.push_back(nrecs[i]); R->flags.push_back(outs[i].flags);
        R->mmrate.push_back(outs[i].mmrate); R->em_iters.push_back(outs[i].em_iters); R->pug.insert(R->pug.end(), outs[i].pug, outs[i].pug + 5); R->add_eq(outs[i]);
    }
    out->n_cells = n_cells; out->first_cell_index = first_cell_index; out->nnz = R->gene.size();
    out->cell_ptr = R->cell_ptr.data(); out->gene = R->gene.data(); out->val = R->val.data();
    out->bc = R->bc.data(); out->nrec = R->nrec.data(); out->flags = R->flags.data();
    out->opaque = R;   // (R->mmrate: `trivial`'s multi-mapping rate, kept for ora_result_mmrate; the reference never reads its own, quant.rs:936)
    return 0;
}

// parsimony resolutions: per cell {molecules, tie events, components with a tie, molecules of those components, tie-free components that differ under the reversed scan} (PugStats)
const uint32_t* ora_result_pug_stats(const afq_result* r) { return r && r->opaque ? ((Result*)r->opaque)->pug.data() : nullptr; }
// 0 = ascending vertex id (canonical), 1 = descending: the cover's scan order when several maximal arborescences tie
void ora_set_tie_break(int mode) { g_tie_desc = mode == 1 || mode == 2 ? mode : 0; }
// 0 = canonical class order of the EM's f32 sums; otherwise the seed of a shuffle of it (canonical_em_order)
void ora_set_em_order(uint64_t seed) { g_em_perm = seed; }
// 0 = the reference's f32 sums (canonical class order); 1 = the order-free fixed-point accumulation of the device EM (em_update_fixed)
void ora_set_em_arith(int mode) { g_em_arith = mode == 1 ? 1 : 0; }
// `trivial`: the multi-mapping rate get_num_molecules_trivial_discard_all_ambig returns next to the counts (pugutils.rs:909)
const double* ora_result_mmrate(const afq_result* r) { return r && r->opaque ? ((Result*)r->opaque)->mmrate.data() : nullptr; }
const uint32_t* ora_result_em_iters(const afq_result* r) { return r && r->opaque ? ((Result*)r->opaque)->em_iters.data() : nullptr; }

// cfg.dump_eq: per-cell gene-level classes (same container as afq_result_eqclasses of include/afquant.h)
int ora_result_eqclasses(const afq_result* r, afq_eqclasses* out) {
    if (!r || !r->opaque || !out) return AFQ_ERR_INVALID_ARG;
    const Result* R = (const Result*)r->opaque;
    out->n_cells = R->eq_cell_ptr.size() - 1; out->n_classes = R->eq_count.size(); out->n_words = R->eq_labels.size();
    out->cell_ptr = R->eq_cell_ptr.data(); out->label_ptr = R->eq_label_ptr.data();
    out->labels = R->eq_labels.data(); out->count = R->eq_count.data();
    return 0;
}

// cfg.num_bootstraps: per-cell bootstrap mean / variance (same container as afq_result_bootstraps)
int ora_result_bootstraps(const afq_result* r, afq_bootstraps* out) {
    if (!r || !r->opaque || !out) return AFQ_ERR_INVALID_ARG;
    const Result* R = (const Result*)r->opaque;
    out->n_cells = R->bm_ptr.size() - 1;
    out->mean_ptr = R->bm_ptr.data(); out->mean_col = R->bm_col.data(); out->mean_val = R->bm_val.data();
    out->var_ptr = R->bv_ptr.data(); out->var_col = R->bv_col.data(); out->var_val = R->bv_val.data();
    return 0;
}

// Philox4x32-10 block, exported so the tests can pin it on the published known-answer vectors
void ora_philox4x32_10(const uint32_t* ctr, const uint32_t* key, uint32_t* out) { philox4x32_10(ctr, key, out); }

void ora_result_release(afq_result* r) {
    if (r && r->opaque) { delete (Result*)r->opaque; std::memset(r, 0, sizeof(*r)); }
}

// Stand-alone EM entry points for the em.rs known-answer cases (em.rs:1035-1215).
// labels/start: CSR of class labels, count per class.  usa: couple S/U/A with
// offsets (uo, ao).  dense: 0 = sparse-support subset variant (em.rs:306-456), 1 = em_optimize
// (em.rs:487-582), 2 = the subset algorithm over every alpha (dense_reference, em.rs:1049-1133).
int ora_em(const uint32_t* labels, const uint32_t* start, const uint32_t* count, uint32_t n_classes,
           uint32_t num_alphas, int only_unique, int init_uniform, int usa, uint32_t uo, uint32_t ao,
           int dense, float* alphas_out, uint32_t* iters_out) {
    std::vector<float> a;
    if (dense == 1) {
        GeneEqc eqc;
        for (uint32_t c = 0; c < n_classes; ++c)
            eqc[std::vector<u32>(labels + start[c], labels + start[c + 1])] += count[c];
        em_optimize_dense(eqc, num_alphas, only_unique != 0, init_uniform != 0, a, iters_out);
    } else {
        IdxEq q;
        q.labels.assign(labels, labels + start[n_classes]);
        q.start.assign(start, start + n_classes + 1);
        q.count.assign(count, count + n_classes);
        em_optimize_subset(q, num_alphas, only_unique != 0, init_uniform != 0, usa != 0, uo, ao, a, iters_out,
                           dense == 2 /* dense_reference of em.rs:1049-1133 */);
    }
    std::memcpy(alphas_out, a.data(), sizeof(float) * num_alphas);
    return 0;
}

// PUG edge predicate (has_edge, pugutils.rs:76-99): 0 none, 1 x->y, 2 y->x, 3 both.
int ora_has_edge(uint64_t xu, uint32_t xc, uint64_t yu, uint32_t yc, int exact) {
    u32 d = exact ? (xu == yu ? 0u : 99u) : hamming2bit(xu, yu);
    if (d == 0) return 3;
    if (d < 2) { if (xc > 2 * yc - 1) return 1; if (yc > 2 * xc - 1) return 2; return 3; }
    return 0;
}

// ATAC per-cell dedup, src/atac/deduplicate.rs:199-237 with HitInfo ordering
// (chr, start, frag_len, barcode) from src/atac/sort.rs:37-64.  The barcode is
// constant within a cell so it does not affect the order.  Counts are u16 and
// (like Vec::dedup_by_key accumulation in the reference) are not saturated.
// n_dup (may be null): += the runs of more than one record - from the run length before `count as u16` cuts it, as
// deduplicate.rs:224 tests it (a run of 65536 records is stored as 0 and is deduplicated all the same)
static void atac_dedup_cells(const uint32_t* ref, const uint32_t* start, const uint16_t* flen, const uint64_t* cell_ptr,
                             uint32_t n_cells, uint64_t* out_cell_ptr, uint32_t* out_ref, uint32_t* out_start,
                             uint16_t* out_flen, uint16_t* out_count, uint64_t* n_dup) {
    struct H { u32 r, s; u16 f; };
    uint64_t w = 0;
    out_cell_ptr[0] = 0;
    std::vector<H> v;
    for (uint32_t c = 0; c < n_cells; ++c) {
        v.clear();
        for (uint64_t i = cell_ptr[c]; i < cell_ptr[c + 1]; ++i) v.push_back({ref[i], start[i], flen[i]});
        std::sort(v.begin(), v.end(), [](const H& a, const H& b) {
            if (a.r != b.r) return a.r < b.r;
            if (a.s != b.s) return a.s < b.s;
            return a.f < b.f;
        });
        for (size_t i = 0; i < v.size();) {
            size_t j = i;
            while (j < v.size() && v[j].r == v[i].r && v[j].s == v[i].s && v[j].f == v[i].f) ++j;
            out_ref[w] = v[i].r; out_start[w] = v[i].s; out_flen[w] = v[i].f; out_count[w] = (u16)(j - i);
            if (n_dup && j - i > 1) ++*n_dup;
            ++w; i = j;
        }
        out_cell_ptr[c + 1] = w;
    }
}

int ora_atac_dedup(const uint32_t* ref, const uint32_t* start, const uint16_t* flen, const uint64_t* cell_ptr,
                   uint32_t n_cells, uint64_t* out_cell_ptr, uint32_t* out_ref, uint32_t* out_start,
                   uint16_t* out_flen, uint16_t* out_count) {
    atac_dedup_cells(ref, start, flen, cell_ptr, n_cells, out_cell_ptr, out_ref, out_start, out_flen, out_count, nullptr);
    return 0;
}


// The record loop of `alevin-fry atac deduplicate` in front of that sort (src/atac/deduplicate.rs:199-218): walk the
// AtacSeqReadRecords of every chunk (`na:u32, bc, na x {ref:u32, type:u8, start_pos:u32, frag_len:u16}`,
// tests/atac_integration.rs:110-121), keep na == 1 && map_type == 4, count na > 1 and the rest; then sort + count as above.
// stats[0..4] = records, multi-mapped, not a mapped pair, fragments seen more than once, fragments of >= 2000 bases
// (what write_bed leaves out, deduplicate.rs:47-63).  out_* must hold one entry per record.  Returns 0, or
// AFQ_ERR_BAD_INPUT when a chunk's records do not tile it.
int ora_atac_dedup_rad(const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_cells, uint32_t bc_bytes,
                       uint64_t* out_cell_ptr, uint64_t* out_bc, uint32_t* out_ref, uint32_t* out_start, uint16_t* out_flen,
                       uint16_t* out_count, uint64_t* stats) {
    std::vector<u32> ref, start; std::vector<u16> flen; std::vector<uint64_t> ptr(1, 0);
    for (int i = 0; i < 5; ++i) stats[i] = 0;
    const size_t H = 4 + bc_bytes;
    for (uint32_t c = 0; c < n_cells; ++c) {
        if (chunk_off[c] + 8 > n_bytes) { g_err = "chunk offset out of range"; return AFQ_ERR_BAD_INPUT; }
        const uint8_t* ch = bytes + chunk_off[c];
        u32 nb, nr; std::memcpy(&nb, ch, 4); std::memcpy(&nr, ch + 4, 4);
        if (nb < 8 || chunk_off[c] + nb > n_bytes) { g_err = "chunk size out of range"; return AFQ_ERR_BAD_INPUT; }
        size_t p = 8;
        u64 bc = 0;
        for (u32 r = 0; r < nr; ++r) {
            if (p + H > nb) { g_err = "cell " + std::to_string(c) + ": records run past the chunk"; return AFQ_ERR_BAD_INPUT; }
            u32 na; std::memcpy(&na, ch + p, 4);
            if (r == 0) std::memcpy(&bc, ch + p + 4, bc_bytes);
            if ((u64)na * 11 > nb - p - H) { g_err = "cell " + std::to_string(c) + ": records run past the chunk"; return AFQ_ERR_BAD_INPUT; }
            stats[0]++;
            if (na == 1 && ch[p + H + 4] == 4) {
                u32 rf, st; u16 fl;
                std::memcpy(&rf, ch + p + H, 4); std::memcpy(&st, ch + p + H + 5, 4); std::memcpy(&fl, ch + p + H + 9, 2);
                ref.push_back(rf); start.push_back(st); flen.push_back(fl);
            } else if (na > 1) stats[1]++;
            else stats[2]++;
            p += H + 11ull * na;
        }
        if (p != nb) { g_err = "cell " + std::to_string(c) + ": records do not tile the chunk"; return AFQ_ERR_BAD_INPUT; }
        out_bc[c] = bc;
        ptr.push_back(ref.size());
    }
    atac_dedup_cells(ref.data(), start.data(), flen.data(), ptr.data(), n_cells, out_cell_ptr, out_ref, out_start, out_flen, out_count, &stats[3]);
    for (uint64_t k = 0; k < out_cell_ptr[n_cells]; ++k) if (out_flen[k] >= 2000) stats[4]++;
    return 0;
}

}  // extern "C"
