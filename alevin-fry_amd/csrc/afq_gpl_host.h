// afq_gpl_host.h — the host half of `generate-permit-list` that needs no device: the confidence parser, the barcode-list parser,
// the knee, the retained-set rules, the neighbourhood a retained barcode generates, and the writers of the five output files.
// Plain C++, no HIP: afq_host.cpp wraps these into the entry points of include/afquant_host.h, and the CPU suite compiles them on
// their own (tests/test_gpl_host_cpu.py, under the address and undefined-behaviour sanitizers).  Every function reports through
// `err` and a negative AFQ_ERR_* code.
#pragma once
#include <sys/stat.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/afquant.h"
#include "../../include/afquant_host.h"

namespace afq {
namespace gplhost {

inline int gfail(std::string& err, int code, const std::string& m) { err = m; return code; }
struct GplFileCloser { void operator()(FILE* f) const { if (f) std::fclose(f); } };
using GplFile = std::unique_ptr<FILE, GplFileCloser>;
inline int gpl_mkdirs(const std::string& p) {   // 0 when the directory exists afterwards
    std::string cur;
    for (size_t i = 0; i <= p.size(); ++i) {
        if (i == p.size() || p[i] == '/') { if (!cur.empty()) ::mkdir(cur.c_str(), 0755); }
        if (i < p.size()) cur.push_back(p[i]);
    }
    struct stat st;
    return (::stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) ? 0 : -1;
}
inline std::string gpl_json_escape(const std::string& s) {
    std::string o;
    for (char ch : s) { if (ch == '"' || ch == '\\') { o.push_back('\\'); o.push_back(ch); } else if (ch == '\n') o += "\\n"; else o.push_back(ch); }
    return o;
}
inline uint64_t gcd_u64(uint64_t a, uint64_t b) { while (b) { const uint64_t r = a % b; a = b; b = r; } return a ? a : 1; }
inline bool all_digits(const std::string& s) { for (char ch : s) if (ch < '0' || ch > '9') return false; return true; }
inline bool parse_u64_strict(const std::string& s, uint64_t& v) {
    if (s.empty() || !all_digits(s)) return false;
    v = 0;
    for (char ch : s) { if (v > (UINT64_MAX - (uint64_t)(ch - '0')) / 10) return false; v = v * 10 + (uint64_t)(ch - '0'); }
    return true;
}
inline int confidence_new(uint64_t num, uint64_t den, uint64_t* onum, uint64_t* oden, std::string& err) {
    if (den == 0 || num > den)
        return gfail(err, AFQ_ERR_INVALID_ARG, "barcode-correction confidence must be between zero and one (got " + std::to_string(num) + "/" + std::to_string(den) + ")");
    const uint64_t g = gcd_u64(num, den);
    *onum = num / g; *oden = den / g;
    return 0;
}
inline uint64_t gpl_base_mask(unsigned n) { return n >= 32 ? ~0ull : (1ull << (2 * n)) - 1ull; }
// for_each_neighbor (barcode_correction.rs:738-782): what a retained source generates
inline void gpl_push_neighbors(uint64_t bc, uint32_t L, bool shift, std::vector<uint64_t>& out) {
    for (uint32_t pos = 0; pos < L; ++pos) {
        const uint32_t sh = 2 * pos;
        const uint64_t base = (bc >> sh) & 3, cleared = bc & ~(3ull << sh);
        for (uint64_t rep = 0; rep < 4; ++rep) if (rep != base) out.push_back(cleared | (rep << sh));
    }
    if (!shift) return;
    for (uint32_t b = 1; b < L; ++b) {
        const uint64_t lower_mask = (1ull << (2 * b)) - 1, upper = bc & ~lower_mask, lower = bc & lower_mask;
        for (uint64_t adm = 0; adm < 4; ++adm) {
            const uint64_t ins = upper | (adm << (2 * (b - 1))) | (lower >> 2);
            const uint64_t del = upper | adm | ((lower & ~(3ull << (2 * b))) << 2);
            if (ins != bc) out.push_back(ins);
            if (del != bc) out.push_back(del);
        }
    }
}
// distance of q from the line p1 p2 (knee_finding.rs:12-26): the operation order of the reference, x * x for powi(2)
inline double knee_distance(double x1, double y1, double x2, double y2, double x0, double y0) {
    const double numer = std::fabs((y2 - y1) * x0 - (x2 - x1) * y0 + x2 * y1 - y2 * x1);
    const double a = y2 - y1, b = x2 - x1;
    const double denom = std::sqrt(a * a + b * b);
    return numer / denom;
}
inline int64_t knee_max_distance_index(const uint64_t* cf, size_t n, std::string& err) {
    if (n < 2)
        return gfail(err, AFQ_ERR_BAD_INPUT, "ERROR: when attempting to find a knee-distance threshold, the list of putative cells is only of length " + std::to_string(n) +
                     ". Cannot proceed. Please check the mapping rate.");
    const double max_x = (double)n, max_y = (double)cf[n - 1];
    const double y1 = (double)cf[0] / max_y, y2 = (double)cf[n - 1] / max_y;
    double max_d = -1.0;
    size_t max_ind = 0;
    for (size_t i = 0; i < n; ++i) {
        const double d = knee_distance(0.0, y1, 1.0, y2, (double)i / max_x, (double)cf[i] / max_y);
        if (d >= max_d) { max_d = d; max_ind = i; }
    }
    return (int64_t)max_ind;
}
inline std::string gpl_json_str(const char* s) { return std::string("\"") + gpl_json_escape(s ? s : "") + "\""; }
inline bool write_freq_file(const std::string& path, uint32_t bclen, const uint64_t* bc, const uint64_t* cnt, uint64_t n) {
    GplFile f(std::fopen(path.c_str(), "wb"));
    if (!f) return false;
    const uint64_t hdr[3] = {1, bclen, n};   // PERMIT_FILE_VER, barcode length, bincode map length
    bool ok = std::fwrite(hdr, 8, 3, f.get()) == 3;
    for (uint64_t i = 0; i < n && ok; ++i) { const uint64_t kv[2] = {bc[i], cnt[i]}; ok = std::fwrite(kv, 8, 2, f.get()) == 2; }
    return ok;
}

inline int parse_confidence(const char* text, uint64_t* num, uint64_t* den, std::string& err) {
    if (!text || !num || !den) return gfail(err, AFQ_ERR_INVALID_ARG, "null argument");
    std::string v = text;
    while (!v.empty() && std::isspace((unsigned char)v.back())) v.pop_back();
    size_t b0 = 0;
    while (b0 < v.size() && std::isspace((unsigned char)v[b0])) ++b0;
    v = v.substr(b0);
    const size_t slash = v.find('/');
    if (slash != std::string::npos) {
        uint64_t a = 0, b = 0;
        if (!parse_u64_strict(v.substr(0, slash), a) || !parse_u64_strict(v.substr(slash + 1), b)) return gfail(err, AFQ_ERR_INVALID_ARG, "invalid barcode-correction confidence '" + v + "'");
        return confidence_new(a, b, num, den, err);
    }
    const size_t dot = v.find('.');
    const std::string whole = v.substr(0, dot), frac = dot == std::string::npos ? std::string() : v.substr(dot + 1);
    if (whole.empty() || !all_digits(whole) || !all_digits(frac) || frac.size() > 18) return gfail(err, AFQ_ERR_INVALID_ARG, "invalid barcode-correction confidence '" + v + "'");
    uint64_t d = 1;
    for (size_t i = 0; i < frac.size(); ++i) d *= 10;   // (at most 10^18: fits)
    uint64_t w = 0, f = 0;
    if (!parse_u64_strict(whole, w) || (!frac.empty() && !parse_u64_strict(frac, f))) return gfail(err, AFQ_ERR_INVALID_ARG, "invalid barcode-correction confidence '" + v + "'");
    if (w && d > UINT64_MAX / w) return gfail(err, AFQ_ERR_INVALID_ARG, "barcode-correction confidence is too large");
    if (w * d > UINT64_MAX - f) return gfail(err, AFQ_ERR_INVALID_ARG, "barcode-correction confidence is too large");
    return confidence_new(w * d + f, d, num, den, err);
}

inline int64_t parse_barcode_list(const uint8_t* text, size_t n, int unfiltered, uint32_t barcode_len, uint64_t* out, size_t cap, uint32_t* first_len, std::string& err) {
    if (!text && n) return gfail(err, AFQ_ERR_INVALID_ARG, "null argument");
    if (!unfiltered && (barcode_len < 1 || barcode_len > 32)) return gfail(err, AFQ_ERR_INVALID_ARG, "barcode length must be between 1 and 32");
    auto code = [](uint8_t ch) -> int { switch (ch) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return -1; } };
    uint64_t cnt = 0;
    size_t first = 0;
    bool have_first = false;
    for (size_t p = 0; p < n;) {
        size_t e = p;
        while (e < n && text[e] != '\n') ++e;
        size_t len = e - p;
        if (len && text[p + len - 1] == '\r') --len;   // (lines() and byte_lines() strip \r\n as well as \n)
        uint32_t k = barcode_len;
        if (unfiltered) {
            if (!have_first) { first = len; have_first = true; }
            else if (len != first) return gfail(err, AFQ_ERR_BAD_INPUT, "found barcodes of different lengths " + std::to_string(first) + " and " + std::to_string(len));
            k = (uint32_t)len;
        }
        // the first window of k valid bases (BitNuclKmer::new(line, k, false).next())
        bool found = false;
        uint64_t v = 0;
        if (k >= 1 && k <= 32 && len >= k) {
            uint32_t run = 0;
            for (size_t i = 0; i < len; ++i) {
                const int c = code(text[p + i]);
                if (c < 0) { run = 0; v = 0; continue; }
                v = ((v << 2) | (uint64_t)c) & gpl_base_mask(k);
                if (++run >= k) { found = true; break; }
            }
        }
        if (found) { if (out && cnt < cap) out[cnt] = v; ++cnt; }
        else if (!unfiltered) return gfail(err, AFQ_ERR_BAD_INPUT, "can't extract kmer: a line of the barcode file holds no valid barcode of length " + std::to_string(barcode_len));
        p = e + 1;
    }
    if (first_len) *first_len = (uint32_t)first;
    return (int64_t)cnt;
}

inline int64_t knee(const uint64_t* freq, size_t n, std::string& err) {
    if (!freq && n) return gfail(err, AFQ_ERR_INVALID_ARG, "null argument");
    static const char* const kZero = "get_knee determined a knee index of 0. This probably should not happen with valid input data.";
    std::vector<uint64_t> cf(n);
    uint64_t acc = 0;
    for (size_t i = 0; i < n; ++i) { acc += freq[i]; cf[i] = acc; }
    size_t prev_max = 0;
    int64_t r = knee_max_distance_index(cf.data(), n, err);
    if (r < 0) return r;
    if (r == 0) return gfail(err, AFQ_ERR_BAD_INPUT, kZero);
    size_t max_idx = (size_t)r, iterations = 0;
    while (max_idx - prev_max != 0) {
        prev_max = max_idx;
        if (++iterations > 100) break;
        const size_t last_idx = std::min(n - 1, max_idx * 5);
        r = knee_max_distance_index(cf.data(), last_idx, err);
        if (r < 0) return r;
        if (r == 0) return gfail(err, AFQ_ERR_BAD_INPUT, kZero);
        max_idx = (size_t)r;
    }
    return (int64_t)max_idx;
}

inline int64_t select_retained(const uint64_t* bc, const uint64_t* count, size_t n, uint32_t method, uint64_t arg, uint64_t* out, size_t cap, std::string& err) {
    if ((!bc || !count) && n) return gfail(err, AFQ_ERR_INVALID_ARG, "null argument");
    if (!n) return 0;
    std::vector<uint64_t> fr(count, count + n);
    std::sort(fr.begin(), fr.end(), std::greater<uint64_t>());
    uint64_t thr = 0;
    switch (method) {
        case AFQ_GPL_UNFILTERED: thr = arg; break;
        case AFQ_GPL_KNEE: { const int64_t k = knee(fr.data(), n, err); if (k < 0) return k; thr = fr[std::min<size_t>((size_t)k, n - 1)]; break; }
        case AFQ_GPL_FORCE: if (arg == 0) return 0; thr = fr[(size_t)std::min<uint64_t>(arg - 1, n - 1)]; break;
        case AFQ_GPL_EXPECT: {
            const double ri_d = std::round((double)arg * 0.99);   // (round: half away from zero, as f64::round)
            const size_t ri = ri_d >= (double)(n - 1) ? n - 1 : (size_t)ri_d;
            thr = std::max<uint64_t>(1, (uint64_t)std::round((double)fr[ri] / 10.0));
            break;
        }
        default: return gfail(err, AFQ_ERR_INVALID_ARG, "afq_gpl_select_retained: the method takes no histogram");
    }
    uint64_t k = 0;
    for (size_t i = 0; i < n; ++i) if (count[i] >= thr) { if (out && k < cap) out[k] = bc[i]; ++k; }
    return (int64_t)k;
}

// permit_freq.bin, all_freq.bin (when t->all_bc), permit_map.bin and correction_plan.bin into the directory `out` (created if missing)
inline int write_table_files(const std::string& out, const afq_gpl_tables* t, std::string& err) {
    if (gpl_mkdirs(out)) return gfail(err, AFQ_ERR_BAD_INPUT, "couldn't create directory path " + out);
    if (!write_freq_file(out + "/permit_freq.bin", t->barcode_len, t->freq_bc, t->freq_count, t->n_freq)) return gfail(err, AFQ_ERR_BAD_INPUT, "could not write permit frequencies");
    if (t->all_bc && !write_freq_file(out + "/all_freq.bin", t->barcode_len, t->all_bc, t->all_count, t->n_all)) return gfail(err, AFQ_ERR_BAD_INPUT, "could not write all_freq.bin");
    {
        GplFile f(std::fopen((out + "/permit_map.bin").c_str(), "wb"));
        if (!f) return gfail(err, AFQ_ERR_BAD_INPUT, "could not create serialization file.");
        bool ok = std::fwrite(&t->n_map, 8, 1, f.get()) == 1;
        for (uint64_t i = 0; i < t->n_map && ok; ++i) { const uint64_t kv[2] = {t->map_obs[i], t->map_cor[i]}; ok = std::fwrite(kv, 8, 2, f.get()) == 2; }
        if (!ok) return gfail(err, AFQ_ERR_BAD_INPUT, "couldn't serialize permit list.");
    }
    {   // correction_plan.bin (correction_plan.rs:20-45): magic, u16 version, bincode of a plan with one global cell scope
        GplFile f(std::fopen((out + "/correction_plan.bin").c_str(), "wb"));
        if (!f) return gfail(err, AFQ_ERR_BAD_INPUT, "could not create correction plan");
        std::string b("AFCORR\0\0", 8);
        auto put = [&](const void* p, size_t n) { b.append((const char*)p, n); };
        auto put8 = [&](uint8_t v) { put(&v, 1); };
        auto put32 = [&](uint32_t v) { put(&v, 4); };
        auto put64 = [&](uint64_t v) { put(&v, 8); };
        const uint16_t ver = 1;
        put(&ver, 2);
        put8(0);                          // sample_barcode_len: None
        put8((uint8_t)t->barcode_len);    // cell_barcode_len
        put8(0);                          // sample_spec: None
        put64(0);                         // sample_corrections: empty
        put64(1);                         // cell_scopes: one
        put8(0);                          // sample_barcode: None
        put8((uint8_t)t->barcode_len); put32(t->neighborhood);   // spec: barcode_len, neighborhood (0 HammingOne, 1 SubstitutionOrShiftOne)
        if (t->frequency) { put32(1); put64(t->conf_num); put64(t->conf_den); put64(t->pseudocount); } else put32(0);
        put64(t->n_plan);
        for (uint64_t i = 0; i < t->n_plan; ++i) { put64(t->plan_obs[i]); put64(t->plan_cor[i]); }
        if (std::fwrite(b.data(), 1, b.size(), f.get()) != b.size()) return gfail(err, AFQ_ERR_BAD_INPUT, "could not write correction plan");
    }
    return 0;
}

inline int write_outputs(const afq_gpl_opts* o, const afq_gpl_tables* t, std::string& err) {
    if (!o || !t || !o->output_dir) return gfail(err, AFQ_ERR_INVALID_ARG, "null option");
    const std::string out = o->output_dir;
    if (int rc = write_table_files(out, t, err)) return rc;
    // generate_permit_list.json; gpl_options restates serde's derive of GenPermitListOpts (parity unpinned)
    static const char* const kOriSym[3] = {"both", "fw", "rc"};
    static const char* const kOriEnum[3] = {"Unknown", "Forward", "Reverse"};
    static const char* const kNbh[2] = {"hamming-1", "substitution-or-shift-1"};
    static const char* const kStat[8] = {"exact_distinct", "exact_reads", "corrected_distinct", "corrected_reads", "ambiguous_distinct", "ambiguous_reads", "not_found_distinct", "not_found_reads"};
    const uint32_t ori = o->expected_ori <= 2 ? o->expected_ori : 0;
    const uint64_t cn = o->conf_den ? o->conf_num : 39, cd = o->conf_den ? o->conf_den : 40;
    std::string fm;
    switch (o->method) {
        case AFQ_GPL_KNEE: fm = "\"KneeFinding\""; break;
        case AFQ_GPL_EXPECT: fm = "{\n      \"ExpectCells\": " + std::to_string(o->method_count) + "\n    }"; break;
        case AFQ_GPL_FORCE: fm = "{\n      \"ForceCells\": " + std::to_string(o->method_count) + "\n    }"; break;
        case AFQ_GPL_VALID_BC: fm = "{\n      \"ExplicitList\": " + gpl_json_str(o->list_file) + "\n    }"; break;
        default: fm = "{\n      \"UnfilteredExternalList\": [\n        " + gpl_json_str(o->list_file) + ",\n        " + std::to_string(o->min_reads) + "\n      ]\n    }"; break;
    }
    const std::string conf = "{\n      \"numerator\": " + std::to_string(cn) + ",\n      \"denominator\": " + std::to_string(cd) + "\n    }";
    std::string j = "{\n";
    j += "  \"velo_mode\": false,\n";
    j += std::string("  \"expected_ori\": \"") + kOriSym[ori] + "\",\n";
    j += "  \"version_str\": \"0.18.0\",\n";
    j += "  \"max-ambig-record\": " + std::to_string(t->max_ambig) + ",\n";
    j += "  \"cmd\": " + gpl_json_str(o->cmdline) + ",\n";
    j += std::string("  \"permit-list-type\": \"") + (t->filtered ? "filtered" : "unfiltered") + "\",\n";
    j += "  \"gpl_options\": {\n";
    j += "    \"input_dir\": " + gpl_json_str(o->input_dir) + ",\n    \"output_dir\": " + gpl_json_str(o->output_dir) + ",\n    \"fmeth\": " + fm + ",\n";
    j += std::string("    \"expected_ori\": \"") + kOriEnum[ori] + "\",\n    \"velo_mode\": false,\n    \"threads\": " + std::to_string(o->num_threads) + ",\n";
    j += "    \"cmdline\": " + gpl_json_str(o->cmdline) + ",\n    \"version\": \"0.18.0\",\n    \"sample_bc_list\": null,\n    \"sample_names\": null,\n";
    j += "    \"sample_correction_mode\": \"exact\",\n    \"sample_bc_ori\": \"Forward\",\n";
    j += std::string("    \"cell_bc_correction\": \"") + (o->frequency ? "frequency" : "unique") + "\",\n";
    j += std::string("    \"cell_bc_neighborhood\": ") + (o->neighborhood < 0 ? std::string("null") : std::string("\"") + kNbh[o->neighborhood ? 1 : 0] + "\"") + ",\n";
    j += "    \"sample_bc_neighborhood\": \"hamming-1\",\n    \"cell_bc_confidence\": " + conf + ",\n    \"sample_bc_confidence\": {\n      \"numerator\": 39,\n      \"denominator\": 40\n    },\n";
    j += "    \"memory_limit\": 536870912,\n    \"tmp_dir\": null\n  },\n";
    j += std::string("  \"resolved_cell_bc_neighborhood\": \"") + kNbh[t->neighborhood ? 1 : 0] + "\",\n";
    j += "  \"resolved_cell_bc_confidence\": \"" + std::to_string(cn) + "/" + std::to_string(cd) + "\",\n";
    j += "  \"correction_stats\": {\n";
    for (int i = 0; i < 8; ++i) j += std::string("    \"") + kStat[i] + "\": " + std::to_string(t->stats[i]) + (i < 7 ? ",\n" : "\n");
    j += "  }\n}";
    GplFile f(std::fopen((out + "/generate_permit_list.json").c_str(), "w"));
    if (!f) return gfail(err, AFQ_ERR_BAD_INPUT, "could not create metadata file.");
    if (std::fwrite(j.data(), 1, j.size(), f.get()) != j.size()) return gfail(err, AFQ_ERR_BAD_INPUT, "cannot write to generate_permit_list.json file");
    return 0;
}

// ---- `atac generate-permit-list` (src/atac/cellfilter.rs)
// initialize_rec_list (cellfilter.rs:39-54): out[0] = 0, out[r + 1] = out[r] + ceil((f32)len / (f32)bin_size).  The quotient and
// its ceiling are taken in f32 as the reference takes them: above 2^24 that is not the integer ceiling (200 000 001 / 100 000
// gives 2000, not 2001).
inline void atac_bin_lens(const uint32_t* ref_lens, size_t n, uint64_t bin_size, uint64_t* out) {
    out[0] = 0;
    for (size_t r = 0; r < n; ++r) {
        const float q = (float)ref_lens[r] / (float)bin_size;
        out[r + 1] = out[r] + (uint64_t)std::ceil(q);
    }
}
// needletail::bitkmer::reverse_complement of a k-mer packed first base highest, A C G T = 0 1 2 3
inline uint64_t reverse_complement(uint64_t v, uint32_t k) {
    uint64_t o = 0;
    for (uint32_t i = 0; i < k; ++i) { o = (o << 2) | (3ull - (v & 3ull)); v >>= 2; }
    return o;
}
inline bool write_vec_u64(const std::string& path, const uint64_t* v, uint64_t n) {   // bincode Vec<u64>: the length, then the values
    GplFile f(std::fopen(path.c_str(), "wb"));
    if (!f) return false;
    return std::fwrite(&n, 8, 1, f.get()) == 1 && (!n || std::fwrite(v, 8, n, f.get()) == n);
}
// The six files of `atac generate-permit-list`: the four table files, bin_recs.bin / bin_lens.bin, and generate_permit_list.json
// (process_unfiltered's json!, cellfilter.rs:273-284; gpl_options restates serde's derive of the ATAC GenPermitListOpts, parity
// unpinned as for RNA).  conf_num / conf_den of `o` are the resolved ones.
inline int write_atac_outputs(const afq_atac_gpl_opts* o, const afq_gpl_tables* t, const uint64_t* bins, uint64_t n_bins, const uint64_t* bin_lens, uint64_t n_lens,
                              uint64_t num_chunks, uint64_t max_bin, std::string& err) {
    if (!o || !t || !o->output_dir) return gfail(err, AFQ_ERR_INVALID_ARG, "null option");
    const std::string out = o->output_dir;
    if (int rc = write_table_files(out, t, err)) return rc;
    if (!write_vec_u64(out + "/bin_recs.bin", bins, n_bins)) return gfail(err, AFQ_ERR_BAD_INPUT, "couldn't serialize bins recs.");
    if (!write_vec_u64(out + "/bin_lens.bin", bin_lens, n_lens)) return gfail(err, AFQ_ERR_BAD_INPUT, "couldn't serialize bins lengths.");
    static const char* const kNbh[2] = {"hamming-1", "substitution-or-shift-1"};
    static const char* const kStat[8] = {"exact_distinct", "exact_reads", "corrected_distinct", "corrected_reads", "ambiguous_distinct", "ambiguous_reads", "not_found_distinct", "not_found_reads"};
    const std::string conf = "{\n      \"numerator\": " + std::to_string(o->conf_num) + ",\n      \"denominator\": " + std::to_string(o->conf_den) + "\n    }";
    std::string j = "{\n";
    j += "  \"version_str\": \"0.18.0\",\n";
    j += "  \"max-ambig-record\": " + std::to_string(t->max_ambig) + ",\n";
    j += "  \"num-chunks\": " + std::to_string(num_chunks) + ",\n";
    j += "  \"cmd\": " + gpl_json_str(o->cmdline) + ",\n";
    j += "  \"permit-list-type\": \"unfiltered\",\n";
    j += "  \"gpl_options\": {\n";
    j += "    \"input_dir\": " + gpl_json_str(o->input_dir) + ",\n    \"output_dir\": " + gpl_json_str(o->output_dir) + ",\n";
    j += "    \"fmeth\": {\n      \"UnfilteredExternalList\": [\n        " + gpl_json_str(o->list_file) + ",\n        " + std::to_string(o->min_reads) + "\n      ]\n    },\n";
    j += "    \"threads\": " + std::to_string(o->num_threads) + ",\n";
    j += std::string("    \"rc\": ") + (o->rc ? "true" : "false") + ",\n";
    j += "    \"cmdline\": " + gpl_json_str(o->cmdline) + ",\n    \"version\": \"0.18.0\",\n";
    j += std::string("    \"cell_bc_correction\": \"") + (o->frequency ? "frequency" : "unique") + "\",\n";
    j += std::string("    \"cell_bc_neighborhood\": \"") + kNbh[o->neighborhood ? 1 : 0] + "\",\n";
    j += "    \"cell_bc_confidence\": " + conf + "\n  },\n";
    j += "  \"max-rec-in-bin\": " + std::to_string(max_bin) + ",\n";
    j += std::string("  \"resolved_cell_bc_neighborhood\": \"") + kNbh[t->neighborhood ? 1 : 0] + "\",\n";
    j += "  \"resolved_cell_bc_confidence\": \"" + std::to_string(o->conf_num) + "/" + std::to_string(o->conf_den) + "\",\n";
    j += "  \"correction_stats\": {\n";
    for (int i = 0; i < 8; ++i) j += std::string("    \"") + kStat[i] + "\": " + std::to_string(t->stats[i]) + (i < 7 ? ",\n" : "\n");
    j += "  }\n}";
    GplFile f(std::fopen((out + "/generate_permit_list.json").c_str(), "w"));
    if (!f) return gfail(err, AFQ_ERR_BAD_INPUT, "could not create metadata file.");
    if (std::fwrite(j.data(), 1, j.size(), f.get()) != j.size()) return gfail(err, AFQ_ERR_BAD_INPUT, "cannot write to generate_permit_list.json file");
    return 0;
}

}  // namespace gplhost
}  // namespace afq
