// afq_gpl_host.h — the host half of `generate-permit-list` that needs no device: the confidence parser, the barcode-list parser,
// the knee, the retained-set rules, the neighbourhood a retained barcode generates, and the writers of the five output files; for the
// multi-barcode step the sample list, the sample index (sources that differ from their targets), the routing entries and the plan's scopes;
// and the checks of multi-barcode collate's device call that precede device work (collate_multi_index).
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
inline int gpl_base_code(uint8_t ch) {   // A C G T = 0 1 2 3 in either case; -1: no base
    switch (ch) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return -1; }
}
// the 3 L barcodes one substitution away from bc
inline void gpl_push_substitutions(uint64_t bc, uint32_t L, std::vector<uint64_t>& out) {
    for (uint32_t pos = 0; pos < L; ++pos) {
        const uint32_t sh = 2 * pos;
        const uint64_t base = (bc >> sh) & 3, cleared = bc & ~(3ull << sh);
        for (uint64_t rep = 0; rep < 4; ++rep) if (rep != base) out.push_back(cleared | (rep << sh));
    }
}
// for_each_neighbor (barcode_correction.rs:738-782): what a retained source generates
inline void gpl_push_neighbors(uint64_t bc, uint32_t L, bool shift, std::vector<uint64_t>& out) {
    gpl_push_substitutions(bc, L, out);
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
                const int c = gpl_base_code(text[p + i]);
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

// correction_plan.bin (correction_plan.rs:20-45, 132-161): magic, u16 version, bincode of CorrectionPlan (u64 lengths, u32 enum
// variants, an Option as a tag byte).  sample_len < 0: a single-barcode plan (no sample length, spec or corrections, one scope
// without a sample barcode).  Every list arrives in the order write_to sorts it into: corrections by observed barcode, scopes by
// sample barcode.
struct PlanSpec { uint32_t barcode_len, neighborhood, frequency; uint64_t conf_num, conf_den, pseudocount; };
struct PlanScope { bool has_sample; uint64_t sample_barcode; PlanSpec spec; const uint64_t* obs; const uint64_t* cor; uint64_t n; };
inline std::string plan_bytes(int sample_len, uint32_t cell_len, const PlanSpec* sample_spec, const uint64_t* s_obs, const uint64_t* s_cor, uint64_t n_s,
                              const std::vector<PlanScope>& scopes) {
    std::string b("AFCORR\0\0", 8);
    auto put = [&](const void* p, size_t n) { b.append((const char*)p, n); };
    auto put8 = [&](uint8_t v) { put(&v, 1); };
    auto put32 = [&](uint32_t v) { put(&v, 4); };
    auto put64 = [&](uint64_t v) { put(&v, 8); };
    auto put_spec = [&](const PlanSpec& sp) {   // barcode_len, neighborhood (0 HammingOne, 1 SubstitutionOrShiftOne), resolution
        put8((uint8_t)sp.barcode_len); put32(sp.neighborhood);
        if (sp.frequency) { put32(1); put64(sp.conf_num); put64(sp.conf_den); put64(sp.pseudocount); } else put32(0);
    };
    const uint16_t ver = 1;
    put(&ver, 2);
    if (sample_len < 0) put8(0); else { put8(1); put8((uint8_t)sample_len); }   // sample_barcode_len
    put8((uint8_t)cell_len);                                                    // cell_barcode_len
    if (sample_spec) { put8(1); put_spec(*sample_spec); } else put8(0);         // sample_spec
    put64(n_s);                                                                 // sample_corrections
    for (uint64_t i = 0; i < n_s; ++i) { put64(s_obs[i]); put64(s_cor[i]); }
    put64(scopes.size());                                                       // cell_scopes
    for (const PlanScope& sc : scopes) {
        if (sc.has_sample) { put8(1); put64(sc.sample_barcode); } else put8(0);
        put_spec(sc.spec);
        put64(sc.n);
        for (uint64_t i = 0; i < sc.n; ++i) { put64(sc.obs[i]); put64(sc.cor[i]); }
    }
    return b;
}
inline bool write_plan_file(const std::string& path, int sample_len, uint32_t cell_len, const PlanSpec* sample_spec, const uint64_t* s_obs, const uint64_t* s_cor,
                            uint64_t n_s, const std::vector<PlanScope>& scopes, uint64_t* n_bytes = nullptr) {
    GplFile f(std::fopen(path.c_str(), "wb"));
    if (!f) return false;
    const std::string b = plan_bytes(sample_len, cell_len, sample_spec, s_obs, s_cor, n_s, scopes);
    if (n_bytes) *n_bytes = b.size();
    return std::fwrite(b.data(), 1, b.size(), f.get()) == b.size();
}
// bincode HashMap<u64, u64>; *created: the file could be opened (for callers that tell that failure from a failed write)
inline bool write_map_file(const std::string& path, const uint64_t* obs, const uint64_t* cor, uint64_t n, bool* created = nullptr) {
    GplFile f(std::fopen(path.c_str(), "wb"));
    if (created) *created = (bool)f;
    if (!f) return false;
    bool ok = std::fwrite(&n, 8, 1, f.get()) == 1;
    for (uint64_t i = 0; i < n && ok; ++i) { const uint64_t kv[2] = {obs[i], cor[i]}; ok = std::fwrite(kv, 8, 2, f.get()) == 2; }
    return ok;
}

// permit_freq.bin, all_freq.bin (when t->all_bc), permit_map.bin and correction_plan.bin into the directory `out` (created if missing)
inline int write_table_files(const std::string& out, const afq_gpl_tables* t, std::string& err) {
    if (gpl_mkdirs(out)) return gfail(err, AFQ_ERR_BAD_INPUT, "couldn't create directory path " + out);
    if (!write_freq_file(out + "/permit_freq.bin", t->barcode_len, t->freq_bc, t->freq_count, t->n_freq)) return gfail(err, AFQ_ERR_BAD_INPUT, "could not write permit frequencies");
    if (t->all_bc && !write_freq_file(out + "/all_freq.bin", t->barcode_len, t->all_bc, t->all_count, t->n_all)) return gfail(err, AFQ_ERR_BAD_INPUT, "could not write all_freq.bin");
    bool created = false;
    if (!write_map_file(out + "/permit_map.bin", t->map_obs, t->map_cor, t->n_map, &created))
        return gfail(err, AFQ_ERR_BAD_INPUT, created ? "couldn't serialize permit list." : "could not create serialization file.");
    {   // correction_plan.bin: one global cell scope
        const PlanSpec spec{t->barcode_len, t->neighborhood, t->frequency, t->conf_num, t->conf_den, t->pseudocount};
        const std::vector<PlanScope> scopes{PlanScope{false, 0, spec, t->plan_obs, t->plan_cor, t->n_plan}};
        if (!write_plan_file(out + "/correction_plan.bin", -1, t->barcode_len, nullptr, nullptr, nullptr, 0, scopes))
            return gfail(err, AFQ_ERR_BAD_INPUT, "could not write correction plan");
    }
    return 0;
}

// What both generate_permit_list.json writers (RNA, ATAC) share: the neighbourhoods' names, the end of the object - the resolved
// correction settings (neighbourhood, confidence cn / cd) and correction_stats - and the file itself.
static const char* const kGplNbh[2] = {"hamming-1", "substitution-or-shift-1"};
inline std::string gpl_json_tail(const afq_gpl_tables* t, uint64_t cn, uint64_t cd) {
    static const char* const kStat[8] = {"exact_distinct", "exact_reads", "corrected_distinct", "corrected_reads", "ambiguous_distinct", "ambiguous_reads", "not_found_distinct", "not_found_reads"};
    std::string j = std::string("  \"resolved_cell_bc_neighborhood\": \"") + kGplNbh[t->neighborhood ? 1 : 0] + "\",\n";
    j += "  \"resolved_cell_bc_confidence\": \"" + std::to_string(cn) + "/" + std::to_string(cd) + "\",\n";
    j += "  \"correction_stats\": {\n";
    for (int i = 0; i < 8; ++i) j += std::string("    \"") + kStat[i] + "\": " + std::to_string(t->stats[i]) + (i < 7 ? ",\n" : "\n");
    return j + "  }\n}";
}
inline int write_gpl_json(const std::string& out, const std::string& j, std::string& err) {
    GplFile f(std::fopen((out + "/generate_permit_list.json").c_str(), "w"));
    if (!f) return gfail(err, AFQ_ERR_BAD_INPUT, "could not create metadata file.");
    if (std::fwrite(j.data(), 1, j.size(), f.get()) != j.size()) return gfail(err, AFQ_ERR_BAD_INPUT, "cannot write to generate_permit_list.json file");
    return 0;
}

inline int write_outputs(const afq_gpl_opts* o, const afq_gpl_tables* t, std::string& err) {
    if (!o || !t || !o->output_dir) return gfail(err, AFQ_ERR_INVALID_ARG, "null option");
    const std::string out = o->output_dir;
    if (int rc = write_table_files(out, t, err)) return rc;
    // generate_permit_list.json; gpl_options restates serde's derive of GenPermitListOpts (parity unpinned)
    static const char* const kOriSym[3] = {"both", "fw", "rc"};
    static const char* const kOriEnum[3] = {"Unknown", "Forward", "Reverse"};
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
    j += std::string("    \"cell_bc_neighborhood\": ") + (o->neighborhood < 0 ? std::string("null") : std::string("\"") + kGplNbh[o->neighborhood ? 1 : 0] + "\"") + ",\n";
    j += "    \"sample_bc_neighborhood\": \"hamming-1\",\n    \"cell_bc_confidence\": " + conf + ",\n    \"sample_bc_confidence\": {\n      \"numerator\": 39,\n      \"denominator\": 40\n    },\n";
    j += "    \"memory_limit\": 536870912,\n    \"tmp_dir\": null\n  },\n";
    return write_gpl_json(out, j + gpl_json_tail(t, cn, cd), err);
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
    j += std::string("    \"cell_bc_neighborhood\": \"") + kGplNbh[o->neighborhood ? 1 : 0] + "\",\n";
    j += "    \"cell_bc_confidence\": " + conf + "\n  },\n";
    j += "  \"max-rec-in-bin\": " + std::to_string(max_bin) + ",\n";
    return write_gpl_json(out, j + gpl_json_tail(t, o->conf_num, o->conf_den), err);
}

// ---- multi-barcode `generate-permit-list` (do_generate_permit_list_multi_bc, src/cellfilter.rs:789-1381)
// the argument checks of afq_gpl_multi_hist_rad that precede device work
inline int multi_check_args(uint32_t b0_bytes, uint32_t b1_bytes, uint32_t umi_bytes, uint32_t expected_ori, const uint64_t* entries, uint64_t n, std::string& err) {
    if (!entries && n) return gfail(err, AFQ_ERR_INVALID_ARG, "null argument");
    if (b0_bytes != 1 && b0_bytes != 2 && b0_bytes != 4) return gfail(err, AFQ_ERR_INVALID_ARG, "b0_bytes must be 1, 2 or 4");
    if (b1_bytes != 1 && b1_bytes != 2 && b1_bytes != 4) return gfail(err, AFQ_ERR_INVALID_ARG, "b1_bytes must be 1, 2 or 4");
    if (umi_bytes != 1 && umi_bytes != 2 && umi_bytes != 4 && umi_bytes != 8) return gfail(err, AFQ_ERR_INVALID_ARG, "umi_bytes must be 1, 2, 4 or 8");
    if (expected_ori > 2) return gfail(err, AFQ_ERR_INVALID_ARG, "expected_ori must be 0 (both), 1 (fw) or 2 (rc)");
    if (n > (1ull << 31)) return gfail(err, AFQ_ERR_UNSUPPORTED, "afq_gpl_multi_hist_rad: more than 2^31 routing entries (" + std::to_string(n) + ")");
    for (uint64_t i = 0; i < n; ++i) {
        if (i && entries[i] <= entries[i - 1]) return gfail(err, AFQ_ERR_INVALID_ARG, "sample barcodes must ascend without duplicates (entry " + std::to_string(i) + ")");
        if (entries[i] >> (8 * b0_bytes)) return gfail(err, AFQ_ERR_BAD_INPUT, "packed sample barcode " + std::to_string(entries[i]) + " does not fit " + std::to_string(b0_bytes) + " bytes");
    }
    return 0;
}

// afq_collate_multi_rad's checks and host step, before any device work: widths, orientation, the three inputs.  val[i] = the index
// among the cells of (corr_sample[i], corr_corrected[i]).  A sample index is below n_samples <= 2^31 (the cell table's key is
// sample << 32 | b1 and must not be all ones); sample barcodes and (sample, observed cell barcode) pairs are distinct, as are the cells.
inline int collate_multi_index(uint32_t b0_bytes, uint32_t b1_bytes, uint32_t umi_bytes, uint32_t expected_ori, const uint64_t* sample_observed,
                               const uint32_t* sample_index, uint64_t n_sample_entries, const uint32_t* corr_sample, const uint64_t* corr_observed,
                               const uint64_t* corr_corrected, uint64_t n_corr, const uint32_t* cell_sample, const uint64_t* cell_bc, uint64_t n_cells,
                               const uint32_t* sample_b0_out, uint64_t n_samples, std::vector<uint32_t>& val, std::string& err) {
    if (((!sample_observed || !sample_index) && n_sample_entries) || ((!corr_sample || !corr_observed || !corr_corrected) && n_corr) ||
        ((!cell_sample || !cell_bc) && n_cells) || (!sample_b0_out && n_samples))
        return gfail(err, AFQ_ERR_INVALID_ARG, "null argument");
    if (b0_bytes != 1 && b0_bytes != 2 && b0_bytes != 4) return gfail(err, AFQ_ERR_INVALID_ARG, "b0_bytes must be 1, 2 or 4");
    if (b1_bytes != 1 && b1_bytes != 2 && b1_bytes != 4) return gfail(err, AFQ_ERR_INVALID_ARG, "b1_bytes must be 1, 2 or 4");
    if (umi_bytes != 1 && umi_bytes != 2 && umi_bytes != 4 && umi_bytes != 8) return gfail(err, AFQ_ERR_INVALID_ARG, "umi_bytes must be 1, 2, 4 or 8");
    if (expected_ori > 2) return gfail(err, AFQ_ERR_INVALID_ARG, "expected_ori must be 0 (both), 1 (fw) or 2 (rc)");
    if (n_samples > (1ull << 31)) return gfail(err, AFQ_ERR_INVALID_ARG, "afq_collate_multi_rad: more than 2^31 samples (" + std::to_string(n_samples) + "): a sample index must be below 2^31");
    if (n_sample_entries >= (1ull << 30) || n_corr >= (1ull << 30)) return gfail(err, AFQ_ERR_UNSUPPORTED, "afq_collate_multi_rad: 2^30 or more correction entries");
    if (n_cells > 0xFFFFFFFEull) return gfail(err, AFQ_ERR_UNSUPPORTED, "afq_collate_multi_rad: more than 2^32 - 2 cells (" + std::to_string(n_cells) + ")");
    const uint64_t top0 = b0_bytes < 4 ? (1ull << (8 * b0_bytes)) : (1ull << 32), top1 = b1_bytes < 4 ? (1ull << (8 * b1_bytes)) : (1ull << 32);
    auto bad_sample = [&](const char* what, uint64_t i, uint32_t s) {
        return gfail(err, AFQ_ERR_INVALID_ARG, std::string(what) + " " + std::to_string(i) + ": sample index " + std::to_string(s) + " is not below the " + std::to_string(n_samples) +
                     " samples (a sample index must be below 2^31)");
    };
    for (uint64_t s = 0; s < n_samples; ++s)
        if (sample_b0_out[s] >= top0) return gfail(err, AFQ_ERR_UNSUPPORTED, "sample " + std::to_string(s) + ": the value " + std::to_string(sample_b0_out[s]) + " written into b0 does not fit " + std::to_string(b0_bytes) + " bytes");
    {
        std::vector<uint64_t> so(sample_observed, sample_observed + n_sample_entries);
        std::sort(so.begin(), so.end());
        for (uint64_t i = 0; i < n_sample_entries; ++i) {
            if (sample_index[i] >= n_samples) return bad_sample("sample entry", i, sample_index[i]);
            if (sample_observed[i] >= top0) return gfail(err, AFQ_ERR_BAD_INPUT, "sample barcode " + std::to_string(sample_observed[i]) + " does not fit " + std::to_string(b0_bytes) + " bytes");
            if (i && so[i] == so[i - 1]) return gfail(err, AFQ_ERR_BAD_INPUT, "sample barcode " + std::to_string(so[i]) + " occurs twice among the sample entries");
        }
    }
    std::vector<std::pair<uint64_t, uint32_t>> by(n_cells);   // (sample << 32 | barcode, cell)
    for (uint64_t j = 0; j < n_cells; ++j) {
        if (cell_sample[j] >= n_samples) return bad_sample("cell", j, cell_sample[j]);
        if (cell_bc[j] >= top1) return gfail(err, AFQ_ERR_BAD_INPUT, "cell " + std::to_string(j) + ": barcode " + std::to_string(cell_bc[j]) + " does not fit " + std::to_string(b1_bytes) + " bytes");
        by[j] = {(uint64_t)cell_sample[j] << 32 | cell_bc[j], (uint32_t)j};
    }
    std::sort(by.begin(), by.end());
    for (uint64_t j = 1; j < n_cells; ++j)
        if (by[j].first == by[j - 1].first)
            return gfail(err, AFQ_ERR_BAD_INPUT, "cells " + std::to_string(by[j - 1].second) + " and " + std::to_string(by[j].second) + " carry one barcode (" + std::to_string(by[j].first & 0xFFFFFFFFull) +
                         ") in sample " + std::to_string(by[j].first >> 32));
    val.assign(n_corr, 0);
    std::vector<uint64_t> keys(n_corr);
    for (uint64_t i = 0; i < n_corr; ++i) {
        if (corr_sample[i] >= n_samples) return bad_sample("correction entry", i, corr_sample[i]);
        if (corr_observed[i] >= top1) return gfail(err, AFQ_ERR_BAD_INPUT, "correction entry " + std::to_string(i) + ": observed barcode " + std::to_string(corr_observed[i]) + " does not fit " + std::to_string(b1_bytes) + " bytes");
        keys[i] = (uint64_t)corr_sample[i] << 32 | corr_observed[i];
        const uint64_t want = (uint64_t)corr_sample[i] << 32 | (corr_corrected[i] & 0xFFFFFFFFull);
        const auto it = std::lower_bound(by.begin(), by.end(), std::make_pair(want, 0u));
        if (corr_corrected[i] >= top1 || it == by.end() || it->first != want)
            return gfail(err, AFQ_ERR_BAD_INPUT, "correction entry " + std::to_string(i) + ": observed barcode " + std::to_string(corr_observed[i]) + " of sample " + std::to_string(corr_sample[i]) +
                         " is corrected to " + std::to_string(corr_corrected[i]) + ", which is not a cell of that sample");
        val[i] = it->second;
    }
    std::sort(keys.begin(), keys.end());
    for (uint64_t i = 1; i < n_corr; ++i)
        if (keys[i] == keys[i - 1])
            return gfail(err, AFQ_ERR_BAD_INPUT, "observed barcode " + std::to_string(keys[i] & 0xFFFFFFFFull) + " occurs twice among the corrections of sample " + std::to_string(keys[i] >> 32));
    return 0;
}

// load_sample_barcode_list (cellfilter.rs:1405-1569).  rotations ascend by observed barcode; names[i] belongs to canonical[i].
struct SampleList {
    std::vector<uint64_t> canonical;                          // in order of first appearance
    std::vector<std::string> names;
    std::vector<std::pair<uint64_t, uint64_t>> rotations;     // (observed, canonical)
    uint32_t barcode_len = 0;
    size_t sample_of(uint64_t canon) const { return (size_t)(std::find(canonical.begin(), canonical.end(), canon) - canonical.begin()); }
};
inline bool gpl_pack_whole(const std::string& seq, uint64_t& v) {   // the whole sequence as one k-mer (BitNuclKmer::new(seq, len, false).next())
    if (seq.empty() || seq.size() > 32) return false;
    v = 0;
    for (unsigned char ch : seq) {
        const int c = gpl_base_code(ch);
        if (c < 0) return false;
        v = (v << 2) | (uint64_t)c;
    }
    return true;
}
inline int parse_sample_list(const std::string& text, bool reverse, SampleList& out, std::string& err) {
    auto is_ws = [](char ch) { return ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n' || ch == '\v' || ch == '\f'; };
    auto rc = [](const std::string& s) {
        std::string o(s.rbegin(), s.rend());
        for (char& ch : o) switch (ch) { case 'A': ch = 'T'; break; case 'T': ch = 'A'; break; case 'C': ch = 'G'; break; case 'G': ch = 'C'; break;
                                         case 'a': ch = 't'; break; case 't': ch = 'a'; break; case 'c': ch = 'g'; break; case 'g': ch = 'c'; break; default: break; }
        return o;
    };
    std::vector<std::pair<uint64_t, uint64_t>>& rot = out.rotations;   // kept sorted by observed
    size_t len = 0;
    bool have_len = false;
    for (size_t p = 0; p < text.size();) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        size_t a = p, b = e;
        while (a < b && is_ws(text[a])) ++a;
        while (b > a && is_ws(text[b - 1])) --b;
        p = e + 1;
        if (a == b || text[a] == '#') continue;
        std::vector<std::string> parts;
        for (size_t q = a;;) { size_t t = text.find('\t', q); if (t == std::string::npos || t >= b) { parts.push_back(text.substr(q, b - q)); break; } parts.push_back(text.substr(q, t - q)); q = t + 1; }
        std::string obs = parts[0], canon = parts.size() >= 3 ? parts[1] : parts[0], name = parts.size() >= 3 ? parts[2] : parts.size() == 2 ? parts[1] : parts[0];
        if (obs.size() != canon.size()) return gfail(err, AFQ_ERR_BAD_INPUT, "sample barcode '" + obs + "' and its canonical barcode '" + canon + "' have different lengths");
        if (obs.size() < 1 || obs.size() > 32) return gfail(err, AFQ_ERR_BAD_INPUT, "sample barcode length " + std::to_string(obs.size()) + " is unsupported; expected 1 through 32 bases");
        if (have_len && len != obs.size()) return gfail(err, AFQ_ERR_BAD_INPUT, "sample barcode file mixes lengths " + std::to_string(len) + " and " + std::to_string(obs.size()));
        len = obs.size(); have_len = true;
        if (reverse) { obs = rc(obs); canon = rc(canon); }
        uint64_t po = 0, pc = 0;
        if (!gpl_pack_whole(obs, po)) return gfail(err, AFQ_ERR_BAD_INPUT, "couldn't pack sample barcode: " + obs);
        if (!gpl_pack_whole(canon, pc)) return gfail(err, AFQ_ERR_BAD_INPUT, "couldn't pack sample barcode: " + canon);
        auto it = std::lower_bound(rot.begin(), rot.end(), std::make_pair(po, (uint64_t)0));
        if (it != rot.end() && it->first == po) {
            if (it->second != pc) return gfail(err, AFQ_ERR_BAD_INPUT, "sample construction barcode '" + obs + "' is assigned to conflicting canonical barcodes");
        } else rot.insert(it, {po, pc});
        const size_t si = out.sample_of(pc);
        if (si < out.canonical.size()) {
            if (out.names[si] != name)
                return gfail(err, AFQ_ERR_BAD_INPUT, "canonical sample barcode '" + canon + "' is assigned conflicting names '" + out.names[si] + "' and '" + name + "'");
        } else { out.canonical.push_back(pc); out.names.push_back(name); }
    }
    if (!have_len) return gfail(err, AFQ_ERR_BAD_INPUT, "sample barcode list contains no barcodes");
    out.barcode_len = (uint32_t)len;
    return 0;
}

// for_each_inverse_shift_candidate (barcode_correction.rs:787-817): the sources that would generate `obs` (repeats and obs itself included)
inline void gpl_push_inverse_shift(uint64_t obs, uint32_t L, std::vector<uint64_t>& out) {
    for (uint32_t b = 1; b < L; ++b) {
        const uint64_t lower_mask = gpl_base_mask(b), low_wo = gpl_base_mask(b - 1);
        const uint64_t ins_fixed = (obs & ~lower_mask) | ((obs & low_wo) << 2);
        for (uint64_t t = 0; t < 4; ++t) out.push_back(ins_fixed | t);
        const uint64_t del_fixed = (obs & ~gpl_base_mask(b + 1)) | ((obs >> 2) & low_wo), ob = (obs >> (2 * b)) & 3;
        for (uint64_t lo = 0; lo < 4; ++lo)
            for (uint64_t up = 0; up < 4; ++up)
                if ((lo | up) == ob) out.push_back(del_fixed | (lo << (2 * (b - 1))) | (up << (2 * b)));
    }
}
// CorrectionIndex over sources that differ from their targets (barcode_correction.rs:349-719), for the sample map: a few thousand
// sources at most, on the host.  (k_gpl_correct, the cell side, assumes identity targets.)
struct SampleSource { uint64_t source, target, count; };
enum { kSampleExact = 0, kSampleCorrected = 1, kSampleAmbiguous = 2, kSampleNotFound = 3 };
struct SampleIndex {
    uint32_t L = 0; bool shift = false, frequency = false;
    uint64_t conf_num = 39, conf_den = 40, pseudocount = 1;
    std::vector<SampleSource> src;   // ascending by source, distinct
    const SampleSource* find(uint64_t b) const {
        auto it = std::lower_bound(src.begin(), src.end(), b, [](const SampleSource& s, uint64_t v) { return s.source < v; });
        return it != src.end() && it->source == b ? &*it : nullptr;
    }
    void candidates(uint64_t obs, std::vector<const SampleSource*>& out) const {   // candidate_sources: every retained source once
        std::vector<uint64_t> c;
        gpl_push_substitutions(obs, L, c);
        if (shift) gpl_push_inverse_shift(obs, L, c);
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        out.clear();
        for (uint64_t b : c) if (const SampleSource* s = find(b)) out.push_back(s);
    }
    uint32_t structural(uint64_t obs, uint64_t& target) const {   // structural_resolution: exact, else unique_neighbor_target
        if (const SampleSource* s = find(obs)) { target = s->target; return kSampleExact; }
        std::vector<const SampleSource*> c;
        candidates(obs, c);
        if (c.empty()) return kSampleNotFound;
        for (const SampleSource* s : c) if (s->target != c[0]->target) return kSampleAmbiguous;
        target = c[0]->target;
        return kSampleCorrected;
    }
    uint32_t resolve(uint64_t obs, uint64_t& target) const {   // resolve (barcode_correction.rs:427-474)
        if (!frequency) return structural(obs, target);
        if (const SampleSource* s = find(obs)) { target = s->target; return kSampleExact; }
        std::vector<const SampleSource*> c;
        candidates(obs, c);
        if (c.empty()) return kSampleNotFound;
        std::vector<std::pair<uint64_t, unsigned __int128>> w;   // (target, weight): a target's aliases sum
        unsigned __int128 total = 0;
        for (const SampleSource* s : c) {
            const unsigned __int128 add = (unsigned __int128)s->count + pseudocount;
            total += add;
            auto it = std::find_if(w.begin(), w.end(), [&](const std::pair<uint64_t, unsigned __int128>& x) { return x.first == s->target; });
            if (it == w.end()) w.push_back({s->target, add}); else it->second += add;
        }
        size_t best = 0;   // the greatest (weight, target)
        for (size_t i = 1; i < w.size(); ++i) if (w[i].second > w[best].second || (w[i].second == w[best].second && w[i].first > w[best].first)) best = i;
        // winner / total >= num / den  <=>  winner * den >= num * total (weights sum below 2^64 here - the callers' counts are read counts - so both products fit 128 bits)
        if (w[best].second * conf_den >= (unsigned __int128)conf_num * total) { target = w[best].first; return kSampleCorrected; }
        return kSampleAmbiguous;
    }
    std::vector<uint64_t> theoretical() const {   // theoretical_observations: every source and everything it generates
        std::vector<uint64_t> o;
        for (const SampleSource& s : src) { o.push_back(s.source); gpl_push_neighbors(s.source, L, shift, o); }
        std::sort(o.begin(), o.end());
        o.erase(std::unique(o.begin(), o.end()), o.end());
        return o;
    }
};

// build_sample_permit_map (cellfilter.rs:1581-1666): what the record pass routes by.  entry ascends; kind 0 = an exact source,
// 1 = a structurally unique neighbour, 2 = deferred (structurally ambiguous, sample frequency only; target 0).
struct SampleRouting { std::vector<uint64_t> entry, target; std::vector<uint8_t> kind; };
inline SampleIndex sample_index(const SampleList& sl, uint32_t sample_correction, uint32_t sample_neighborhood) {
    SampleIndex ix;
    ix.L = sl.barcode_len;
    ix.shift = sample_correction == AFQ_GPL_SAMPLE_ONE_EDIT || (sample_correction != AFQ_GPL_SAMPLE_EXACT && sample_neighborhood == 1);
    ix.frequency = sample_correction == AFQ_GPL_SAMPLE_FREQUENCY;
    for (const auto& r : sl.rotations) ix.src.push_back(SampleSource{r.first, r.second, 0});
    return ix;
}
inline void build_sample_routing(const SampleList& sl, uint32_t sample_correction, uint32_t sample_neighborhood, SampleRouting& out) {
    out = SampleRouting{};
    if (sample_correction == AFQ_GPL_SAMPLE_EXACT) {
        for (const auto& r : sl.rotations) { out.entry.push_back(r.first); out.target.push_back(r.second); out.kind.push_back(0); }
        return;
    }
    const SampleIndex ix = sample_index(sl, sample_correction, sample_neighborhood);
    for (uint64_t b : ix.theoretical()) {
        uint64_t t = 0;
        const uint32_t d = ix.structural(b, t);
        if (d == kSampleExact || d == kSampleCorrected) { out.entry.push_back(b); out.target.push_back(t); out.kind.push_back(d == kSampleExact ? 0 : 1); }
        else if (d == kSampleAmbiguous && ix.frequency) { out.entry.push_back(b); out.target.push_back(0); out.kind.push_back(2); }
    }
}

}  // namespace gplhost
}  // namespace afq
