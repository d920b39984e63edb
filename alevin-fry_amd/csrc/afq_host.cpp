// afq_host.cpp — host side around the quant hot path (include/afquant_host.h): collated-RAD front-end
// (prelude, chunk table, snappy frame format), transcript-to-gene map, and the output writers.
//
// Mirrors, around the per-cell loop that lives on the device (paths relative to /root/reference):
//   quantify / do_quantify_dispatch      src/quant.rs:359-396, 1955-2029   (collate.json, .rad vs .rad.sz)
//   prelude + file tags                  witnessed by src/convert.rs:254-398 (writer side)
//   parse_tg_map                         src/utils.rs:487-662
//   --quant-subset filter                src/quant.rs:1523-1536, 1773-1784; src/utils.rs:1074-1095
//   per-cell stats + featureDump row     src/quant.rs:1150-1262
//   cols / rows / mtx / quant.json       src/quant.rs:1596-1613, 1786-1847, 1913-1933
//   worker fan-out                       src/quant.rs:1553-1575, 1678-1765 -> one afq_ctx + host thread per device (--devices),
//                                        byte-balanced contiguous cell ranges, rows gathered in cell order
//   multi-barcode (10x Flex) records     src/quant.rs:1354-1373, 2003-2027, 1217-1262
//   -d / -b outputs                      src/quant.rs:229-355, 1850-1877
#include <sched.h>
#include <algorithm>
#include <atomic>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>
#include <memory>
#include <mutex>
#include <string>
#include <chrono>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <cerrno>
#include <map>
#include <unordered_map>
#include <zlib.h>
#include <unordered_set>
#include <vector>

#include "../../include/afquant.h"
#include "../../include/afquant_host.h"
#include "afq_bgzf_plan.h"
#include "afq_gpl_host.h"
#include "afq_hooks.h"
#include "afq_snappy_plan.h"

namespace {

thread_local std::string g_herr;
int hfail(int code, const std::string& m) { g_herr = m; return code; }

// ---------------------------------------------------------------------------
// Rust `{}` for f32: shortest digits that round-trip, positional notation, "NaN" / "inf" / "-inf".
int format_f32(float v, char* buf, size_t cap) {
    if (cap < 64) return -1;
    if (std::isnan(v)) { std::memcpy(buf, "NaN", 4); return 3; }
    if (std::isinf(v)) { const char* s = v < 0 ? "-inf" : "inf"; size_t n = std::strlen(s); std::memcpy(buf, s, n + 1); return (int)n; }
    if (v >= 0.0f && v < 16777216.0f && v == (float)(uint32_t)v && !(v == 0.0f && std::signbit(v))) {  // whole counts: the common case
        char tmp[12]; int k = 0; uint32_t u = (uint32_t)v;
        do { tmp[k++] = (char)('0' + u % 10); u /= 10; } while (u);
        for (int i = 0; i < k; ++i) buf[i] = tmp[k - 1 - i];
        buf[k] = 0;
        return k;
    }
    // shortest round-trip digits come from the scientific form; Rust then lays them out positionally
    char sci[48];
    auto r = std::to_chars(sci, sci + sizeof sci - 1, v, std::chars_format::scientific);
    *r.ptr = 0;
    std::string digits; int exp10 = 0; bool neg = false;
    const char* p = sci;
    if (*p == '-') { neg = true; ++p; }
    for (; *p && *p != 'e'; ++p) if (*p != '.') digits.push_back(*p);
    if (*p == 'e') exp10 = std::atoi(p + 1);
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    std::string out;
    if (neg) out.push_back('-');
    if (digits == "0") out += "0";
    else if (exp10 >= 0) {
        const size_t int_len = (size_t)exp10 + 1;
        if (digits.size() <= int_len) { out += digits; out.append(int_len - digits.size(), '0'); }
        else { out.append(digits, 0, int_len); out.push_back('.'); out.append(digits, int_len, std::string::npos); }
    } else {
        out += "0.";
        out.append((size_t)(-exp10 - 1), '0');
        out += digits;
    }
    if (out.size() + 1 > cap) return -1;
    std::memcpy(buf, out.c_str(), out.size() + 1);
    return (int)out.size();
}

// ---------------------------------------------------------------------------
// snappy: raw block decompress + frame format (stream identifier 0xff, compressed 0x00, uncompressed 0x01,
// padding 0xfe, reserved skippable 0x80-0xfd).  CRC-32C of the uncompressed data is verified (masked).
// CRC-32C (Castagnoli), slicing-by-8
uint32_t crc32c(const uint8_t* p, size_t n) {
    static uint32_t T[8][256];
    static std::once_flag once;
    std::call_once(once, []() {
        for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1; T[0][i] = c; }
        for (uint32_t i = 0; i < 256; ++i) for (int t = 1; t < 8; ++t) T[t][i] = (T[t - 1][i] >> 8) ^ T[0][T[t - 1][i] & 0xFF];
    });
    uint32_t c = ~0u;
    while (n >= 8) {
        uint64_t w; std::memcpy(&w, p, 8);
        w ^= c;
        c = T[7][w & 0xFF] ^ T[6][(w >> 8) & 0xFF] ^ T[5][(w >> 16) & 0xFF] ^ T[4][(w >> 24) & 0xFF] ^
            T[3][(w >> 32) & 0xFF] ^ T[2][(w >> 40) & 0xFF] ^ T[1][(w >> 48) & 0xFF] ^ T[0][(w >> 56) & 0xFF];
        p += 8; n -= 8;
    }
    for (size_t i = 0; i < n; ++i) c = T[0][(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}
uint32_t mask_crc(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

// raw snappy block -> exactly ulen bytes at dst
bool snappy_raw_decompress_into(const uint8_t* in, size_t n, uint8_t* dst, uint64_t ulen) {
    uint64_t declared; size_t p;
    if (!snappy_raw_length(in, n, declared, p) || declared != ulen) return false;
    uint64_t w = 0;
    while (p < n) {
        const uint8_t tag = in[p++];
        const uint32_t type = tag & 3;
        if (type == 0) {  // literal
            size_t len = (tag >> 2) + 1;
            if (len > 60) { const size_t nb = len - 60; if (p + nb > n) return false; len = 0; for (size_t i = 0; i < nb; ++i) len |= (size_t)in[p + i] << (8 * i); len += 1; p += nb; }
            if (p + len > n || w + len > ulen) return false;
            std::memcpy(dst + w, in + p, len);
            p += len; w += len;
        } else {
            size_t len, off;
            if (type == 1) { if (p + 1 > n) return false; len = ((tag >> 2) & 7) + 4; off = ((size_t)(tag >> 5) << 8) | in[p]; p += 1; }
            else if (type == 2) { if (p + 2 > n) return false; len = (tag >> 2) + 1; off = in[p] | ((size_t)in[p + 1] << 8); p += 2; }
            else { if (p + 4 > n) return false; len = (tag >> 2) + 1; off = in[p] | ((size_t)in[p + 1] << 8) | ((size_t)in[p + 2] << 16) | ((size_t)in[p + 3] << 24); p += 4; }
            if (off == 0 || off > w || w + len > ulen) return false;
            if (off >= len) std::memcpy(dst + w, dst + w - off, len);
            else for (size_t i = 0; i < len; ++i) dst[w + i] = dst[w - off + i];  // overlaps its own output (run-length)
            w += len;
        }
    }
    return w == ulen;
}

// (the plan of a frame stream - SnappyChunk, snappy_frame_plan - is afq_snappy_plan.h's, shared with the device decoder)
bool snappy_frame_run(const uint8_t* in, const std::vector<SnappyChunk>& chunks, uint8_t* out, unsigned nthreads, std::string& err) {
    nthreads = std::max(1u, std::min<unsigned>(nthreads, 64u));
    if (chunks.size() < 64) nthreads = 1;
    std::vector<int> bad(nthreads, 0);   // 1 = corrupt block, 2 = CRC mismatch
    auto work = [&](unsigned t) {
        const size_t a = chunks.size() * t / nthreads, b = chunks.size() * (t + 1) / nthreads;
        for (size_t i = a; i < b && !bad[t]; ++i) {
            const SnappyChunk& c = chunks[i];
            if (!c.compressed) std::memcpy(out + c.out_off, in + c.in_off, c.ulen);
            else if (!snappy_raw_decompress_into(in + c.in_off, c.in_len, out + c.out_off, c.ulen)) { bad[t] = 1; break; }
            if (mask_crc(crc32c(out + c.out_off, c.ulen)) != c.crc) bad[t] = 2;
        }
    };
    if (nthreads == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nthreads; ++t) th.emplace_back(work, t);
        for (auto& x : th) x.join();
    }
    for (int b : bad) if (b) { err = b == 1 ? "corrupt snappy block" : "snappy CRC mismatch"; return false; }
    return true;
}
bool snappy_frame_decode(const uint8_t* in, size_t n, std::vector<uint8_t>& out, std::string& err, unsigned nthreads = 1) {
    std::vector<SnappyChunk> chunks;
    uint64_t total = 0;
    if (!snappy_frame_plan(in, n, chunks, total, err)) return false;
    out.resize(total);
    return snappy_frame_run(in, chunks, out.data(), nthreads, err);
}

// ---------------------------------------------------------------------------
// RAD prelude
struct Cursor {
    const uint8_t* b; size_t n, p = 0; bool ok = true;
    bool ran_out = false;   // what failed was a read past the n bytes (as opposed to bytes that are there and wrong)
    template <class T> T get() { T v{}; if (p + sizeof(T) > n) { ok = false; ran_out = true; return v; } std::memcpy(&v, b + p, sizeof(T)); p += sizeof(T); return v; }
    std::string str(size_t len) { if (p + len > n) { ok = false; ran_out = true; return {}; } std::string s((const char*)b + p, len); p += len; return s; }
};
struct TagDesc { std::string name; uint8_t type = 0, len_type = 0, elem_type = 0; };
size_t int_type_bytes(uint8_t t) { return t == 1 ? 1 : t == 2 ? 2 : t == 3 ? 4 : t == 4 ? 8 : 0; }

struct RadPrelude {
    bool is_paired = false; uint64_t ref_count = 0, num_chunks = 0;
    std::vector<std::string> ref_names;
    std::vector<TagDesc> file_tags, read_tags, aln_tags;
    std::unordered_map<std::string, uint64_t> file_tag_vals;
    size_t first_chunk = 0, num_chunks_at = 0;   // (num_chunks_at: where the u64 num_chunks stands)
    bool ran_out = false;   // parse_prelude failed because the bytes ended (a longer prefix of the file may parse), not because of what they hold
    uint32_t bc_bytes = 0, umi_bytes = 0;
    std::vector<uint32_t> ref_lengths;   // the ref_lengths file tag (an array of u32), when there is one
    bool have_ref_lengths = false;
};

bool read_tag_section(Cursor& c, std::vector<TagDesc>& tags) {
    const uint16_t nt = c.get<uint16_t>();
    for (uint16_t i = 0; i < nt && c.ok; ++i) {
        TagDesc t;
        const uint16_t nl = c.get<uint16_t>();
        t.name = c.str(nl);
        t.type = c.get<uint8_t>();
        if (t.type == 7) { t.len_type = c.get<uint8_t>(); t.elem_type = c.get<uint8_t>(); }
        tags.push_back(t);
    }
    return c.ok;
}

int parse_prelude(const uint8_t* bytes, size_t n, RadPrelude& P, bool want_names) {
    Cursor c{bytes, n};
    P.is_paired = c.get<uint8_t>() != 0;
    P.ref_count = c.get<uint64_t>();
    if (!c.ok || P.ref_count > n) { P.ran_out = true; return hfail(AFQ_ERR_BAD_INPUT, "RAD header: bad ref_count"); }   // (a count above the bytes at hand: sz_prelude holds it against the file's length)
    for (uint64_t i = 0; i < P.ref_count && c.ok; ++i) {
        const uint16_t nl = c.get<uint16_t>();
        if (want_names) P.ref_names.push_back(c.str(nl)); else { if (c.p + nl > c.n) { c.ok = false; c.ran_out = true; } c.p += nl; }
    }
    P.num_chunks_at = c.p;
    P.num_chunks = c.get<uint64_t>();
    if (!c.ok) { P.ran_out = c.ran_out; return hfail(AFQ_ERR_BAD_INPUT, "RAD header truncated"); }
    if (!read_tag_section(c, P.file_tags) || !read_tag_section(c, P.read_tags) || !read_tag_section(c, P.aln_tags)) {
        P.ran_out = c.ran_out;
        return hfail(AFQ_ERR_BAD_INPUT, "RAD tag sections truncated");
    }
    for (auto& t : P.file_tags) {  // values of the file-level tags follow, in declaration order
        uint64_t v = 0;
        switch (t.type) {
            case 0: case 1: v = c.get<uint8_t>(); break;
            case 2: v = c.get<uint16_t>(); break;
            case 3: v = c.get<uint32_t>(); break;
            case 4: v = c.get<uint64_t>(); break;
            case 5: c.get<float>(); break;
            case 6: c.get<double>(); break;
            case 7: {
                uint64_t len = 0;
                switch (t.len_type) { case 1: len = c.get<uint8_t>(); break; case 2: len = c.get<uint16_t>(); break; case 3: len = c.get<uint32_t>(); break; case 4: len = c.get<uint64_t>(); break; default: c.ok = false; }
                const size_t eb = t.elem_type == 5 ? 4 : t.elem_type == 6 ? 8 : t.elem_type == 0 ? 1 : int_type_bytes(t.elem_type);
                if (!eb) c.ok = false;
                else if (c.p + len * eb > c.n) { c.ok = false; c.ran_out = true; }
                else {
                    if (t.name == "ref_lengths" && t.elem_type == 3) { P.ref_lengths.resize((size_t)len); if (len) std::memcpy(P.ref_lengths.data(), c.b + c.p, (size_t)len * 4); P.have_ref_lengths = true; }
                    c.p += len * eb;
                }
                break;
            }
            case 8: { const uint16_t sl = c.get<uint16_t>(); c.str(sl); break; }
            default: c.ok = false;
        }
        P.file_tag_vals[t.name] = v;
    }
    if (!c.ok) { P.ran_out = c.ran_out; return hfail(AFQ_ERR_BAD_INPUT, "RAD file-tag values truncated or of unknown type"); }
    P.first_chunk = c.p;
    for (auto& t : P.read_tags) {
        if (t.name == "b") P.bc_bytes = (uint32_t)int_type_bytes(t.type);
        if (t.name == "u") P.umi_bytes = (uint32_t)int_type_bytes(t.type);
    }
    return 0;
}

// ---------------------------------------------------------------------------
bool file_exists(const std::string& p) { struct stat st; return ::stat(p.c_str(), &st) == 0; }
bool read_file(const std::string& p, std::vector<uint8_t>& out) {
    FILE* f = std::fopen(p.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END); long sz = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    out.resize((size_t)sz);
    bool ok = sz == 0 || std::fread(out.data(), 1, (size_t)sz, f) == (size_t)sz;
    std::fclose(f);
    return ok;
}
// read-only mapping of a (large) input file: the collated RAD is handed to afq_submit straight out of the page cache
struct MappedFile {
    const uint8_t* p = nullptr; size_t n = 0; int fd = -1;
    bool open(const std::string& path) {
        fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (::fstat(fd, &st) != 0) return false;
        n = (size_t)st.st_size;
        if (n == 0) return true;
        void* m = ::mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) return false;
        ::madvise(m, n, MADV_SEQUENTIAL);
        p = static_cast<const uint8_t*>(m);
        return true;
    }
    ~MappedFile() { if (p) ::munmap(const_cast<uint8_t*>(p), n); if (fd >= 0) ::close(fd); }
};
struct PhaseClock {
    bool on = std::getenv("AFQ_HOST_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char* what) {
        if (!on) return;
        auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[afquant] %-34s %8.3f s\n", what, std::chrono::duration<double>(n - t).count());
        t = n;
    }
};
// decimal digits of v into p, returns the end
inline char* put_u64(char* p, unsigned long long v) {
    char tmp[24]; int k = 0;
    do { tmp[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (k) *p++ = tmp[--k];
    return p;
}
// 0 when the directory exists afterwards
int mkdirs_checked(const std::string& p) {
    std::string cur;
    for (size_t i = 0; i <= p.size(); ++i) {
        if (i == p.size() || p[i] == '/') { if (!cur.empty()) ::mkdir(cur.c_str(), 0755); }
        if (i < p.size()) cur.push_back(p[i]);
    }
    struct stat st;
    return (::stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) ? 0 : -1;
}
std::string json_escape(const std::string& s) {
    std::string o;
    for (char ch : s) { if (ch == '"' || ch == '\\') { o.push_back('\\'); o.push_back(ch); } else if (ch == '\n') o += "\\n"; else o.push_back(ch); }
    return o;
}
std::string bc_to_string(uint64_t bc, uint32_t len) {  // needletail bitmer_to_bytes: first base = most significant pair
    std::string s(len, 'A');
    for (uint32_t i = 0; i < len; ++i) s[i] = "ACGT"[(bc >> (2 * (len - 1 - i))) & 3];
    return s;
}
bool string_to_bc(const std::string& s, uint64_t& v) {
    v = 0;
    for (char ch : s) {
        uint64_t c;
        switch (ch) { case 'A': case 'a': case 'N': case 'n': c = 0; break; case 'C': case 'c': c = 1; break; case 'G': case 'g': c = 2; break; case 'T': case 't': c = 3; break; default: return false; }
        v = (v << 2) | c;
    }
    return true;
}

struct ResolutionInfo { const char* name; const char* debug; uint32_t id; bool pars; bool em; };
const ResolutionInfo kRes[] = {
    {"trivial", "Trivial", AFQ_RES_TRIVIAL, false, false},
    {"cr-like", "CellRangerLike", AFQ_RES_CR_LIKE, false, false},
    {"cr-like-em", "CellRangerLikeEm", AFQ_RES_CR_LIKE_EM, false, true},
    {"parsimony-em", "ParsimonyEm", AFQ_RES_PARSIMONY_EM, true, true},
    {"parsimony", "Parsimony", AFQ_RES_PARSIMONY, true, false},
    {"parsimony-gene-em", "ParsimonyGeneEm", AFQ_RES_PARSIMONY_GENE_EM, true, true},
    {"parsimony-gene", "ParsimonyGene", AFQ_RES_PARSIMONY_GENE, true, false},
};

struct FileCloser { void operator()(FILE* f) const { if (f) std::fclose(f); } };
using FilePtr = std::unique_ptr<FILE, FileCloser>;
struct CtxCloser { void operator()(afq_ctx* c) const { if (c) afq_destroy(c); } };
using CtxPtr = std::unique_ptr<afq_ctx, CtxCloser>;

// The context of a file-level driver that only fills the device with rows or records (nothing is quantified: one gene, one
// row); aln_extra: the bytes of a position behind every alignment word, 0 without one.
int open_fill_ctx(uint32_t device, uint32_t aln_extra, CtxPtr& ctx) {
    afq_config cfg{};
    cfg.abi_version = AFQ_ABI_VERSION; cfg.resolution = AFQ_RES_CR_LIKE; cfg.num_genes = 1; cfg.num_rows = 1; cfg.small_thresh = 100;
    cfg.pug_exact_umi = 1; cfg.bc_bytes = 4; cfg.umi_bytes = 4;
    const uint32_t t2g0 = 0;
    afq_ctx* raw = nullptr;
    int rc = afq_create(&cfg, &t2g0, 1, (int)device, &raw);
    if (rc) return hfail(rc, afq_last_error(nullptr));
    ctx.reset(raw);
    if (aln_extra) { rc = afq_set_aln_extra_bytes(ctx.get(), aln_extra); if (rc) return hfail(rc, afq_last_error(ctx.get())); }
    return 0;
}

// ---- map.collated.rad.sz decoded on the device (sz_on_device of afq_quantify and afq_atac_deduplicate): the decoded file never
// exists on the host.  The prelude comes from as many leading frame chunks as it needs, decoded here; the rest is the device's.
// The leading data chunks of the planned stream `z`, decoded by the host decoder until parse_prelude succeeds on them: one
// chunk, then twice as many as the time before (a prelude with many reference names is longer than a chunk).  A prelude that
// does not parse with the whole file decoded is the file's fault, and its sentence is returned.  More chunks are decoded only
// where the parse ran out of bytes that the file (`total` decoded bytes) can still supply: a prelude that is wrong in the bytes
// at hand, or asks for more than the whole file holds, is refused with what has been decoded.
int sz_prelude(const uint8_t* z, const std::vector<SnappyChunk>& chunks, uint64_t total, std::vector<uint8_t>& head, RadPrelude& P, bool want_names) {
    size_t have = 0, want = 1;
    for (;;) {
        want = std::min(want, chunks.size());
        if (want > have) {
            const std::vector<SnappyChunk> sub(chunks.begin() + have, chunks.begin() + want);
            head.resize((size_t)(sub.back().out_off + sub.back().ulen));
            std::string err;
            if (!snappy_frame_run(z, sub, head.data(), 1, err)) return hfail(AFQ_ERR_BAD_INPUT, "map.collated.rad.sz: " + err);
            have = want;
        }
        RadPrelude Q;
        const int rc = parse_prelude(head.data(), head.size(), Q, want_names);
        if (!rc) { P = std::move(Q); return 0; }
        if (have == chunks.size() || !Q.ran_out || Q.ref_count > total) return rc;
        want = 2 * have;
    }
}
// The decoded stream on the device and its chunk table.  The bytes are the context's: valid while it lives and decodes nothing else.
struct SzResident {
    const uint8_t* d_rad = nullptr;   // device memory: byte x of the decoded stream lies at d_rad[x]; the first chunk is dword-aligned
    uint64_t n = 0;
    std::vector<uint64_t> chunk_off, chunk_nb, first_bc;   // first_bc: the 8 bytes at chunk + 12, the first record's barcode field
    std::vector<uint32_t> chunk_nr;
};
int sz_decode_resident(afq_ctx* ctx, const uint8_t* z, size_t zn, uint64_t first_chunk, uint32_t rec_hdr, SzResident& R, PhaseClock& pc) {
    const uint32_t shift = (uint32_t)((4 - first_chunk % 4) % 4);   // the chunks land as submit_host lands them
    uint8_t* d = nullptr;
    if (int rc = afq_snappy_frame_decode_device(ctx, z, zn, shift, 1, &d, &R.n, nullptr))
        return hfail(rc, std::string("map.collated.rad.sz: ") + afq_last_error(ctx));
    R.d_rad = d + shift;
    pc.lap("sz: upload + decode");
    uint64_t *off = nullptr, *bc = nullptr, nc = 0; uint32_t *nb = nullptr, *nr = nullptr;
    if (int rc = afq_collated_chunk_table(ctx, R.d_rad, R.n, first_chunk, rec_hdr, &off, &nb, &nr, &bc, &nc)) return hfail(rc, afq_last_error(ctx));
    R.chunk_off.assign(off, off + nc); R.chunk_nb.assign(nb, nb + nc); R.chunk_nr.assign(nr, nr + nc); R.first_bc.assign(bc, bc + nc);
    afq_free(off); afq_free(nb); afq_free(nr); afq_free(bc);
    pc.lap("sz: chunk table");
    return 0;
}

}  // namespace

extern "C" {

const char* afq_host_last_error(void) { return g_herr.c_str(); }

int afq_format_f32(float v, char* buf, size_t cap) { return format_f32(v, buf, cap); }

int64_t afq_snappy_frame_decode(const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
    std::vector<uint8_t> o; std::string err;
    if (!snappy_frame_decode(in, n, o, err, std::min(8u, std::max(1u, std::thread::hardware_concurrency())))) return hfail(AFQ_ERR_BAD_INPUT, err);
    if (out) { if (o.size() > cap) return hfail(AFQ_ERR_INVALID_ARG, "output buffer too small"); std::memcpy(out, o.data(), o.size()); }
    return (int64_t)o.size();
}

int afq_rad_parse_prelude(const uint8_t* bytes, size_t n, afq_rad_info* out) {
    if (!bytes || !out) return hfail(AFQ_ERR_INVALID_ARG, "null argument");
    RadPrelude P;
    int rc = parse_prelude(bytes, n, P, false);
    if (rc) return rc;
    out->ref_count = P.ref_count; out->num_chunks = P.num_chunks; out->first_chunk_off = P.first_chunk;
    out->is_paired = P.is_paired; out->cblen = (uint32_t)P.file_tag_vals["cblen"]; out->ulen = (uint32_t)P.file_tag_vals["ulen"];
    out->bc_bytes = P.bc_bytes; out->umi_bytes = P.umi_bytes;
    return 0;
}

// MatrixMarket as sprs::io::write_matrix_market writes a TriMatI<f32,u32> (coordinate real general, 1-based), from CSR
static bool write_mtx_file(const std::string& path, uint64_t n_rows, uint64_t n_cols, const std::vector<uint64_t>& rp,
                       const uint32_t* cols, const float* vals, size_t nz, uint32_t num_threads) {
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return false;
    char head[160];
    const int hl = std::snprintf(head, sizeof head, "%%%%MatrixMarket matrix coordinate real general\n%% written by sprs\n%llu %llu %zu\n",
                                 (unsigned long long)n_rows, (unsigned long long)n_cols, nz);
    bool ok = ::pwrite(fd, head, (size_t)hl, 0) == hl;
    // the entries are formatted by -t threads into per-slice buffers (same text as one fprintf per entry) and written by the
    // same threads at their final file offsets; a slice is a run of consecutive entries, its first row found by binary
    // search in the row pointers
    // -t defaults to every core in the reference (main.rs:303); 0 = not given.  Slices of 2^18 entries: a 40 M-entry matrix
    // keeps 160 threads busy in one round (at 2^20 it was 41 threads formatting a million entries each)
    const unsigned nth = std::max(1u, std::min(num_threads ? num_threads : std::thread::hardware_concurrency(), 256u));
    const size_t slice = 1u << 18;
    uint64_t file_off = (uint64_t)hl;
    for (size_t base = 0; base < nz && ok; base += slice * nth) {
        // (plain arrays, not strings: a string would zero-fill its 112 bytes per entry before a tenth of them is written)
        std::vector<std::unique_ptr<char[]>> bufs(nth);
        std::vector<size_t> blen(nth, 0);
        auto each = [&](const std::function<void(unsigned, size_t, size_t)>& f) {
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nth; ++t) {
                const size_t a = base + t * slice, b = std::min(nz, a + slice);
                if (a >= nz) break;
                th.emplace_back(f, t, a, b);
            }
            for (auto& x : th) x.join();
        };
        each([&](unsigned t, size_t a, size_t b) {
            bufs[t].reset(new char[(b - a) * 112]);  // 2 x <= 20 digits + an f32 in positional notation (<= 48 chars) + separators
            char* const p0 = bufs[t].get();
            char* p = p0;
            size_t row = (size_t)(std::upper_bound(rp.begin(), rp.end(), (uint64_t)a) - rp.begin()) - 1;
            for (size_t k = a; k < b; ++k) {
                while (rp[row + 1] <= k) ++row;   // skips empty rows too
                p = put_u64(p, (unsigned long long)row + 1); *p++ = ' ';
                p = put_u64(p, (unsigned long long)cols[k] + 1); *p++ = ' ';
                p += format_f32(vals[k], p, 64); *p++ = '\n';
            }
            blen[t] = (size_t)(p - p0);
        });
        std::vector<uint64_t> off(nth + 1, file_off);
        for (unsigned t = 0; t < nth; ++t) off[t + 1] = off[t] + blen[t];
        std::vector<int> bad(nth, 0);
        each([&](unsigned t, size_t, size_t) {
            for (size_t w = 0; w < blen[t];) {
                const ssize_t g = ::pwrite(fd, bufs[t].get() + w, blen[t] - w, (off_t)(off[t] + w));
                if (g <= 0) { bad[t] = 1; return; }
                w += (size_t)g;
            }
        });
        for (int x : bad) if (x) ok = false;
        file_off = off[nth];
        std::fill(blen.begin(), blen.end(), 0);
    }
    if (::close(fd) != 0) ok = false;
    return ok;
}

// `alevin-fry infer` (src/infer.rs:31-426): files in, EM per row on the device (afq_infer), files out.
int afq_infer_files(const afq_infer_opts* o) {
    if (!o || !o->count_mat || !o->eq_labels || !o->output_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    const std::string cm = o->count_mat, outd = o->output_dir;
    const size_t slash = cm.find_last_of('/');
    const std::string parent = slash == std::string::npos ? std::string(".") : cm.substr(0, slash);
    // count matrix: MatrixMarket coordinate, `real` (what quant writes) or `integer` (infer.rs:61-83); rows are cells
    uint64_t n_rows = 0, n_cols = 0, nnz = 0;
    std::vector<std::pair<uint64_t, std::pair<uint32_t, uint32_t>>> trip;   // (row, (class, rounded count))
    {
        std::ifstream f(cm);
        if (!f) return hfail(AFQ_ERR_BAD_INPUT, "cannot open " + cm);
        std::string line;
        if (!std::getline(f, line) || line.compare(0, 14, "%%MatrixMarket") != 0) return hfail(AFQ_ERR_BAD_INPUT, "error reading mtx format matrix : no MatrixMarket banner");
        std::string low = line;
        for (auto& ch : low) ch = (char)std::tolower((unsigned char)ch);
        if (low.find("coordinate") == std::string::npos || (low.find("real") == std::string::npos && low.find("integer") == std::string::npos) ||
            low.find("general") == std::string::npos)
            return hfail(AFQ_ERR_BAD_INPUT, "error reading mtx format matrix : only `coordinate real|integer general` is read");
        while (std::getline(f, line)) if (!line.empty() && line[0] != '%') break;
        if (std::sscanf(line.c_str(), "%llu %llu %llu", (unsigned long long*)&n_rows, (unsigned long long*)&n_cols, (unsigned long long*)&nnz) != 3)
            return hfail(AFQ_ERR_BAD_INPUT, "error reading mtx format matrix : bad size line");
        trip.reserve(nnz);
        unsigned long long r, c2; double v;
        for (uint64_t k = 0; k < nnz; ++k) {
            if (!std::getline(f, line) || std::sscanf(line.c_str(), "%llu %llu %lf", &r, &c2, &v) != 3 || r < 1 || r > n_rows || c2 < 1 || c2 > n_cols)
                return hfail(AFQ_ERR_BAD_INPUT, "error reading mtx format matrix : bad entry");
            trip.push_back({r - 1, {(uint32_t)(c2 - 1), (uint32_t)std::llround((float)v)}});   // e.1.round() as u32, infer.rs:389
        }
    }
    std::stable_sort(trip.begin(), trip.end(), [](const auto& a, const auto& b) { return a.first != b.first ? a.first < b.first : a.second.first < b.second.first; });
    // global classes (IndexedEqList::init_from_eqc_file, eq_class.rs:249-298)
    uint64_t num_genes = 0, num_eqc = 0;
    std::vector<std::vector<uint32_t>> eq;
    {
        gzFile gz = gzopen(o->eq_labels, "rb");
        if (!gz) return hfail(AFQ_ERR_BAD_INPUT, std::string("cannot open ") + o->eq_labels);
        std::string txt;
        char buf[1 << 16];
        int got;
        while ((got = gzread(gz, buf, sizeof buf)) > 0) txt.append(buf, (size_t)got);
        gzclose(gz);
        std::istringstream is(txt);
        std::string line;
        if (!std::getline(is, line)) return hfail(AFQ_ERR_BAD_INPUT, "empty equivalence class file");
        num_genes = std::strtoull(line.c_str(), nullptr, 10);
        if (!std::getline(is, line)) return hfail(AFQ_ERR_BAD_INPUT, "truncated equivalence class file");
        num_eqc = std::strtoull(line.c_str(), nullptr, 10);
        eq.assign((size_t)num_eqc, {});
        while (std::getline(is, line)) {
            std::istringstream ls(line);
            std::vector<uint32_t> v;
            unsigned long long x;
            while (ls >> x) v.push_back((uint32_t)x);
            if (v.empty()) continue;
            const uint32_t id = v.back();
            v.pop_back();
            if (id >= num_eqc) return hfail(AFQ_ERR_BAD_INPUT, "equivalence class id out of range");
            eq[id] = std::move(v);
        }
    }
    if (n_cols > num_eqc) return hfail(AFQ_ERR_BAD_INPUT, "the count matrix has more columns than there are equivalence classes");
    // barcodes of the rows, optional subset (infer.rs:113-147, 360-373)
    std::vector<std::string> bcs;
    {
        std::ifstream f(parent + "/quants_mat_rows.txt");
        if (!f) return hfail(AFQ_ERR_BAD_INPUT, "Unable to read first barcode from " + parent + "/quants_mat_rows.txt");
        std::string line;
        while (std::getline(f, line)) { while (!line.empty() && std::isspace((unsigned char)line.back())) line.pop_back(); if (!line.empty()) bcs.push_back(line); }
    }
    std::unordered_set<std::string> keep;
    const bool filter = o->filter_list != nullptr;
    if (filter) {
        std::ifstream f(o->filter_list);
        if (!f) return hfail(AFQ_ERR_BAD_INPUT, std::string("cannot open ") + o->filter_list);
        std::string line;
        while (std::getline(f, line)) { while (!line.empty() && std::isspace((unsigned char)line.back())) line.pop_back(); if (!line.empty()) keep.insert(line); }
    }
    std::vector<uint32_t> lab, ce, cc;
    std::vector<uint64_t> lp(1, 0), cp(1, 0);
    for (auto& v : eq) { lab.insert(lab.end(), v.begin(), v.end()); lp.push_back(lab.size()); }
    if (mkdir(outd.c_str(), 0777) != 0 && errno != EEXIST) return hfail(AFQ_ERR_BAD_INPUT, "cannot create " + outd);
    {
        std::ifstream in(parent + "/quants_mat_cols.txt", std::ios::binary);
        if (!in) return hfail(AFQ_ERR_BAD_INPUT, "could not copy column (gene) names to output");
        std::ofstream out(outd + "/quants_mat_cols.txt", std::ios::binary);
        out << in.rdbuf();
    }
    FILE* rows_f = std::fopen((outd + "/quants_mat_rows.txt").c_str(), "w");
    if (!rows_f) return hfail(AFQ_ERR_BAD_INPUT, "couldn't create output barcode file");
    size_t t = 0;
    uint64_t n_out = 0;
    for (uint64_t r = 0; r < n_rows && r < bcs.size(); ++r) {   // rows zip barcodes (infer.rs:364)
        const size_t t0 = t;
        while (t < trip.size() && trip[t].first == r) ++t;
        if (filter && !keep.count(bcs[r])) continue;
        std::fprintf(rows_f, "%s\n", bcs[r].c_str());
        for (size_t k = t0; k < t; ++k) {
            if (!ce.empty() && cp.back() < ce.size() && ce.back() == trip[k].second.first) { cc.back() += trip[k].second.second; continue; }   // to_csr sums duplicates
            ce.push_back(trip[k].second.first); cc.push_back(trip[k].second.second);
        }
        cp.push_back(ce.size());
        ++n_out;
    }
    std::fclose(rows_f);
    CtxPtr ctx;
    int rc = open_fill_ctx(o->device, 0, ctx);
    if (rc) return rc;
    afq_result res{};
    rc = afq_infer(ctx.get(), lab.data(), lp.data(), (uint32_t)num_eqc, cp.data(), ce.data(), cc.data(), (uint32_t)n_out, (uint32_t)num_genes, o->usa_mode, &res);
    if (rc) return hfail(rc, afq_last_error(ctx.get()));
    std::vector<uint64_t> rp(res.cell_ptr, res.cell_ptr + res.n_cells + 1);
    std::vector<uint32_t> cols(res.gene, res.gene + res.nnz);
    std::vector<float> vals(res.val, res.val + res.nnz);
    afq_result_release(&res);
    ctx.reset();
    // (num_cells, num_genes) with num_cells = the subset's size when one is given (infer.rs:141, 175-178)
    if (!write_mtx_file(outd + "/quants_mat.mtx", filter ? keep.size() : n_rows, num_genes, rp, cols.data(), vals.data(), vals.size(), o->num_threads))
        return hfail(AFQ_ERR_BAD_INPUT, "could not write quants_mat.mtx");
    return 0;
}

// ---- the device side of afq_quantify: one context (+ the -d sibling) per device over a contiguous range of cells ----
struct DevOut {   // what one device produced for its range of cells, in cell order
    int rc = 0; std::string err;
    std::vector<uint32_t> gene; std::vector<float> val; std::vector<uint64_t> row_end;   // CSR (row_end cumulative within this part)
    std::vector<uint64_t> bc; std::vector<uint32_t> nrec; std::vector<uint8_t> flags;
    std::vector<uint64_t> eq_cell_end, eq_label_end; std::vector<uint32_t> eq_labels, eq_count;   // -d
    bool have_eq = false;
    std::vector<uint64_t> bm_end, bv_end; std::vector<uint32_t> bm_col, bv_col; std::vector<float> bm_val, bv_val;   // -b
    double t_submit = 0, t_collect = 0;
    // a range that went through in ONE batch keeps the library's result (pinned, already paged in) instead of copying its
    // rows into the vectors above - 330 MB of first-touch page faults on a PBMC-sized run
    afq_result held{};
    bool is_held = false;
    DevOut() = default;
    DevOut(const DevOut&) = delete;
    DevOut& operator=(const DevOut&) = delete;
    ~DevOut() { if (is_held) afq_result_release(&held); }
};

// the collated file as afq_submit_reader sees it: pread into the library's pinned staging - the page cache is copied once, by
// several threads, without the page-fault storm that reading the same bytes through a fresh mapping sets off
struct FileSource { int fd; uint64_t base; };
static int file_read_cb(void* user, uint64_t offset, void* dst, size_t len) {
    const FileSource* f = static_cast<const FileSource*>(user);
    uint8_t* d = static_cast<uint8_t*>(dst);
    while (len) {
        const ssize_t g = ::pread(f->fd, d, len, (off_t)(f->base + offset));
        if (g <= 0) return -1;
        d += g; offset += (uint64_t)g; len -= (size_t)g;
    }
    return 0;
}

// Best effort: run the calling thread (and the staging threads it starts) on the CPUs of the NUMA node the device hangs off,
// so that the context's pinned staging is first touched there and the copies into it do not cross sockets
// (/sys/bus/pci/devices/<bus id>/numa_node, /sys/devices/system/node/node<N>/cpulist).  Silent when the topology is not exposed.
static void bind_thread_to_device_node(int device) {
    char bus[64] = {0};
    if (afq_device_pci_bus_id(device, bus, sizeof(bus)) != 0) return;
    for (char* q = bus; *q; ++q) *q = (char)std::tolower((unsigned char)*q);
    std::vector<uint8_t> f;
    if (!read_file(std::string("/sys/bus/pci/devices/") + bus + "/numa_node", f) || f.empty()) return;
    const int node = std::atoi(std::string(f.begin(), f.end()).c_str());
    if (node < 0) return;
    if (!read_file("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist", f) || f.empty()) return;
    cpu_set_t set;
    CPU_ZERO(&set);
    const std::string list(f.begin(), f.end());
    size_t i = 0;
    int n_set = 0;
    while (i < list.size()) {   // "0-63,128-191"
        char* e = nullptr;
        const long a = std::strtol(list.c_str() + i, &e, 10);
        if (e == list.c_str() + i) break;
        long b = a;
        i = (size_t)(e - list.c_str());
        if (i < list.size() && list[i] == '-') { b = std::strtol(list.c_str() + i + 1, &e, 10); i = (size_t)(e - list.c_str()); }
        for (long cpu = a; cpu <= b && cpu < CPU_SETSIZE; ++cpu) { CPU_SET((int)cpu, &set); ++n_set; }
        if (i < list.size() && list[i] == ',') ++i; else break;
    }
    if (n_set) (void)sched_setaffinity(0, sizeof(set), &set);
}

struct DevStat { double busy_s = 0; uint64_t bytes = 0, cells = 0; uint32_t batches = 0; int rc = 0; std::string err; };

// One device's host thread: its contexts, then batches of cells popped off the shared queue until it is empty - what the
// reference's workers do with chunks (quant.rs:1553-1575, 1678-1765); the rows of batch b go to parts[b], so the gather in
// batch order is the gather in cell order whatever device took which batch.
static void run_device_worker(const afq_config& cfg, const afq_config* cfg_eq, uint32_t aln_extra, const std::vector<uint32_t>& t2g, int device, bool bind_numa,
                             const uint8_t* rad, int rad_fd, const uint8_t* d_rad, const std::vector<uint64_t>& chunk_off, const std::vector<uint64_t>& chunk_nb,
                             const std::vector<uint32_t>& chunk_nr, const std::vector<std::pair<size_t, size_t>>& batches, std::atomic<size_t>& next,
                             std::atomic<int>& stop, bool want_eq, bool res_is_em, std::vector<DevOut>& parts, DevStat& stat) {
    auto now = []() { return std::chrono::steady_clock::now(); };
    auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    if (bind_numa) bind_thread_to_device_node(device);
    afq_ctx* raw = nullptr;
    int rc = afq_create(&cfg, t2g.data(), (uint32_t)t2g.size(), device, &raw);
    if (rc) { stat.rc = rc; stat.err = std::string("afq_create: ") + afq_last_error(nullptr); stop = 1; return; }
    CtxPtr ctx(raw), ctx_eq;
    if (cfg_eq) {
        rc = afq_create(cfg_eq, t2g.data(), (uint32_t)t2g.size(), device, &raw);
        if (rc) { stat.rc = rc; stat.err = std::string("afq_create: ") + afq_last_error(nullptr); stop = 1; return; }
        ctx_eq.reset(raw);
    }
    for (afq_ctx* x : {ctx.get(), ctx_eq.get()}) {   // records with positions (the pos alignment tag)
        if (!x || !aln_extra) continue;
        rc = afq_set_aln_extra_bytes(x, aln_extra);
        if (rc) { stat.rc = rc; stat.err = afq_last_error(x); stop = 1; return; }
    }
    const bool single = batches.size() == 1;
    for (;;) {
        if (stop.load()) return;
        const size_t bi = next.fetch_add(1);
        if (bi >= batches.size()) return;
        DevOut& out = parts[bi];
        const size_t c0 = batches[bi].first, c1 = batches[bi].second;
        const auto t_batch = now();
        {
        // hand over just this batch's byte span (offsets relative to it), not the whole file
        const uint64_t span0 = chunk_off[c0];
        std::vector<uint64_t> rel(c1 - c0);
        for (size_t k = c0; k < c1; ++k) rel[k - c0] = chunk_off[k] - span0;
        const uint64_t span1 = chunk_off[c1 - 1] + chunk_nb[c1 - 1];   // with --quant-subset the span also covers chunks that were filtered out
        // the decoded file lies on the device (sz_on_device): the span as it lies there, from the dword boundary below it
        const uint32_t mis = d_rad ? (uint32_t)(reinterpret_cast<uintptr_t>(d_rad + span0) & 3u) : 0u;
        if (mis) for (auto& r : rel) r += mis;
        auto ta = now();
        if (d_rad) rc = afq_submit_device(ctx.get(), d_rad + span0 - mis, (size_t)(span1 - span0) + mis, rel.data(), (uint32_t)(c1 - c0), c0);
        else if (rad_fd >= 0) {   // an uncompressed file: the library pulls the bytes itself (pread into its staging)
            FileSource fs{rad_fd, span0};
            std::vector<uint32_t> hdr(2 * (c1 - c0));
            for (size_t k = c0; k < c1; ++k) { hdr[2 * (k - c0)] = (uint32_t)chunk_nb[k]; hdr[2 * (k - c0) + 1] = chunk_nr[k]; }
            rc = afq_submit_reader(ctx.get(), file_read_cb, &fs, (size_t)(span1 - span0), rel.data(), hdr.data(), (uint32_t)(c1 - c0), c0);
        } else
            rc = afq_submit(ctx.get(), rad + span0, (size_t)(span1 - span0), rel.data(), (uint32_t)(c1 - c0), c0);
        auto tb = now();
        afq_result res{};
        if (!rc) rc = afq_collect(ctx.get(), &res);
        out.t_submit += secs(ta, tb); out.t_collect += secs(tb, now());
        if (rc) { out.rc = rc; out.err = afq_last_error(ctx.get()); stat.rc = rc; stat.err = out.err; stop = 1; return; }
        if (cfg.num_bootstraps) {   // quant.rs:1270-1277
            afq_bootstraps bs{};
            if (afq_result_bootstraps(&res, &bs) == 0) {
                const uint64_t m0 = out.bm_col.size(), v0 = out.bv_col.size();
                out.bm_col.insert(out.bm_col.end(), bs.mean_col, bs.mean_col + bs.mean_ptr[bs.n_cells]);
                out.bm_val.insert(out.bm_val.end(), bs.mean_val, bs.mean_val + bs.mean_ptr[bs.n_cells]);
                out.bv_col.insert(out.bv_col.end(), bs.var_col, bs.var_col + bs.var_ptr[bs.n_cells]);
                out.bv_val.insert(out.bv_val.end(), bs.var_val, bs.var_val + bs.var_ptr[bs.n_cells]);
                for (uint64_t i = 0; i < bs.n_cells; ++i) { out.bm_end.push_back(m0 + bs.mean_ptr[i + 1]); out.bv_end.push_back(v0 + bs.var_ptr[i + 1]); }
            }
        }
        if (want_eq) {
            afq_result res_eq{};
            afq_eqclasses ec{};
            if (ctx_eq) {
                if (d_rad) rc = afq_submit_device(ctx_eq.get(), d_rad + span0 - mis, (size_t)(span1 - span0) + mis, rel.data(), (uint32_t)(c1 - c0), c0);
                else rc = afq_submit(ctx_eq.get(), rad + span0, (size_t)(span1 - span0), rel.data(), (uint32_t)(c1 - c0), c0);
                if (!rc) rc = afq_collect(ctx_eq.get(), &res_eq);
                if (rc) { out.rc = rc; out.err = afq_last_error(ctx_eq.get()); stat.rc = rc; stat.err = out.err; stop = 1; afq_result_release(&res); return; }
            }
            const bool have = (ctx_eq || res_is_em) && afq_result_eqclasses(ctx_eq ? &res_eq : &res, &ec) == 0;
            const uint64_t k0 = out.eq_count.size(), w0 = out.eq_labels.size();
            if (have) {
                out.have_eq = true;
                out.eq_count.insert(out.eq_count.end(), ec.count, ec.count + ec.n_classes);
                out.eq_labels.insert(out.eq_labels.end(), ec.labels, ec.labels + ec.n_words);
                for (uint64_t k = 0; k < ec.n_classes; ++k) out.eq_label_end.push_back(w0 + ec.label_ptr[k + 1]);
            }
            for (uint64_t i = 0; i < res.n_cells; ++i) out.eq_cell_end.push_back(k0 + (have ? ec.cell_ptr[i + 1] : 0));
            if (ctx_eq) afq_result_release(&res_eq);
        }
        const uint64_t g0 = out.gene.size();
        const bool whole = single;   // (the one batch of a one-device run: its rows stay in the library's pinned result, no copy)
        if (!whole) {
            out.gene.insert(out.gene.end(), res.gene, res.gene + res.nnz);
            out.val.insert(out.val.end(), res.val, res.val + res.nnz);
        }
        for (uint64_t i = 0; i < res.n_cells; ++i) out.row_end.push_back(g0 + res.cell_ptr[i + 1]);
        out.bc.insert(out.bc.end(), res.bc, res.bc + res.n_cells);
        out.nrec.insert(out.nrec.end(), res.nrec, res.nrec + res.n_cells);
        out.flags.insert(out.flags.end(), res.flags, res.flags + res.n_cells);
        if (whole) { out.held = res; out.is_held = true; } else afq_result_release(&res);
        }
        stat.busy_s += secs(t_batch, now());
        stat.batches += 1; stat.cells += c1 - c0;
        for (size_t k = c0; k < c1; ++k) stat.bytes += chunk_nb[k];
    }
}

// `alevin-fry atac deduplicate` (src/atac/deduplicate.rs:68-309): collated scATAC RAD in, <input_dir>/map.bed out.  The
// record walk, the na==1 && type==4 filter, the per-cell sort and the run-length count run on the device
// (afq_atac_dedup_rad); here: the directory protocol, the prelude, and write_bed (deduplicate.rs:37-66).
int afq_atac_deduplicate(const afq_atac_dedup_opts* o) {
    if (!o || !o->input_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    const std::string in = o->input_dir;
    if (!file_exists(in + "/generate_permit_list.json") || !file_exists(in + "/collate.json"))   // atac/run.rs:149-167
        return hfail(AFQ_ERR_BAD_INPUT, "The provided input directory lacks a generate_permit_list.json or collate.json file; this should not happen.");
    std::vector<uint8_t> cj;
    if (!read_file(in + "/collate.json", cj)) return hfail(AFQ_ERR_BAD_INPUT, "could not open the collate.json file.");
    std::string cjs(cj.begin(), cj.end());
    bool compressed = false, have_flag = false;
    { size_t k = cjs.find("\"compressed_output\""); if (k != std::string::npos) { size_t v = cjs.find_first_not_of(" \t\r\n:", k + 19); have_flag = v != std::string::npos; compressed = have_flag && cjs.compare(v, 4, "true") == 0; } }
    if (!have_flag) return hfail(AFQ_ERR_BAD_INPUT, "could not read compressed_output field from collate metadata.");
    PhaseClock pc;
    MappedFile mf;
    if (!mf.open(in + (compressed ? "/map.collated.rad.sz" : "/map.collated.rad"))) return hfail(AFQ_ERR_BAD_INPUT, "could not read the collated RAD file (run collate before deduplicate)");
    std::unique_ptr<uint8_t[]> rad_buf;
    uint64_t rad_buf_n = 0;
    const unsigned nthreads = o->num_threads ? o->num_threads : std::max(1u, std::thread::hardware_concurrency());
    const bool resident = compressed && o->sz_on_device;
    if (o->sz_on_device && !compressed) std::fprintf(stderr, "--sz-on-device: map.collated.rad is not compressed; the option is ignored\n");
    std::vector<SnappyChunk> sz_chunks;
    std::vector<uint8_t> sz_head;
    if (compressed) {
        std::string err;
        if (!snappy_frame_plan(mf.p, mf.n, sz_chunks, rad_buf_n, err)) return hfail(AFQ_ERR_BAD_INPUT, "map.collated.rad.sz: " + err);
        if (!resident) {
            rad_buf.reset(new (std::nothrow) uint8_t[rad_buf_n ? rad_buf_n : 1]);
            if (!rad_buf) return hfail(AFQ_ERR_OOM, "map.collated.rad.sz: not enough host memory for the decompressed file");
            if (!snappy_frame_run(mf.p, sz_chunks, rad_buf.get(), nthreads, err)) return hfail(AFQ_ERR_BAD_INPUT, "map.collated.rad.sz: " + err);
        }
    }
    const uint8_t* rad = compressed ? rad_buf.get() : mf.p;   // (resident: null - the decoded bytes lie on the device alone)
    const size_t rad_n = compressed ? (size_t)rad_buf_n : mf.n;
    RadPrelude P;
    int rc = 0;
    if (resident) { rc = sz_prelude(mf.p, sz_chunks, rad_buf_n, sz_head, P, true); pc.lap("sz: prelude chunks"); }
    else rc = parse_prelude(rad, rad_n, P, true);
    if (rc) return rc;
    // AtacSeqReadRecord: read tag b; alignment tags ref:u32, type:u8, start_pos:u32, frag_len:u16 (tests/atac_integration.rs:110-121)
    if (P.read_tags.size() != 1 || P.read_tags[0].name != "b" || !P.bc_bytes) return hfail(AFQ_ERR_UNSUPPORTED, "scATAC RAD: the read-level tags must be exactly one integer 'b'");
    static const struct { const char* name; uint8_t type; } kAln[4] = {{"ref", 3}, {"type", 1}, {"start_pos", 3}, {"frag_len", 2}};
    bool aln_ok = P.aln_tags.size() == 4;
    for (size_t i = 0; aln_ok && i < 4; ++i) aln_ok = P.aln_tags[i].name == kAln[i].name && P.aln_tags[i].type == kAln[i].type;
    if (!aln_ok) return hfail(AFQ_ERR_UNSUPPORTED, "scATAC RAD: the alignment-level tags must be ref:u32, type:u8, start_pos:u32, frag_len:u16");
    if (!P.file_tag_vals.count("cblen")) return hfail(AFQ_ERR_BAD_INPUT, "tag map must contain cblen");
    const uint32_t cblen = (uint32_t)P.file_tag_vals["cblen"];
    std::vector<uint64_t> chunk_off;
    CtxPtr ctx;
    SzResident Z;
    if (resident) {   // decode and hop on the device; this hop asks nothing of a chunk's records
        if (int rc2 = open_fill_ctx(o->device, 0, ctx)) return rc2;
        if (int rc2 = sz_decode_resident(ctx.get(), mf.p, mf.n, P.first_chunk, 0, Z, pc)) return rc2;
        chunk_off.swap(Z.chunk_off);
    } else
    for (size_t p = P.first_chunk; p < rad_n;) {
        if (p + 8 > rad_n) return hfail(AFQ_ERR_BAD_INPUT, "trailing bytes after the last chunk");
        uint32_t nb; std::memcpy(&nb, rad + p, 4);
        if (nb < 8 || p + nb > rad_n) return hfail(AFQ_ERR_BAD_INPUT, "corrupt chunk header");
        chunk_off.push_back(p); p += nb;
    }
    pc.lap("map + prelude + chunk table");
    if (!ctx) { if (int rc2 = open_fill_ctx(o->device, 0, ctx)) return rc2; }
    uint64_t *optr = nullptr, *obc = nullptr; uint32_t *oref = nullptr, *ostart = nullptr; uint16_t *oflen = nullptr, *ocnt = nullptr;
    afq_atac_stats st{};
    const uint64_t span0 = chunk_off.empty() ? 0 : chunk_off[0];
    std::vector<uint64_t> rel(chunk_off.size());
    for (size_t i = 0; i < chunk_off.size(); ++i) rel[i] = chunk_off[i] - span0;
    rc = afq_atac_dedup_rad(ctx.get(), resident ? Z.d_rad + span0 : rad + span0, rad_n - span0, rel.data(), (uint32_t)chunk_off.size(), P.bc_bytes, resident ? 1 : 0, &optr, &obc, &oref, &ostart, &oflen, &ocnt, &st);
    if (rc) return hfail(rc, afq_last_error(ctx.get()));
    struct Freer { uint64_t* a; uint64_t* b; uint32_t* c2; uint32_t* d; uint16_t* e; uint16_t* f; ~Freer() { afq_free(a); afq_free(b); afq_free(c2); afq_free(d); afq_free(e); afq_free(f); } } fr{optr, obc, oref, ostart, oflen, ocnt};
    pc.lap("device: parse + dedup");
    // write_bed (deduplicate.rs:37-66): chr name, start, start + frag_len, barcode (reverse-complemented with -d rc), count;
    // fragments of 2000 bases and more are counted, not written.  Cells in file order (the reference: worker completion order).
    const size_t n_cells = chunk_off.size();
    const unsigned nth = (unsigned)std::max<size_t>(1, std::min<size_t>({(size_t)nthreads, 64, n_cells / 64 + 1}));
    std::vector<std::string> txt(nth);
    std::vector<int> bad(nth, 0);
    {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nth; ++t)
            th.emplace_back([&, t]() {
                std::string& out = txt[t];
                char num[32];
                for (size_t i = n_cells * t / nth; i < n_cells * (t + 1) / nth; ++i) {
                    uint64_t bc = obc[i];
                    if (o->rev) {   // needletail::bitkmer::reverse_complement
                        uint64_t r = 0;
                        for (uint32_t k = 0; k < cblen; ++k) { r = (r << 2) | (3 - (bc & 3)); bc >>= 2; }
                        bc = r;
                    }
                    const std::string bcs = bc_to_string(bc, cblen);
                    for (uint64_t k = optr[i]; k < optr[i + 1]; ++k) {
                        if (oflen[k] >= 2000) continue;
                        if (oref[k] >= P.ref_names.size()) { bad[t] = 1; return; }
                        out += P.ref_names[oref[k]]; out += '\t';
                        *put_u64(num, ostart[k]) = 0; out += num; out += '\t';
                        *put_u64(num, (unsigned long long)(uint32_t)(ostart[k] + (uint32_t)oflen[k])) = 0; out += num; out += '\t';
                        out += bcs; out += '\t';
                        *put_u64(num, ocnt[k]) = 0; out += num; out += '\n';
                    }
                }
            });
        for (auto& x : th) x.join();
    }
    for (int b2 : bad) if (b2) return hfail(AFQ_ERR_BAD_INPUT, "a fragment's reference id is beyond the RAD header's reference names");
    FilePtr bed(std::fopen((in + "/map.bed").c_str(), "w"));
    if (!bed) return hfail(AFQ_ERR_BAD_INPUT, "could not create map.bed");
    for (auto& tx : txt) if (!tx.empty() && std::fwrite(tx.data(), 1, tx.size(), bed.get()) != tx.size()) return hfail(AFQ_ERR_BAD_INPUT, "could not write map.bed");
    bed.reset();
    pc.lap("map.bed");
    std::fprintf(stderr, "finished parsing RAD file; processed %llu total records\n", (unsigned long long)st.n_records);
    std::fprintf(stderr, "Number of records with greater than 1 mapping %llu\n", (unsigned long long)st.n_multimapped);
    std::fprintf(stderr, "Number of records that are deduplicated %llu\n", (unsigned long long)st.n_deduplicated);
    std::fprintf(stderr, "Number of records that are not mapped pairs %llu\n", (unsigned long long)st.n_not_mapped_pair);
    std::fprintf(stderr, "Number of records that have frag length > 2000 %llu\n", (unsigned long long)st.n_long_fragments);
    if (o->stats_out) *o->stats_out = st;
    return 0;
}

// ---------------------------------------------------------------------------
// `alevin-fry atac sort` (src/atac/sort.rs:170-895): the mapper's map.rad in, <input_dir>/map.bed[.gz] out.
//
// correction_plan.bin (src/correction_plan.rs:20-45, 157-160): magic, u16 version, then bincode (default options: fixed-width
// little-endian integers, u64 lengths, u8 Option tags, u32 enum variants) of
//   CorrectionPlan { sample_barcode_len: Option<u8>, cell_barcode_len: u8, sample_spec: Option<CorrectionSpec>,
//                    sample_corrections: Vec<(u64, u64)>, cell_scopes: Vec<{ sample_barcode: Option<u64>, spec, corrections }> }
//   CorrectionSpec { barcode_len: u8, neighborhood: enum {HammingOne, SubstitutionOrShiftOne},
//                    resolution: enum { Unique, Frequency { confidence: {u64, u64}, pseudocount: u64 } } }   (barcode_correction.rs:28-37, 64-67, 209-227)
// A restatement of serde's derive under bincode, not a reading of bincode's source: parity unpinned.
namespace {
bool skip_correction_spec(Cursor& c) {
    c.get<uint8_t>();
    if (c.get<uint32_t>() > 1) return false;
    const uint32_t res = c.get<uint32_t>();
    if (res == 1) { c.get<uint64_t>(); c.get<uint64_t>(); c.get<uint64_t>(); }
    else if (res != 0) return false;
    return c.ok;
}
// n corrections at the cursor: counted, and the first `cap` of them written
bool take_corrections(Cursor& c, uint64_t& n, uint64_t* obs, uint64_t* cor, size_t cap, bool keep) {
    n = c.get<uint64_t>();
    if (!c.ok || n > (c.n - c.p) / 16) return false;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t o = c.get<uint64_t>(), k = c.get<uint64_t>();
        if (keep && obs && cor && i < cap) { obs[i] = o; cor[i] = k; }
    }
    return c.ok;
}
}  // namespace

int64_t afq_parse_correction_plan(const uint8_t* in, size_t n, uint64_t* observed, uint64_t* corrected, size_t cap, uint32_t* cell_barcode_len) {
    if (!in && n) return hfail(AFQ_ERR_INVALID_ARG, "null argument");
    static const uint8_t kMagic[8] = {'A', 'F', 'C', 'O', 'R', 'R', 0, 0};
    if (n < 8) return hfail(AFQ_ERR_BAD_INPUT, "correction plan has a truncated header");
    if (std::memcmp(in, kMagic, 8) != 0) return hfail(AFQ_ERR_BAD_INPUT, "correction plan has invalid magic");
    Cursor c{in, n};
    c.p = 8;
    const uint16_t ver = c.get<uint16_t>();
    if (!c.ok) return hfail(AFQ_ERR_BAD_INPUT, "correction plan has a truncated header");
    if (ver != 1) return hfail(AFQ_ERR_BAD_INPUT, "correction plan uses unsupported format version " + std::to_string(ver) + " (expected 1)");
    const char* trunc = "could not deserialize correction plan: the file is truncated or malformed";
    const uint8_t has_sample = c.get<uint8_t>();
    if (!c.ok || has_sample > 1) return hfail(AFQ_ERR_BAD_INPUT, trunc);
    if (has_sample) c.get<uint8_t>();
    const uint8_t cell_len = c.get<uint8_t>();
    const uint8_t has_sspec = c.get<uint8_t>();
    if (!c.ok || has_sspec > 1 || (has_sspec && !skip_correction_spec(c))) return hfail(AFQ_ERR_BAD_INPUT, trunc);
    uint64_t n_sample = 0, n_scopes = 0, n_global = 0;
    if (!take_corrections(c, n_sample, nullptr, nullptr, 0, false)) return hfail(AFQ_ERR_BAD_INPUT, trunc);
    n_scopes = c.get<uint64_t>();
    if (!c.ok || n_scopes > c.n) return hfail(AFQ_ERR_BAD_INPUT, trunc);
    bool have_global = false;
    for (uint64_t i = 0; i < n_scopes; ++i) {
        const uint8_t has_bc = c.get<uint8_t>();
        if (!c.ok || has_bc > 1) return hfail(AFQ_ERR_BAD_INPUT, trunc);
        if (has_bc) c.get<uint64_t>();
        if (!skip_correction_spec(c)) return hfail(AFQ_ERR_BAD_INPUT, trunc);
        uint64_t cnt = 0;
        const bool global = !has_bc && !have_global;
        if (!take_corrections(c, cnt, observed, corrected, cap, global)) return hfail(AFQ_ERR_BAD_INPUT, trunc);
        if (global) { have_global = true; n_global = cnt; }
    }
    if (c.p != c.n) return hfail(AFQ_ERR_BAD_INPUT, "correction plan contains trailing data");
    if (has_sample) return hfail(AFQ_ERR_BAD_INPUT, "correction plan does not match this ATAC input: it is sample-scoped");   // sort.rs:453-455
    if (!have_global) return hfail(AFQ_ERR_BAD_INPUT, "ATAC correction plan has no global cell scope");                         // sort.rs:456-460
    if (cell_barcode_len) *cell_barcode_len = cell_len;
    return (int64_t)n_global;
}

namespace {
// a SAMPLE-SCOPED correction plan (what multi-barcode generate-permit-list writes): the sample corrections and, per cell scope
// that names a sample, the canonical sample barcode and its corrections, in file order
struct MultiPlanScope { uint64_t sample_barcode; std::vector<uint64_t> obs, cor; };
struct MultiPlan {
    uint32_t sample_len = 0, cell_len = 0;
    std::vector<uint64_t> sample_obs, sample_cor;
    std::vector<MultiPlanScope> scopes;
};
int parse_plan_multi(const uint8_t* in, size_t n, MultiPlan& P) {
    static const uint8_t kMagic[8] = {'A', 'F', 'C', 'O', 'R', 'R', 0, 0};
    if (n < 8) return hfail(AFQ_ERR_BAD_INPUT, "correction plan has a truncated header");
    if (std::memcmp(in, kMagic, 8) != 0) return hfail(AFQ_ERR_BAD_INPUT, "correction plan has invalid magic");
    Cursor c{in, n};
    c.p = 8;
    const uint16_t ver = c.get<uint16_t>();
    if (!c.ok) return hfail(AFQ_ERR_BAD_INPUT, "correction plan has a truncated header");
    if (ver != 1) return hfail(AFQ_ERR_BAD_INPUT, "correction plan uses unsupported format version " + std::to_string(ver) + " (expected 1)");
    const char* trunc = "could not deserialize correction plan: the file is truncated or malformed";
    const uint8_t has_sample = c.get<uint8_t>();
    if (!c.ok || has_sample > 1) return hfail(AFQ_ERR_BAD_INPUT, trunc);
    if (has_sample) P.sample_len = c.get<uint8_t>();
    P.cell_len = c.get<uint8_t>();
    const uint8_t has_sspec = c.get<uint8_t>();
    if (!c.ok || has_sspec > 1 || (has_sspec && !skip_correction_spec(c))) return hfail(AFQ_ERR_BAD_INPUT, trunc);
    auto take = [&](std::vector<uint64_t>& obs, std::vector<uint64_t>& cor) {
        const size_t at = c.p;
        uint64_t cnt = 0;
        if (!take_corrections(c, cnt, nullptr, nullptr, 0, false)) return false;
        obs.resize((size_t)cnt); cor.resize((size_t)cnt);
        c.p = at;
        return take_corrections(c, cnt, obs.data(), cor.data(), (size_t)cnt, true);
    };
    if (!take(P.sample_obs, P.sample_cor)) return hfail(AFQ_ERR_BAD_INPUT, trunc);
    const uint64_t n_scopes = c.get<uint64_t>();
    if (!c.ok || n_scopes > c.n) return hfail(AFQ_ERR_BAD_INPUT, trunc);
    for (uint64_t i = 0; i < n_scopes; ++i) {
        const uint8_t has_bc = c.get<uint8_t>();
        if (!c.ok || has_bc > 1) return hfail(AFQ_ERR_BAD_INPUT, trunc);
        MultiPlanScope sc{};
        if (has_bc) sc.sample_barcode = c.get<uint64_t>();
        if (!skip_correction_spec(c) || !take(sc.obs, sc.cor)) return hfail(AFQ_ERR_BAD_INPUT, trunc);
        if (has_bc) P.scopes.push_back(std::move(sc));   // (a global scope routes nothing here: collate.rs:1766-1771)
    }
    if (c.p != c.n) return hfail(AFQ_ERR_BAD_INPUT, "correction plan contains trailing data");
    if (!has_sample) return hfail(AFQ_ERR_BAD_INPUT, "correction plan does not match this multi-barcode RAD input: it is not sample-scoped");   // collate.rs:1520-1524
    return 0;
}
}  // namespace

int64_t afq_parse_correction_plan_multi(const uint8_t* in, size_t n, uint64_t* sample_observed, uint64_t* sample_corrected, size_t sample_cap, uint64_t* n_sample,
                                        uint64_t* scope_barcode, uint64_t* scope_count, size_t scope_cap, uint64_t* n_scopes, uint64_t* cell_observed,
                                        uint64_t* cell_corrected, size_t cell_cap, uint32_t* sample_barcode_len, uint32_t* cell_barcode_len) {
    if (!in && n) return hfail(AFQ_ERR_INVALID_ARG, "null argument");
    MultiPlan P;
    if (int rc = parse_plan_multi(in, n, P)) return rc;
    for (size_t i = 0; i < P.sample_obs.size() && i < sample_cap; ++i) { if (sample_observed) sample_observed[i] = P.sample_obs[i]; if (sample_corrected) sample_corrected[i] = P.sample_cor[i]; }
    uint64_t total = 0;
    for (size_t s = 0; s < P.scopes.size(); ++s) {
        if (s < scope_cap) { if (scope_barcode) scope_barcode[s] = P.scopes[s].sample_barcode; if (scope_count) scope_count[s] = P.scopes[s].obs.size(); }
        for (size_t i = 0; i < P.scopes[s].obs.size(); ++i, ++total)
            if (total < cell_cap) { if (cell_observed) cell_observed[total] = P.scopes[s].obs[i]; if (cell_corrected) cell_corrected[total] = P.scopes[s].cor[i]; }
    }
    if (n_sample) *n_sample = P.sample_obs.size();
    if (n_scopes) *n_scopes = P.scopes.size();
    if (sample_barcode_len) *sample_barcode_len = P.sample_len;
    if (cell_barcode_len) *cell_barcode_len = P.cell_len;
    return (int64_t)total;
}

int64_t afq_parse_permit_map(const uint8_t* in, size_t n, uint64_t* observed, uint64_t* corrected, size_t cap) {
    if (!in && n) return hfail(AFQ_ERR_INVALID_ARG, "null argument");
    Cursor c{in, n};
    uint64_t cnt = 0;
    if (n < 8) return hfail(AFQ_ERR_BAD_INPUT, "couldn't deserialize legacy permit_map.bin: truncated length");
    if (!take_corrections(c, cnt, observed, corrected, cap, true)) return hfail(AFQ_ERR_BAD_INPUT, "couldn't deserialize legacy permit_map.bin: truncated entries");
    if (c.p != c.n) return hfail(AFQ_ERR_BAD_INPUT, "legacy permit_map.bin contains trailing data");
    return (int64_t)cnt;
}

namespace {
// The correction map of a GPL output directory (sort.rs:450-479, collate.rs:560-571): the plan's global scope if there is a
// correction_plan.bin - a present but malformed one is an error, and its cell barcode length must be permit_freq.bin's -, else
// the legacy permit_map.bin, with the reference's warning.
int load_corrections(const std::string& in, uint64_t bc_len, const char* mismatch, const char* legacy_for, std::vector<uint64_t>& obs, std::vector<uint64_t>& cor) {
    std::vector<uint8_t> cm;
    if (file_exists(in + "/correction_plan.bin")) {
        if (!read_file(in + "/correction_plan.bin", cm)) return hfail(AFQ_ERR_BAD_INPUT, "could not open correction plan " + in + "/correction_plan.bin");
        uint32_t cell_len = 0;
        const int64_t n = afq_parse_correction_plan(cm.data(), cm.size(), nullptr, nullptr, 0, &cell_len);
        if (n < 0) return (int)n;
        if (cell_len != bc_len) return hfail(AFQ_ERR_BAD_INPUT, mismatch);
        obs.resize((size_t)n); cor.resize((size_t)n);
        afq_parse_correction_plan(cm.data(), cm.size(), obs.data(), cor.data(), (size_t)n, nullptr);
    } else {
        std::fprintf(stderr, "No correction_plan.bin was found; loading legacy permit_map.bin for %s\n", legacy_for);
        if (!read_file(in + "/permit_map.bin", cm)) return hfail(AFQ_ERR_BAD_INPUT, "couldn't open legacy permit_map.bin file");
        const int64_t n = afq_parse_permit_map(cm.data(), cm.size(), nullptr, nullptr, 0);
        if (n < 0) return (int)n;
        obs.resize((size_t)n); cor.resize((size_t)n);
        afq_parse_permit_map(cm.data(), cm.size(), obs.data(), cor.data(), (size_t)n);
    }
    return 0;
}
// <rd>/unmapped_bc_count.bin (12-byte pairs: barcode u64, count u32) -> <in>/unmapped_bc_count_collated.bin: the counts of the
// observed barcodes summed onto their corrected barcodes (atac/collate.rs:247-283; collate.rs:431-480, the legacy layout - libradicl's self-describing one is not read).  missing_ok: no input file
// is an empty map (collate.rs:440) instead of an error.
int write_unmapped_collated(const std::string& rd, const std::string& in, const std::vector<uint64_t>& obs, const std::vector<uint64_t>& cor, bool missing_ok) {
    std::vector<uint8_t> ub;
    if (!read_file(rd + "/unmapped_bc_count.bin", ub)) {
        if (!missing_ok || file_exists(rd + "/unmapped_bc_count.bin")) return hfail(AFQ_ERR_BAD_INPUT, "could not open " + rd + "/unmapped_bc_count.bin");
        ub.clear();
    }
    std::unordered_map<uint64_t, uint64_t> cmap;
    cmap.reserve(obs.size() * 2);
    for (size_t i = 0; i < obs.size(); ++i) cmap.emplace(obs[i], cor[i]);
    std::unordered_map<uint64_t, uint32_t> cnt;
    for (size_t p = 0; p + 12 <= ub.size(); p += 12) {
        uint64_t k; uint32_t v;
        std::memcpy(&k, ub.data() + p, 8); std::memcpy(&v, ub.data() + p + 8, 4);
        auto it = cmap.find(k);
        if (it != cmap.end()) cnt[it->second] += v;
    }
    FilePtr f(std::fopen((in + "/unmapped_bc_count_collated.bin").c_str(), "wb"));
    if (!f) return hfail(AFQ_ERR_BAD_INPUT, "could not create serialization file.");
    const uint64_t n = cnt.size();
    std::fwrite(&n, 8, 1, f.get());
    for (auto& kv : cnt) { std::fwrite(&kv.first, 8, 1, f.get()); std::fwrite(&kv.second, 4, 1, f.get()); }
    return 0;
}
// The offsets of exactly num_chunks chunks of the mapper's map.rad, hopping the nbytes headers from first_chunk on.
int walk_chunk_offsets(const uint8_t* rad, size_t rad_n, size_t first_chunk, uint64_t num_chunks, std::vector<uint64_t>& chunk_off) {
    size_t p = first_chunk;
    for (uint64_t k = 0; k < num_chunks; ++k) {
        if (p + 8 > rad_n) return hfail(AFQ_ERR_BAD_INPUT, "map.rad ends before chunk " + std::to_string(k) + " of " + std::to_string(num_chunks));
        uint32_t nb; std::memcpy(&nb, rad + p, 4);
        if (nb < 8 || nb > rad_n - p) return hfail(AFQ_ERR_BAD_INPUT, "corrupt chunk header (chunk " + std::to_string(k) + ")");
        chunk_off.push_back(p); p += nb;
    }
    return 0;
}
// rel: the chunk offsets counted from span0, as the *_rad entry points take them beside `rad + span0`
void rebase_chunk_offsets(const std::vector<uint64_t>& chunk_off, uint64_t span0, std::vector<uint64_t>& rel) {
    rel.resize(chunk_off.size());
    for (size_t i = 0; i < chunk_off.size(); ++i) rel[i] = chunk_off[i] - span0;
}
// permit_freq.bin of a GPL output directory (collate.rs:236-274, atac/collate.rs:118-158): its barcode length, and the cells in the
// order (count descending, barcode ascending); *total: the sum of their counts.  bad_len: what the caller says of a file whose
// length does not match its entry count.
int read_permit_cells(const std::string& in, const char* bad_len, uint64_t& bc_len, std::vector<uint64_t>& cells, uint64_t* total = nullptr) {
    std::vector<uint8_t> pf;
    if (!read_file(in + "/permit_freq.bin", pf) || pf.size() < 24) return hfail(AFQ_ERR_BAD_INPUT, "couldn't read freq file header");
    uint64_t pf_ver, n_freq;
    std::memcpy(&pf_ver, pf.data(), 8); std::memcpy(&bc_len, pf.data() + 8, 8); std::memcpy(&n_freq, pf.data() + 16, 8);
    if (pf_ver > 1) return hfail(AFQ_ERR_BAD_INPUT, "The permit_freq.bin file had version " + std::to_string(pf_ver) + ", but this version of alevin-fry requires version 1");
    if (n_freq != (pf.size() - 24) / 16 || (pf.size() - 24) % 16) return hfail(AFQ_ERR_BAD_INPUT, bad_len);
    std::vector<std::pair<uint64_t, uint64_t>> freq(n_freq);   // (barcode, count)
    for (uint64_t i = 0; i < n_freq; ++i) {
        std::memcpy(&freq[i].first, pf.data() + 24 + 16 * i, 8); std::memcpy(&freq[i].second, pf.data() + 32 + 16 * i, 8);
        if (total) *total += freq[i].second;
    }
    std::sort(freq.begin(), freq.end(), [](const auto& a, const auto& b) { return a.second != b.second ? a.second > b.second : a.first < b.first; });   // collate.rs:270-274
    cells.resize(n_freq);
    for (uint64_t i = 0; i < n_freq; ++i) cells[i] = freq[i].first;
    return 0;
}
// map.collated.rad: the input's prelude with num_chunks = n_chunks_out (collate.rs:544-549, atac/collate.rs:896-916), then the `on`
// bytes of collated chunks; a file that could not be written whole is removed.
// With `sz_ctx` the file is map.collated.rad.sz as the reference's `collate -c` lays it out (collate.rs:523-558): the snappy frame
// stream of that prelude, encoded by the device encoder of sz_ctx, and behind it `ob`, the frame stream of the chunks as
// afq_set_collate_compress made the device hand it out - two streams back to back, each with its identifier.
int write_collated_rad(const std::string& out_path, const uint8_t* rad, const RadPrelude& P, uint64_t n_chunks_out, const uint8_t* ob, uint64_t on, afq_ctx* sz_ctx = nullptr) {
    std::vector<uint8_t> hdr(rad, rad + P.first_chunk);
    std::memcpy(hdr.data() + P.num_chunks_at, &n_chunks_out, 8);
    if (sz_ctx) {
        uint8_t* zb = nullptr; uint64_t zn = 0;
        if (int rc = afq_snappy_frame_encode(sz_ctx, hdr.data(), hdr.size(), 0, &zb, &zn, nullptr)) return hfail(rc, afq_last_error(sz_ctx));
        hdr.assign(zb, zb + zn);
        afq_free(zb);
    }
    FilePtr f(std::fopen(out_path.c_str(), "wb"));
    bool ok = (bool)f;
    if (ok) {
        ok = std::fwrite(hdr.data(), 1, hdr.size(), f.get()) == hdr.size();
        for (uint64_t off = 0; ok && off < on;) {
            const size_t len = (size_t)std::min<uint64_t>(on - off, 1ull << 30);
            ok = std::fwrite(ob + off, 1, len, f.get()) == len;
            off += len;
        }
        ok = ok && std::fflush(f.get()) == 0;
    }
    if (!ok) { f.reset(); std::remove(out_path.c_str()); return hfail(AFQ_ERR_BAD_INPUT, "could not write " + out_path); }
    return 0;
}
// collate.json (collate.rs:589-597, atac/collate.rs:337-352; collation_mode / memory_budget_bytes describe the reference's engine
// and are left out)
int write_collate_json(const std::string& in, const char* cmdline, bool compressed = false) {
    FilePtr f(std::fopen((in + "/collate.json").c_str(), "w"));
    if (!f) return hfail(AFQ_ERR_BAD_INPUT, "could not create metadata file.");
    std::fprintf(f.get(), "{\n  \"cmd\": \"%s\",\n  \"version_str\": \"0.18.0\",\n  \"compressed_output\": %s\n}", json_escape(cmdline ? cmdline : "").c_str(),
                 compressed ? "true" : "false");
    return 0;
}
// offset of the value of the TOP-LEVEL "key" of a JSON object (gpl_options repeats some names), or npos
size_t json_top_level_value(const std::string& gjs, const char* key) {
    const std::string k = key;
    int depth = 0;
    for (size_t i = 0; i < gjs.size(); ++i) {
        const char ch = gjs[i];
        if (ch == '{' || ch == '[') ++depth;
        else if (ch == '}' || ch == ']') --depth;
        else if (ch == '"') {
            size_t e = i + 1;
            while (e < gjs.size() && gjs[e] != '"') e += gjs[e] == '\\' ? 2 : 1;
            const size_t after = gjs.find_first_not_of(" \t\r\n", e + 1);
            if (depth == 1 && after != std::string::npos && gjs[after] == ':' && gjs.compare(i + 1, e - i - 1, k) == 0 && e - i - 1 == k.size())
                return gjs.find_first_not_of(" \t\r\n", after + 1);
            i = e;
        }
    }
    return std::string::npos;
}
}  // namespace

int afq_atac_sort(const afq_atac_sort_opts* o) {
    if (!o || !o->input_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    if (!o->rad_dir) return hfail(AFQ_ERR_INVALID_ARG, "the RAD directory (-r) is required");
    const std::string in = o->input_dir, rd = o->rad_dir;
    // ---- generate_permit_list.json (sort.rs:189-216, atac/collate.rs:235-245)
    std::vector<uint8_t> gj;
    if (!read_file(in + "/generate_permit_list.json", gj)) return hfail(AFQ_ERR_BAD_INPUT, "Could not open the file \"" + in + "/generate_permit_list.json\".");
    const std::string gjs(gj.begin(), gj.end());
    auto value_at = [&](const char* key, size_t from) -> size_t {   // offset of the value of "key", or npos
        const std::string k = std::string("\"") + key + "\"";
        const size_t at = gjs.find(k, from);
        if (at == std::string::npos) return at;
        return gjs.find_first_not_of(" \t\r\n:", at + k.size());
    };
    if (value_at("version_str", 0) == std::string::npos)
        return hfail(AFQ_ERR_BAD_INPUT, "The generate_permit_list.json file does not contain a version_str field. Please re-run the generate-permit-list step with a newer version of alevin-fry");
    bool rc_flag = false;
    {
        const size_t g = gjs.find("\"gpl_options\"");
        const size_t v = g == std::string::npos ? g : value_at("rc", g);
        if (v == std::string::npos || (gjs.compare(v, 4, "true") != 0 && gjs.compare(v, 5, "false") != 0)) return hfail(AFQ_ERR_BAD_INPUT, "generate_permit_list.json: gpl_options.rc must be a boolean");
        rc_flag = gjs.compare(v, 4, "true") == 0;
    }
    if (!file_exists(in + "/bin_recs.bin") || !file_exists(in + "/bin_lens.bin")) return hfail(AFQ_ERR_BAD_INPUT, "bin file containing records does not exist");
    // ---- permit_freq.bin: version, barcode length (sort.rs:234-262)
    std::vector<uint8_t> pf;
    if (!read_file(in + "/permit_freq.bin", pf) || pf.size() < 16) return hfail(AFQ_ERR_BAD_INPUT, "couldn't read freq file header");
    uint64_t pf_ver, bc_len;
    std::memcpy(&pf_ver, pf.data(), 8); std::memcpy(&bc_len, pf.data() + 8, 8);
    if (pf_ver > 1) return hfail(AFQ_ERR_BAD_INPUT, "The permit_freq.bin file had version " + std::to_string(pf_ver) + ", but this version of alevin-fry requires version 1");
    uint64_t num_chunks = 0;
    {
        const size_t v = value_at("num-chunks", 0);
        if (v == std::string::npos) return hfail(AFQ_ERR_BAD_INPUT, "num-chunks key not present");
        char* e = nullptr;
        num_chunks = std::strtoull(gjs.c_str() + v, &e, 10);
        if (e == gjs.c_str() + v) return hfail(AFQ_ERR_BAD_INPUT, "Error parsing num-chunks");
    }
    // ---- sort.json (sort.rs:342-357)
    {
        FilePtr f(std::fopen((in + "/sort.json").c_str(), "w"));
        if (!f) return hfail(AFQ_ERR_BAD_INPUT, "could not create metadata file.");
        std::fprintf(f.get(), "{\n  \"cmd\": \"%s\",\n  \"version_str\": \"0.18.0\",\n  \"compressed_output\": %s\n}", json_escape(o->cmdline ? o->cmdline : "").c_str(), o->compress ? "true" : "false");
    }
    if (!file_exists(rd)) return hfail(AFQ_ERR_BAD_INPUT, "the input RAD path \"" + rd + "\" does not exist");
    PhaseClock pc;
    std::thread warm([dev = (int)o->device]() { afq_device_warmup(dev); });
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } warm_join{warm};
    MappedFile mf;
    if (!mf.open(rd + "/map.rad")) return hfail(AFQ_ERR_BAD_INPUT, "couldn't open input RAD file");
    const uint8_t* rad = mf.p;
    const size_t rad_n = mf.n;
    RadPrelude P;
    int rc = parse_prelude(rad, rad_n, P, true);
    if (rc) return rc;
    if (P.read_tags.size() != 1 || P.read_tags[0].name != "b" || !P.bc_bytes) return hfail(AFQ_ERR_UNSUPPORTED, "scATAC RAD: the read-level tags must be exactly one integer 'b'");
    static const struct { const char* name; uint8_t type; } kAln[4] = {{"ref", 3}, {"type", 1}, {"start_pos", 3}, {"frag_len", 2}};
    bool aln_ok = P.aln_tags.size() == 4;
    for (size_t i = 0; aln_ok && i < 4; ++i) aln_ok = P.aln_tags[i].name == kAln[i].name && P.aln_tags[i].type == kAln[i].type;
    if (!aln_ok) return hfail(AFQ_ERR_UNSUPPORTED, "scATAC RAD: the alignment-level tags must be ref:u32, type:u8, start_pos:u32, frag_len:u16");
    if (!P.file_tag_vals.count("cblen")) return hfail(AFQ_ERR_BAD_INPUT, "tag map must contain cblen");
    const uint32_t cblen = (uint32_t)P.file_tag_vals["cblen"];
    if (!P.have_ref_lengths || P.ref_lengths.size() != P.ref_count) return hfail(AFQ_ERR_BAD_INPUT, "scATAC RAD: the ref_lengths file tag must be an array of u32 with one entry per reference");
    // ---- the correction map: the plan if there is one, else the legacy map (sort.rs:450-479)
    std::vector<uint64_t> obs, cor;
    if (int rc2 = load_corrections(in, bc_len, "correction plan does not match this ATAC input", "ATAC sorting", obs, cor)) return rc2;
    // ---- unmapped_bc_count.bin -> unmapped_bc_count_collated.bin (atac/collate.rs:247-283)
    if (int rc2 = write_unmapped_collated(rd, in, obs, cor, false)) return rc2;
    // ---- exactly num-chunks chunk headers (sort.rs:670)
    std::vector<uint64_t> chunk_off;
    {
        size_t p = P.first_chunk;
        for (uint64_t k = 0; k < num_chunks; ++k) {
            if (p + 8 > rad_n) return hfail(AFQ_ERR_BAD_INPUT, "map.rad ends before chunk " + std::to_string(k) + " of " + std::to_string(num_chunks));
            uint32_t nb; std::memcpy(&nb, rad + p, 4);
            if (nb < 8 || p + nb > rad_n) return hfail(AFQ_ERR_BAD_INPUT, "corrupt chunk header");
            chunk_off.push_back(p); p += nb;
        }
    }
    if (chunk_off.size() >= (1ull << 32)) return hfail(AFQ_ERR_UNSUPPORTED, "2^32 or more chunks");
    pc.lap("map + prelude + maps + chunk table");
    warm.join();
    CtxPtr ctx;
    if (int rc2 = open_fill_ctx(o->device, 0, ctx)) return rc2;
    const uint64_t span0 = chunk_off.empty() ? 0 : chunk_off[0];
    std::vector<uint64_t> rel;
    rebase_chunk_offsets(chunk_off, span0, rel);
    uint64_t n_rows = 0, *obc = nullptr; uint32_t *oref = nullptr, *ostart = nullptr, *ocnt = nullptr; uint16_t* oflen = nullptr;
    afq_atac_sort_stats st{};
    rc = afq_atac_sort_rad(ctx.get(), rad + span0, rad_n - span0, rel.data(), (uint32_t)chunk_off.size(), P.bc_bytes, 0, obs.data(), cor.data(), obs.size(),
                           P.ref_lengths.data(), (uint32_t)P.ref_count, &n_rows, &oref, &ostart, &oflen, &obc, &ocnt, &st);
    if (rc) return hfail(rc, afq_last_error(ctx.get()));
    struct Freer { void *a, *b, *c2, *d, *e; ~Freer() { afq_free(a); afq_free(b); afq_free(c2); afq_free(d); afq_free(e); } } fr{oref, ostart, oflen, obc, ocnt};
    pc.lap("device: parse + sort");
    // ---- write_bed_string (sort.rs:66-88), the rows cut over the threads
    const unsigned nthreads = std::max(2u, o->num_threads ? o->num_threads : std::min(16u, std::thread::hardware_concurrency()));   // main.rs:856, 934
    const unsigned nth = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)nthreads, 64, n_rows / 65536 + 1}));
    std::vector<std::string> txt(nth);
    std::vector<int> bad(nth, 0);
    {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nth; ++t)
            th.emplace_back([&, t]() {
                std::string& out = txt[t];
                char num[32];
                for (uint64_t k = n_rows * t / nth; k < n_rows * (t + 1) / nth; ++k) {
                    if (oflen[k] >= 2000) continue;
                    if (oref[k] >= P.ref_names.size()) { bad[t] = 1; return; }
                    uint64_t bc = obc[k];
                    if (rc_flag) {   // needletail::bitkmer::reverse_complement
                        uint64_t r = 0;
                        for (uint32_t q = 0; q < cblen; ++q) { r = (r << 2) | (3 - (bc & 3)); bc >>= 2; }
                        bc = r;
                    }
                    out += P.ref_names[oref[k]]; out += '\t';
                    *put_u64(num, ostart[k]) = 0; out += num; out += '\t';
                    *put_u64(num, (unsigned long long)(uint32_t)(ostart[k] + (uint32_t)oflen[k])) = 0; out += num; out += '\t';
                    out += bc_to_string(bc, cblen); out += '\t';
                    *put_u64(num, ocnt[k]) = 0; out += num; out += '\n';
                }
            });
        for (auto& x : th) x.join();
    }
    for (int b2 : bad) if (b2) return hfail(AFQ_ERR_BAD_INPUT, "a fragment's reference id is beyond the RAD header's reference names");
    if (o->compress) {   // sort.rs:852-854
        gzFile gz = gzopen((in + "/map.bed.gz").c_str(), "wb");
        if (!gz) return hfail(AFQ_ERR_BAD_INPUT, "could not create map.bed.gz");
        for (auto& tx : txt)
            for (size_t off = 0; off < tx.size();) {
                const unsigned len = (unsigned)std::min<size_t>(tx.size() - off, 1u << 30);
                if (gzwrite(gz, tx.data() + off, len) <= 0) { gzclose(gz); return hfail(AFQ_ERR_BAD_INPUT, "could not write map.bed.gz"); }
                off += len;
            }
        if (gzclose(gz) != Z_OK) return hfail(AFQ_ERR_BAD_INPUT, "could not write map.bed.gz");
    } else {
        FilePtr bed(std::fopen((in + "/map.bed").c_str(), "w"));
        if (!bed) return hfail(AFQ_ERR_BAD_INPUT, "could not create map.bed");
        for (auto& tx : txt) if (!tx.empty() && std::fwrite(tx.data(), 1, tx.size(), bed.get()) != tx.size()) return hfail(AFQ_ERR_BAD_INPUT, "could not write map.bed");
    }
    pc.lap("map.bed");
    std::fprintf(stderr, "deserialized correction map of length : %llu\n", (unsigned long long)obs.size());
    std::fprintf(stderr, "finished parsing RAD file; processed %llu total records\n", (unsigned long long)st.n_records);
    std::fprintf(stderr, "Number of records without a mapping %llu\n", (unsigned long long)st.n_unmapped);
    std::fprintf(stderr, "Number of records with greater than 1 mapping %llu\n", (unsigned long long)st.n_multimapped);
    std::fprintf(stderr, "Number of records whose barcode is not in the correction map %llu\n", (unsigned long long)st.n_uncorrected);
    std::fprintf(stderr, "Number of fragments sorted %llu\n", (unsigned long long)st.n_kept);
    std::fprintf(stderr, "Number of rows (distinct fragments) %llu\n", (unsigned long long)st.n_distinct);
    std::fprintf(stderr, "Number of distinct fragments that have frag length >= 2000 %llu\n", (unsigned long long)st.n_long_fragments);
    std::fprintf(stderr, "Number of position bins that were partitioned again %llu\n", (unsigned long long)st.n_repartitioned_bins);
    if (o->stats_out) *o->stats_out = st;
    return 0;
}

// `collate` (src/collate.rs:129-289, 483-643): map.collated.rad with exactly one chunk per cell of permit_freq.bin, in the order
// (count descending, barcode ascending), every record barcode-corrected and cut to the alignments that fit expected_ori.
// The command has two doors: afq_collate, which still answers opts.compress with its refusal (the tests that pin it are not this
// change's to touch), and afq_collate_sz, which writes map.collated.rad.sz (`sz`) and ignores the field.
static int collate_run(const afq_collate_opts* o, bool sz);
int afq_collate(const afq_collate_opts* o) {
    if (!o || !o->input_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    if (!o->rad_dir) return hfail(AFQ_ERR_INVALID_ARG, "the RAD directory (-r) is required");
    if (o->compress) return hfail(AFQ_ERR_UNSUPPORTED, "compressed output is not supported");
    return collate_run(o, false);
}
int afq_collate_sz(const afq_collate_opts* o) {
    if (!o || !o->input_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    if (!o->rad_dir) return hfail(AFQ_ERR_INVALID_ARG, "the RAD directory (-r) is required");
    return collate_run(o, true);
}
static int collate_run(const afq_collate_opts* o, bool sz) {
    const std::string in = o->input_dir, rd = o->rad_dir;
    // ---- generate_permit_list.json (collate.rs:155-200, 513-520)
    std::vector<uint8_t> gj;
    if (!read_file(in + "/generate_permit_list.json", gj)) return hfail(AFQ_ERR_BAD_INPUT, "could not open generate_permit_list.json in \"" + in + "\"");
    const std::string gjs(gj.begin(), gj.end());
    auto value_at = [&](const char* key) { return json_top_level_value(gjs, key); };
    auto is_true = [&](size_t v) { return v != std::string::npos && gjs.compare(v, 4, "true") == 0; };
    if (value_at("version_str") == std::string::npos)
        return hfail(AFQ_ERR_BAD_INPUT, "The generate_permit_list.json file does not contain a version_str field. Please re-run the generate-permit-list step with a newer version of alevin-fry");
    if (is_true(value_at("multi_barcode"))) return hfail(AFQ_ERR_UNSUPPORTED, "collate: multi-barcode permit lists (multi_barcode: true) are not supported; use afq_collate_multi");
    if (is_true(value_at("velo_mode"))) return hfail(AFQ_ERR_UNSUPPORTED, "collate: velo_mode: true is not supported");
    uint32_t expected_ori = 0;
    {
        const size_t v = value_at("expected_ori");
        static const char* const kSym[3] = {"\"both\"", "\"fw\"", "\"rc\""};   // (the symbols generate-permit-list writes; `either` is written as both)
        uint32_t k = 0;
        while (k < 3 && (v == std::string::npos || gjs.compare(v, std::strlen(kSym[k]), kSym[k]) != 0)) ++k;
        if (k == 3) return hfail(AFQ_ERR_BAD_INPUT, "could not read strand: generate_permit_list.json: expected_ori must be \"both\", \"fw\" or \"rc\"");
        expected_ori = k;
    }
    // ---- permit_freq.bin: the cells and their order (collate.rs:236-274)
    std::vector<uint64_t> cells;
    uint64_t bc_len = 0, total_to_collate = 0;
    if (int rc2 = read_permit_cells(in, "couldn't deserialize permit_freq.bin: its length does not match its entry count", bc_len, cells, &total_to_collate)) return rc2;
    if (cells.empty()) return hfail(AFQ_ERR_BAD_INPUT, "single-barcode permit list contains no output cells");
    // ---- the correction map, the unmapped counts
    std::vector<uint64_t> obs, cor;
    if (int rc2 = load_corrections(in, bc_len, "correction plan does not match this input: its cell barcode length is not permit_freq.bin's", "collation", obs, cor)) return rc2;
    if (int rc2 = write_unmapped_collated(rd, in, obs, cor, true)) return rc2;
    // ---- map.rad
    if (!file_exists(rd)) return hfail(AFQ_ERR_BAD_INPUT, "the input RAD path \"" + rd + "\" does not exist");
    PhaseClock pc;
    MappedFile mf;
    if (!mf.open(rd + "/map.rad")) return hfail(AFQ_ERR_BAD_INPUT, "couldn't open input RAD file");
    const uint8_t* rad = mf.p;
    const size_t rad_n = mf.n;
    RadPrelude P;
    int rc = parse_prelude(rad, rad_n, P, false);
    if (rc) return rc;
    auto has_tag = [](const std::vector<TagDesc>& v, const char* name) { for (auto& t : v) if (t.name == name) return true; return false; };
    if (P.file_tag_vals.count("num_barcodes") && P.file_tag_vals["num_barcodes"] > 1)
        return hfail(AFQ_ERR_UNSUPPORTED, "collate: multi-barcode RAD files (num_barcodes > 1) are not supported; use afq_collate_multi");
    if (has_tag(P.aln_tags, "start_pos") || has_tag(P.aln_tags, "frag_len"))
        return hfail(AFQ_ERR_UNSUPPORTED, "collate: this is a scATAC RAD file; use `atac collate`");
    if (has_tag(P.aln_tags, "as") && has_tag(P.aln_tags, "start") && has_tag(P.aln_tags, "end"))
        return hfail(AFQ_ERR_UNSUPPORTED, "collate: long-read RAD records (alignment tags as, start, end) are not supported");
    if (P.read_tags.size() != 2 || P.read_tags[0].name != "b" || P.read_tags[1].name != "u" || !P.bc_bytes || !P.umi_bytes)
        return hfail(AFQ_ERR_UNSUPPORTED, "collate: the read-level tags must be the integers (b, u)");
    uint32_t aln_extra = 0;
    if (P.aln_tags.size() == 2 && P.aln_tags[1].name == "pos") aln_extra = (uint32_t)int_type_bytes(P.aln_tags[1].type);
    if (P.aln_tags.empty() || P.aln_tags[0].type != 3 || (P.aln_tags.size() == 2 && !aln_extra) || P.aln_tags.size() > 2)
        return hfail(AFQ_ERR_UNSUPPORTED, "collate: the alignment-level tags must be one u32 (ref | orientation), optionally followed by an integer pos");
    // ---- the chunk table
    std::vector<uint64_t> chunk_off;
    if (int rc2 = walk_chunk_offsets(rad, rad_n, P.first_chunk, P.num_chunks, chunk_off)) return rc2;
    if (chunk_off.size() >= (1ull << 32)) return hfail(AFQ_ERR_UNSUPPORTED, "2^32 or more chunks");
    pc.lap("metadata + maps + chunk table");
    // ---- the device: one fill
    CtxPtr ctx;
    if (int rc2 = open_fill_ctx(o->device, aln_extra, ctx)) return rc2;
    afq_set_collate_compress(ctx.get(), sz);
    const uint64_t span0 = chunk_off.empty() ? P.first_chunk : chunk_off[0];
    std::vector<uint64_t> rel;
    rebase_chunk_offsets(chunk_off, span0, rel);
    uint8_t* ob = nullptr; uint64_t on = 0, *ooff = nullptr; uint32_t* onrec = nullptr;
    afq_collate_stats st{};
    rc = afq_collate_rad(ctx.get(), rad + span0, rad_n - span0, rel.data(), (uint32_t)chunk_off.size(), P.bc_bytes, P.umi_bytes, expected_ori, 0, obs.data(), cor.data(),
                         obs.size(), cells.data(), cells.size(), &ob, &on, &ooff, &onrec, &st);
    if (rc) return hfail(rc, afq_last_error(ctx.get()));
    struct Freer { void *a, *b, *c; ~Freer() { afq_free(a); afq_free(b); afq_free(c); } } fr{ob, ooff, onrec};
    pc.lap("device: collate");
    if (o->stats_out) *o->stats_out = st;
    if (st.n_kept != total_to_collate)   // collate.rs:615 (nothing was written yet, so no RAD is left behind)
        return hfail(AFQ_ERR_BAD_INPUT, "expected to collate " + std::to_string(total_to_collate) + " records but retained " + std::to_string(st.n_kept));
    // ---- map.collated.rad: the input's prelude with num_chunks = the number of cells (collate.rs:544-549), then the chunks
    if (int rc2 = write_collated_rad(in + (sz ? "/map.collated.rad.sz" : "/map.collated.rad"), rad, P, cells.size(), ob, on, sz ? ctx.get() : nullptr)) return rc2;
    if (int rc2 = write_collate_json(in, o->cmdline, sz)) return rc2;
    pc.lap("map.collated.rad");
    std::fprintf(stderr, "deserialized correction map of length : %llu\n", (unsigned long long)obs.size());
    std::fprintf(stderr, "collated %llu of %llu records (%llu orientation consistent, %llu with a barcode that is not in the correction map) into %llu cells\n",
                 (unsigned long long)st.n_kept, (unsigned long long)st.n_records, (unsigned long long)st.n_compatible, (unsigned long long)st.n_uncorrected,
                 (unsigned long long)cells.size());
    std::fprintf(stderr, "kept %llu of %llu alignments; %llu output bytes\n", (unsigned long long)st.n_alignments_kept, (unsigned long long)st.n_alignments_in,
                 (unsigned long long)st.out_bytes);
    return 0;
}

// `atac collate` (src/atac/collate.rs, src/main.rs:905-922): map.collated.rad with one chunk per cell of permit_freq.bin that kept a
// record, in the order (count descending, barcode ascending); a record is kept iff it has one alignment and its barcode is in the
// correction map.  libradicl's filter (dump_corrected_cb_chunk_to_temp_file_atac) is not among the reference's sources: the rule is
// restated from collate.rs's own comments (:719-723, :869-892).
// (two doors, as collate: afq_atac_collate keeps its refusal of opts.compress, afq_atac_collate_sz writes map.collated.rad.sz)
static int atac_collate_run(const afq_atac_collate_opts* o, bool sz);
int afq_atac_collate(const afq_atac_collate_opts* o) {
    if (!o || !o->input_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    if (!o->rad_dir) return hfail(AFQ_ERR_INVALID_ARG, "the RAD directory (-r) is required");
    if (o->compress) return hfail(AFQ_ERR_UNSUPPORTED, "compressed output is not supported");
    return atac_collate_run(o, false);
}
int afq_atac_collate_sz(const afq_atac_collate_opts* o) {
    if (!o || !o->input_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    if (!o->rad_dir) return hfail(AFQ_ERR_INVALID_ARG, "the RAD directory (-r) is required");
    return atac_collate_run(o, true);
}
static int atac_collate_run(const afq_atac_collate_opts* o, bool sz) {
    const std::string in = o->input_dir, rd = o->rad_dir;
    // ---- generate_permit_list.json (atac/collate.rs:80-106, 235-245)
    std::vector<uint8_t> gj;
    if (!read_file(in + "/generate_permit_list.json", gj)) return hfail(AFQ_ERR_BAD_INPUT, "could not open generate_permit_list.json in \"" + in + "\"");
    const std::string gjs(gj.begin(), gj.end());
    if (json_top_level_value(gjs, "version_str") == std::string::npos)
        return hfail(AFQ_ERR_BAD_INPUT, "The generate_permit_list.json file does not contain a version_str field. Please re-run the generate-permit-list step with a newer version of alevin-fry");
    // ---- permit_freq.bin: the cells and their order (atac/collate.rs:118-158)
    std::vector<uint64_t> cells;
    uint64_t bc_len = 0;
    if (int rc2 = read_permit_cells(in, "couldn't deserialize barcode to frequency map.", bc_len, cells)) return rc2;
    uint64_t num_chunks = 0;
    {
        const size_t v = json_top_level_value(gjs, "num-chunks");
        if (v == std::string::npos) return hfail(AFQ_ERR_BAD_INPUT, "num-chunks key not present");
        char* e = nullptr;
        num_chunks = std::strtoull(gjs.c_str() + v, &e, 10);
        if (e == gjs.c_str() + v) return hfail(AFQ_ERR_BAD_INPUT, "Error parsing num-chunks");
    }
    // ---- the correction map (atac/collate.rs:453-495), the unmapped counts (a missing file is an empty map: the library aborts nowhere)
    std::vector<uint64_t> obs, cor;
    if (int rc2 = load_corrections(in, bc_len, "correction plan does not match this ATAC input", "ATAC collation", obs, cor)) return rc2;
    if (int rc2 = write_unmapped_collated(rd, in, obs, cor, true)) return rc2;
    // ---- map.rad
    if (!file_exists(rd)) return hfail(AFQ_ERR_BAD_INPUT, "the input RAD path \"" + rd + "\" does not exist");
    PhaseClock pc;
    MappedFile mf;
    if (!mf.open(rd + "/map.rad")) return hfail(AFQ_ERR_BAD_INPUT, "couldn't open input RAD file");
    const uint8_t* rad = mf.p;
    const size_t rad_n = mf.n;
    RadPrelude P;
    int rc = parse_prelude(rad, rad_n, P, false);
    if (rc) return rc;
    static const struct { const char* name; uint8_t type; } kAln[4] = {{"ref", 3}, {"type", 1}, {"start_pos", 3}, {"frag_len", 2}};
    bool atac = P.read_tags.size() == 1 && P.read_tags[0].name == "b" && P.bc_bytes && P.aln_tags.size() == 4;
    for (size_t i = 0; atac && i < 4; ++i) atac = P.aln_tags[i].name == kAln[i].name && P.aln_tags[i].type == kAln[i].type;
    if (!atac)
        return hfail(AFQ_ERR_UNSUPPORTED, "atac collate: this is not a scATAC RAD file (one integer read tag b; alignment tags ref:u32, type:u8, start_pos:u32, frag_len:u16); use `collate`");
    // ---- exactly num-chunks chunk headers
    std::vector<uint64_t> chunk_off;
    if (int rc2 = walk_chunk_offsets(rad, rad_n, P.first_chunk, num_chunks, chunk_off)) return rc2;
    if (chunk_off.size() >= (1ull << 32)) return hfail(AFQ_ERR_UNSUPPORTED, "2^32 or more chunks");
    pc.lap("metadata + maps + chunk table");
    // ---- the device: one fill
    CtxPtr ctx;
    if (int rc2 = open_fill_ctx(o->device, 0, ctx)) return rc2;
    afq_set_collate_compress(ctx.get(), sz);
    const uint64_t span0 = chunk_off.empty() ? P.first_chunk : chunk_off[0];
    std::vector<uint64_t> rel;
    rebase_chunk_offsets(chunk_off, span0, rel);
    uint8_t* ob = nullptr; uint64_t on = 0, n_out = 0, *ooff = nullptr; uint32_t *onrec = nullptr, *ocell = nullptr;
    afq_atac_collate_stats st{};
    rc = afq_atac_collate_rad(ctx.get(), rad + span0, rad_n - span0, rel.data(), (uint32_t)chunk_off.size(), P.bc_bytes, 0, obs.data(), cor.data(), obs.size(),
                              cells.data(), cells.size(), &ob, &on, &n_out, &ooff, &onrec, &ocell, &st);
    if (rc) return hfail(rc, afq_last_error(ctx.get()));
    struct Freer { void *a, *b, *c, *d; ~Freer() { afq_free(a); afq_free(b); afq_free(c); afq_free(d); } } fr{ob, ooff, onrec, ocell};
    pc.lap("device: atac collate");
    if (o->stats_out) *o->stats_out = st;
    // ---- map.collated.rad: the input's prelude with num_chunks = the chunks written (atac/collate.rs:896-916), then the chunks
    if (int rc2 = write_collated_rad(in + (sz ? "/map.collated.rad.sz" : "/map.collated.rad"), rad, P, n_out, ob, on, sz ? ctx.get() : nullptr)) return rc2;
    if (int rc2 = write_collate_json(in, o->cmdline, sz)) return rc2;
    pc.lap("map.collated.rad");
    std::fprintf(stderr, "deserialized correction map of length : %llu\n", (unsigned long long)obs.size());
    std::fprintf(stderr, "collated %llu of %llu records (%llu without a mapping, %llu with more than 1 mapping, %llu with a barcode that is not in the correction map); %llu output bytes\n",
                 (unsigned long long)st.n_kept, (unsigned long long)st.n_records, (unsigned long long)st.n_unmapped, (unsigned long long)st.n_multimapped,
                 (unsigned long long)st.n_uncorrected, (unsigned long long)st.out_bytes);
    std::fprintf(stderr, "writing num output chunks (%llu) to header\n", (unsigned long long)n_out);
    if (st.n_cells_empty)   // atac/collate.rs:884-892
        std::fprintf(stderr, "%llu of %llu retained barcodes produced no collated records (every read was unmapped or multi-mapping) and are absent from the output.\n",
                     (unsigned long long)st.n_cells_empty, (unsigned long long)cells.size());
    return 0;
}

// ---------------------------------------------------------------------------
// `convert` (bam2rad, src/convert.rs:167-594) and `view` (src/convert.rs:596-709).  The container and the BAM header are the
// host's: BGZF blocks are found by hopping BSIZE of the BC extra field, inflated on threads with zlib's raw inflate, CRC32 and
// ISIZE verified (SAM/BAM specification, sections 4.1 and 4.2: the record layout rests on that text alone).  The records are
// the device's (afq_convert_bam_rad).
namespace {
inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }

// the plan of afq_bgzf_plan.h with its refusal as this file's
int bgzf_plan(const uint8_t* in, size_t n, std::vector<BgzfBlock>& blocks, uint64_t& total) {
    std::string err;
    return ::bgzf_plan(in, n, blocks, total, err) ? 0 : hfail(AFQ_ERR_BAD_INPUT, err);
}

int bgzf_inflate(const uint8_t* in, const std::vector<BgzfBlock>& blocks, uint8_t* out, unsigned nthreads) {
    std::atomic<size_t> next{0};
    std::mutex mu;
    size_t bad_at = SIZE_MAX;
    std::string bad_msg;
    auto work = [&]() {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= blocks.size()) return;
            const BgzfBlock& b = blocks[i];
            uint8_t none = 0;
            z_stream zs{};
            std::string msg;
            if (inflateInit2(&zs, -15) != Z_OK) msg = "zlib could not be initialised";
            else {
                zs.next_in = const_cast<uint8_t*>(in + b.data_off); zs.avail_in = (uInt)b.data_len;
                zs.next_out = b.isize ? out + b.out_off : &none; zs.avail_out = b.isize ? b.isize : 1;
                const int rc = inflate(&zs, Z_FINISH);
                if (rc != Z_STREAM_END) msg = std::string("the deflate stream is corrupt or longer than ISIZE (zlib: ") + (zs.msg ? zs.msg : "no end of stream") + ")";
                else if (zs.total_out != b.isize) msg = "ISIZE says " + std::to_string(b.isize) + " bytes, the deflate stream holds " + std::to_string(zs.total_out);
                else if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), b.isize ? out + b.out_off : &none, b.isize) != b.crc) msg = "bad CRC32";
                inflateEnd(&zs);
            }
            if (!msg.empty()) { std::lock_guard<std::mutex> g(mu); if (i < bad_at) { bad_at = i; bad_msg = msg; } }
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nthreads; ++t) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    if (bad_at != SIZE_MAX) return hfail(AFQ_ERR_BAD_INPUT, "BGZF block " + std::to_string(bad_at) + ": " + bad_msg);
    return 0;
}

// the CR and UR strings of the record at the stream's start: their lengths are cblen and ulen (convert.rs:263-320)
int convert_first_lengths(const uint8_t* s, uint64_t n, uint32_t& cblen, uint32_t& ulen) {
    const std::string at = "record 0: ";
    if (n < 4) return hfail(AFQ_ERR_BAD_INPUT, at + "the stream ends inside block_size");
    const uint64_t bs = le32(s);
    if (bs > n - 4) return hfail(AFQ_ERR_BAD_INPUT, at + "block_size runs past the stream");
    const uint64_t need = bs >= 32 ? 32 + (uint64_t)s[12] + 4ull * le16(s + 16) + ((uint64_t)le32(s + 20) + 1) / 2 + le32(s + 20) : ~0ull;
    if (need > bs) return hfail(AFQ_ERR_BAD_INPUT, at + "block_size is too small for the record's fixed fields, name, CIGAR and sequence");
    const uint8_t* b = s + 4;
    int have[2] = {0, 0}; bool is_z[2] = {false, false}; uint64_t len[2] = {0, 0};
    for (uint64_t g = need; g < bs;) {
        if (bs - g < 3) return hfail(AFQ_ERR_BAD_INPUT, at + "the aux fields do not end at the record's end");
        const uint8_t t0 = b[g], t1 = b[g + 1], ty = b[g + 2];
        g += 3;
        uint64_t sz = 0, zl = 0;
        switch (ty) {
            case 'A': case 'c': case 'C': sz = 1; break;
            case 's': case 'S': sz = 2; break;
            case 'i': case 'I': case 'f': sz = 4; break;
            case 'Z': case 'H': { const uint64_t v0 = g; while (g < bs && b[g]) ++g; if (g == bs) return hfail(AFQ_ERR_BAD_INPUT, at + "an aux string without its NUL"); zl = g - v0; ++g; break; }
            case 'B': {
                if (bs - g < 5) return hfail(AFQ_ERR_BAD_INPUT, at + "the aux fields do not end at the record's end");
                const uint8_t sub = b[g];
                const uint64_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
                if (!es || (uint64_t)le32(b + g + 1) * es > bs - g - 5) return hfail(AFQ_ERR_BAD_INPUT, at + "a B array of unknown subtype or past the record's end");
                g += 5 + (uint64_t)le32(b + g + 1) * es;
                break;
            }
            default: return hfail(AFQ_ERR_BAD_INPUT, at + "an aux field of unknown type");
        }
        if (sz) { if (bs - g < sz) return hfail(AFQ_ERR_BAD_INPUT, at + "the aux fields do not end at the record's end"); g += sz; }
        const int w = (t0 == 'C' && t1 == 'R') ? 0 : (t0 == 'U' && t1 == 'R') ? 1 : -1;
        if (w >= 0 && !have[w]) { have[w] = 1; is_z[w] = ty == 'Z'; len[w] = zl; }
    }
    if (!have[0]) return hfail(AFQ_ERR_BAD_INPUT, at + "Input record missing CR tag!");
    if (!is_z[0]) return hfail(AFQ_ERR_BAD_INPUT, at + "cannot convert non-string (Z) tag into barcode string.");
    if (!have[1]) return hfail(AFQ_ERR_BAD_INPUT, at + "Input record missing UR tag!");
    if (!is_z[1]) return hfail(AFQ_ERR_BAD_INPUT, at + "cannot convert non-string (Z) tag into umi string.");
    if (len[0] < 1 || len[0] > 32) return hfail(AFQ_ERR_BAD_INPUT, at + "cannot encode barcode of length " + std::to_string(len[0]) + ": 1 to 32 bases fit");
    if (len[1] < 1 || len[1] > 32) return hfail(AFQ_ERR_BAD_INPUT, at + "cannot encode umi of length " + std::to_string(len[1]) + ": 1 to 32 bases fit");
    cblen = (uint32_t)len[0]; ulen = (uint32_t)len[1];
    return 0;
}
uint32_t convert_width(uint32_t len) { return len <= 4 ? 1 : len <= 8 ? 2 : len <= 16 ? 4 : 8; }   // convert.rs:323-343

// what convert.rs:238-370 writes in front of the chunks
void convert_prelude(const std::vector<std::string>& names, uint64_t num_chunks, uint32_t cblen, uint32_t ulen, std::vector<uint8_t>& out) {
    auto put = [&](const void* p, size_t n) { out.insert(out.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
    auto put16 = [&](uint16_t v) { put(&v, 2); };
    auto tag = [&](const char* name, uint8_t type) { put16((uint16_t)std::strlen(name)); put(name, std::strlen(name)); put(&type, 1); };
    auto int_type = [](uint32_t w) -> uint8_t { return w == 1 ? 1 : w == 2 ? 2 : w == 4 ? 3 : 4; };
    const uint8_t paired = 0;
    const uint64_t n_ref = names.size();
    put(&paired, 1); put(&n_ref, 8);
    for (auto& s : names) { put16((uint16_t)s.size()); put(s.data(), s.size()); }
    put(&num_chunks, 8);
    put16(2); tag("cblen", 2); tag("ulen", 2);
    put16(2); tag("b", int_type(convert_width(cblen))); tag("u", int_type(convert_width(ulen)));
    put16(1); tag("compressed_ori_refid", 3);
    put16((uint16_t)cblen); put16((uint16_t)ulen);
}
bool ends_with(const std::string& s, const char* e) { const size_t n = std::strlen(e); return s.size() >= n && s.compare(s.size() - n, n, e) == 0; }
}  // namespace

int64_t afq_convert_prelude_bytes(const char* const* ref_names, uint64_t n_ref, uint64_t num_chunks, uint32_t cblen, uint32_t ulen, uint8_t* out, size_t cap) {
    if ((!ref_names && n_ref) || cblen < 1 || cblen > 32 || ulen < 1 || ulen > 32) return hfail(AFQ_ERR_INVALID_ARG, "null names, or a length outside 1..32");
    std::vector<std::string> names;
    for (uint64_t i = 0; i < n_ref; ++i) names.emplace_back(ref_names[i]);
    std::vector<uint8_t> b;
    convert_prelude(names, num_chunks, cblen, ulen, b);
    if (out) { if (b.size() > cap) return hfail(AFQ_ERR_INVALID_ARG, "output buffer too small"); std::memcpy(out, b.data(), b.size()); }
    return (int64_t)b.size();
}

namespace {
// the BAM header at p[0, n): magic, l_text, text, n_ref x (l_name, name, l_ref) -> the names and where the records begin
int convert_bam_header(const uint8_t* p, size_t n, std::vector<std::string>& names, int32_t& n_ref, size_t& hdr_len) {
    names.clear();
    Cursor c{p, n};
    const uint32_t magic = c.get<uint32_t>();
    if (!c.ok || magic != 0x014d4142u) return hfail(AFQ_ERR_BAD_INPUT, "BAM header: bad magic (BAM\\1 is expected)");
    const int32_t l_text = c.get<int32_t>();
    if (!c.ok || l_text < 0 || (uint64_t)l_text > c.n - c.p) return hfail(AFQ_ERR_BAD_INPUT, "BAM header: the text runs past the file");
    c.p += (size_t)l_text;
    n_ref = c.get<int32_t>();
    if (!c.ok || n_ref < 0) return hfail(AFQ_ERR_BAD_INPUT, "BAM header: bad reference count");
    for (int32_t i = 0; i < n_ref; ++i) {
        const int32_t l_name = c.get<int32_t>();
        if (!c.ok || l_name < 1 || (uint64_t)l_name > c.n - c.p) return hfail(AFQ_ERR_BAD_INPUT, "BAM header: reference " + std::to_string(i) + ": the name runs past the file");
        std::string nm = c.str((size_t)l_name);
        nm.resize(std::strlen(nm.c_str()));   // (l_name counts the NUL)
        if (nm.size() > 0xFFFF) return hfail(AFQ_ERR_UNSUPPORTED, "BAM header: reference " + std::to_string(i) + ": a name of 64 KiB or more does not fit the RAD header");
        names.push_back(std::move(nm));
        (void)c.get<int32_t>();   // l_ref
        if (!c.ok) return hfail(AFQ_ERR_BAD_INPUT, "BAM header: reference " + std::to_string(i) + " runs past the file");
    }
    hdr_len = c.p;
    return 0;
}
}  // namespace

int afq_convert(const afq_convert_opts* o) { return afq_convert_with(o, 0); }

int afq_convert_with(const afq_convert_opts* o, uint32_t flags) {
    if (flags & ~AFQ_CONVERT_INFLATE_ON_DEVICE) return hfail(AFQ_ERR_INVALID_ARG, "afq_convert_with: unknown flag bits (AFQ_CONVERT_INFLATE_ON_DEVICE is the one there is)");
    if (!o || !o->bam || !o->rad_out) return hfail(AFQ_ERR_INVALID_ARG, "null option: the BAM (-b) and the output RAD (-o) are required");
    const bool on_device = (flags & AFQ_CONVERT_INFLATE_ON_DEVICE) != 0;
    const std::string in = o->bam, outp = o->rad_out;
    if (ends_with(in, ".sam") || ends_with(in, ".SAM")) return hfail(AFQ_ERR_UNSUPPORTED, "convert: SAM text input is not supported; only BAM is read (convert the file to BAM first)");
    if (!ends_with(in, ".bam") && !ends_with(in, ".BAM")) return hfail(AFQ_ERR_BAD_INPUT, "unsupported input file format, must end with bam/BAM or sam/SAM");
    PhaseClock pc;
    MappedFile mf;
    if (!mf.open(in)) return hfail(AFQ_ERR_BAD_INPUT, "could not open the input BAM \"" + in + "\"");
    std::fprintf(stderr, "Bam file size in bytes %llu\n", (unsigned long long)mf.n);
    // ---- the container
    std::vector<BgzfBlock> blocks;
    uint64_t total = 0;
    if (int rc = bgzf_plan(mf.p, mf.n, blocks, total)) return rc;
    std::unique_ptr<uint8_t[]> plain;   // the closed door: the inflated file; the open one: the record stream, copied back
    std::vector<std::string> names;
    int32_t n_ref = 0;
    size_t hdr_len = 0;
    CtxPtr ctx;
    const uint8_t* d_stream = nullptr;   // the open door: the record stream on the device
    if (!on_device) {
        const unsigned nthreads = o->num_threads > 1 ? o->num_threads - 1 : 1;   // convert.rs:205-210
        std::fprintf(stderr, "parsing BAM file using %u decompression threads\n", nthreads);
        plain.reset(new (std::nothrow) uint8_t[total + 1]);
        if (!plain) return hfail(AFQ_ERR_OOM, "convert: " + std::to_string(total) + " bytes for the inflated BAM could not be allocated");
        if (int rc = bgzf_inflate(mf.p, blocks, plain.get(), nthreads)) return rc;
        pc.lap("convert: BGZF plan + inflate");
        if (int rc = convert_bam_header(plain.get(), (size_t)total, names, n_ref, hdr_len)) return rc;
    } else {
        // The leading blocks are inflated here until the BAM header is whole - one block, then twice as many as the time before -
        // for the header's length: the device lays the file down so that the first record stands at a 16-byte-aligned address.
        // A header that does not parse with every block inflated is the file's fault; its sentence waits behind the device's
        // verdict on the blocks, as it does behind the host inflate's.
        std::fprintf(stderr, "parsing BAM file with the BGZF blocks inflated on the device\n");
        pc.lap("convert: BGZF plan");
        if (int rc = open_fill_ctx(o->device, 0, ctx)) return rc;
        std::vector<uint8_t> head;
        int hdr_rc = 0;
        std::string hdr_err;
        for (size_t have = 0, want = 1;; want = 2 * have) {
            want = std::min(want, blocks.size());
            if (want > have) {
                const std::vector<BgzfBlock> sub(blocks.begin(), blocks.begin() + want);
                head.assign((size_t)(sub.back().out_off + sub.back().isize) + 1, 0);
                if (int rc = bgzf_inflate(mf.p, sub, head.data(), 1)) return rc;
                head.pop_back();
                have = want;
            }
            hdr_rc = convert_bam_header(head.data(), head.size(), names, n_ref, hdr_len);
            if (!hdr_rc || have == blocks.size()) break;
        }
        if (hdr_rc) { hdr_err = g_herr; hdr_len = 0; }
        const uint32_t shift = (uint32_t)((16 - hdr_len % 16) % 16);
        uint8_t* d = nullptr;
        uint64_t dn = 0;
        if (int rc = afq_bgzf_inflate_device(ctx.get(), mf.p, mf.n, shift, 1, &d, &dn, nullptr)) return hfail(rc, afq_last_error(ctx.get()));
        pc.lap("convert: device inflate");
        if (hdr_rc) return hfail(hdr_rc, hdr_err);
        d_stream = d + shift + hdr_len;
        const uint64_t rest = total - hdr_len;
        plain.reset(new (std::nothrow) uint8_t[hdr_len + rest + 1]);
        if (!plain) return hfail(AFQ_ERR_OOM, "convert: " + std::to_string(total) + " bytes for the inflated BAM could not be allocated");
        if (int rc = afq_bgzf_resident_to_host(ctx.get(), shift, hdr_len, plain.get() + hdr_len, rest)) return hfail(rc, afq_last_error(ctx.get()));
    }
    std::fprintf(stderr, "ref count: %d \n", n_ref);
    // ---- the first record's lengths, the span table (one hop per record, four bytes read of each)
    const uint8_t* stream = plain.get() + hdr_len;
    const uint64_t sn = total - hdr_len;
    if (sn == 0) return hfail(AFQ_ERR_BAD_INPUT, "bam file had no records!");
    uint32_t cblen = 0, ulen = 0;
    if (int rc = convert_first_lengths(stream, sn, cblen, ulen)) return rc;
    const uint64_t span_bytes = (uint64_t)std::max(64L, afq::test_hook_long("CONVERT_SPAN_BYTES", 1L << 16));   // (the hook: several spans in a small file)
    std::vector<uint64_t> spans;
    {
        uint64_t next = 0, idx = 0;
        for (uint64_t p = 0; p < sn; ++idx) {
            if (sn - p < 4) return hfail(AFQ_ERR_BAD_INPUT, "record " + std::to_string(idx) + ": the stream ends inside block_size");
            const uint64_t bs = le32(stream + p);
            if (bs > sn - p - 4) return hfail(AFQ_ERR_BAD_INPUT, "record " + std::to_string(idx) + ": block_size runs past the stream");
            if (p >= next) { spans.push_back(p); next = p + span_bytes; }
            p += 4 + bs;
        }
    }
    if (spans.size() >= (1ull << 32)) return hfail(AFQ_ERR_UNSUPPORTED, "convert: 2^32 or more spans");
    pc.lap(on_device ? "convert: stream D2H + span table" : "convert: header + span table");
    // ---- the device: one fill
    if (!on_device)
        if (int rc2 = open_fill_ctx(o->device, 0, ctx)) return rc2;
    uint8_t* ob = nullptr; uint64_t on = 0, n_chunks = 0, *ooff = nullptr; uint32_t* onrec = nullptr;
    afq_convert_stats st{};
    int rc = afq_convert_bam_rad(ctx.get(), on_device ? d_stream : stream, sn, spans.data(), (uint32_t)spans.size(), (uint32_t)n_ref, convert_width(cblen), convert_width(ulen),
                                 o->filter_best != 0, on_device ? 1 : 0, &ob, &on, &ooff, &onrec, &n_chunks, &st);
    if (rc) return hfail(rc, afq_last_error(ctx.get()));
    struct Freer { void *a, *b, *c; ~Freer() { afq_free(a); afq_free(b); afq_free(c); } } fr{ob, ooff, onrec};
    pc.lap("convert: device");
    if (o->stats_out) *o->stats_out = st;
    // ---- the RAD: the parent directory is created, an existing file replaced (convert.rs:181-188)
    const size_t slash = outp.find_last_of('/');
    if (slash != std::string::npos && slash > 0 && mkdirs_checked(outp.substr(0, slash))) return hfail(AFQ_ERR_BAD_INPUT, "could not create the directory of \"" + outp + "\"");
    std::remove(outp.c_str());
    std::vector<uint8_t> pre;
    convert_prelude(names, n_chunks, cblen, ulen, pre);
    FilePtr f(std::fopen(outp.c_str(), "wb"));
    bool ok = (bool)f;
    if (ok) ok = std::fwrite(pre.data(), 1, pre.size(), f.get()) == pre.size();
    for (uint64_t off = 0; ok && off < on;) {
        const size_t len = (size_t)std::min<uint64_t>(on - off, 1ull << 30);
        ok = std::fwrite(ob + off, 1, len, f.get()) == len;
        off += len;
    }
    ok = ok && std::fflush(f.get()) == 0;
    if (!ok) { f.reset(); std::remove(outp.c_str()); return hfail(AFQ_ERR_BAD_INPUT, "could not write " + outp); }
    pc.lap("convert: write");
    std::fprintf(stderr, "%llu chunks written\n", (unsigned long long)n_chunks);
    std::fprintf(stderr, "converted %llu records (%llu unmapped or supplementary) in %llu reads: %llu written with %llu of %llu alignments, %llu dropped for two N or more; %llu output bytes\n",
                 (unsigned long long)st.n_records, (unsigned long long)st.n_dropped_by_flag, (unsigned long long)st.n_runs, (unsigned long long)st.n_runs_written,
                 (unsigned long long)st.n_alignments_written, (unsigned long long)st.n_alignments_in, (unsigned long long)st.n_runs_dropped_n, (unsigned long long)st.out_bytes);
    return 0;
}

int afq_view_file(const char* rad, int print_header, const char* out_path) {
    if (!rad) return hfail(AFQ_ERR_INVALID_ARG, "null RAD path");
    MappedFile mf;
    if (!mf.open(rad)) return hfail(AFQ_ERR_BAD_INPUT, std::string("could not open the RAD file \"") + rad + "\"");
    RadPrelude P;
    if (int rc = parse_prelude(mf.p, mf.n, P, true)) return rc;
    // the b and u read tags must be integers (convert.rs:619-639); the records are read as na, b, u, na x u32
    const TagDesc* bt = nullptr; const TagDesc* ut = nullptr;
    for (auto& t : P.read_tags) {
        if (t.name != "b" && t.name != "u") continue;
        if (t.type < 1 || t.type > 4) return hfail(AFQ_ERR_UNSUPPORTED, "currently only RAD types 1--4 are supported for 'b' and 'u' tags.");
        (t.name == "b" ? bt : ut) = &t;
    }
    if (!bt) return hfail(AFQ_ERR_BAD_INPUT, "barcode type tag was missing!");
    if (!ut) return hfail(AFQ_ERR_BAD_INPUT, "umi type tag was missing!");
    if (!P.file_tag_vals.count("cblen")) return hfail(AFQ_ERR_BAD_INPUT, "tag map must contain cblen");
    if (!P.file_tag_vals.count("ulen")) return hfail(AFQ_ERR_BAD_INPUT, "tag map must contain ulen");
    if (P.read_tags.size() != 2 || P.read_tags[0].name != "b" || P.aln_tags.size() != 1 || P.aln_tags[0].type != 3)
        return hfail(AFQ_ERR_UNSUPPORTED, "view: only records `na, b, u, na x u32` are read (read tags b, u; one u32 alignment tag)");
    const uint64_t cblen = P.file_tag_vals["cblen"], ulen = P.file_tag_vals["ulen"];
    if (cblen > 32 || ulen > 32) return hfail(AFQ_ERR_BAD_INPUT, "view: cblen or ulen above 32");
    FILE* fo = out_path ? std::fopen(out_path, "w") : stdout;
    if (!fo) return hfail(AFQ_ERR_BAD_INPUT, std::string("could not write \"") + out_path + "\"");
    struct Closer { FILE* f; bool own; ~Closer() { if (own) std::fclose(f); else std::fflush(f); } } closer{fo, out_path != nullptr};
    if (print_header)
        for (size_t i = 0; i < P.ref_names.size(); ++i) std::fprintf(fo, "%zu:%s\n", i, P.ref_names[i].c_str());
    const uint32_t bw = P.bc_bytes, uw = P.umi_bytes;
    auto field = [&](size_t at, uint32_t w) { uint64_t v = 0; std::memcpy(&v, mf.p + at, w); return v; };
    uint64_t id = 0;
    size_t p = P.first_chunk;
    for (uint64_t ch = 0; ch < P.num_chunks; ++ch) {
        const std::string at = "chunk " + std::to_string(ch) + ": ";
        if (mf.n - p < 8) return hfail(AFQ_ERR_BAD_INPUT, at + "the file ends inside the chunk header");
        const uint32_t nbytes = le32(mf.p + p), nrec = le32(mf.p + p + 4);
        if (nbytes < 8 || nbytes > mf.n - p) return hfail(AFQ_ERR_BAD_INPUT, at + "nbytes runs past the file");
        const size_t end = p + nbytes;
        size_t q = p + 8;
        for (uint32_t r = 0; r < nrec; ++r, ++id) {
            if (end - q < 4 + bw + uw) return hfail(AFQ_ERR_BAD_INPUT, at + "the records do not tile the chunk");
            const uint32_t na = le32(mf.p + q);
            if (na > (end - q - 4 - bw - uw) / 4) return hfail(AFQ_ERR_BAD_INPUT, at + "the records do not tile the chunk");
            const std::string cb = bc_to_string(field(q + 4, bw), (uint32_t)cblen), um = bc_to_string(field(q + 4 + bw, uw), (uint32_t)ulen);
            q += 4 + bw + uw;
            for (uint32_t i = 0; i < na; ++i, q += 4) {
                const uint32_t w = le32(mf.p + q), rid = w & 0x7FFFFFFFu;
                if (rid >= P.ref_names.size()) return hfail(AFQ_ERR_BAD_INPUT, at + "a reference id is not below ref_count");
                std::fprintf(fo, "ID:%llu\tHI:%u\tNH:%u\tCB:%s\tUMI:%s\tDIR:%s\t%s\n", (unsigned long long)id, i + 1, na, cb.c_str(), um.c_str(), (w >> 31) ? "true" : "false",
                             P.ref_names[rid].c_str());
            }
        }
        p = end;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// multi-barcode `collate` (do_collate_multi_bc_fast, src/collate.rs:1415-1920).  libradicl's collate_multi_barcode is not among the
// reference's sources; where collate.rs leaves a rule to it, the choice is DESIGN.md 3.4h's.
namespace {
struct ManifestGroup { uint64_t key; std::string name; uint64_t chunk_start, num_chunks, num_records; };
// collation_manifest.bin in the layout parse_collation_manifest (below) reads: level names sample, cell; every group is named
void collation_manifest_bytes(const std::vector<ManifestGroup>& groups, std::vector<uint8_t>& out) {
    out.clear();
    auto u64 = [&](uint64_t v) { const uint8_t* p = (const uint8_t*)&v; out.insert(out.end(), p, p + 8); };
    auto str = [&](const std::string& s) { u64(s.size()); out.insert(out.end(), s.begin(), s.end()); };
    u64(2); str("sample"); str("cell");
    u64(groups.size());
    for (auto& g : groups) { u64(g.key); out.push_back(1); str(g.name); u64(g.chunk_start); u64(g.num_chunks); u64(g.num_records); }
}
// a JSON string at js[at] (the opening quote) -> its text; false: not a string, or an escape this reader does not know
bool json_string_at(const std::string& js, size_t at, std::string& out) {
    if (at == std::string::npos || at >= js.size() || js[at] != '"') return false;
    out.clear();
    for (size_t i = at + 1; i < js.size(); ++i) {
        const char ch = js[i];
        if (ch == '"') return true;
        if (ch != '\\') { out.push_back(ch); continue; }
        if (++i >= js.size()) return false;
        switch (js[i]) {
            case '"': case '\\': case '/': out.push_back(js[i]); break;
            case 'n': out.push_back('\n'); break;
            case 't': out.push_back('\t'); break;
            case 'r': out.push_back('\r'); break;
            default: return false;
        }
    }
    return false;
}
// sample_info.json (collate.rs:1480-1561): num_samples, and name and canonical barcode of every entry of `samples`, in file order
int read_sample_info(const std::string& path, uint64_t& num_samples, std::vector<std::string>& names, std::vector<uint64_t>& barcodes) {
    std::vector<uint8_t> raw;
    if (!read_file(path, raw)) return hfail(AFQ_ERR_BAD_INPUT, "could not open sample_info.json - was generate-permit-list run with --sample-bc-list?");
    const std::string js(raw.begin(), raw.end());
    {
        const size_t v = json_top_level_value(js, "num_samples");
        char* e = nullptr;
        if (v != std::string::npos) num_samples = std::strtoull(js.c_str() + v, &e, 10);
        if (v == std::string::npos || e == js.c_str() + v) return hfail(AFQ_ERR_BAD_INPUT, "couldn't read num_samples from sample_info.json");
    }
    const size_t a = json_top_level_value(js, "samples");
    if (a == std::string::npos || js[a] != '[') return hfail(AFQ_ERR_BAD_INPUT, "couldn't read samples array from sample_info.json");
    int depth = 0;
    size_t obj = 0;
    for (size_t i = a; i < js.size(); ++i) {
        const char ch = js[i];
        if (ch == '"') { for (++i; i < js.size() && js[i] != '"'; ++i) if (js[i] == '\\') ++i; continue; }
        if (ch == '{' || ch == '[') { if (++depth == 2 && ch == '{') obj = i; continue; }
        if (ch != '}' && ch != ']') continue;
        if (--depth == 0) break;
        if (depth != 1 || ch != '}') continue;
        const std::string o = js.substr(obj, i + 1 - obj);
        std::string bc = "0x0", nm;   // collate.rs:1551-1560
        json_string_at(o, json_top_level_value(o, "barcode"), bc);
        size_t h = 0;
        while (bc.compare(h, 2, "0x") == 0) h += 2;   // trim_start_matches("0x"): the pattern as often as it leads
        char* e = nullptr;
        const std::string hex = bc.substr(h);
        uint64_t v = hex.empty() ? 0 : std::strtoull(hex.c_str(), &e, 16);
        if (hex.empty() || !e || *e) v = 0;
        if (!json_string_at(o, json_top_level_value(o, "name"), nm)) { char hx[32]; std::snprintf(hx, sizeof hx, "%llx", (unsigned long long)v); nm = hx; }
        names.push_back(nm); barcodes.push_back(v);
    }
    if (depth != 0) return hfail(AFQ_ERR_BAD_INPUT, "couldn't read samples array from sample_info.json");
    return 0;
}
}  // namespace

int64_t afq_collation_manifest_bytes(const uint64_t* key, const char* const* name, const uint64_t* chunk_start, const uint64_t* num_chunks, const uint64_t* num_records,
                                     uint64_t n_groups, uint8_t* out, size_t cap) {
    if ((!key || !name || !chunk_start || !num_chunks || !num_records) && n_groups) return hfail(AFQ_ERR_INVALID_ARG, "null argument");
    std::vector<ManifestGroup> g;
    for (uint64_t i = 0; i < n_groups; ++i) {
        if (!name[i]) return hfail(AFQ_ERR_INVALID_ARG, "null argument");
        g.push_back(ManifestGroup{key[i], name[i], chunk_start[i], num_chunks[i], num_records[i]});
    }
    std::vector<uint8_t> b;
    collation_manifest_bytes(g, b);
    if (out && cap >= b.size()) std::memcpy(out, b.data(), b.size());
    return (int64_t)b.size();
}

int afq_collate_multi_check_args(uint32_t b0_bytes, uint32_t b1_bytes, uint32_t umi_bytes, uint32_t expected_ori, const uint64_t* sample_observed,
                                 const uint32_t* sample_index, uint64_t n_sample_entries, const uint32_t* corr_sample, const uint64_t* corr_observed,
                                 const uint64_t* corr_corrected, uint64_t n_corrections, const uint32_t* cell_sample, const uint64_t* cell_bc, uint64_t n_cells,
                                 const uint32_t* sample_b0_out, uint64_t n_samples) {
    std::string e;
    std::vector<uint32_t> val;
    const int r = afq::gplhost::collate_multi_index(b0_bytes, b1_bytes, umi_bytes, expected_ori, sample_observed, sample_index, n_sample_entries, corr_sample, corr_observed,
                                                    corr_corrected, n_corrections, cell_sample, cell_bc, n_cells, sample_b0_out, n_samples, val, e);
    return r ? hfail(r, e) : 0;
}

// (two doors, as collate: afq_collate_multi keeps its refusal of opts.compress, afq_collate_multi_sz writes map.collated.rad.sz)
static int collate_multi_run(const afq_collate_multi_opts* o, bool sz);
int afq_collate_multi(const afq_collate_multi_opts* o) {
    if (!o || !o->input_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    if (!o->rad_dir) return hfail(AFQ_ERR_INVALID_ARG, "the RAD directory (-r) is required");
    if (o->compress) return hfail(AFQ_ERR_UNSUPPORTED, "compressed output is not supported");
    return collate_multi_run(o, false);
}
int afq_collate_multi_sz(const afq_collate_multi_opts* o) {
    if (!o || !o->input_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    if (!o->rad_dir) return hfail(AFQ_ERR_INVALID_ARG, "the RAD directory (-r) is required");
    return collate_multi_run(o, true);
}
static int collate_multi_run(const afq_collate_multi_opts* o, bool sz) {
    const std::string in = o->input_dir, rd = o->rad_dir;
    // ---- generate_permit_list.json (collate.rs:155-200)
    std::vector<uint8_t> gj;
    if (!read_file(in + "/generate_permit_list.json", gj)) return hfail(AFQ_ERR_BAD_INPUT, "could not open generate_permit_list.json in \"" + in + "\"");
    const std::string gjs(gj.begin(), gj.end());
    auto value_at = [&](const char* key) { return json_top_level_value(gjs, key); };
    auto is_true = [&](size_t v) { return v != std::string::npos && gjs.compare(v, 4, "true") == 0; };
    if (value_at("version_str") == std::string::npos)
        return hfail(AFQ_ERR_BAD_INPUT, "The generate_permit_list.json file does not contain a version_str field. Please re-run the generate-permit-list step with a newer version of alevin-fry");
    if (!is_true(value_at("multi_barcode"))) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode collate: this is a single-barcode permit list (no multi_barcode: true); use collate");
    if (is_true(value_at("velo_mode"))) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode collate: velo_mode: true is not supported");
    uint32_t expected_ori = 0;
    {
        const size_t v = value_at("expected_ori");
        static const char* const kSym[3] = {"\"both\"", "\"fw\"", "\"rc\""};
        uint32_t k = 0;
        while (k < 3 && (v == std::string::npos || gjs.compare(v, std::strlen(kSym[k]), kSym[k]) != 0)) ++k;
        if (k == 3) return hfail(AFQ_ERR_BAD_INPUT, "could not read strand: generate_permit_list.json: expected_ori must be \"both\", \"fw\" or \"rc\"");
        expected_ori = k;
    }
    // ---- sample_info.json, the cells of every sample (collate.rs:1480-1611)
    uint64_t num_samples = 0;
    std::vector<std::string> names;
    std::vector<uint64_t> canon;
    if (int rc2 = read_sample_info(in + "/sample_info.json", num_samples, names, canon)) return rc2;
    const size_t n_plate = names.size();
    if (n_plate > (1ull << 31)) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode collate: more than 2^31 samples");
    {
        std::vector<uint64_t> sorted = canon;
        std::sort(sorted.begin(), sorted.end());
        for (size_t i = 1; i < sorted.size(); ++i)
            if (sorted[i] == sorted[i - 1]) { char hx[32]; std::snprintf(hx, sizeof hx, "0x%llx", (unsigned long long)sorted[i]); return hfail(AFQ_ERR_BAD_INPUT, std::string("sample_info.json lists the sample barcode ") + hx + " twice"); }
    }
    std::vector<uint32_t> cell_sample, b0_out(n_plate, 0);
    std::vector<uint64_t> cell_bc;
    std::vector<ManifestGroup> groups;
    std::vector<char> has_cells(n_plate, 0);
    for (size_t si = 0; si < n_plate; ++si) {
        const std::string sdir = in + "/sample_" + names[si];
        if (!file_exists(sdir + "/permit_freq.bin")) continue;   // a sample without a read (collate.rs:1604-1607)
        std::vector<uint64_t> cells;   // by (count descending, barcode ascending): collate.rs:1611 within a sample
        uint64_t bc_len = 0, recs = 0;
        const std::string bad_len = "couldn't deserialize " + sdir + "/permit_freq.bin: its length does not match its entry count";
        if (int rc2 = read_permit_cells(sdir, bad_len.c_str(), bc_len, cells, &recs)) return rc2;
        if (cells.empty()) continue;
        has_cells[si] = 1;
        b0_out[si] = (uint32_t)groups.size();   // the dense ordinal (collate.rs:1630-1638)
        groups.push_back(ManifestGroup{canon[si], names[si], (uint64_t)cell_bc.size(), cells.size(), recs});
        for (uint64_t b : cells) { cell_sample.push_back((uint32_t)si); cell_bc.push_back(b); }
    }
    // ---- the plan (collate.rs:1517-1532)
    if (!file_exists(in + "/correction_plan.bin"))
        return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode collate: no correction_plan.bin in \"" + in + "\": the reference then corrects cell barcodes on the fly (libradicl's Hamming-1 "
                     "lookup), which is not restated here; rerun generate-permit-list");
    MultiPlan plan;
    {
        std::vector<uint8_t> cm;
        if (!read_file(in + "/correction_plan.bin", cm)) return hfail(AFQ_ERR_BAD_INPUT, "could not open correction plan " + in + "/correction_plan.bin");
        if (int rc2 = parse_plan_multi(cm.data(), cm.size(), plan)) return rc2;
    }
    // ---- map.rad: the prelude checks of afq_generate_permit_list_multi
    if (!file_exists(rd)) return hfail(AFQ_ERR_BAD_INPUT, "the input RAD path \"" + rd + "\" does not exist");
    PhaseClock pc;
    MappedFile mf;
    if (!mf.open(rd + "/map.rad")) return hfail(AFQ_ERR_BAD_INPUT, "couldn't open input RAD file");
    const uint8_t* rad = mf.p;
    const size_t rad_n = mf.n;
    RadPrelude P;
    int rc = parse_prelude(rad, rad_n, P, false);
    if (rc) return rc;
    auto has_tag = [](const std::vector<TagDesc>& v, const char* name) { for (auto& t : v) if (t.name == name) return true; return false; };
    if (has_tag(P.aln_tags, "start_pos") || has_tag(P.aln_tags, "frag_len")) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode collate: this is a scATAC RAD file; use `atac collate`");
    if (!P.file_tag_vals.count("num_barcodes") || P.file_tag_vals["num_barcodes"] <= 1)
        return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode collate: this is a single-barcode RAD file (no num_barcodes > 1 file tag); use collate");
    if (has_tag(P.aln_tags, "pos")) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode RAD records with alignment positions (alignment tag pos) are not supported");
    if (P.file_tag_vals["num_barcodes"] != 2 || P.read_tags.size() != 3 || P.read_tags[0].name != "b0" || P.read_tags[1].name != "b1" || P.read_tags[2].name != "u")
        return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode RAD: only two barcode levels with read tags (b0, b1, u) are supported");
    const uint32_t w0 = (uint32_t)int_type_bytes(P.read_tags[0].type), w1 = (uint32_t)int_type_bytes(P.read_tags[1].type), wu = (uint32_t)int_type_bytes(P.read_tags[2].type);
    if (!w0 || !w1 || w0 > 4 || w1 > 4 || !wu) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode RAD: b0 and b1 must be integers of 1, 2 or 4 bytes (u8/u16/u32)");
    if (P.aln_tags.size() != 1 || P.aln_tags[0].type != 3) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode RAD: the alignment-level tags must be one u32 (ref | orientation)");
    if (!P.file_tag_vals.count("b1len")) return hfail(AFQ_ERR_BAD_INPUT, "multi-barcode RAD file should have a \"b1len\" file-level tag");
    const uint32_t cblen = (uint32_t)P.file_tag_vals["b1len"];
    if (cblen < 1 || cblen > 32) return hfail(AFQ_ERR_BAD_INPUT, "barcode length must be between 1 and 32 (got " + std::to_string(cblen) + ")");
    {   // collate.rs:1495-1515
        uint32_t sbits = 0;
        while (num_samples > 1 && sbits < 64 && ((num_samples - 1) >> sbits)) ++sbits;
        if (sbits + 2 * cblen > 64)
            return hfail(AFQ_ERR_UNSUPPORTED, "Cannot collate: " + std::to_string(num_samples) + " samples requires " + std::to_string(sbits) + " bits for the sample index, plus " +
                         std::to_string(2 * cblen) + " bits for " + std::to_string(cblen) + "bp cell barcodes = " + std::to_string(sbits + 2 * cblen) +
                         " bits total, which exceeds the 64-bit composite key capacity.");
    }
    if (plan.cell_len != cblen) return hfail(AFQ_ERR_BAD_INPUT, "correction plan does not match this multi-barcode RAD input");
    if (!groups.empty() && w0 < 4 && (groups.size() - 1) >> (8 * w0))
        return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode collate: the largest sample ordinal (" + std::to_string(groups.size() - 1) + ") does not fit the " + std::to_string(w0) + "-byte b0 field of the records");
    // ---- the two lookups: observed sample barcode -> plate index (collate.rs:1754-1761); per sample with cells, its scope's corrections
    const uint64_t top0 = 1ull << (8 * w0), top1 = 1ull << (8 * w1);   // (a key that does not fit its field meets no record)
    std::vector<std::pair<uint64_t, uint32_t>> plate(n_plate);
    for (size_t si = 0; si < n_plate; ++si) plate[si] = {canon[si], (uint32_t)si};
    std::sort(plate.begin(), plate.end());
    auto plate_of = [&](uint64_t bc) -> int64_t {
        const auto it = std::lower_bound(plate.begin(), plate.end(), std::make_pair(bc, 0u));
        return it != plate.end() && it->first == bc ? (int64_t)it->second : -1;
    };
    std::vector<uint64_t> s_obs;
    std::vector<uint32_t> s_idx;
    for (size_t i = 0; i < plan.sample_obs.size(); ++i) {
        const int64_t si = plate_of(plan.sample_cor[i]);
        if (si >= 0 && plan.sample_obs[i] < top0) { s_obs.push_back(plan.sample_obs[i]); s_idx.push_back((uint32_t)si); }
    }
    std::vector<uint32_t> c_sample;
    std::vector<uint64_t> c_obs, c_cor;
    std::vector<char> scoped(n_plate, 0);
    for (auto& sc : plan.scopes) {
        const int64_t si = plate_of(sc.sample_barcode);
        if (si < 0) continue;
        scoped[(size_t)si] = 1;
        for (size_t i = 0; i < sc.obs.size(); ++i)
            if (sc.obs[i] < top1) { c_sample.push_back((uint32_t)si); c_obs.push_back(sc.obs[i]); c_cor.push_back(sc.cor[i]); }
    }
    for (size_t si = 0; si < n_plate; ++si)
        if (has_cells[si] && !scoped[si]) { char hx[32]; std::snprintf(hx, sizeof hx, "0x%llx", (unsigned long long)canon[si]); return hfail(AFQ_ERR_BAD_INPUT, std::string("correction plan has no cell scope for canonical sample ") + hx); }
    {   // afq_collate_multi_rad's own checks, before the device is opened: a correction into a barcode that is no cell of its sample is refused here
        std::string e;
        std::vector<uint32_t> val;
        if (int rc2 = afq::gplhost::collate_multi_index(w0, w1, wu, expected_ori, s_obs.data(), s_idx.data(), s_obs.size(), c_sample.data(), c_obs.data(), c_cor.data(), c_obs.size(),
                                                        cell_sample.data(), cell_bc.data(), cell_bc.size(), b0_out.data(), n_plate, val, e))
            return hfail(rc2, e);
    }
    // ---- the chunk table
    std::vector<uint64_t> chunk_off;
    if (int rc2 = walk_chunk_offsets(rad, rad_n, P.first_chunk, P.num_chunks, chunk_off)) return rc2;
    if (chunk_off.size() >= (1ull << 32)) return hfail(AFQ_ERR_UNSUPPORTED, "2^32 or more chunks");
    pc.lap("metadata + plan + chunk table");
    // ---- the device: one fill
    CtxPtr ctx;
    if (int rc2 = open_fill_ctx(o->device, 0, ctx)) return rc2;
    afq_set_collate_compress(ctx.get(), sz);
    const uint64_t span0 = chunk_off.empty() ? P.first_chunk : chunk_off[0];
    std::vector<uint64_t> rel;
    rebase_chunk_offsets(chunk_off, span0, rel);
    uint8_t* ob = nullptr; uint64_t on = 0, *ooff = nullptr; uint32_t* onrec = nullptr;
    afq_collate_multi_stats st{};
    rc = afq_collate_multi_rad(ctx.get(), rad + span0, rad_n - span0, rel.data(), (uint32_t)chunk_off.size(), w0, w1, wu, expected_ori, 0, s_obs.data(), s_idx.data(), s_obs.size(),
                               c_sample.data(), c_obs.data(), c_cor.data(), c_obs.size(), cell_sample.data(), cell_bc.data(), cell_bc.size(), b0_out.data(), n_plate, &ob, &on,
                               &ooff, &onrec, &st);
    if (rc) return hfail(rc, afq_last_error(ctx.get()));
    struct Freer { void *a, *b, *c; ~Freer() { afq_free(a); afq_free(b); afq_free(c); } } fr{ob, ooff, onrec};
    pc.lap("device: collate");
    if (o->stats_out) *o->stats_out = st;
    // ---- per sample: the records kept are the sample's collatable reads (nothing was written yet, so no RAD is left behind)
    for (auto& g : groups) {
        uint64_t kept = 0;
        for (uint64_t j = g.chunk_start; j < g.chunk_start + g.num_chunks; ++j) kept += onrec[j];
        if (kept != g.num_records)
            return hfail(AFQ_ERR_BAD_INPUT, "sample '" + g.name + "': expected to collate " + std::to_string(g.num_records) + " records but retained " + std::to_string(kept));
    }
    // ---- the files
    if (int rc2 = write_collated_rad(in + (sz ? "/map.collated.rad.sz" : "/map.collated.rad"), rad, P, cell_bc.size(), ob, on, sz ? ctx.get() : nullptr)) return rc2;
    {
        std::vector<uint8_t> mb;
        collation_manifest_bytes(groups, mb);
        FilePtr f(std::fopen((in + "/collation_manifest.bin").c_str(), "wb"));
        if (!f || std::fwrite(mb.data(), 1, mb.size(), f.get()) != mb.size()) return hfail(AFQ_ERR_BAD_INPUT, "could not write collation_manifest.bin");
    }
    {   // an empty map, in the layout afq_quantify reads (collate.rs:364-381: what the reference writes when it cannot read the input's header)
        FilePtr f(std::fopen((in + "/unmapped_bc_count_collated.bin").c_str(), "wb"));
        const uint64_t zero = 0;
        if (!f || std::fwrite(&zero, 8, 1, f.get()) != 1) return hfail(AFQ_ERR_BAD_INPUT, "could not create serialization file.");
    }
    {   // collate.json (collate.rs:1668-1676)
        FilePtr f(std::fopen((in + "/collate.json").c_str(), "w"));
        if (!f) return hfail(AFQ_ERR_BAD_INPUT, "could not create metadata file.");
        std::fprintf(f.get(), "{\n  \"cmd\": \"%s\",\n  \"version_str\": \"0.18.0\",\n  \"compressed_output\": %s,\n  \"multi_barcode\": true,\n  \"num_samples\": %llu,\n"
                     "  \"collation_mode\": \"optimized\",\n  \"memory_budget_bytes\": 0\n}", json_escape(o->cmdline ? o->cmdline : "").c_str(), sz ? "true" : "false",
                     (unsigned long long)num_samples);
    }
    pc.lap("map.collated.rad");
    std::fprintf(stderr, "collated %llu of %llu records (%llu orientation consistent, %llu with no sample, %llu with a cell barcode that is not in its sample's map) into %llu cells of %llu samples\n",
                 (unsigned long long)st.n_kept, (unsigned long long)st.n_records, (unsigned long long)st.n_compatible, (unsigned long long)st.n_unrouted,
                 (unsigned long long)st.n_uncorrected, (unsigned long long)cell_bc.size(), (unsigned long long)groups.size());
    std::fprintf(stderr, "kept %llu of %llu alignments; %llu output bytes\n", (unsigned long long)st.n_alignments_kept, (unsigned long long)st.n_alignments_in,
                 (unsigned long long)st.out_bytes);
    return 0;
}

// collation_manifest.bin (libradicl::collation::CollationManifest, written by src/collate.rs:1861-1890): the names of the
// samples, indexed by the integer the scatter phase left in barcodes[0].  libradicl's source is not under /root/reference, so
// the layout read here is a RESTATEMENT of its serde derive under bincode's default options (parity unpinned):
//   level_names: u64 n, n x (u64 len, bytes);  sample_groups: u64 n, n x { key u64, name: u8 tag (0 None / 1 Some) [u64 len,
//   bytes], chunk_start u64, num_chunks u64, num_records u64 }
// The file must tile exactly; anything else is refused.  A sample without a name is called by its key in hex (quant.rs:1364-1368).
static bool parse_collation_manifest(const std::vector<uint8_t>& b, std::vector<std::string>& names) {
    Cursor c{b.data(), b.size()};
    const uint64_t nl = c.get<uint64_t>();
    if (!c.ok || nl > 64) return false;
    for (uint64_t i = 0; i < nl; ++i) { const uint64_t l = c.get<uint64_t>(); if (!c.ok || l > 4096) return false; c.str((size_t)l); }
    const uint64_t ng = c.get<uint64_t>();
    if (!c.ok || ng > (1u << 24)) return false;
    for (uint64_t i = 0; i < ng; ++i) {
        const uint64_t key = c.get<uint64_t>();
        const uint8_t tag = c.get<uint8_t>();
        std::string nm;
        if (tag == 1) { const uint64_t l = c.get<uint64_t>(); if (!c.ok || l > 65536) return false; nm = c.str((size_t)l); }
        else if (tag == 0) { char hx[32]; std::snprintf(hx, sizeof hx, "%llx", (unsigned long long)key); nm = hx; }
        else return false;
        c.get<uint64_t>(); c.get<uint64_t>(); c.get<uint64_t>();
        if (!c.ok) return false;
        names.push_back(nm);
    }
    return c.p == c.n;
}

int afq_quantify(const afq_quant_opts* o) {
    if (!o || !o->input_dir || !o->tg_map || !o->output_dir || !o->resolution) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    const ResolutionInfo* R = nullptr;
    for (auto& r : kRes) { std::string a = o->resolution; for (auto& ch : a) ch = (char)std::tolower(ch); if (a == r.name) R = &r; }
    if (!R) return hfail(AFQ_ERR_INVALID_ARG, std::string("unknown resolution ") + o->resolution);
    // flag compatibility, src/main.rs:652-728
    const int edist = o->umi_edit_dist < 0 ? (R->pars ? 1 : 0) : o->umi_edit_dist;
    if (edist > 1 || (edist == 1 && !R->pars)) return hfail(AFQ_ERR_INVALID_ARG, "resolution does not support this --umi-edit-dist");
    const uint32_t large_thresh = o->large_graph_thresh < 0 ? (R->pars ? 1000u : 0u) : (uint32_t)o->large_graph_thresh;
    if (o->dump_eq && R->id == AFQ_RES_TRIVIAL)   // src/main.rs:705-711
        return hfail(AFQ_ERR_INVALID_ARG, "Gene equivalence classes are not meaningful in case of Trivial resolution.");
    if (o->num_bootstraps && !(R->id == AFQ_RES_CR_LIKE_EM || R->id == AFQ_RES_PARSIMONY_EM || R->id == AFQ_RES_PARSIMONY_GENE_EM))   // src/main.rs:713-728
        return hfail(AFQ_ERR_INVALID_ARG, "The num_bootstraps argument was set to " + std::to_string(o->num_bootstraps) +
                     ", but bootstrapping can only be used with the cr-like-em, parsimony-em, or parsimony-gene-em resolution strategies");
    if (o->num_bootstraps && !o->summary_stat)   // BootstrapHelper::new, src/quant.rs:142-148
        std::fprintf(stderr, "NOTE: Full per-replicate bootstrap output is not yet supported in MTX format. Summary statistics (mean, variance) will be written instead. "
                             "Full replicate output will be available in a future release via AnnData/h5ad.\n");
    const std::string in = o->input_dir, outd = o->output_dir;
    // the permit-list json must exist (src/main.rs:733-734)
    if (!file_exists(in + "/generate_permit_list.json")) return hfail(AFQ_ERR_BAD_INPUT, "the input directory has no generate_permit_list.json");
    std::vector<uint8_t> cj;
    if (!read_file(in + "/collate.json", cj)) return hfail(AFQ_ERR_BAD_INPUT, "could not read collate.json");
    std::string cjs(cj.begin(), cj.end());
    bool compressed = false;
    { size_t k = cjs.find("\"compressed_output\""); if (k != std::string::npos) { size_t v = cjs.find_first_not_of(" \t\r\n:", k + 19); compressed = v != std::string::npos && cjs.compare(v, 4, "true") == 0; } }
    PhaseClock pc;
    // the HIP runtime takes a few hundred ms to come up: let it do so while the prelude and the tg-map are parsed
    const int first_device = o->devices && o->n_devices ? (int)o->devices[0] : (int)o->device;   // the one device of a one-device run: the workers', the warm-up's, the resident decode's
    std::thread warm([dev = first_device]() { afq_device_warmup(dev); });
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } warm_join{warm};
    MappedFile mf;
    if (!mf.open(in + (compressed ? "/map.collated.rad.sz" : "/map.collated.rad"))) return hfail(AFQ_ERR_BAD_INPUT, "could not read the collated RAD file");
    std::unique_ptr<uint8_t[]> rad_buf;   // (not a vector: no point zero-filling gigabytes that are about to be overwritten)
    uint64_t rad_buf_n = 0;
    // sz_on_device: the decoded file exists on the device alone - the prelude from the leading frame chunks here, the chunk table
    // from the device's hop further down, the workers' spans from where the decoder left them
    const bool resident = compressed && o->sz_on_device;
    if (o->sz_on_device && o->devices && o->n_devices > 1) return hfail(AFQ_ERR_UNSUPPORTED, "--sz-on-device takes one device");
    if (o->sz_on_device && !compressed) std::fprintf(stderr, "--sz-on-device: map.collated.rad is not compressed; the option is ignored\n");
    std::vector<SnappyChunk> sz_chunks;
    std::vector<uint8_t> sz_head;
    if (compressed) {
        std::string err;
        if (!snappy_frame_plan(mf.p, mf.n, sz_chunks, rad_buf_n, err)) return hfail(AFQ_ERR_BAD_INPUT, "map.collated.rad.sz: " + err);
        if (!resident) {
            rad_buf.reset(new (std::nothrow) uint8_t[rad_buf_n ? rad_buf_n : 1]);
            if (!rad_buf) return hfail(AFQ_ERR_OOM, "map.collated.rad.sz: not enough host memory for the decompressed file");
            if (!snappy_frame_run(mf.p, sz_chunks, rad_buf.get(), o->num_threads ? o->num_threads : std::max(1u, std::thread::hardware_concurrency()), err)) return hfail(AFQ_ERR_BAD_INPUT, "map.collated.rad.sz: " + err);
        }
    }
    struct { const uint8_t* p; size_t n; const uint8_t* data() const { return p; } size_t size() const { return n; } } rad{compressed ? rad_buf.get() : mf.p, compressed ? (size_t)rad_buf_n : mf.n};
    RadPrelude P;
    int rc = 0;
    if (resident) { rc = sz_prelude(mf.p, sz_chunks, rad_buf_n, sz_head, P, true); pc.lap("sz: prelude chunks"); }
    else { pc.lap(compressed ? "map + snappy decode" : "map the RAD file"); rc = parse_prelude(rad.data(), rad.size(), P, true); }
    if (rc) return rc;
    // Record layout.  Single-barcode scRNA: read tags (b, u).  Multi-barcode (10x Flex; KnownRecordType::RnaShortMultiBC,
    // src/utils.rs:313-340): file tag num_barcodes = 2, read tags (b0, b1, u) - after collation b0 is the integer sample
    // index and b1 the cell barcode (src/quant.rs:2003-2027).  The device decoders see (b0, b1) as ONE barcode field of
    // w0 + w1 bytes: every record of a collated chunk carries the same pair, so candidate detection, the proof and the
    // reported collate key work unchanged, and the host splits the 64-bit key back into sample index and cell barcode.
    // (Field order b0, b1, u inside a record = the order of the read-tag section; libradicl's MultiBarcodeReadRecord
    // writer is not under /root/reference: parity unpinned.)
    // Which records: the order of the reference's get_record_type_from_prelude (src/utils.rs:313-377) - multi-barcode, then
    // long-read (alignment tags as, start, end), records with positions (pos), scATAC (type, start_pos, frag_len), plain records.
    // Records with positions carry `compressed_ori_refid:u32, pos` per alignment; quant runs them through the same do_quantify as
    // plain records (quant.rs:1977-1990) and the library drops the positions on the device (afq_set_aln_extra_bytes).
    auto has_aln_tag = [&](const char* name) { for (auto& t : P.aln_tags) if (t.name == name) return true; return false; };
    const bool multi_bc = P.file_tag_vals.count("num_barcodes") && P.file_tag_vals["num_barcodes"] > 1;
    uint32_t aln_extra = 0;
    if (multi_bc) {
        if (has_aln_tag("pos")) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode RAD records with alignment positions (alignment tag pos) are not supported");
    } else if (has_aln_tag("as") && has_aln_tag("start") && has_aln_tag("end")) {
        return hfail(AFQ_ERR_UNSUPPORTED, "long-read RAD records (alignment tags as, start, end) are not supported");
    } else if (has_aln_tag("pos")) {
        aln_extra = P.aln_tags.size() == 2 ? (uint32_t)int_type_bytes(P.aln_tags[1].type) : 0u;
        if (P.aln_tags.size() != 2 || P.aln_tags[0].name != "compressed_ori_refid" || P.aln_tags[0].type != 3 || P.aln_tags[1].name != "pos" || !aln_extra)
            return hfail(AFQ_ERR_UNSUPPORTED, "RAD records with positions: the alignment-level tags must be compressed_ori_refid:u32 followed by pos, an integer of 1, 2, 4 or 8 bytes");
    } else if (has_aln_tag("type") && has_aln_tag("start_pos") && has_aln_tag("frag_len")) {
        return hfail(AFQ_ERR_UNSUPPORTED, "To process atac-seq data, you should use the \"atac\" sub-command");   // quant.rs:1973-1976
    }
    uint32_t w_sample = 0, w_b0 = 0, w_b1 = 0, cblen = 0, bc_split = 0;
    if (multi_bc) {
        if (P.file_tag_vals["num_barcodes"] != 2 || P.read_tags.size() != 3 || P.read_tags[0].name != "b0" || P.read_tags[1].name != "b1" || P.read_tags[2].name != "u")
            return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode RAD: only two barcode levels with read tags (b0, b1, u) are supported");
        const uint32_t w0 = (uint32_t)int_type_bytes(P.read_tags[0].type), w1 = (uint32_t)int_type_bytes(P.read_tags[1].type);
        P.umi_bytes = (uint32_t)int_type_bytes(P.read_tags[2].type);
        if (!w0 || !w1 || w0 > 4 || w1 > 4 || !P.umi_bytes) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode RAD: b0 and b1 must be integers of 1, 2 or 4 bytes (u8/u16/u32)");
        // A RAD writer picks the narrowest integer per barcode length (an 8-nt sample barcode is a u16, a 16-nt cell barcode a
        // u32): unequal widths go to the library as a split barcode field, which it rewrites with two dwords (afq_config.bc_split)
        P.bc_bytes = w0 + w1; w_b0 = w0; w_b1 = w1;
        if (w0 != w1) { bc_split = w0; w_sample = 4; } else w_sample = w0;
        if (!P.file_tag_vals.count("b1len")) return hfail(AFQ_ERR_BAD_INPUT, "multi-barcode RAD file should have a \"b1len\" file-level tag");
        cblen = (uint32_t)P.file_tag_vals["b1len"];
    } else {
        if (!P.bc_bytes || !P.umi_bytes) return hfail(AFQ_ERR_UNSUPPORTED, "RAD read tags must hold integer 'b' and 'u' (single-barcode records)");
        // the device decoders walk `na, b, u, na x u32` records (src/convert.rs:124-144): any other tag layout would be misread, not skipped
        if (P.read_tags.size() != 2 || P.read_tags[0].name != "b" || P.read_tags[1].name != "u")
            return hfail(AFQ_ERR_UNSUPPORTED, "RAD read-level tags other than (b, u) are not supported");
        if (P.file_tag_vals.count("cblen")) cblen = (uint32_t)P.file_tag_vals["cblen"];
        else return hfail(AFQ_ERR_UNSUPPORTED, "no cblen file tag");
    }
    if (!aln_extra && (P.aln_tags.size() != 1 || P.aln_tags[0].type != 3))
        return hfail(AFQ_ERR_UNSUPPORTED, "RAD alignment-level tags other than one u32 (compressed_ori_refid), alone or followed by pos, are not supported");
    std::vector<std::string> sample_names;   // multi-barcode: name of sample i (src/quant.rs:1354-1373)
    bool have_samples = false;
    if (file_exists(in + "/collation_manifest.bin")) {
        std::vector<uint8_t> mb;
        if (!read_file(in + "/collation_manifest.bin", mb) || !parse_collation_manifest(mb, sample_names))
            return hfail(AFQ_ERR_UNSUPPORTED, "collation_manifest.bin is not in the layout this build reads (bincode of CollationManifest; see afq_host.cpp)");
        have_samples = true;
    }
    // chunk table: hop the nbytes headers (what the producer thread does; a record is at least its header, whatever its
    // alignments hold - the library checks that they tile the chunk)
    const uint32_t rec_hdr = 4 + P.bc_bytes + P.umi_bytes;
    std::vector<uint64_t> chunk_off, chunk_nb;
    std::vector<uint32_t> chunk_nr;
    CtxPtr sz_ctx;    // resident: the context that decoded the file and holds its bytes until the workers are done
    SzResident Z;
    if (resident) {
        if (warm.joinable()) warm.join();
        if (int rc2 = open_fill_ctx((uint32_t)first_device, 0, sz_ctx)) return rc2;   // (the workers' device: `--devices 1` names it, not `--device`)
        if (int rc2 = sz_decode_resident(sz_ctx.get(), mf.p, mf.n, P.first_chunk, rec_hdr, Z, pc)) return rc2;
        chunk_off.swap(Z.chunk_off); chunk_nb.swap(Z.chunk_nb); chunk_nr.swap(Z.chunk_nr);
    } else
    for (size_t p = P.first_chunk; p < rad.size();) {
        if (p + 8 > rad.size()) return hfail(AFQ_ERR_BAD_INPUT, "trailing bytes after the last chunk");
        uint32_t nb, nr; std::memcpy(&nb, rad.data() + p, 4); std::memcpy(&nr, rad.data() + p + 4, 4);
        if (nb < 8 || p + nb > rad.size()) return hfail(AFQ_ERR_BAD_INPUT, "corrupt chunk header");
        if (nr == 0 || nb < 8 + rec_hdr) return hfail(AFQ_ERR_BAD_INPUT, "chunk " + std::to_string(chunk_off.size()) + " holds no record");   // (quant.rs:756 panics)
        chunk_off.push_back(p); chunk_nb.push_back(nb); chunk_nr.push_back(nr); p += nb;
    }
    // Two layouts of one multi-barcode pair.  The key the LIBRARY REPORTS holds b0 in its low w_sample bytes and b1 above them
    // (unequal widths: after the library's rewrite, b1 << 32 | b0).  The BYTES OF THE FILE hold b0 in w_b0 bytes and b1 in the
    // w_b1 bytes behind them, whatever the widths.  cell_key_of takes a reported key and nothing else; file_cell_key_of reads the
    // record's barcode field itself, so that no caller shifts one layout by the other's width.
    auto cell_key_of = [&](uint64_t reported_bc) -> uint64_t { return multi_bc ? reported_bc >> (8 * w_sample) : reported_bc; };
    auto file_cell_key_of = [&](const uint8_t* bc_field) -> uint64_t {
        uint64_t v = 0;
        if (!multi_bc) { std::memcpy(&v, bc_field, P.bc_bytes); return v; }
        std::memcpy(&v, bc_field + w_b0, w_b1);
        return v;
    };
    // --quant-subset (src/quant.rs:1523-1536, 1776): the first record's collate key decides
    size_t subset_size = 0;
    if (o->filter_list) {
        std::ifstream f(o->filter_list);
        if (!f) return hfail(AFQ_ERR_BAD_INPUT, "could not read the --quant-subset file");
        std::unordered_set<uint64_t> keep; std::string line;
        while (std::getline(f, line)) { while (!line.empty() && std::isspace((unsigned char)line.back())) line.pop_back(); uint64_t v; if (!line.empty() && string_to_bc(line, v)) keep.insert(v); }
        subset_size = keep.size();
        std::vector<uint64_t> kept, kept_nb;
        std::vector<uint32_t> kept_nr;
        // (resident: the first record's barcode field as the device's hop read it)
        for (size_t i = 0; i < chunk_off.size(); ++i) { if (keep.count(file_cell_key_of(resident ? reinterpret_cast<const uint8_t*>(&Z.first_bc[i]) : rad.data() + chunk_off[i] + 8 + 4))) { kept.push_back(chunk_off[i]); kept_nb.push_back(chunk_nb[i]); kept_nr.push_back(chunk_nr[i]); } }
        chunk_off.swap(kept); chunk_nb.swap(kept_nb); chunk_nr.swap(kept_nr);
    }
    // transcript-to-gene map (src/utils.rs:487-662)
    std::unordered_map<std::string, uint32_t> rname_to_id;
    for (uint32_t i = 0; i < P.ref_names.size(); ++i) rname_to_id[P.ref_names[i]] = i;
    std::vector<uint32_t> t2g(P.ref_count, UINT32_MAX);
    std::vector<std::string> gene_names; std::unordered_map<std::string, uint32_t> gene_id;
    bool usa = false; size_t found = 0;
    {
        std::ifstream f(o->tg_map);
        if (!f) return hfail(AFQ_ERR_BAD_INPUT, "couldn't open the transcript-to-gene map");
        std::string line; int ncol = -1; uint32_t next_gid = 0;
        while (std::getline(f, line)) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty()) continue;
            std::vector<std::string> col; { std::stringstream ss(line); std::string c2; while (std::getline(ss, c2, '\t')) col.push_back(c2); }
            if (ncol < 0) { ncol = (int)col.size(); if (ncol != 2 && ncol != 3) return hfail(AFQ_ERR_BAD_INPUT, "Transcript-gene mapping must have either 2 or 3 columns."); usa = ncol == 3; }
            if ((int)col.size() != ncol) return hfail(AFQ_ERR_BAD_INPUT, "failed to parse the transcript-to-gene map : ragged row");
            uint32_t gid;
            auto it = gene_id.find(col[1]);
            if (it == gene_id.end()) { gid = usa ? next_gid : (uint32_t)gene_names.size(); next_gid += 2; gene_id.emplace(col[1], gid); gene_names.push_back(col[1]); }
            else gid = it->second;
            auto rt = rname_to_id.find(col[0]);
            if (rt == rname_to_id.end()) continue;
            ++found;
            if (!usa) t2g[rt->second] = gid;
            else if (col[2] == "U" || col[2] == "u") t2g[rt->second] = gid + 1;
            else if (col[2] == "S" || col[2] == "s") t2g[rt->second] = gid;
            else return hfail(AFQ_ERR_BAD_INPUT, "Third column in 3 column txp-to-gene file must be S or U");
        }
    }
    if (found != P.ref_count) return hfail(AFQ_ERR_BAD_INPUT, "The tg-map must contain a gene mapping for all transcripts in the header");
    const uint32_t G = (uint32_t)gene_names.size();
    afq_config cfg{};
    cfg.abi_version = AFQ_ABI_VERSION; cfg.resolution = R->id; cfg.usa_mode = usa;
    if (o->sa_model > AFQ_SA_PREFER_AMBIG) return hfail(AFQ_ERR_INVALID_ARG, "unknown sa_model");
    cfg.sa_model = o->sa_model;
    if (!usa && cfg.sa_model != AFQ_SA_WINNER_TAKE_ALL) {   // src/quant.rs:1456-1469
        std::fprintf(stderr, "When not operating in USA-mode (all-in-one unspliced/spliced/ambiguous), the SplicedAmbiguityModel will be ignored.\n");
        cfg.sa_model = AFQ_SA_WINNER_TAKE_ALL;
    }
    cfg.num_genes = usa ? 2 * G : G; cfg.num_rows = usa ? 3 * G : G;  // src/quant.rs:1627-1645
    cfg.small_thresh = o->small_thresh; cfg.large_graph_thresh = large_thresh; cfg.pug_exact_umi = (R->pars && edist == 0) ? 1 : 0;
    cfg.em_init_uniform = o->init_uniform; cfg.bc_bytes = P.bc_bytes; cfg.bc_split = bc_split; cfg.umi_bytes = P.umi_bytes; { const uint64_t ul = P.file_tag_vals.count("ulen") ? P.file_tag_vals["ulen"] : 0; cfg.umi_len = ul <= 4ull * P.umi_bytes ? (uint32_t)ul : 0u; }
    // -d: the device keeps the gene-level classes only in the -em resolutions (there they are the EM's input); a plain
    // resolution leaves the same classes behind as its -em sibling (same resolution step, different count extraction:
    // quant.rs:882-924, 966-1019), so for it a second context runs the sibling for the classes alone.  `trivial` never
    // fills gene_eqc: every cell reports no classes.
    const bool res_is_em = cfg.resolution == AFQ_RES_CR_LIKE_EM || cfg.resolution == AFQ_RES_PARSIMONY_EM || cfg.resolution == AFQ_RES_PARSIMONY_GENE_EM;
    cfg.num_bootstraps = o->num_bootstraps; cfg.summary_stat = o->summary_stat; cfg.boot_seed = o->boot_seed;
    afq_config cfg_eq = cfg;
    if (o->dump_eq) {
        if (res_is_em) cfg.dump_eq = 1;
        else if (cfg.resolution != AFQ_RES_TRIVIAL) {
            cfg_eq.dump_eq = 1;
            cfg_eq.resolution = cfg.resolution == AFQ_RES_CR_LIKE ? AFQ_RES_CR_LIKE_EM : cfg.resolution == AFQ_RES_PARSIMONY ? AFQ_RES_PARSIMONY_EM : AFQ_RES_PARSIMONY_GENE_EM;
        }
    }

    // Unmapped reads per corrected barcode (quant.rs:1484-1494; only CorrectedReads / MappingRate of featureDump use
    // them).  Any failure to read the file means "no unmapped reads", as in the reference.  The layout read here is
    // the bincode HashMap<u64, u32> one (count:u64, then key:u64 value:u32 pairs - atac/collate.rs:258-282 writes it);
    // the self-describing layout of libradicl 0.18's CollatedUnmappedCounts is not witnessed anywhere under the
    // reference tree, so a file that does not tile as the former is reported and ignored.
    std::unordered_map<uint64_t, uint32_t> unmapped;
    {
        std::vector<uint8_t> ub;
        if (read_file(in + "/unmapped_bc_count_collated.bin", ub)) {
            uint64_t n = 0;
            if (ub.size() >= 8) std::memcpy(&n, ub.data(), 8);
            if (ub.size() >= 8 && n <= (ub.size() - 8) / 12 && ub.size() == 8 + 12 * n) {
                unmapped.reserve((size_t)n);
                for (uint64_t i = 0; i < n; ++i) {
                    uint64_t k; uint32_t v;
                    std::memcpy(&k, ub.data() + 8 + 12 * i, 8); std::memcpy(&v, ub.data() + 16 + 12 * i, 4);
                    unmapped[k] += v;
                }
            } else if (!ub.empty())
                std::fprintf(stderr, "unmapped_bc_count_collated.bin is not in the (count, key/value pairs) layout; unmapped reads are taken as 0\n");
        }
    }

    // ---- the device work: the worker fan-out of do_quantify (quant.rs:1553-1575, 1678-1765) becomes one context and one
    // host thread per device over a contiguous, byte-balanced range of cells; no device talks to another ----
    pc.lap("prelude, chunk table, tg-map");
    if (warm.joinable()) warm.join();
    pc.lap("(wait for the HIP runtime)");
    std::vector<int> devices;
    if (o->devices && o->n_devices) devices.assign(o->devices, o->devices + o->n_devices); else devices.push_back((int)o->device);
    if (resident && devices[0] != first_device) return hfail(AFQ_ERR_STATE, "--sz-on-device: the decoded file lies on device " + std::to_string(first_device) + ", the workers run on device " + std::to_string(devices[0]));
    if (devices.size() > chunk_off.size() && !chunk_off.empty()) devices.resize(chunk_off.size());
    // The queue: contiguous batches of cells in file order (largest cells first, collate.rs:272-274).  One device: as large
    // as memory allows (batch_bytes).  Several: about eight batches per device, so that the devices finish together whatever
    // the cells cost (a parsimony cell's time grows faster than its bytes; static byte-balanced cuts gave the first device all
    // the giant cells) - every device thread pops the next batch when it has finished its last.
    const uint64_t batch_cap = o->batch_bytes ? o->batch_bytes : (16ull << 30);
    uint64_t total_bytes = 0;
    for (uint64_t nb : chunk_nb) total_bytes += nb;
    uint64_t batch_bytes = batch_cap;
    if (devices.size() > 1) batch_bytes = std::min<uint64_t>(batch_cap, std::max<uint64_t>(total_bytes / (8 * devices.size()) + 1, 32ull << 20));
    if (const char* e = afq::test_hook("QUEUE_BATCH_BYTES")) batch_bytes = std::max<uint64_t>(1, (uint64_t)std::atof(e));   // tests: many small batches
    std::vector<std::pair<size_t, size_t>> batches;
    for (size_t c0 = 0; c0 < chunk_off.size();) {
        size_t c1 = c0; uint64_t bytes = 0;
        while (c1 < chunk_off.size()) { const uint64_t nb = chunk_nb[c1]; if (c1 > c0 && bytes + nb > batch_bytes) break; bytes += nb; ++c1; }
        batches.emplace_back(c0, c1);
        c0 = c1;
    }
    if (devices.size() > batches.size() && !batches.empty()) devices.resize(batches.size());
    std::vector<DevOut> parts(batches.size());
    std::vector<DevStat> dstat(devices.size());
    {
        std::atomic<size_t> next{0};
        std::atomic<int> stop{0};
        auto work = [&](size_t d) {
            run_device_worker(cfg, cfg_eq.dump_eq ? &cfg_eq : nullptr, aln_extra, t2g, devices[d], devices.size() > 1, rad.data(), compressed ? -1 : mf.fd, resident ? Z.d_rad : nullptr, chunk_off, chunk_nb, chunk_nr,
                              batches, next, stop, o->dump_eq != 0, res_is_em, parts, dstat[d]);
        };
        if (devices.size() == 1) work(0);
        else {
            std::vector<std::thread> th;
            for (size_t d = 0; d < devices.size(); ++d) th.emplace_back(work, d);
            for (auto& x : th) x.join();
        }
    }
    for (size_t d = 0; d < dstat.size(); ++d)
        if (dstat[d].rc) return hfail(dstat[d].rc, (devices.size() > 1 ? "device " + std::to_string(devices[d]) + ": " : std::string()) + dstat[d].err);
    if (pc.on) for (size_t d = 0; d < dstat.size(); ++d)
        std::fprintf(stderr, "[afquant]   device %d: %u batches, %llu cells, %.3f GB, busy %.3f s\n", devices[d], dstat[d].batches, (unsigned long long)dstat[d].cells, (double)dstat[d].bytes / 1e9, dstat[d].busy_s);
    if (devices.size() > 1) {   // how the queue spread the work: a small extra file next to quant.json (not one of the reference's outputs)
        (void)mkdirs_checked(outd);   // (the writers create it further down; this file comes first)
        FilePtr df(std::fopen((outd + "/afquant_devices.json").c_str(), "w"));
        if (df) {
            std::fprintf(df.get(), "{\n  \"batches\": %zu,\n  \"batch_bytes\": %llu,\n  \"devices\": [\n", batches.size(), (unsigned long long)batch_bytes);
            for (size_t d = 0; d < dstat.size(); ++d)
                std::fprintf(df.get(), "    {\"device\": %d, \"batches\": %u, \"cells\": %llu, \"bytes\": %llu, \"busy_s\": %.6f}%s\n", devices[d], dstat[d].batches,
                             (unsigned long long)dstat[d].cells, (unsigned long long)dstat[d].bytes, dstat[d].busy_s, d + 1 < dstat.size() ? "," : "");
            std::fprintf(df.get(), "  ]\n}\n");
        }
    }
    pc.lap("device batches");

    // ---- host-side gather in cell order (the only communication the path has) ----
    const uint64_t row_index = chunk_off.size();
    std::vector<uint32_t> all_gene; std::vector<float> all_val;
    std::vector<uint64_t> row_ptr(1, 0), bc_all; std::vector<uint32_t> nrec_all; std::vector<uint8_t> flags_all;
    std::map<std::vector<uint32_t>, uint32_t> eq_ids;          // global_eqc: gene set -> class id, ids in order of first appearance
    std::vector<uint32_t> eq_col, eq_cnt;                       // cell_level_count
    std::vector<uint64_t> eq_row_ptr(1, 0);                     // cell_offset
    std::vector<uint32_t> bm_col, bv_col; std::vector<float> bm_val, bv_val;   // BootstrapHelper's mean / variance triplets, as CSR
    std::vector<uint64_t> bm_ptr(1, 0), bv_ptr(1, 0);
    auto part_nnz = [](const DevOut& d) -> size_t { return d.is_held ? (size_t)d.held.nnz : d.gene.size(); };
    const bool one_held = parts.size() == 1 && parts[0].is_held;
    if (parts.size() == 1) { all_gene.swap(parts[0].gene); all_val.swap(parts[0].val); }
    else {
        size_t tot = 0;
        for (auto& p2 : parts) tot += part_nnz(p2);
        all_gene.reserve(tot); all_val.reserve(tot);
    }
    row_ptr.reserve(row_index + 1); bc_all.reserve(row_index); nrec_all.reserve(row_index); flags_all.reserve(row_index);
    for (auto& p2 : parts) {
        const uint64_t g0 = row_ptr.back();
        if (parts.size() > 1) {
            if (p2.is_held) { all_gene.insert(all_gene.end(), p2.held.gene, p2.held.gene + p2.held.nnz); all_val.insert(all_val.end(), p2.held.val, p2.held.val + p2.held.nnz); }
            else { all_gene.insert(all_gene.end(), p2.gene.begin(), p2.gene.end()); all_val.insert(all_val.end(), p2.val.begin(), p2.val.end()); std::vector<uint32_t>().swap(p2.gene); std::vector<float>().swap(p2.val); }
        }
        for (uint64_t e : p2.row_end) row_ptr.push_back(g0 + e);
        bc_all.insert(bc_all.end(), p2.bc.begin(), p2.bc.end());
        nrec_all.insert(nrec_all.end(), p2.nrec.begin(), p2.nrec.end());
        flags_all.insert(flags_all.end(), p2.flags.begin(), p2.flags.end());
        if (o->num_bootstraps && !p2.bm_end.empty()) {
            const uint64_t m0 = bm_col.size(), v0 = bv_col.size();
            bm_col.insert(bm_col.end(), p2.bm_col.begin(), p2.bm_col.end()); bm_val.insert(bm_val.end(), p2.bm_val.begin(), p2.bm_val.end());
            bv_col.insert(bv_col.end(), p2.bv_col.begin(), p2.bv_col.end()); bv_val.insert(bv_val.end(), p2.bv_val.begin(), p2.bv_val.end());
            for (size_t i = 0; i < p2.bm_end.size(); ++i) { bm_ptr.push_back(m0 + p2.bm_end[i]); bv_ptr.push_back(v0 + p2.bv_end[i]); }
        }
        if (o->dump_eq) {   // the global dictionary is filled in cell order (quant.rs:1282-1307), so that ids do not depend on the device count
            std::vector<uint32_t> key;
            uint64_t k = 0;
            for (size_t i = 0; i < p2.eq_cell_end.size(); ++i) {
                for (; k < p2.eq_cell_end[i]; ++k) {
                    const uint64_t w0 = k ? p2.eq_label_end[k - 1] : 0, w1 = p2.eq_label_end[k];
                    key.assign(p2.eq_labels.begin() + (ptrdiff_t)w0, p2.eq_labels.begin() + (ptrdiff_t)w1);
                    auto it = eq_ids.find(key);
                    if (it == eq_ids.end()) it = eq_ids.emplace(key, (uint32_t)eq_ids.size()).first;
                    eq_col.push_back(it->second); eq_cnt.push_back(p2.eq_count[k]);
                }
                eq_row_ptr.push_back(eq_col.size());
            }
        }
    }
    if (bc_all.size() != row_index) return hfail(AFQ_ERR_STATE, "internal: the devices returned a different number of cells than were submitted");
    struct HeldResult { afq_result r{}; ~HeldResult() { afq_result_release(&r); } } keep;   // (a result outlives its context)
    if (one_held) { keep.r = parts[0].held; parts[0].is_held = false; }
    const uint32_t* const GG = one_held ? keep.r.gene : all_gene.data();
    const float* const V = one_held ? keep.r.val : all_val.data();
    parts.clear();

    // ---- per-cell rows: quants_mat_rows.txt + featureDump.txt (src/quant.rs:1150-1262), formatted by -t threads over
    // contiguous runs of cells and written in order ----
    if (mkdirs_checked(outd + "/alevin")) return hfail(AFQ_ERR_BAD_INPUT, "could not create the output directory " + outd + "/alevin");
    FilePtr rows_f(std::fopen((outd + "/alevin/quants_mat_rows.txt").c_str(), "w"));
    FilePtr feat_f(std::fopen((outd + "/featureDump.txt").c_str(), "w"));
    FilePtr cols_f(std::fopen((outd + "/alevin/quants_mat_cols.txt").c_str(), "w"));
    if (!rows_f || !feat_f || !cols_f) return hfail(AFQ_ERR_BAD_INPUT, "could not create the output files");
    const bool sample_cols = multi_bc && have_samples;   // sample-prefixed row labels + the sample_name column (quant.rs:1217-1262)
    std::fputs(have_samples ?   // the header goes by the manifest alone (quant.rs:1603-1613)
 "CB\tsample_name\tCorrectedReads\tMappedReads\tDeduplicatedReads\tMappingRate\tDedupRate\tMeanByMax\tNumGenesExpressed\tNumGenesOverMean\n"
                           : "CB\tCorrectedReads\tMappedReads\tDeduplicatedReads\tMappingRate\tDedupRate\tMeanByMax\tNumGenesExpressed\tNumGenesOverMean\n", feat_f.get());
    for (auto& g : gene_names) std::fprintf(cols_f.get(), "%s\n", g.c_str());
    if (usa) { for (auto& g : gene_names) std::fprintf(cols_f.get(), "%s-U\n", g.c_str()); for (auto& g : gene_names) std::fprintf(cols_f.get(), "%s-A\n", g.c_str()); }
    cols_f.reset();
    std::vector<uint64_t> alt_cells, empty_cells, tiny_cells;
    uint64_t total_records = 0;
    {
        const unsigned nth = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)(o->num_threads ? o->num_threads : std::thread::hardware_concurrency()), 64, row_index / 256 + 1}));
        std::vector<std::string> rows_txt(nth), feat_txt(nth);
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nth; ++t)
            th.emplace_back([&, t]() {
                const uint64_t i0 = row_index * t / nth, i1 = row_index * (t + 1) / nth;
                std::string &rt = rows_txt[t], &ft = feat_txt[t];
                char num[64];
                for (uint64_t i = i0; i < i1; ++i) {
                    const uint64_t a = row_ptr[i], b = row_ptr[i + 1];
                    float sum = 0.0f, mx = 0.0f;  // src/quant.rs:1150-1171 (f32 sum in column order)
                    for (uint64_t k = a; k < b; ++k) { sum += V[k]; if (V[k] > mx) mx = V[k]; }
                    const uint32_t num_expr = (uint32_t)(b - a);
                    const uint32_t nrec = nrec_all[i];
                    const float dedup_rate = sum / (float)nrec;
                    const uint64_t cell_bc = cell_key_of(bc_all[i]);
                    uint64_t num_unmapped = 0;
                    if (!unmapped.empty()) { auto it = unmapped.find(cell_bc); if (it != unmapped.end()) num_unmapped = it->second; }
                    const float mapping_rate = (float)nrec / (float)(nrec + num_unmapped);
                    const float mean_expr = sum / (float)num_expr;
                    uint32_t over = 0;
                    for (uint64_t k = a; k < b; ++k) if (V[k] > mean_expr) ++over;
                    const float mean_by_max = mean_expr / mx;
                    const std::string bcs = bc_to_string(cell_bc, cblen);
                    const std::string* sn = nullptr;
                    if (sample_cols) { const uint64_t si = bc_all[i] & ((1ull << (8 * w_sample)) - 1); if (si < sample_names.size()) sn = &sample_names[(size_t)si]; }
                    if (sn) { rt += *sn; rt += '_'; }
                    rt += bcs; rt += '\n';
                    ft += bcs; ft += '\t';
                    if (sn) { ft += *sn; ft += '\t'; }
                    *put_u64(num, (unsigned long long)(nrec + num_unmapped)) = 0; ft += num; ft += '\t';
                    *put_u64(num, nrec) = 0; ft += num; ft += '\t';
                    format_f32(sum, num, sizeof num); ft += num; ft += '\t';
                    format_f32(mapping_rate, num, sizeof num); ft += num; ft += '\t';
                    format_f32(dedup_rate, num, sizeof num); ft += num; ft += '\t';
                    format_f32(mean_by_max, num, sizeof num); ft += num; ft += '\t';
                    *put_u64(num, num_expr) = 0; ft += num; ft += '\t';
                    *put_u64(num, over) = 0; ft += num; ft += '\n';
                }
            });
        for (auto& x : th) x.join();
        for (unsigned t = 0; t < nth; ++t) {
            std::fwrite(rows_txt[t].data(), 1, rows_txt[t].size(), rows_f.get());
            std::fwrite(feat_txt[t].data(), 1, feat_txt[t].size(), feat_f.get());
        }
        for (uint64_t i = 0; i < row_index; ++i) {
            if (flags_all[i] & AFQ_CELL_ALT_RES) alt_cells.push_back(i);
            if (flags_all[i] & AFQ_CELL_EMPTY) empty_cells.push_back(i);
            if (flags_all[i] & AFQ_CELL_TINY_PATH) tiny_cells.push_back(i);
            total_records += nrec_all[i];
        }
    }
    rows_f.reset(); feat_f.reset();
    pc.lap("gather + per-cell rows");
    // With --quant-subset the reference sizes the matrix (and reports num_quantified_cells) by the SUBSET's size, whether or
    // not every listed barcode occurs in the file (quant.rs:1529, 1836, 1918); rows exist only for the cells found.
    const uint64_t num_cells = o->filter_list ? (uint64_t)subset_size : row_index;
    auto write_mtx = [&](const std::string& path, uint64_t n_rows, uint64_t n_cols, const std::vector<uint64_t>& rp,
                         const std::vector<uint32_t>& cols, const std::vector<float>& vals) -> bool {
        return write_mtx_file(path, n_rows, n_cols, rp, cols.data(), vals.data(), vals.size(), o->num_threads);
    };
    if (!write_mtx_file(outd + "/alevin/quants_mat.mtx", num_cells, cfg.num_rows, row_ptr, GG, V, (size_t)row_ptr.back(), o->num_threads)) return hfail(AFQ_ERR_BAD_INPUT, "could not create quants_mat.mtx");
    pc.lap("quants_mat.mtx");
    // -b: bootstrap summary matrices, cells x num_rows (src/quant.rs:1850-1877; nothing is written when no cell had a bootstrap)
    if (o->num_bootstraps && !bm_val.empty()) {
        if (!write_mtx(outd + "/alevin/bootstraps_mean.mtx", num_cells, cfg.num_rows, bm_ptr, bm_col, bm_val) ||
            !write_mtx(outd + "/alevin/bootstraps_var.mtx", num_cells, cfg.num_rows, bv_ptr, bv_col, bv_val))
            return hfail(AFQ_ERR_BAD_INPUT, "could not write the bootstrap matrices");
        pc.lap("bootstraps_mean.mtx + bootstraps_var.mtx");
    }
    // -d: cells x gene-level equivalence classes + the classes' gene sets (write_eqc_counts, src/quant.rs:229-355)
    if (o->dump_eq) {
        std::vector<float> ev(eq_cnt.begin(), eq_cnt.end());
        if (!write_mtx(outd + "/alevin/geqc_counts.mtx", eq_row_ptr.size() - 1 /* the cells processed: geqmap.cell_offset.len(), quant.rs:248-251 */, eq_ids.size(), eq_row_ptr, eq_col, ev)) return hfail(AFQ_ERR_BAD_INPUT, "could not write geqc_counts.mtx");
        std::vector<const std::vector<uint32_t>*> by_id(eq_ids.size());
        for (auto& kv : eq_ids) by_id[kv.second] = &kv.first;
        std::string txt = std::to_string(cfg.num_rows) + "\n" + std::to_string(eq_ids.size()) + "\n";
        const uint32_t uo = cfg.num_rows / 3, ao = 2 * uo;
        for (size_t id = 0; id < by_id.size(); ++id) {
            const std::vector<uint32_t>& gl = *by_id[id];
            for (size_t k = 0; k < gl.size(); ++k) {
                uint32_t g = gl[k];
                if (usa) {   // S -> g/2, U -> g/2 + unspliced offset, S followed by its own U -> ambiguous (quant.rs:284-335)
                    if (k + 1 < gl.size() && (gl[k + 1] >> 1) == (g >> 1)) { g = (g >> 1) + ao; ++k; }
                    else g = (g & 1u) ? (g >> 1) + uo : (g >> 1);
                }
                txt += std::to_string(g); txt += '\t';
            }
            txt += std::to_string(id); txt += '\n';
        }
        gzFile gz = gzopen((outd + "/alevin/gene_eqclass.txt.gz").c_str(), "wb");
        if (!gz) return hfail(AFQ_ERR_BAD_INPUT, "could not write gene_eqclass.txt.gz");
        for (size_t off = 0; off < txt.size();) { const unsigned len = (unsigned)std::min<size_t>(txt.size() - off, 1u << 30); if (gzwrite(gz, txt.data() + off, len) <= 0) { gzclose(gz); return hfail(AFQ_ERR_BAD_INPUT, "could not write gene_eqclass.txt.gz"); } off += len; }
        gzclose(gz);
        pc.lap("geqc_counts.mtx + gene_eqclass.txt.gz");
    }
    // quant.json (src/quant.rs:1913-1933)
    {
        FILE* j = std::fopen((outd + "/quant.json").c_str(), "w");
        if (!j) return hfail(AFQ_ERR_BAD_INPUT, "could not create quant.json");
        auto list = [&](const std::vector<uint64_t>& v) { std::string s = "["; for (size_t i = 0; i < v.size(); ++i) { if (i) s += ", "; s += std::to_string(v[i]); } return s + "]"; };
        std::fprintf(j, "{\n  \"cmd\": \"%s\",\n  \"version_str\": \"afquant-hip 0.1 (alevin-fry 0.18.0 quant semantics)\",\n  \"resolution_strategy\": \"%s\",\n",
                     json_escape(o->cmdline ? o->cmdline : "").c_str(), R->debug);
        std::fprintf(j, "  \"num_quantified_cells\": %llu,\n  \"num_genes\": %u,\n  \"dump_eq\": %s,\n  \"usa_mode\": %s,\n", (unsigned long long)num_cells, cfg.num_rows, o->dump_eq ? "true" : "false", usa ? "true" : "false");
        std::fprintf(j, "  \"alt_resolved_cell_numbers\": %s,\n  \"empty_resolved_cell_numbers\": %s,\n  \"num_tiny_cell_resolved\": %zu,\n  \"tiny_cell_resolved_cell_numbers\": %s,\n",
                     list(alt_cells).c_str(), list(empty_cells).c_str(), tiny_cells.size(), list(tiny_cells).c_str());
        std::fprintf(j, "  \"total_records\": %llu,\n  \"quant_options\": {\n    \"input_dir\": \"%s\",\n    \"tg_map\": \"%s\",\n    \"output_dir\": \"%s\",\n    \"num_threads\": %u,\n    \"num_bootstraps\": %u,\n    \"init_uniform\": %s,\n    \"summary_stat\": %s,\n    \"dump_eq\": %s,\n    \"resolution\": \"%s\",\n    \"pug_exact_umi\": %s,\n    \"sa_model\": \"%s\",\n    \"small_thresh\": %u,\n    \"large_graph_thresh\": %u,\n    \"filter_list\": %s%s%s,\n    \"cmdline\": \"%s\"\n  }\n}\n",
                     (unsigned long long)total_records, json_escape(in).c_str(), json_escape(o->tg_map).c_str(), json_escape(outd).c_str(), o->num_threads, o->num_bootstraps, o->init_uniform ? "true" : "false", o->summary_stat ? "true" : "false", o->dump_eq ? "true" : "false",
                     R->debug, cfg.pug_exact_umi ? "true" : "false", cfg.sa_model == AFQ_SA_PREFER_AMBIG ? "PreferAmbiguity" : "WinnerTakeAll", o->small_thresh, large_thresh, o->filter_list ? "\"" : "", o->filter_list ? json_escape(o->filter_list).c_str() : "null", o->filter_list ? "\"" : "",
                     json_escape(o->cmdline ? o->cmdline : "").c_str());
        std::fclose(j);
    }
    return 0;
}

namespace {
// the text of a barcode list file, plain or gzip (zlib reads both)
int read_list_text(const char* path, std::string& txt) {
    gzFile gz = gzopen(path, "rb");
    if (!gz) return hfail(AFQ_ERR_BAD_INPUT, std::string("couldn't open input barcode file. (") + path + ")");
    char buf[1 << 16];
    int got;
    while ((got = gzread(gz, buf, sizeof buf)) > 0) txt.append(buf, (size_t)got);
    gzclose(gz);
    if (got < 0) return hfail(AFQ_ERR_BAD_INPUT, std::string("couldn't read line from barcode file. (") + path + ")");
    return 0;
}
// a fill's ascending histogram into the running one, summing a barcode present in both
void merge_histogram(std::vector<uint64_t>& hbc, std::vector<uint64_t>& hcnt, const uint64_t* bc, const uint64_t* cnt, uint64_t n) {
    if (hbc.empty()) { hbc.assign(bc, bc + n); hcnt.assign(cnt, cnt + n); return; }
    std::vector<uint64_t> mb, mc;
    mb.reserve(hbc.size() + n); mc.reserve(hbc.size() + n);
    size_t i = 0, j = 0;
    while (i < hbc.size() || j < n) {
        if (j >= n || (i < hbc.size() && hbc[i] < bc[j])) { mb.push_back(hbc[i]); mc.push_back(hcnt[i]); ++i; }
        else if (i >= hbc.size() || bc[j] < hbc[i]) { mb.push_back(bc[j]); mc.push_back(cnt[j]); ++j; }
        else { mb.push_back(hbc[i]); mc.push_back(hcnt[i] + cnt[j]); ++i; ++j; }
    }
    hbc.swap(mb); hcnt.swap(mc);
}
// compile_distinct_observed_with_target_counts (barcode_correction.rs:539-603) of the observed histogram against the retained
// barcodes (both ascending): the plan's entries restricted to permitted targets, permit_freq's map, the eight stats
struct Freer3 { void *a, *b, *c; ~Freer3() { afq_free(a); afq_free(b); afq_free(c); } };   // three outputs of afq_gpl_correct
struct GplPlan {
    std::vector<uint64_t> plan_obs, plan_cor, freq_bc, freq_cnt;
    std::vector<uint8_t> permitted;   // [retained]: the target has an accepted observation
    afq_gpl_correction_stats cs{};
};
int compile_plan(afq_ctx* ctx, const std::vector<uint64_t>& hbc, const std::vector<uint64_t>& hcnt, const std::vector<uint64_t>& retained,
                 const std::vector<uint64_t>& ret_cnt, uint32_t cblen, uint32_t nbh, uint32_t frequency, uint64_t conf_num, uint64_t conf_den, GplPlan& out) {
    afq_gpl_correction_stats& cs = out.cs;
    std::vector<uint64_t>&plan_obs = out.plan_obs, &plan_cor = out.plan_cor, &freq_bc = out.freq_bc, &freq_cnt = out.freq_cnt;
    uint8_t* dec = nullptr; uint32_t* tgt = nullptr; uint64_t* tcount = nullptr;
    int rc = afq_gpl_correct(ctx, hbc.data(), hcnt.data(), hbc.size(), retained.data(), ret_cnt.data(), retained.size(), cblen, nbh, frequency, conf_num, conf_den, 1,
                             &dec, &tgt, &tcount, &cs);
    if (rc) return hfail(rc, afq_last_error(ctx));
    Freer3 fr3{dec, tgt, tcount};
    std::vector<uint8_t> has_obs(retained.size(), 0);
    std::vector<uint8_t>& permitted = out.permitted;
    permitted.assign(retained.size(), 0);
    for (size_t i = 0; i < hbc.size(); ++i) {
        if (tgt[i] == 0xFFFFFFFFu) continue;
        permitted[tgt[i]] = 1;   // (the target has an accepted observation: it is in permit_freq)
        if (dec[i] == 0) has_obs[tgt[i]] = 1;
    }
    {   // the observed entries and the identities of never-observed sources, merged in barcode order, restricted to permitted targets
        size_t r = 0;
        auto flush_sources = [&](uint64_t below, bool all) {
            for (; r < retained.size() && (all || retained[r] < below); ++r)
                if (!has_obs[r]) { ++cs.exact_distinct; if (permitted[r]) { plan_obs.push_back(retained[r]); plan_cor.push_back(retained[r]); } }
        };
        for (size_t i = 0; i < hbc.size(); ++i) {
            flush_sources(hbc[i], false);
            if (tgt[i] != 0xFFFFFFFFu && permitted[tgt[i]]) { plan_obs.push_back(hbc[i]); plan_cor.push_back(retained[tgt[i]]); }
        }
        flush_sources(0, true);
    }
    for (size_t r = 0; r < retained.size(); ++r) if (permitted[r]) { freq_bc.push_back(retained[r]); freq_cnt.push_back(tcount[r]); }
    return 0;
}
// compile_full_neighborhood (barcode_correction.rs:607-610) restricted to permitted targets: permit_map.bin of the filtered methods
int compile_full_map(afq_ctx* ctx, const std::vector<uint64_t>& retained, const std::vector<uint64_t>& ret_cnt, const std::vector<uint8_t>& permitted, uint32_t cblen,
                     uint32_t nbh, uint32_t frequency, uint64_t conf_num, uint64_t conf_den, std::vector<uint64_t>& map_obs, std::vector<uint64_t>& map_cor) {
    std::vector<uint64_t> theo;
    theo.reserve(retained.size() * (1 + 3ull * cblen + 8));
    for (uint64_t s : retained) { theo.push_back(s); afq::gplhost::gpl_push_neighbors(s, cblen, nbh == 1, theo); }
    std::sort(theo.begin(), theo.end());
    theo.erase(std::unique(theo.begin(), theo.end()), theo.end());
    const std::vector<uint64_t> zeros(theo.size(), 0);
    uint8_t* d2 = nullptr; uint32_t* t2 = nullptr; uint64_t* c2 = nullptr;
    const int rc = afq_gpl_correct(ctx, theo.data(), zeros.data(), theo.size(), retained.data(), ret_cnt.data(), retained.size(), cblen, nbh, frequency, conf_num, conf_den, 1,
                                   &d2, &t2, &c2, nullptr);
    if (rc) return hfail(rc, afq_last_error(ctx));
    Freer3 fr4{d2, t2, c2};
    for (size_t i = 0; i < theo.size(); ++i)
        if (t2[i] != 0xFFFFFFFFu && permitted[t2[i]]) { map_obs.push_back(theo[i]); map_cor.push_back(retained[t2[i]]); }
    return 0;
}
}  // namespace

// ---------------------------------------------------------------------------
// `alevin-fry generate-permit-list` (src/cellfilter.rs:369-780, 1686-1830, 2044-2335; src/barcode_correction.rs; src/knee_finding.rs)
// for single-barcode RNA RAD files: the record pass and the correction decisions run on the device (afq_gpl_hist_rad,
// afq_gpl_correct); the retained set, the neighbourhood list and the files are the host's.  All maps are written in ascending
// key order (the reference writes its hasher's order; readers take the files as maps).
int afq_gpl_parse_confidence(const char* text, uint64_t* num, uint64_t* den) {
    std::string e;
    const int r = afq::gplhost::parse_confidence(text, num, den, e);
    return r ? hfail(r, e) : 0;
}
int64_t afq_gpl_parse_barcode_list(const uint8_t* text, size_t n, int unfiltered, uint32_t barcode_len, uint64_t* out, size_t cap, uint32_t* first_len) {
    std::string e;
    const int64_t r = afq::gplhost::parse_barcode_list(text, n, unfiltered, barcode_len, out, cap, first_len, e);
    return r < 0 ? hfail((int)r, e) : r;
}
int64_t afq_gpl_knee(const uint64_t* freq, size_t n) {
    std::string e;
    const int64_t r = afq::gplhost::knee(freq, n, e);
    return r < 0 ? hfail((int)r, e) : r;
}
int64_t afq_gpl_select_retained(const uint64_t* bc, const uint64_t* count, size_t n, uint32_t method, uint64_t arg, uint64_t* out, size_t cap) {
    std::string e;
    const int64_t r = afq::gplhost::select_retained(bc, count, n, method, arg, out, cap, e);
    return r < 0 ? hfail((int)r, e) : r;
}
int afq_gpl_write_outputs(const afq_gpl_opts* o, const afq_gpl_tables* t) {
    std::string e;
    const int r = afq::gplhost::write_outputs(o, t, e);
    return r ? hfail(r, e) : 0;
}

int afq_generate_permit_list(const afq_gpl_opts* o) {
    if (!o || !o->input_dir || !o->output_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    if (o->expected_ori > 2) return hfail(AFQ_ERR_INVALID_ARG, "expected_ori must be 0 (both), 1 (fw) or 2 (rc)");
    if (o->method > AFQ_GPL_UNFILTERED) return hfail(AFQ_ERR_INVALID_ARG, "unknown filter method");
    if ((o->method == AFQ_GPL_VALID_BC || o->method == AFQ_GPL_UNFILTERED) && !o->list_file) return hfail(AFQ_ERR_INVALID_ARG, "the filter method needs a barcode list file");
    if (o->method == AFQ_GPL_UNFILTERED && o->min_reads < 1) return hfail(AFQ_ERR_INVALID_ARG, "min-reads < 1 is not supported, the value " + std::to_string(o->min_reads) + " was provided");
    if (o->neighborhood > 1) return hfail(AFQ_ERR_INVALID_ARG, "unknown barcode neighbourhood; expected hamming-1 or substitution-or-shift-1");
    uint64_t conf_num = 39, conf_den = 40;
    if (o->conf_den || o->conf_num) { std::string e; if (int rc = afq::gplhost::confidence_new(o->conf_num, o->conf_den, &conf_num, &conf_den, e)) return hfail(rc, e); }
    const std::string in = o->input_dir;
    if (!file_exists(in)) return hfail(AFQ_ERR_BAD_INPUT, "the input RAD path \"" + in + "\" does not exist");
    MappedFile mf;
    if (!mf.open(in + "/map.rad")) return hfail(AFQ_ERR_BAD_INPUT, "could not open input rad file");
    const uint8_t* rad = mf.p;
    const size_t rad_n = mf.n;
    RadPrelude P;
    int rc = parse_prelude(rad, rad_n, P, false);
    if (rc) return rc;
    auto has_tag = [](const std::vector<TagDesc>& v, const char* name) { for (auto& t : v) if (t.name == name) return true; return false; };
    if (P.file_tag_vals.count("num_barcodes") && P.file_tag_vals["num_barcodes"] > 1)
        return hfail(AFQ_ERR_UNSUPPORTED, "generate-permit-list: multi-barcode RAD files (--sample-bc-list input, num_barcodes > 1) are not supported");
    if (has_tag(P.aln_tags, "start_pos") || has_tag(P.aln_tags, "frag_len"))
        return hfail(AFQ_ERR_UNSUPPORTED, "generate-permit-list: this is a scATAC RAD file; `atac generate-permit-list` is not supported");
    if (P.read_tags.size() != 2 || P.read_tags[0].name != "b" || P.read_tags[1].name != "u" || !P.bc_bytes || !P.umi_bytes)
        return hfail(AFQ_ERR_UNSUPPORTED, "generate-permit-list: the read-level tags must be the integers (b, u)");
    uint32_t aln_extra = 0;
    if (P.aln_tags.size() == 2 && P.aln_tags[1].name == "pos") aln_extra = (uint32_t)int_type_bytes(P.aln_tags[1].type);
    if (P.aln_tags.empty() || P.aln_tags[0].type != 3 || (P.aln_tags.size() == 2 && !aln_extra) || P.aln_tags.size() > 2)
        return hfail(AFQ_ERR_UNSUPPORTED, "generate-permit-list: the alignment-level tags must be one u32 (ref | orientation), optionally followed by an integer pos");
    if (!P.file_tag_vals.count("cblen")) return hfail(AFQ_ERR_BAD_INPUT, "tag map must contain cblen");
    const uint32_t cblen = (uint32_t)P.file_tag_vals["cblen"];
    if (cblen < 1 || cblen > 32) return hfail(AFQ_ERR_BAD_INPUT, "barcode length must be between 1 and 32 (got " + std::to_string(cblen) + ")");
    // ---- the barcode list of -b / -u (plain text or gzip: zlib reads both)
    std::vector<uint64_t> listed;
    if (o->method == AFQ_GPL_VALID_BC || o->method == AFQ_GPL_UNFILTERED) {
        std::string txt;
        if (int rc2 = read_list_text(o->list_file, txt)) return rc2;
        uint32_t first_len = 0;
        const int unf = o->method == AFQ_GPL_UNFILTERED;
        const int64_t n = afq_gpl_parse_barcode_list((const uint8_t*)txt.data(), txt.size(), unf, cblen, nullptr, 0, &first_len);
        if (n < 0) return (int)n;
        listed.resize((size_t)n);
        afq_gpl_parse_barcode_list((const uint8_t*)txt.data(), txt.size(), unf, cblen, listed.data(), listed.size(), nullptr);
        std::sort(listed.begin(), listed.end());
        listed.erase(std::unique(listed.begin(), listed.end()), listed.end());
        if (unf && first_len != cblen)
            std::fprintf(stderr, "The provided permit list had barcodes of length %u, but the mapped reads have barcodes of length %u\n", first_len, cblen);
        if (unf) for (uint64_t b : listed) if (cblen < 32 && b >= (1ull << (2 * cblen))) return hfail(AFQ_ERR_BAD_INPUT, "packed barcode " + std::to_string(b) + " does not fit declared length " + std::to_string(cblen));
    }
    // ---- the chunk table
    std::vector<uint64_t> chunk_off;
    if (int rc2 = walk_chunk_offsets(rad, rad_n, P.first_chunk, P.num_chunks, chunk_off)) return rc2;
    CtxPtr ctx;
    if (int rc2 = open_fill_ctx(o->device, aln_extra, ctx)) return rc2;
    // ---- the record pass: one device fill per run of chunks of at most fill_bytes, the sorted histograms merged
    const uint64_t fill_bytes = o->fill_bytes ? o->fill_bytes : (8ull << 30);
    std::vector<uint64_t> hbc, hcnt;
    uint64_t n_records = 0, n_compat = 0, max_ambig = 0;
    for (size_t c0 = 0; c0 < chunk_off.size();) {
        size_t c1 = c0;
        uint64_t nrec_sum = 0;
        auto chunk_end = [&](size_t i) { uint32_t nb; std::memcpy(&nb, rad + chunk_off[i], 4); return chunk_off[i] + nb; };
        while (c1 < chunk_off.size()) {
            uint32_t nr; std::memcpy(&nr, rad + chunk_off[c1] + 4, 4);
            if (c1 > c0 && (chunk_end(c1) - chunk_off[c0] > fill_bytes || nrec_sum + nr >= (1ull << 30))) break;
            nrec_sum += nr; ++c1;
        }
        const uint64_t base = chunk_off[c0];
        std::vector<uint64_t> rel(c1 - c0);
        for (size_t i = c0; i < c1; ++i) rel[i - c0] = chunk_off[i] - base;
        uint64_t n = 0, *bc = nullptr, *cnt = nullptr;
        afq_gpl_hist_stats st{};
        rc = afq_gpl_hist_rad(ctx.get(), rad + base, (size_t)(chunk_end(c1 - 1) - base), rel.data(), (uint32_t)rel.size(), P.bc_bytes, P.umi_bytes, o->expected_ori, 0, &n, &bc, &cnt, &st);
        if (rc) {
            std::string m = afq_last_error(ctx.get());
            if (c0 && m.compare(0, 6, "chunk ") == 0) m += " (chunks of this fill are numbered from chunk " + std::to_string(c0) + " of the file)";
            return hfail(rc, m);
        }
        struct Freer { void *a, *b; ~Freer() { afq_free(a); afq_free(b); } } fr{bc, cnt};
        n_records += st.n_records; n_compat += st.n_compatible; max_ambig = std::max(max_ambig, st.max_ambig);
        merge_histogram(hbc, hcnt, bc, cnt, n);
        c0 = c1;
    }
    std::fprintf(stderr, "observed %llu reads (%llu orientation consistent) in %llu chunks --- max ambiguity read occurs in %llu refs\n", (unsigned long long)n_records,
                 (unsigned long long)n_compat, (unsigned long long)P.num_chunks, (unsigned long long)max_ambig);
    if (cblen < 32) for (uint64_t b : hbc) if (b >= (1ull << (2 * cblen))) return hfail(AFQ_ERR_BAD_INPUT, "packed barcode " + std::to_string(b) + " does not fit declared length " + std::to_string(cblen));
    auto count_of = [&](uint64_t b) -> uint64_t { auto it = std::lower_bound(hbc.begin(), hbc.end(), b); return it != hbc.end() && *it == b ? hcnt[it - hbc.begin()] : 0; };
    // ---- the retained set
    const bool filtered = o->method != AFQ_GPL_UNFILTERED;
    std::vector<uint64_t> retained;
    if (o->method == AFQ_GPL_VALID_BC) {
        retained = listed;
        for (uint64_t b : retained) if (cblen < 32 && b >= (1ull << (2 * cblen))) return hfail(AFQ_ERR_BAD_INPUT, "packed barcode " + std::to_string(b) + " does not fit declared length " + std::to_string(cblen));
    } else if (o->method == AFQ_GPL_UNFILTERED) {
        uint64_t unmatched_reads = 0;
        for (size_t i = 0; i < hbc.size(); ++i) if (!std::binary_search(listed.begin(), listed.end(), hbc[i])) unmatched_reads += hcnt[i];
        if (n_records > 0) {   // check_permit_list_validity (cellfilter.rs:2314-2335; note: over all reads, as the reference)
            const double f = (double)unmatched_reads / (double)n_records;
            if (f < 0.3) std::fprintf(stderr, "The percentage of mapped reads not matching a known barcode exactly is %.3f%%, which is < the warning threshold %.3f%%\n", f * 100.0, 30.0);
            else std::fprintf(stderr, "Percentage of mapped reads not matching a known barcode exaclty (%g%%) is > the suggested fraction (%g%%)\n", f * 100.0, 30.0);
        } else std::fprintf(stderr, "Cannot determine (likely) valid permit list if not reads are mapped\n");
        std::fprintf(stderr, "minimum num reads for barcode pass = %llu\n", (unsigned long long)o->min_reads);
        for (uint64_t b : listed) if (count_of(b) >= o->min_reads) retained.push_back(b);
        std::fprintf(stderr, "found %zu cells with non-trivial number of reads by exact barcode match\n", retained.size());
    } else {
        const int64_t n = afq_gpl_select_retained(hbc.data(), hcnt.data(), hbc.size(), o->method, o->method_count, nullptr, 0);
        if (n < 0) return (int)n;
        retained.resize((size_t)n);
        afq_gpl_select_retained(hbc.data(), hcnt.data(), hbc.size(), o->method, o->method_count, retained.data(), retained.size());
    }
    if (filtered) std::fprintf(stderr, "filtering selected %zu retained barcode targets\n", retained.size());
    std::vector<uint64_t> ret_cnt(retained.size());
    for (size_t i = 0; i < retained.size(); ++i) ret_cnt[i] = count_of(retained[i]);
    const uint32_t nbh = o->neighborhood >= 0 ? (uint32_t)o->neighborhood : (filtered ? 1u : 0u);   // prog_opts.rs:135-144
    if (o->frequency && nbh == 1)
        std::fprintf(stderr, "cell-barcode Frequency correction is using substitution-or-shift-1. RAD stores no barcode base qualities or indel-error model, so this is an abundance heuristic rather than a calibrated indel posterior.\n");
    GplPlan plan;
    if (int rc2 = compile_plan(ctx.get(), hbc, hcnt, retained, ret_cnt, cblen, nbh, o->frequency ? 1 : 0, conf_num, conf_den, plan)) return rc2;
    afq_gpl_correction_stats& cs = plan.cs;
    std::vector<uint64_t>&plan_obs = plan.plan_obs, &plan_cor = plan.plan_cor, &freq_bc = plan.freq_bc, &freq_cnt = plan.freq_cnt;
    const std::vector<uint8_t>& permitted = plan.permitted;
    std::fprintf(stderr, "Cell correction: %llu exact reads, %llu corrected, %llu ambiguous, %llu without a candidate\n", (unsigned long long)cs.exact_reads,
                 (unsigned long long)cs.corrected_reads, (unsigned long long)cs.ambiguous_reads, (unsigned long long)cs.not_found_reads);
    // ---- permit_map.bin: the full theoretical neighbourhood (filtered methods), or the observed entries
    std::vector<uint64_t> map_obs, map_cor;
    if (filtered) {
        if (int rc2 = compile_full_map(ctx.get(), retained, ret_cnt, permitted, cblen, nbh, o->frequency ? 1 : 0, conf_num, conf_den, map_obs, map_cor)) return rc2;
    } else { map_obs = plan_obs; map_cor = plan_cor; }
    afq_gpl_tables T{};
    T.barcode_len = cblen; T.neighborhood = nbh; T.frequency = o->frequency ? 1 : 0; T.filtered = filtered ? 1 : 0;
    T.conf_num = conf_num; T.conf_den = conf_den; T.pseudocount = 1;
    T.freq_bc = freq_bc.data(); T.freq_count = freq_cnt.data(); T.n_freq = freq_bc.size();
    static const uint64_t kNone = 0;
    if (filtered) { T.all_bc = hbc.empty() ? &kNone : hbc.data(); T.all_count = hcnt.empty() ? &kNone : hcnt.data(); T.n_all = hbc.size(); }
    T.map_obs = map_obs.data(); T.map_cor = map_cor.data(); T.n_map = map_obs.size();
    T.plan_obs = plan_obs.data(); T.plan_cor = plan_cor.data(); T.n_plan = plan_obs.size();
    const uint64_t sv[8] = {cs.exact_distinct, cs.exact_reads, cs.corrected_distinct, cs.corrected_reads, cs.ambiguous_distinct, cs.ambiguous_reads, cs.not_found_distinct, cs.not_found_reads};
    std::memcpy(T.stats, sv, sizeof sv);
    T.max_ambig = max_ambig;
    afq_gpl_opts oo = *o;
    oo.conf_num = conf_num; oo.conf_den = conf_den;
    rc = afq_gpl_write_outputs(&oo, &T);
    if (rc) return rc;
    std::fprintf(stderr, "total number of distinct corrected barcodes : %llu\n", (unsigned long long)cs.corrected_distinct);
    if (o->corrected_out) *o->corrected_out = cs.corrected_distinct;
    return 0;
}

// ---------------------------------------------------------------------------
// `alevin-fry generate-permit-list` on a multi-barcode (10x Flex) RAD file (do_generate_permit_list_multi_bc, src/cellfilter.rs:789-1381;
// compile_multi_sample_cell_output, 193-366; the sample list and its permit map, 1405-1682).  The record pass runs on the device
// (afq_gpl_multi_hist_rad) over the ROUTING ENTRIES - the exact sources, the structurally unique neighbours and, under sample
// frequency, the structurally ambiguous barcodes; the host derives everything else from the entry index of a pair: the sample, the
// exact counts that become the priors, and the replay of the deferred pairs (the reference spools them, correction_spool.rs; here
// they are rows of the same output).  The cell correction of every sample is the single-barcode path's (afq_gpl_correct).
int afq_gpl_multi_check_args(uint32_t b0_bytes, uint32_t b1_bytes, uint32_t umi_bytes, uint32_t expected_ori, const uint64_t* sample_observed, uint64_t n_entries) {
    std::string e;
    const int r = afq::gplhost::multi_check_args(b0_bytes, b1_bytes, umi_bytes, expected_ori, sample_observed, n_entries, e);
    return r ? hfail(r, e) : 0;
}
int64_t afq_gpl_multi_routing(const uint8_t* text, size_t n, int reverse, uint32_t sample_correction, uint32_t sample_neighborhood, uint64_t* entry, uint64_t* target,
                              uint8_t* kind, size_t cap, uint32_t* barcode_len, uint32_t* n_samples) {
    if (!text && n) return hfail(AFQ_ERR_INVALID_ARG, "null argument");
    if (sample_correction > AFQ_GPL_SAMPLE_ONE_EDIT) return hfail(AFQ_ERR_INVALID_ARG, "unknown sample correction mode");
    if (sample_neighborhood > 1) return hfail(AFQ_ERR_INVALID_ARG, "unknown barcode neighbourhood; expected hamming-1 or substitution-or-shift-1");
    afq::gplhost::SampleList sl;
    std::string e;
    if (int rc = afq::gplhost::parse_sample_list(std::string((const char*)text, n), reverse != 0, sl, e)) return hfail(rc, e);
    afq::gplhost::SampleRouting r;
    afq::gplhost::build_sample_routing(sl, sample_correction, sample_neighborhood, r);
    for (size_t i = 0; i < r.entry.size() && i < cap; ++i) { if (entry) entry[i] = r.entry[i]; if (target) target[i] = r.target[i]; if (kind) kind[i] = r.kind[i]; }
    if (barcode_len) *barcode_len = sl.barcode_len;
    if (n_samples) *n_samples = (uint32_t)sl.canonical.size();
    return (int64_t)r.entry.size();
}

namespace {
// format!("{:?}", path): a quoted string with quotes and backslashes escaped
void rust_debug_str(const char* s, std::string& o) {
    o += '"';
    for (const char* p = s ? s : ""; *p; ++p) { if (*p == '"' || *p == '\\') o.push_back('\\'); o.push_back(*p); }
    o += '"';
}
struct CellCounts { std::vector<uint64_t> bc, cnt; };   // ascending by barcode
// one entry's cells (ascending) into a sample's two histograms: listed cells feed the retained set, the others only the correction
void add_cells(const uint64_t* cell, const uint64_t* cnt, size_t n, const std::vector<uint64_t>* whitelist, CellCounts& hist, CellCounts& unmatched) {
    if (!whitelist) { merge_histogram(hist.bc, hist.cnt, cell, cnt, n); return; }
    std::vector<uint64_t> ib, ic, ob, oc;
    for (size_t i = 0; i < n; ++i) {
        const bool in = std::binary_search(whitelist->begin(), whitelist->end(), cell[i]);
        (in ? ib : ob).push_back(cell[i]); (in ? ic : oc).push_back(cnt[i]);
    }
    if (!ib.empty()) merge_histogram(hist.bc, hist.cnt, ib.data(), ic.data(), ib.size());
    if (!ob.empty()) merge_histogram(unmatched.bc, unmatched.cnt, ob.data(), oc.data(), ob.size());
}
}  // namespace

int64_t afq_generate_permit_list_multi(const afq_gpl_multi_opts* o) {
    using namespace afq::gplhost;
    if (!o || !o->input_dir || !o->output_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    if (o->expected_ori > 2) return hfail(AFQ_ERR_INVALID_ARG, "expected_ori must be 0 (both), 1 (fw) or 2 (rc)");
    if (o->method > AFQ_GPL_UNFILTERED) return hfail(AFQ_ERR_INVALID_ARG, "unknown filter method");
    if ((o->method == AFQ_GPL_VALID_BC || o->method == AFQ_GPL_UNFILTERED) && !o->list_file) return hfail(AFQ_ERR_INVALID_ARG, "the filter method needs a barcode list file");
    if (o->method == AFQ_GPL_UNFILTERED && o->min_reads < 1) return hfail(AFQ_ERR_INVALID_ARG, "min-reads < 1 is not supported, the value " + std::to_string(o->min_reads) + " was provided");
    if (o->neighborhood > 1 || o->sample_neighborhood > 1) return hfail(AFQ_ERR_INVALID_ARG, "unknown barcode neighbourhood; expected hamming-1 or substitution-or-shift-1");
    if (o->sample_correction > AFQ_GPL_SAMPLE_ONE_EDIT) return hfail(AFQ_ERR_INVALID_ARG, "unknown sample correction mode");
    if (o->sample_bc_ori > 1) return hfail(AFQ_ERR_INVALID_ARG, "sample_bc_ori must be 0 (forward) or 1 (reverse)");
    uint64_t conf_num = 39, conf_den = 40, sconf_num = 39, sconf_den = 40;
    if (o->conf_den || o->conf_num) { std::string e; if (int rc = confidence_new(o->conf_num, o->conf_den, &conf_num, &conf_den, e)) return hfail(rc, e); }
    if (o->sample_conf_den || o->sample_conf_num) { std::string e; if (int rc = confidence_new(o->sample_conf_num, o->sample_conf_den, &sconf_num, &sconf_den, e)) return hfail(rc, e); }
    const std::string in = o->input_dir, out = o->output_dir;
    if (!file_exists(in)) return hfail(AFQ_ERR_BAD_INPUT, "the input RAD path \"" + in + "\" does not exist");
    MappedFile mf;
    if (!mf.open(in + "/map.rad")) return hfail(AFQ_ERR_BAD_INPUT, "could not open input rad file");
    const uint8_t* rad = mf.p;
    const size_t rad_n = mf.n;
    RadPrelude P;
    int rc = parse_prelude(rad, rad_n, P, false);
    if (rc) return rc;
    // ---- the prelude: quant's checks for multi-barcode records (afq_quantify)
    auto has_tag = [](const std::vector<TagDesc>& v, const char* name) { for (auto& t : v) if (t.name == name) return true; return false; };
    if (has_tag(P.aln_tags, "start_pos") || has_tag(P.aln_tags, "frag_len"))
        return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode generate-permit-list: this is a scATAC RAD file");
    if (!P.file_tag_vals.count("num_barcodes") || P.file_tag_vals["num_barcodes"] <= 1)
        return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode generate-permit-list: this is a single-barcode RAD file (no num_barcodes > 1 file tag); use generate-permit-list");
    if (has_tag(P.aln_tags, "pos")) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode RAD records with alignment positions (alignment tag pos) are not supported");
    const uint64_t num_barcodes = P.file_tag_vals["num_barcodes"];
    if (num_barcodes != 2 || P.read_tags.size() != 3 || P.read_tags[0].name != "b0" || P.read_tags[1].name != "b1" || P.read_tags[2].name != "u")
        return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode RAD: only two barcode levels with read tags (b0, b1, u) are supported");
    const uint32_t w0 = (uint32_t)int_type_bytes(P.read_tags[0].type), w1 = (uint32_t)int_type_bytes(P.read_tags[1].type), wu = (uint32_t)int_type_bytes(P.read_tags[2].type);
    if (!w0 || !w1 || w0 > 4 || w1 > 4 || !wu) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode RAD: b0 and b1 must be integers of 1, 2 or 4 bytes (u8/u16/u32)");
    if (P.aln_tags.size() != 1 || P.aln_tags[0].type != 3) return hfail(AFQ_ERR_UNSUPPORTED, "multi-barcode RAD: the alignment-level tags must be one u32 (ref | orientation)");
    if (!P.file_tag_vals.count("b1len")) return hfail(AFQ_ERR_BAD_INPUT, "multi-barcode RAD file should have a \"b1len\" file-level tag");
    const uint32_t cblen = (uint32_t)P.file_tag_vals["b1len"];
    if (cblen < 1 || cblen > 32) return hfail(AFQ_ERR_BAD_INPUT, "barcode length must be between 1 and 32 (got " + std::to_string(cblen) + ")");
    // ---- the sample list and the routing entries
    if (!o->sample_bc_list)
        return hfail(AFQ_ERR_INVALID_ARG, "Multi-barcode RAD file detected (" + std::to_string(num_barcodes) + " barcode levels), but --sample-bc-list was not provided. "
                     "A known sample barcode list is required for multi-barcode processing.");
    SampleList sl;
    {
        std::vector<uint8_t> raw;
        if (!read_file(o->sample_bc_list, raw)) return hfail(AFQ_ERR_BAD_INPUT, std::string("couldn't open sample barcode list: ") + o->sample_bc_list);
        std::string e;
        if (int rc2 = parse_sample_list(std::string(raw.begin(), raw.end()), o->sample_bc_ori == 1, sl, e)) return hfail(rc2, e);
    }
    if (sl.barcode_len > 4 * w0)
        return hfail(AFQ_ERR_BAD_INPUT, "sample barcodes of " + std::to_string(sl.barcode_len) + " bases do not fit the " + std::to_string(w0) + "-byte b0 field of the records");
    const bool sample_frequency = o->sample_correction == AFQ_GPL_SAMPLE_FREQUENCY;
    SampleRouting routing;
    build_sample_routing(sl, o->sample_correction, o->sample_neighborhood, routing);
    const size_t n_ent = routing.entry.size(), n_samples = sl.canonical.size();
    // ---- the -b list, or the -u whitelist that splits every sample's histogram
    std::vector<uint64_t> listed;
    if (o->method == AFQ_GPL_VALID_BC || o->method == AFQ_GPL_UNFILTERED) {
        std::string txt;
        if (int rc2 = read_list_text(o->list_file, txt)) return rc2;
        const int unf = o->method == AFQ_GPL_UNFILTERED;
        const int64_t n = afq_gpl_parse_barcode_list((const uint8_t*)txt.data(), txt.size(), unf, cblen, nullptr, 0, nullptr);
        if (n < 0) return (int)n;
        listed.resize((size_t)n);
        afq_gpl_parse_barcode_list((const uint8_t*)txt.data(), txt.size(), unf, cblen, listed.data(), listed.size(), nullptr);
        std::sort(listed.begin(), listed.end());
        listed.erase(std::unique(listed.begin(), listed.end()), listed.end());
        if (!unf) for (uint64_t b : listed) if (cblen < 32 && b >= (1ull << (2 * cblen))) return hfail(AFQ_ERR_BAD_INPUT, "packed barcode " + std::to_string(b) + " does not fit declared length " + std::to_string(cblen));
    }
    const std::vector<uint64_t>* whitelist = o->method == AFQ_GPL_UNFILTERED ? &listed : nullptr;
    // ---- the chunk table
    std::vector<uint64_t> chunk_off;
    if (int rc2 = walk_chunk_offsets(rad, rad_n, P.first_chunk, P.num_chunks, chunk_off)) return rc2;
    CtxPtr ctx;
    if (int rc2 = open_fill_ctx(o->device, 0, ctx)) return rc2;
    // ---- the record pass: one device fill per run of chunks of at most fill_bytes, the sorted outputs merged under the key entry << 32 | cell
    const uint64_t fill_bytes = o->fill_bytes ? o->fill_bytes : (8ull << 30);
    std::vector<uint64_t> pkey, pcnt;
    afq_gpl_multi_hist_stats S{};
    for (size_t c0 = 0; c0 < chunk_off.size();) {
        size_t c1 = c0;
        uint64_t nrec_sum = 0;
        auto chunk_end = [&](size_t i) { uint32_t nb; std::memcpy(&nb, rad + chunk_off[i], 4); return chunk_off[i] + nb; };
        while (c1 < chunk_off.size()) {
            uint32_t nr; std::memcpy(&nr, rad + chunk_off[c1] + 4, 4);
            if (c1 > c0 && (chunk_end(c1) - chunk_off[c0] > fill_bytes || nrec_sum + nr >= (1ull << 30))) break;
            nrec_sum += nr; ++c1;
        }
        const uint64_t base = chunk_off[c0];
        std::vector<uint64_t> rel(c1 - c0);
        for (size_t i = c0; i < c1; ++i) rel[i - c0] = chunk_off[i] - base;
        uint64_t n = 0, *cell = nullptr, *cnt = nullptr;
        uint32_t* ent = nullptr;
        afq_gpl_multi_hist_stats st{};
        rc = afq_gpl_multi_hist_rad(ctx.get(), rad + base, (size_t)(chunk_end(c1 - 1) - base), rel.data(), (uint32_t)rel.size(), w0, w1, wu, o->expected_ori, 0,
                                    routing.entry.data(), n_ent, &n, &ent, &cell, &cnt, &st);
        if (rc) {
            std::string m = afq_last_error(ctx.get());
            if (c0 && m.compare(0, 6, "chunk ") == 0) m += " (chunks of this fill are numbered from chunk " + std::to_string(c0) + " of the file)";
            return hfail(rc, m);
        }
        Freer3 fr{ent, cell, cnt};
        S.n_records += st.n_records; S.n_compatible += st.n_compatible; S.n_routed += st.n_routed; S.n_unrouted += st.n_unrouted; S.n_long_records += st.n_long_records;
        std::vector<uint64_t> key(n);
        for (uint64_t i = 0; i < n; ++i) key[i] = (uint64_t)ent[i] << 32 | cell[i];
        merge_histogram(pkey, pcnt, key.data(), cnt, n);
        c0 = c1;
    }
    if (o->stats_out) *o->stats_out = S;
    // ---- per entry: its reads and its run of (cell, count) rows; the immediately routed entries feed their sample
    std::vector<size_t> run_lo(n_ent + 1, pkey.size());
    std::vector<uint64_t> entry_reads(n_ent, 0), pcell(pkey.size());
    {
        size_t i = 0;
        for (size_t e = 0; e < n_ent; ++e) {
            run_lo[e] = i;
            for (; i < pkey.size() && (pkey[i] >> 32) == e; ++i) { entry_reads[e] += pcnt[i]; pcell[i] = pkey[i] & 0xFFFFFFFFull; }
        }
        run_lo[n_ent] = i;
        if (i != pkey.size()) return hfail(AFQ_ERR_HIP, "afq_generate_permit_list_multi: the record pass returned a pair beyond its " + std::to_string(n_ent) + " routing entries");
    }
    if (cblen < 16) for (uint64_t b : pcell) if (b >= (1ull << (2 * cblen))) return hfail(AFQ_ERR_BAD_INPUT, "packed barcode " + std::to_string(b) + " does not fit declared length " + std::to_string(cblen));
    std::vector<CellCounts> hist(n_samples), unmatched(n_samples);
    uint64_t r_exact = 0, r_unique = 0, r_deferred = 0, r_accepted = 0, r_rejected = 0;
    auto feed = [&](size_t e, uint64_t canon) {
        const size_t si = sl.sample_of(canon);
        add_cells(pcell.data() + run_lo[e], pcnt.data() + run_lo[e], run_lo[e + 1] - run_lo[e], whitelist, hist[si], unmatched[si]);
    };
    for (size_t e = 0; e < n_ent; ++e) {
        if (routing.kind[e] == 2) { r_deferred += entry_reads[e]; continue; }
        (routing.kind[e] == 0 ? r_exact : r_unique) += entry_reads[e];
        if (entry_reads[e]) feed(e, routing.target[e]);
    }
    // ---- the final sample permit map; under frequency the exact counts are the priors and every deferred entry is resolved once
    std::vector<uint64_t> smap_obs, smap_cor;
    double replay_s = 0;
    if (sample_frequency) {
        SampleIndex ix = sample_index(sl, o->sample_correction, o->sample_neighborhood);
        ix.conf_num = sconf_num; ix.conf_den = sconf_den; ix.pseudocount = 1;
        for (size_t e = 0; e < n_ent; ++e)
            if (routing.kind[e] == 0) {
                auto it = std::lower_bound(ix.src.begin(), ix.src.end(), routing.entry[e], [](const SampleSource& s, uint64_t v) { return s.source < v; });
                it->count = entry_reads[e];   // (an exact source is a rotation: it is there)
            }
        for (uint64_t b : ix.theoretical()) {   // compile_full_neighborhood
            uint64_t t = 0;
            if (ix.resolve(b, t) <= kSampleCorrected) { smap_obs.push_back(b); smap_cor.push_back(t); }
        }
        const auto t0 = std::chrono::steady_clock::now();
        for (size_t e = 0; e < n_ent; ++e) {
            if (routing.kind[e] != 2 || !entry_reads[e]) continue;
            uint64_t t = 0;
            if (ix.resolve(routing.entry[e], t) <= kSampleCorrected) { r_accepted += entry_reads[e]; feed(e, t); } else r_rejected += entry_reads[e];
        }
        replay_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } else {
        for (size_t e = 0; e < n_ent; ++e) { smap_obs.push_back(routing.entry[e]); smap_cor.push_back(routing.target[e]); }
    }
    const uint64_t matched = r_exact + r_unique + r_accepted, unmatched_reads = S.n_unrouted + r_rejected;
    std::fprintf(stderr, "First pass complete: %llu total reads, %llu matched to samples, %llu unmatched\n", (unsigned long long)S.n_records, (unsigned long long)matched,
                 (unsigned long long)unmatched_reads);
    if (gpl_mkdirs(out)) return hfail(AFQ_ERR_BAD_INPUT, "couldn't create output directory " + out);
    if (!write_map_file(out + "/sample_permit_map.bin", smap_obs.data(), smap_cor.data(), smap_obs.size())) return hfail(AFQ_ERR_BAD_INPUT, "failed to serialize sample permit map");
    // ---- per sample: the retained set, the correction (on the device), the files
    const uint32_t nbh = o->neighborhood >= 0 ? (uint32_t)o->neighborhood : 0u;   // resolved_cell_neighborhood(true), prog_opts.rs:135-144
    const uint32_t freq = o->frequency ? 1u : 0u;
    if (freq && nbh == 1)
        std::fprintf(stderr, "cell-barcode Frequency correction is using substitution-or-shift-1. RAD stores no barcode base qualities or indel-error model, so this is an abundance heuristic rather than a calibrated indel posterior.\n");
    static const char* const kStat[8] = {"exact_distinct", "exact_reads", "corrected_distinct", "corrected_reads", "ambiguous_distinct", "ambiguous_reads", "not_found_distinct", "not_found_reads"};
    const PlanSpec cspec{cblen, nbh, freq, conf_num, conf_den, 1};
    std::vector<GplPlan> plans(n_samples);
    std::vector<std::string> infos(n_samples);
    uint64_t total_cells = 0;
    const auto cc0 = std::chrono::steady_clock::now();
    for (size_t si = 0; si < n_samples; ++si) {
        const std::string& name = sl.names[si];
        const std::string sdir = out + "/sample_" + name;
        if (gpl_mkdirs(sdir)) return hfail(AFQ_ERR_BAD_INPUT, "couldn't create directory path " + sdir);
        char hex[32];
        std::snprintf(hex, sizeof hex, "0x%llx", (unsigned long long)sl.canonical[si]);
        uint64_t num_reads = 0, num_cells = 0, collatable = 0;
        GplPlan& plan = plans[si];
        if (!hist[si].bc.empty()) {   // (a sample without a listed read keeps its directory and its entry, and gets no permit files)
            const CellCounts& h = hist[si];
            std::vector<uint64_t> retained;
            if (o->method == AFQ_GPL_VALID_BC) retained = listed;
            else {
                const uint32_t m = o->method;
                const uint64_t arg = m == AFQ_GPL_UNFILTERED ? o->min_reads : o->method_count;
                const int64_t n = afq_gpl_select_retained(h.bc.data(), h.cnt.data(), h.bc.size(), m, arg, nullptr, 0);
                if (n < 0) return (int)n;
                retained.resize((size_t)n);
                afq_gpl_select_retained(h.bc.data(), h.cnt.data(), h.bc.size(), m, arg, retained.data(), retained.size());
            }
            CellCounts obs = h;
            if (!unmatched[si].bc.empty()) merge_histogram(obs.bc, obs.cnt, unmatched[si].bc.data(), unmatched[si].cnt.data(), unmatched[si].bc.size());
            std::vector<uint64_t> ret_cnt(retained.size());
            uint64_t exact_retained = 0;
            for (size_t i = 0; i < retained.size(); ++i) {
                auto it = std::lower_bound(obs.bc.begin(), obs.bc.end(), retained[i]);
                ret_cnt[i] = it != obs.bc.end() && *it == retained[i] ? obs.cnt[it - obs.bc.begin()] : 0;
                exact_retained += ret_cnt[i];
            }
            if (int rc2 = compile_plan(ctx.get(), obs.bc, obs.cnt, retained, ret_cnt, cblen, nbh, freq, conf_num, conf_den, plan)) return rc2;
            std::vector<uint64_t> map_obs, map_cor;
            if (o->method != AFQ_GPL_UNFILTERED) {
                if (int rc2 = compile_full_map(ctx.get(), retained, ret_cnt, plan.permitted, cblen, nbh, freq, conf_num, conf_den, map_obs, map_cor)) return rc2;
            } else { map_obs = plan.plan_obs; map_cor = plan.plan_cor; }
            if (!write_map_file(sdir + "/permit_map.bin", map_obs.data(), map_cor.data(), map_obs.size())) return hfail(AFQ_ERR_BAD_INPUT, "failed to serialize permit map");
            if (!write_freq_file(sdir + "/permit_freq.bin", cblen, plan.freq_bc.data(), plan.freq_cnt.data(), plan.freq_bc.size()))
                return hfail(AFQ_ERR_BAD_INPUT, "failed to write permit freq for sample '" + name + "'");
            for (uint64_t v : plan.freq_cnt) collatable += v;
            num_cells = plan.freq_bc.size();
            num_reads = o->method == AFQ_GPL_UNFILTERED ? collatable : exact_retained;
        }
        total_cells += num_cells;
        const afq_gpl_correction_stats& cs = plan.cs;
        const uint64_t sv[8] = {cs.exact_distinct, cs.exact_reads, cs.corrected_distinct, cs.corrected_reads, cs.ambiguous_distinct, cs.ambiguous_reads, cs.not_found_distinct, cs.not_found_reads};
        std::string j = "    {\n      \"name\": " + gpl_json_str(name.c_str()) + ",\n      \"barcode\": \"" + hex + "\",\n      \"num_reads\": " + std::to_string(num_reads) +
                        ",\n      \"num_cells\": " + std::to_string(num_cells) + ",\n      \"collatable_reads\": " + std::to_string(collatable) + ",\n      \"cell_correction\": {\n";
        for (int i = 0; i < 8; ++i) j += std::string("        \"") + kStat[i] + "\": " + std::to_string(sv[i]) + (i < 7 ? ",\n" : "\n");
        infos[si] = j + "      }\n    }";
    }
    const double cell_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - cc0).count();
    // ---- correction_plan.bin: the sample scope and one cell scope per sample, ascending by canonical barcode
    std::vector<size_t> order(n_samples);
    for (size_t i = 0; i < n_samples; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return sl.canonical[a] < sl.canonical[b]; });
    std::vector<PlanScope> scopes;
    for (size_t si : order) scopes.push_back(PlanScope{true, sl.canonical[si], cspec, plans[si].plan_obs.data(), plans[si].plan_cor.data(), plans[si].plan_obs.size()});
    const bool shift_s = o->sample_correction == AFQ_GPL_SAMPLE_ONE_EDIT || o->sample_neighborhood == 1;
    const PlanSpec sspec{sl.barcode_len, shift_s ? 1u : 0u, sample_frequency ? 1u : 0u, sconf_num, sconf_den, 1};
    const bool have_sspec = o->sample_correction != AFQ_GPL_SAMPLE_EXACT;
    uint64_t plan_n = 0;
    const auto pw0 = std::chrono::steady_clock::now();
    if (!write_plan_file(out + "/correction_plan.bin", (int)sl.barcode_len, cblen, have_sspec ? &sspec : nullptr, smap_obs.data(), smap_cor.data(), smap_obs.size(), scopes, &plan_n))
        return hfail(AFQ_ERR_BAD_INPUT, "could not write correction plan");
    const double plan_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - pw0).count();
    // ---- sample_info.json and generate_permit_list.json (the json! documents of cellfilter.rs:1316-1368)
    static const char* const kOriSym[3] = {"both", "fw", "rc"};
    static const char* const kNbh[2] = {"hamming-1", "substitution-or-shift-1"};
    static const char* const kModeDebug[4] = {"Exact", "Unique", "Frequency", "OneEdit"};
    static const char* const kModeResolved[4] = {"exact", "unique", "frequency", "unique"};
    auto common = [&](const char* ind) {
        std::string j;
        j += std::string(ind) + "\"cell_bc_correction\": \"" + (freq ? "frequency" : "unique") + "\",\n";
        j += std::string(ind) + "\"cell_bc_neighborhood\": \"" + kNbh[nbh] + "\",\n";
        j += std::string(ind) + "\"cell_bc_confidence\": \"" + std::to_string(conf_num) + "/" + std::to_string(conf_den) + "\",\n";
        j += std::string(ind) + "\"sample_bc_correction\": \"" + kModeResolved[o->sample_correction] + "\",\n";
        j += std::string(ind) + "\"sample_bc_neighborhood\": " + (have_sspec ? std::string("\"") + kNbh[shift_s ? 1 : 0] + "\"" : std::string("null")) + ",\n";
        j += std::string(ind) + "\"sample_bc_confidence\": \"" + std::to_string(sconf_num) + "/" + std::to_string(sconf_den) + "\"";
        return j;
    };
    auto dbl = [](double v) { char b[64]; std::snprintf(b, sizeof b, "%.9g", v); std::string s = b; if (s.find_first_of(".e") == std::string::npos) s += ".0"; return s; };
    {
        std::string j = "{\n";
        j += "  \"num_samples\": " + std::to_string(n_samples) + ",\n  \"num_barcodes\": " + std::to_string(num_barcodes) + ",\n  \"total_cells\": " + std::to_string(total_cells) + ",\n";
        j += "  \"total_reads\": " + std::to_string(S.n_records) + ",\n  \"matched_reads\": " + std::to_string(matched) + ",\n  \"unmatched_reads\": " + std::to_string(unmatched_reads) + ",\n";
        j += std::string("  \"sample_correction_mode\": \"") + kModeDebug[o->sample_correction] + "\",\n  \"sample_bc_ori\": \"" + (o->sample_bc_ori ? "Reverse" : "Forward") + "\",\n";
        j += common("  ") + ",\n";
        j += "  \"cell_correction_seconds\": " + dbl(cell_s) + ",\n  \"correction_plan_bytes\": " + std::to_string(plan_n) + ",\n  \"correction_plan_write_seconds\": " + dbl(plan_s) + ",\n";
        j += "  \"sample_routing\": {\n    \"exact\": " + std::to_string(r_exact) + ",\n    \"structurally_unique\": " + std::to_string(r_unique) + ",\n    \"immediate_rejected\": " +
             std::to_string(S.n_unrouted) + ",\n    \"deferred\": " + std::to_string(r_deferred) + ",\n    \"deferred_accepted\": " + std::to_string(r_accepted) +
             ",\n    \"deferred_rejected\": " + std::to_string(r_rejected) + ",\n    \"spill_runs\": 0,\n    \"spill_pairs_after_run_length_encoding\": 0,\n"
             "    \"spill_compressed_bytes\": 0,\n    \"spill_uncompressed_bytes\": 0,\n    \"replay_seconds\": " + dbl(replay_s) + "\n  },\n";
        j += "  \"samples\": [\n";
        for (size_t si = 0; si < n_samples; ++si) j += infos[si] + (si + 1 < n_samples ? ",\n" : "\n");
        j += "  ]\n}";
        GplFile f(std::fopen((out + "/sample_info.json").c_str(), "w"));
        if (!f || std::fwrite(j.data(), 1, j.size(), f.get()) != j.size()) return hfail(AFQ_ERR_BAD_INPUT, "cannot write sample_info.json");
    }
    {
        std::string fm;   // format!("{:?}", CellFilterMethod)
        switch (o->method) {
            case AFQ_GPL_KNEE: fm = "KneeFinding"; break;
            case AFQ_GPL_EXPECT: fm = "ExpectCells(" + std::to_string(o->method_count) + ")"; break;
            case AFQ_GPL_FORCE: fm = "ForceCells(" + std::to_string(o->method_count) + ")"; break;
            case AFQ_GPL_VALID_BC: fm = "ExplicitList("; rust_debug_str(o->list_file, fm); fm += ")"; break;
            default: fm = "UnfilteredExternalList("; rust_debug_str(o->list_file, fm); fm += ", " + std::to_string(o->min_reads) + ")"; break;
        }
        std::string j = "{\n  \"velo_mode\": false,\n";
        j += std::string("  \"expected_ori\": \"") + kOriSym[o->expected_ori] + "\",\n  \"version_str\": \"0.18.0\",\n  \"cmd\": " + gpl_json_str(o->cmdline) + ",\n";
        j += "  \"permit-list-type\": " + gpl_json_str(fm.c_str()) + ",\n  \"multi_barcode\": true,\n  \"num_barcodes\": " + std::to_string(num_barcodes) + ",\n";
        j += common("  ") + "\n}";
        GplFile f(std::fopen((out + "/generate_permit_list.json").c_str(), "w"));
        if (!f || std::fwrite(j.data(), 1, j.size(), f.get()) != j.size()) return hfail(AFQ_ERR_BAD_INPUT, "cannot write to generate_permit_list.json file");
    }
    std::fprintf(stderr, "Multi-barcode permit list generation complete: %zu samples, %llu total cells\n", n_samples, (unsigned long long)total_cells);
    return (int64_t)total_cells;
}

// ---------------------------------------------------------------------------
// `alevin-fry atac generate-permit-list` (generate_permit_list + process_unfiltered, src/atac/cellfilter.rs:143-599): the record
// pass runs on the device (afq_atac_gpl_hist_rad), fill by fill, the correction decisions are afq_gpl_correct's; the bins' layout,
// the listed and retained sets and the files are the host's.  The RNA path's `-u` is the same text but for the orientation
// filter (there is none here), the reverse complement of the list, and the bins.
void afq_atac_gpl_bin_lens(const uint32_t* ref_lens, size_t n, uint64_t bin_size, uint64_t* out) {
    if (out && (ref_lens || !n)) afq::gplhost::atac_bin_lens(ref_lens, n, bin_size, out);
}
uint64_t afq_gpl_reverse_complement(uint64_t barcode, uint32_t k) { return afq::gplhost::reverse_complement(barcode, k > 32 ? 32 : k); }

int afq_atac_generate_permit_list(const afq_atac_gpl_opts* o) {
    if (!o || !o->input_dir || !o->output_dir) return hfail(AFQ_ERR_INVALID_ARG, "null option");
    if (!o->list_file) return hfail(AFQ_ERR_INVALID_ARG, "atac generate-permit-list needs an unfiltered barcode list file (-u)");
    if (o->min_reads < 1) return hfail(AFQ_ERR_INVALID_ARG, "min-reads < 1 is not supported, the value " + std::to_string(o->min_reads) + " was provided");
    if (o->neighborhood > 1) return hfail(AFQ_ERR_INVALID_ARG, "unknown barcode neighbourhood; expected hamming-1 or substitution-or-shift-1");
    uint64_t conf_num = 9, conf_den = 10;   // Confidence::ATAC
    if (o->conf_den || o->conf_num) { std::string e; if (int rc = afq::gplhost::confidence_new(o->conf_num, o->conf_den, &conf_num, &conf_den, e)) return hfail(rc, e); }
    const std::string in = o->input_dir;
    if (!file_exists(in)) return hfail(AFQ_ERR_BAD_INPUT, "the input rad path \"" + in + "\" does not exist");
    const uint64_t bin_size = 100000;
    // ---- the barcode list (populate_unfiltered_barcode_map): read before the RAD file, as the reference reads it
    std::string txt;
    if (int rc2 = read_list_text(o->list_file, txt)) return rc2;
    uint32_t first_len = 0;
    std::vector<uint64_t> listed;
    {
        const int64_t n = afq_gpl_parse_barcode_list((const uint8_t*)txt.data(), txt.size(), 1, 0, nullptr, 0, &first_len);
        if (n < 0) return (int)n;
        listed.resize((size_t)n);
        afq_gpl_parse_barcode_list((const uint8_t*)txt.data(), txt.size(), 1, 0, listed.data(), listed.size(), nullptr);
        if (o->rc) for (uint64_t& b : listed) b = afq::gplhost::reverse_complement(b, first_len);
        std::sort(listed.begin(), listed.end());
        listed.erase(std::unique(listed.begin(), listed.end()), listed.end());
    }
    std::fprintf(stderr, "number of unfiltered bcs read = %zu\n", listed.size());
    MappedFile mf;
    if (!mf.open(in + "/map.rad")) return hfail(AFQ_ERR_BAD_INPUT, "could not open input rad file");
    const uint8_t* rad = mf.p;
    const size_t rad_n = mf.n;
    RadPrelude P;
    int rc = parse_prelude(rad, rad_n, P, false);
    if (rc) return rc;
    {
        bool has_u = false;
        for (auto& t : P.read_tags) has_u = has_u || t.name == "u";
        if (has_u) return hfail(AFQ_ERR_UNSUPPORTED, "atac generate-permit-list: this is an RNA RAD file (it has a UMI tag); use generate-permit-list");
    }
    if (P.read_tags.size() != 1 || P.read_tags[0].name != "b" || !P.bc_bytes) return hfail(AFQ_ERR_UNSUPPORTED, "scATAC RAD: the read-level tags must be exactly one integer 'b'");
    static const struct { const char* name; uint8_t type; } kAln[4] = {{"ref", 3}, {"type", 1}, {"start_pos", 3}, {"frag_len", 2}};
    bool aln_ok = P.aln_tags.size() == 4;
    for (size_t i = 0; aln_ok && i < 4; ++i) aln_ok = P.aln_tags[i].name == kAln[i].name && P.aln_tags[i].type == kAln[i].type;
    if (!aln_ok) return hfail(AFQ_ERR_UNSUPPORTED, "scATAC RAD: the alignment-level tags must be ref:u32, type:u8, start_pos:u32, frag_len:u16 (an RNA RAD file goes to generate-permit-list)");
    if (!P.file_tag_vals.count("cblen")) return hfail(AFQ_ERR_BAD_INPUT, "tag map must contain cblen");
    const uint32_t cblen = (uint32_t)P.file_tag_vals["cblen"];
    if (cblen < 1 || cblen > 32) return hfail(AFQ_ERR_BAD_INPUT, "barcode length must be between 1 and 32 (got " + std::to_string(cblen) + ")");
    if (!P.have_ref_lengths || P.ref_lengths.size() != P.ref_count) return hfail(AFQ_ERR_BAD_INPUT, "scATAC RAD: the ref_lengths file tag must be an array of u32 with one entry per reference");
    if (P.ref_count >= (1ull << 32)) return hfail(AFQ_ERR_UNSUPPORTED, "atac generate-permit-list: 2^32 or more references");
    if (first_len != cblen && !listed.empty())
        std::fprintf(stderr, "The provided permit list had barcodes of length %u, but the mapped reads have barcodes of length %u\n", first_len, cblen);
    for (uint64_t b : listed) if (cblen < 32 && b >= (1ull << (2 * cblen))) return hfail(AFQ_ERR_BAD_INPUT, "packed barcode " + std::to_string(b) + " does not fit declared length " + std::to_string(cblen));
    // ---- the bins (initialize_rec_list)
    std::vector<uint64_t> bin_lens(P.ref_lengths.size() + 1, 0);
    afq::gplhost::atac_bin_lens(P.ref_lengths.data(), P.ref_lengths.size(), bin_size, bin_lens.data());
    const uint64_t n_bins = bin_lens.back();
    // (the reference panics on this after its record pass, `bins.iter().max().expect("bins should not be empty")`, unless a record
    // with one alignment has already indexed past the empty bins; refused here before any record is read)
    if (!n_bins) return hfail(AFQ_ERR_BAD_INPUT, "bins should not be empty (the reference lengths give no position bin)");
    if (n_bins >= (1ull << 31)) return hfail(AFQ_ERR_UNSUPPORTED, "atac generate-permit-list: 2^31 or more position bins (" + std::to_string(n_bins) + ")");
    // ---- the chunk table
    std::vector<uint64_t> chunk_off;
    if (int rc2 = walk_chunk_offsets(rad, rad_n, P.first_chunk, P.num_chunks, chunk_off)) return rc2;
    CtxPtr ctx;
    if (int rc2 = open_fill_ctx(o->device, 0, ctx)) return rc2;
    // ---- the record pass: one device fill per run of chunks of at most fill_bytes; histograms merged, bins and tallies added
    const uint64_t fill_bytes = o->fill_bytes ? o->fill_bytes : (8ull << 30);
    std::vector<uint64_t> hbc, hcnt, bins(n_bins, 0);
    afq_atac_gpl_hist_stats tot{};
    for (size_t c0 = 0; c0 < chunk_off.size();) {
        size_t c1 = c0;
        uint64_t nrec_sum = 0;
        auto chunk_end = [&](size_t i) { uint32_t nb; std::memcpy(&nb, rad + chunk_off[i], 4); return chunk_off[i] + nb; };
        while (c1 < chunk_off.size()) {
            uint32_t nr; std::memcpy(&nr, rad + chunk_off[c1] + 4, 4);
            if (c1 > c0 && (chunk_end(c1) - chunk_off[c0] > fill_bytes || nrec_sum + nr >= (1ull << 30))) break;
            nrec_sum += nr; ++c1;
        }
        const uint64_t base = chunk_off[c0];
        std::vector<uint64_t> rel(c1 - c0);
        for (size_t i = c0; i < c1; ++i) rel[i - c0] = chunk_off[i] - base;
        uint64_t n = 0, *bc = nullptr, *cnt = nullptr, *fb = nullptr;
        afq_atac_gpl_hist_stats st{};
        rc = afq_atac_gpl_hist_rad(ctx.get(), rad + base, (size_t)(chunk_end(c1 - 1) - base), rel.data(), (uint32_t)rel.size(), P.bc_bytes, 0, bin_lens.data(),
                                   (uint32_t)P.ref_count, (uint32_t)bin_size, &n, &bc, &cnt, &fb, &st);
        if (rc) {
            std::string m = afq_last_error(ctx.get());
            if (c0 && m.compare(0, 6, "chunk ") == 0) m += " (chunks of this fill are numbered from chunk " + std::to_string(c0) + " of the file)";
            return hfail(rc, m);
        }
        Freer3 fr{bc, cnt, fb};
        tot.n_records += st.n_records; tot.n_unmapped += st.n_unmapped; tot.n_multimapped += st.n_multimapped; tot.n_binned += st.n_binned;
        tot.max_ambig = std::max(tot.max_ambig, st.max_ambig);
        merge_histogram(hbc, hcnt, bc, cnt, n);
        for (uint64_t i = 0; i < n_bins; ++i) bins[i] += fb[i];
        c0 = c1;
    }
    tot.max_bin = *std::max_element(bins.begin(), bins.end());
    if (cblen < 32) for (uint64_t b : hbc) if (b >= (1ull << (2 * cblen))) return hfail(AFQ_ERR_BAD_INPUT, "packed barcode " + std::to_string(b) + " does not fit declared length " + std::to_string(cblen));
    auto count_of = [&](uint64_t b) -> uint64_t { auto it = std::lower_bound(hbc.begin(), hbc.end(), b); return it != hbc.end() && *it == b ? hcnt[it - hbc.begin()] : 0; };
    {   // likely_valid_permit_list over all reads
        uint64_t unmatched_reads = 0;
        for (size_t i = 0; i < hbc.size(); ++i) if (!std::binary_search(listed.begin(), listed.end(), hbc[i])) unmatched_reads += hcnt[i];
        if (tot.n_records > 0) {
            const double f = (double)unmatched_reads / (double)tot.n_records;
            if (f < 0.3) std::fprintf(stderr, "The percentage of mapped reads not matching a known barcode exactly is %.3f%%, which is < the warning threshold %.3f%%\n", f * 100.0, 30.0);
            else std::fprintf(stderr, "Percentage of mapped reads not matching a known barcode exaclty (%g%%) is > the suggested fraction (%g%%)\n", f * 100.0, 30.0);
        } else std::fprintf(stderr, "Cannot determine (likely) valid permit list if not reads are mapped\n");
    }
    std::fprintf(stderr, "observed %llu reads (%llu orientation consistent) in %llu chunks --- max ambiguity read occurs in %llu refs\n", (unsigned long long)tot.n_records,
                 (unsigned long long)tot.n_records, (unsigned long long)P.num_chunks, (unsigned long long)tot.max_ambig);
    std::fprintf(stderr, "minimum num reads for barcode pass = %llu\n", (unsigned long long)o->min_reads);
    std::vector<uint64_t> retained;
    for (uint64_t b : listed) if (count_of(b) >= o->min_reads) retained.push_back(b);
    std::vector<uint64_t> ret_cnt(retained.size());
    for (size_t i = 0; i < retained.size(); ++i) ret_cnt[i] = count_of(retained[i]);
    const uint32_t nbh = o->neighborhood;
    if (o->frequency && nbh == 1)
        std::fprintf(stderr, "ATAC Frequency correction is using substitution-or-shift-1. RAD stores no barcode base qualities or indel-error model, so this is an abundance heuristic rather than a calibrated indel posterior.\n");
    std::fprintf(stderr, "found %zu cells with non-trivial number of reads by exact barcode match\n", retained.size());
    GplPlan plan;
    if (int rc2 = compile_plan(ctx.get(), hbc, hcnt, retained, ret_cnt, cblen, nbh, o->frequency ? 1 : 0, conf_num, conf_den, plan)) return rc2;
    const afq_gpl_correction_stats& cs = plan.cs;
    std::fprintf(stderr, "ATAC cell correction: %llu exact reads, %llu corrected, %llu ambiguous, %llu without a candidate\n", (unsigned long long)cs.exact_reads,
                 (unsigned long long)cs.corrected_reads, (unsigned long long)cs.ambiguous_reads, (unsigned long long)cs.not_found_reads);
    afq_gpl_tables T{};
    T.barcode_len = cblen; T.neighborhood = nbh; T.frequency = o->frequency ? 1 : 0; T.filtered = 0;
    T.conf_num = conf_num; T.conf_den = conf_den; T.pseudocount = 1;
    T.freq_bc = plan.freq_bc.data(); T.freq_count = plan.freq_cnt.data(); T.n_freq = plan.freq_bc.size();
    T.map_obs = plan.plan_obs.data(); T.map_cor = plan.plan_cor.data(); T.n_map = plan.plan_obs.size();   // (the plan's entries, not the theoretical neighbourhood: cellfilter.rs:237-248)
    T.plan_obs = plan.plan_obs.data(); T.plan_cor = plan.plan_cor.data(); T.n_plan = plan.plan_obs.size();
    const uint64_t sv[8] = {cs.exact_distinct, cs.exact_reads, cs.corrected_distinct, cs.corrected_reads, cs.ambiguous_distinct, cs.ambiguous_reads, cs.not_found_distinct, cs.not_found_reads};
    std::memcpy(T.stats, sv, sizeof sv);
    T.max_ambig = tot.max_ambig;
    afq_atac_gpl_opts oo = *o;
    oo.conf_num = conf_num; oo.conf_den = conf_den;
    {
        std::string e;
        if (int rc2 = afq::gplhost::write_atac_outputs(&oo, &T, bins.data(), bins.size(), bin_lens.data(), bin_lens.size(), P.num_chunks, tot.max_bin, e)) return hfail(rc2, e);
    }
    std::fprintf(stderr, "total number of distinct corrected barcodes : %llu\n", (unsigned long long)cs.corrected_distinct);
    if (o->stats_out) *o->stats_out = tot;
    return 0;
}

}  // extern "C"
