// afq_ctx.h — what the afq_api*.cpp files share: the context, its buffer sets, timers, the error latch, the owned host outputs,
// and the record pass (RadPass) of the *_rad entry points.  Internal: not installed, and everything in it is hidden from the
// library's exports.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/afquant.h"
#include "afq_chunk_table.h"
#include "afq_common.h"
#include "afq_hooks.h"
#include "afq_kernels.h"

#pragma GCC visibility push(hidden)

using namespace afq;

inline thread_local std::string g_create_err;   // afq_create has no context to put its refusal in

// AFQ_HOST_TIMING=1 prints where the host side of a batch spends its time (stderr)
struct HostClock {
    bool on = std::getenv("AFQ_HOST_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char* what) {
        if (!on) return;
        auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[afq host] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = n + n / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { e = hipMalloc(&p, n); want = n; }
        if (e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() { return reinterpret_cast<T*>(p); }
};

enum KernelId { K_GATHER = 0, K_DECODE_PAR, K_DECODE, K_SCATTER, K_RESOLVE, K_RESOLVE_BIG, K_PUG, K_CELL_HIST, K_EM, K_BOOT, K_COMPACT, K_ATAC, K_ATAC_PARSE, K_FIX_SLABS, K_P2_SPLIT, K_P2_PART, K_P2_SEARCH, K_P2_LONE, K_P2_GRAPH, K_ASORT_TABLE, K_ASORT_PARSE, K_ASORT_PART, K_ASORT_LEAF, K_ASORT_EMIT, K_GPL_PARSE, K_GPL_COUNT, K_GPL_COMPACT, K_GPL_TABLE, K_GPL_CORRECT, K_COLLATE_TABLE, K_COLLATE_MEASURE, K_COLLATE_SORT, K_COLLATE_SCAN, K_COLLATE_WRITE, K_ACOLLATE_TABLE, K_ACOLLATE_MEASURE, K_ACOLLATE_PLACE, K_ACOLLATE_WRITE, K_AGPL_PARSE, K_AGPL_BINS, K_GPLM_TABLE, K_GPLM_PARSE, K_COLLATEM_TABLE, K_COLLATEM_MEASURE, K_COLLATEM_SORT, K_COLLATEM_SCAN, K_COLLATEM_WRITE, K_CONVERT_WALK, K_CONVERT_RUNS, K_CONVERT_PLACE, K_CONVERT_WRITE, K_SNAPPY_BLOCKS, K_SNAPPY_PACK, K_SNAPPY_DECODE, K_CHUNK_TABLE, K_BGZF_INFLATE, K_COUNT };
inline constexpr const char* kKernelNames[K_COUNT] = {"k_gather_headers", "k_decode_par", "k_decode", "k_scatter",
                                                      "k_resolve", "k_resolve_big", "k_pug_cell", "k_cell_hist", "k_em", "k_boot", "k_compact", "k_atac_dedup", "k_atac_parse", "k_fix_slabs",
                                                      "k_p2_split", "k_p2_part", "k_p2_search", "k_p2_lone", "k_p2_graph",
                                                      "k_sort_table", "k_sort_parse", "k_sort_partition", "k_sort_leaf", "k_sort_emit",
                                                      "k_gpl_parse", "k_gpl_count", "k_gpl_compact", "k_gpl_table", "k_gpl_correct",
                                                      "k_collate_table", "k_collate_measure", "k_collate_sort", "k_collate_scan", "k_collate_write",
                                                      "k_atac_collate_table", "k_atac_collate_measure", "k_atac_collate_place", "k_atac_collate_write",
                                                      "k_atac_gpl_parse", "k_atac_gpl_bins",
                                                      "k_gpl_multi_table", "k_gpl_multi_parse",
                                                      "k_collate_multi_table", "k_collate_multi_measure", "k_collate_multi_sort", "k_collate_multi_scan", "k_collate_multi_write",
                                                      "k_convert_walk", "k_convert_runs", "k_convert_place", "k_convert_write",
                                                      "k_snappy_blocks", "k_snappy_pack", "k_snappy_decode", "k_collated_chunk_table", "k_bgzf_inflate"};

struct TimedLaunch { int id; hipEvent_t a, b; bool own_a = true; };   // own_a false: a is the b of the bracket in front (TimerChain) - it goes back to the event pool once

// Pinned, grow-only host array (D2H lands here directly; handed to the caller zero-copy).
template <class T>
struct PinnedVec {
    T* p = nullptr;
    size_t n = 0, cap = 0;
    hipError_t reserve(size_t want) {
        if (want <= cap) return hipSuccess;
        size_t nc = std::max(want + want / 4, (size_t)4096);
        T* q = nullptr;
        hipError_t e = hipHostMalloc((void**)&q, nc * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) return e;
        if (n) std::memcpy(q, p, n * sizeof(T));
        if (p) (void)hipHostFree(p);
        p = q; cap = nc;
        return hipSuccess;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = cap = 0; }
};

struct ResultPool;
struct HostResult {
    std::vector<uint64_t> cell_ptr, bc;
    std::vector<uint32_t> nrec;
    PinnedVec<uint32_t> gene;
    PinnedVec<float> val;
    std::vector<uint8_t> flags;
    // -d: gene-level equivalence classes per cell (cfg.dump_eq): CSR cell -> classes -> label words
    std::vector<uint64_t> eq_cell_ptr, eq_label_ptr;
    std::vector<uint32_t> eq_labels, eq_count;
    // -b: bootstrap mean / variance per cell, non-zero entries (cfg.num_bootstraps)
    std::vector<uint64_t> bm_ptr, bv_ptr;
    std::vector<uint32_t> bm_col, bv_col;
    std::vector<float> bm_val, bv_val;
    ResultPool* pool = nullptr;
    void clear() {
        cell_ptr.clear(); bc.clear(); nrec.clear(); flags.clear(); gene.n = 0; val.n = 0;
        eq_cell_ptr.clear(); eq_label_ptr.clear(); eq_labels.clear(); eq_count.clear();
        bm_ptr.clear(); bv_ptr.clear(); bm_col.clear(); bv_col.clear(); bm_val.clear(); bv_val.clear();
    }
};

// Results outlive a collect call (library-owned until afq_result_release), and pinning
// host memory is slow, so result storage is recycled through a small per-context pool.
struct ResultPool {
    std::mutex mu;
    std::vector<HostResult*> free_list;
    bool ctx_alive = true;
    int outstanding = 0;
};

struct Range { uint32_t c0, c1; };

struct RangeState;   // a range's device state: afq_api.cpp's

// afq_atac_dedup[_rad]'s device buffers, kept between calls (hipMalloc / hipFree of gigabytes is not free)
struct AtacBufs {
    DevBuf ref, start, flen, ptr, scr, oref, ostart, oflen, ocnt, on, optr, cref, cstart, cflen, ccnt, flag, cells, bm, cnt, bc, stat, walk, nwalk, status, tally, rstat, runctr;
    std::vector<DevBuf*> all() {
        return {&ref, &start, &flen, &ptr, &scr, &oref, &ostart, &oflen, &ocnt, &on, &optr, &cref, &cstart, &cflen, &ccnt, &flag, &cells, &bm, &cnt,
                &bc, &stat, &walk, &nwalk, &status, &tally, &rstat, &runctr};
    }
};

// afq_atac_sort_rad's
struct AtacSortBufs {
    DevBuf chunks, obs, rank, tkey, tval, rinfo, bbase, rbc, bin, key0, cstat, status, hist, cur, segs, ka, kb, andor, leaves, ids, on, lout, out, tally;
    std::vector<DevBuf*> all() {
        return {&chunks, &obs, &rank, &tkey, &tval, &rinfo, &bbase, &rbc, &bin, &key0, &cstat, &status, &hist, &cur, &segs, &ka, &kb, &andor,
                &leaves, &ids, &on, &lout, &out, &tally};
    }
};

// afq_gpl_hist_rad's and afq_gpl_correct's (afq_gpl_multi_hist_rad keeps its entry list and entry table in the correction's obs, idx, rkey, rval, cstatus)
struct GplBufs {
    DevBuf chunks, bc, cstat, status, tkey, tcnt, ones, okey, ocnt, nout;            // histogram
    DevBuf bbase, bins, bins64, bmax;                                                // afq_atac_gpl_hist_rad's position bins
    DevBuf obs, obscnt, ret, retcnt, idx, rkey, rval, dec, tgt, stats, tcount, cstatus;   // correction
    std::vector<DevBuf*> all() {
        return {&chunks, &bc, &cstat, &status, &tkey, &tcnt, &ones, &okey, &ocnt, &nout, &obs, &obscnt, &ret, &retcnt, &idx, &rkey, &rval, &dec, &tgt,
                &stats, &tcount, &cstatus, &bbase, &bins, &bins64, &bmax};
    }
};

// afq_collate_rad's, and afq_collate_multi_rad's (its sample entries and their table in sobs, sidx, skey, sval)
struct CollateBufs {
    DevBuf chunks, obs, val, tkey, tval, cells, rec, ka, kb, hist, bsum, ex, cstat, status, out, off, nrec;
    DevBuf sobs, sidx, skey, sval;
    std::vector<DevBuf*> all() {
        return {&chunks, &obs, &val, &tkey, &tval, &cells, &rec, &ka, &kb, &hist, &bsum, &ex, &cstat, &status, &out, &off, &nrec, &sobs, &sidx, &skey, &sval};
    }
};

// afq_atac_collate_rad's
struct AtacCollateBufs {
    DevBuf chunks, obs, val, tkey, tval, cells, cellof, ka, kb, hist, first, rank, cstat, status, out, off, nrec, ocell;
    std::vector<DevBuf*> all() { return {&chunks, &obs, &val, &tkey, &tval, &cells, &cellof, &ka, &kb, &hist, &first, &rank, &cstat, &status, &out, &off, &nrec, &ocell}; }
};

// the snappy frame encoder's (afq_snappy_frame_encode, and the collates' copy down under afq_set_collate_compress)
// and the decoder's (afq_snappy_frame_decode_device): two pieces of compressed bytes, the plan, status + tallies, the decoded bytes
struct SnappyBufs {
    DevBuf in, slots, meta, off, stream;
    DevBuf dec_in[2], dec_plan, dec_stat, dec_out;
    DevBuf ct_off, ct_nb, ct_nr, ct_bc, ct_stat;   // afq_collated_chunk_table's
    std::vector<DevBuf*> all() { return {&in, &slots, &meta, &off, &stream, &dec_in[0], &dec_in[1], &dec_plan, &dec_stat, &dec_out, &ct_off, &ct_nb, &ct_nr, &ct_bc, &ct_stat}; }
};

// afq_bgzf_inflate_device's: two pieces of compressed blocks, the plan, status + tallies, the inflated bytes
struct InflateBufs {
    DevBuf in[2], plan, stat, out;
    std::vector<DevBuf*> all() { return {&in[0], &in[1], &plan, &stat, &out}; }
};

// afq_convert_bam_rad's
struct ConvertBufs {
    DevBuf spans, scnt, sbase, ssum, roff, ridx, word, head, score, has, rfirst, rbc, rumi, rflag, rna, rmax, stat, key, rec, bsum, ex, dest, out, off, nrec, err, status;
    std::vector<DevBuf*> all() {
        return {&spans, &scnt, &sbase, &ssum, &roff, &ridx, &word, &head, &score, &has, &rfirst, &rbc, &rumi, &rflag, &rna, &rmax, &stat, &key, &rec, &bsum, &ex, &dest,
                &out, &off, &nrec, &err, &status};
    }
};

struct afq_ctx {
    afq_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t ref_count = 0;
    std::string err;
    std::mutex err_mu;   // (the upload thread of afq_submit reports through fail() too)
    DevBuf d_t2g;
    // input
    DevBuf d_bytes_own;
    const uint8_t* d_bytes = nullptr;
    size_t n_bytes = 0;
    DevBuf d_chunk_off, d_hdr;
    AtacBufs atac;
    AtacSortBufs asort;
    GplBufs gpl;
    CollateBufs collate;
    AtacCollateBufs acollate;
    ConvertBufs convert;
    SnappyBufs snappy;
    InflateBufs inflate;
    void* stage[3] = {nullptr, nullptr, nullptr};          // pinned staging for large host->device input copies
    hipEvent_t stage_ev[3] = {nullptr, nullptr, nullptr};
    // afq_submit: the input crosses PCIe range by range while earlier ranges already run (h2d_ev[i] = range i's bytes landed)
    std::vector<hipEvent_t> h2d_ev;
    bool h2d_piped = false;
    std::mutex up_mu;
    std::condition_variable up_cv;
    size_t up_enqueued = 0;
    int up_rc = 0;
    std::string up_err;
    // Two sets of per-range device state: while the rows of range i cross PCIe, the kernels of range i+1 run.
    RangeState* rs = nullptr;   // (the pair is made by afq_create: the type is afq_api.cpp's own)
    // The rows cross on a stream of their own, range behind range, and the host does not wait for them until afq_collect
    // (finish_range; DESIGN.md 3.1 "Round 11").  It never holds a kernel.
    hipStream_t copy_stream = nullptr;
    DevBuf d_kick;                   // a few bytes that go up in front of every range's rows (finish_range says why)
    void* h_kick = nullptr;          // ... out of pinned memory that never changes
    bool copies_in_flight = false;   // row copies enqueued since the copy stream was last drained
    bool in_retry = false;           // finish_range is running a range again: the nested ranges take the waiting path
    uint64_t n_pipe[4] = {0};        // afq_range_pipeline_counts
    uint64_t last_total = 0;         // rows of the batch collected last: begin_batch sizes the result arrays from it
    bool all_aligned = true;  // every chunk offset is a multiple of 4
    // 1/2-byte barcode or UMI fields: the batch is rewritten on the device with 4-byte fields (k_widen) and everything
    // downstream works on that copy - w_off / w_nbytes are the chunks of the copy, chunk_off / hdr stay the caller's
    bool widen = false;
    uint32_t eff_bc = 0, eff_umi = 0;
    // afq_set_aln_extra_bytes: every alignment word of a record is followed by a position of this many bytes (0: none).  Such a
    // batch always takes the copy: k_strip_aln writes it without the positions (and with the widened fields)
    uint32_t aln_extra = 0;
    // afq_set_collate_compress: the three collates hand their chunk bytes out as a snappy frame stream, encoded on the device
    bool collate_compress = false;
    std::vector<uint64_t> w_off;
    std::vector<uint32_t> w_nbytes;
    uint64_t wide_bytes = 0;
    DevBuf d_wide;
    ResultPool* pool = nullptr;
    // host planning state
    std::vector<uint64_t> chunk_off;
    std::vector<uint32_t> hdr;  // nbytes, nrec per cell
    std::vector<Range> ranges;
    size_t next_range = 0;
    uint64_t first_cell_index = 0;
    uint32_t n_cells = 0;
    bool pending = false;
    HostResult* res = nullptr;
    // stats / timers
    afq_batch_stats stats{};
    uint64_t n_label_rehash = 0;   // ranges decoded again under another label-hash salt (life of the context)
    uint64_t n_pool_regrow = 0;    // ranges run again with a larger parsimony pool
    uint64_t n_mono_cells = 0;     // parsimony cells resolved by the one-workgroup kernel (sent there directly, or handed back by the phase kernels)
    uint64_t n_divert = 0;         // buckets the hash resolve of the last batch handed to the sort path
    uint64_t n_em_resized = 0;     // ranges whose EM scratch was sized on the host after the device-side plan did not fit
    uint64_t n_em_inst[6] = {0};   // cells of the last batch per rounds instance of the order-free EM (tiers 0-4), then tier 4 cells with 32-bit ids
    bool handback_seen = false;    // the phase kernels have handed a cell back to the one-workgroup kernel in some range of this context
    uint32_t retry_cuts = 0;       // how many times the range being finished has been cut around a failing cell (finish_range)
    uint32_t retry_halvings = 0, retry_halving_cap = 0;   // ... halved after a range-wide failure, and how often it may be (finish_range)
    std::vector<TimedLaunch> launches;
    std::vector<hipEvent_t> event_pool;
    double k_ms[K_COUNT] = {0};
    uint32_t k_launches[K_COUNT] = {0};
};

inline int fail(afq_ctx* c, int code, const std::string& msg) {
    if (c) { std::lock_guard<std::mutex> g(c->err_mu); c->err = msg; } else g_create_err = msg;
    return code;
}
#define HIP_TRY(c, expr)                                                                          \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess)                                                                    \
            return fail((c), e__ == hipErrorOutOfMemory ? AFQ_ERR_OOM : AFQ_ERR_HIP,              \
                        std::string(#expr) + ": " + hipGetErrorString(e__));                      \
    } while (0)

// The first error of a run of HIP calls; the calls behind it are skipped (`if (T.ok())`) or made and ignored.
struct HipLatch {
    hipError_t e = hipSuccess;
    void operator()(hipError_t x) { if (e == hipSuccess) e = x; }
    bool ok() const { return e == hipSuccess; }
    int fail(afq_ctx* c, const char* who, const std::string& detail = "") const {
        (void)hipGetLastError();   // (the runtime keeps the error until it is read)
        return ::fail(c, e == hipErrorOutOfMemory ? AFQ_ERR_OOM : AFQ_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e) + detail);
    }
};

inline void reset_kernel_times(afq_ctx* c) { for (int i = 0; i < K_COUNT; ++i) { c->k_ms[i] = 0; c->k_launches[i] = 0; } }

inline hipEvent_t get_event(afq_ctx* c) {
    if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

struct ScopedTimer {
    afq_ctx* c; int id; hipStream_t s; std::vector<TimedLaunch>* sink; hipEvent_t a = nullptr, b = nullptr;
    ScopedTimer(afq_ctx* c_, int id_, hipStream_t s_ = nullptr, std::vector<TimedLaunch>* sink_ = nullptr)
        : c(c_), id(id_), s(s_ ? s_ : c_->stream), sink(sink_ ? sink_ : &c_->launches) {
        if (c->cfg.profile) { a = get_event(c); b = get_event(c); (void)hipEventRecord(a, s); }
    }
    ~ScopedTimer() {
        if (c->cfg.profile) { (void)hipEventRecord(b, s); sink->push_back({id, a, b}); }
    }
};

inline void recycle_events(afq_ctx* c, const TimedLaunch& t) {
    if (t.own_a) c->event_pool.push_back(t.a);
    c->event_pool.push_back(t.b);
}

inline void harvest_timers(afq_ctx* c, std::vector<TimedLaunch>* list = nullptr) {
    if (list) { c->launches.insert(c->launches.end(), list->begin(), list->end()); list->clear(); }
    for (auto& t : c->launches) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) { c->k_ms[t.id] += ms; c->k_launches[t.id] += 1; }
        recycle_events(c, t);
    }
    c->launches.clear();
}

inline bool valid_width(uint32_t w) { return w == 1 || w == 2 || w == 4 || w == 8; }

// The ATAC entry points hand out gigabytes of results: into pageable malloc memory the D2H runs at a fraction of the link.
// Their output arrays are pinned instead and recycled through a process-wide pool (afq_free returns them to it).
struct PinnedPool {
    std::mutex mu;
    struct Ent { void* p; size_t cap; bool busy; };
    std::vector<Ent> ents;
    void* get(size_t n) {
        std::lock_guard<std::mutex> g(mu);
        Ent* best = nullptr;
        for (auto& e : ents) if (!e.busy && e.cap >= n && (!best || e.cap < best->cap)) best = &e;
        if (best) { best->busy = true; return best->p; }
        void* q = nullptr;
        const size_t cap = n + n / 8 + 4096;
        if (hipHostMalloc(&q, cap, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        ents.push_back({q, cap, true});
        return q;
    }
    bool put(void* p) {
        std::lock_guard<std::mutex> g(mu);
        for (auto& e : ents) if (e.p == p) { e.busy = false; return true; }
        return false;
    }
};
inline PinnedPool* pinned_pool() { static PinnedPool* P = new PinnedPool(); return P; }
// What an ATAC call hands out: arrays from pinned_pool() or malloc, given back (afq_free takes either) unless release()d into the
// caller's out-parameters on success.  Copies and threads may still be writing into a block when an exit is taken, so before one
// of these is destroyed or free_all()ed after work was started on its blocks: the filler threads are joined and both streams are
// synchronised (atac_dedup_piped does that ahead of its first exit), and the pipeline's `runs` and `pin` go back to the pool
// before a redo falls through to the plain route, which draws on the same pool.
struct HostOuts {
    void* p[6] = {};
    int n = 0;
    void* keep(void* q) { if (q) p[n++] = q; return q; }
    void* pinned(size_t bytes) { return keep(pinned_pool()->get(bytes)); }
    void* mallocd(size_t bytes) { return keep(std::malloc(bytes)); }
    void free_all() { while (n) afq_free(p[--n]); }
    void release() { n = 0; }
    ~HostOuts() { free_all(); }
};

// afq_api.cpp: large host input to the device through pinned pieces (memory the caller pinned goes straight to the DMA engine)
struct ByteSource;
bool host_ptr_is_pinned(const void* p);
unsigned stage_threads();
hipStream_t second_stream(afq_ctx* c);   // a stream beside c->stream that is idle outside a quant batch (range slot 0's)
int staged_h2d(afq_ctx* c, uint8_t* dst, const uint8_t* src, size_t n, hipStream_t s, bool pinned, const ByteSource* rd = nullptr, uint64_t rd_off = 0);

// afq_api_rad.cpp: the checks of afq_chunk_table.h with the entry points' error texts, and the chunk headers they are made on
int chunk_fault(afq_ctx* c, const char* noun, uint32_t i, ChunkFault f);
int check_chunk_offsets(afq_ctx* c, const uint64_t* chunk_off, uint32_t n, size_t n_bytes, const char* noun);
int fetch_chunk_headers(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n, bool on_device, uint32_t* hdr, const char* noun = "cell", bool timed = false);
// ... and host bytes of a pass to the device (c->d_bytes_own); an allocation that fails is left in T, for the caller to word
int stage_rad_bytes(afq_ctx* c, HipLatch& T, const uint8_t* bytes, size_t n_bytes, bool on_device, hipStream_t s, const uint8_t** d_bytes);

// What a record pass takes of the device beside its input, in the terms of the one refusal (RadPass::fits); the counts are the entry's.
struct RadNeed {
    uint64_t rec = 0, tab_misc = 0;     // "for N records", and the tables with the rest
    std::string tables = "of tables";   // how the entry words tab_misc
    bool has_out = false;               // the collates: "up to `out` of output", and the snappy encoder's bytes beside it (0: not asked for)
    uint64_t out = 0, snappy = 0;
};

// The record pass of the *_rad entry points over an uncollated RAD (afq_api_rad.cpp): the chunk table and the record ceiling, the
// fit check, the input and the chunk table on the device, and - behind the entry's parse or measure launch - the status word and
// the chunks' counters back.  What lies between is the entry's: its `ensure`s on T, its table uploads and memsets, its kernels.
struct RadPass {
    const char* who;                // the entry's name in messages
    std::string detail;             // what hip_fail says behind the records: ", 12 cells"
    std::vector<SortChunk> chunks;
    const uint8_t* bytes = nullptr;
    uint64_t n_bytes = 0, n_slots = 0;
    uint32_t n_chunks = 0;
    bool on_device = false;
    HipLatch T;
    const uint8_t* d_bytes = nullptr;   // where the kernels read the input (stage)
    DevStatus st{};                     // read_back's: the status word ...
    std::vector<uint32_t> cstat;        // ... and [n_chunks][words_per_chunk] counters, the entry's to sum
    int hip_fail(afq_ctx* c) const {
        return T.fail(c, who, " (" + std::to_string(n_bytes) + " input bytes, " + std::to_string(n_slots) + " records" + detail + ")");
    }
    // every header fetched and checked (`min_rec`: a record without alignments); 2^ceiling_log2 records and more are refused, `tail` behind the count
    int open(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, bool on_device, uint32_t min_rec, uint32_t ceiling_log2,
             const char* tail = ": fill the device in smaller parts");
    int fits(afq_ctx* c, const RadNeed& need);
    // behind the entry's `ensure`s (T holds their first failure) and in front of its own uploads
    int stage(afq_ctx* c, DevBuf& chunks_buf);
    // the launches' error, status and counters down, one sync (it also waits for copies the entry enqueued on T just before), the lap, the refusals
    int read_back(afq_ctx* c, HostClock& hc, DevBuf& status_buf, DevBuf& cstat_buf, uint32_t words_per_chunk, const char* lap, const char* start_range = nullptr);
};

#pragma GCC visibility pop
