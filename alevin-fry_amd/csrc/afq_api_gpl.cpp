// afq_api_gpl.cpp — generate-permit-list: the three *_hist_rad entry points, their limits and table slots, afq_gpl_correct.
#include "afq_ctx.h"
#include "afq_gpl_host.h"

// The barcode column of a parse (c->gpl.bc; chunk i's first cstat[4 i + 1] slots) through the counting table: the distinct barcodes
// with their counts, ascending.  afq_gpl_hist_rad's and afq_atac_gpl_hist_rad's.
static int gpl_count_sorted(afq_ctx* c, RadPass& P, uint64_t n_kept, uint32_t bc_bytes, std::vector<std::pair<uint64_t, uint64_t>>& pairs) {
    auto& B = c->gpl;
    HipLatch& T = P.T;
    const char* const who = P.who;
    hipStream_t s = c->stream;
    DevStatus st{};
    const uint64_t cap = gpl_table_capacity(n_kept, bc_bytes);
    T(B.tkey.ensure(8 * cap)); T(B.tcnt.ensure(8 * cap)); T(B.okey.ensure(4 * cap)); T(B.ocnt.ensure(4 * cap));   // (at most cap / 2 distinct barcodes)
    if (!T.ok()) return P.hip_fail(c);
    T(hipMemsetAsync(B.tkey.p, 0xFF, 8 * cap, s));
    T(hipMemsetAsync(B.tcnt.p, 0, 8 * cap, s));
    {
        ScopedTimer t(c, K_GPL_COUNT, s);
        launch_gpl_count(s, B.chunks.as<SortChunk>(), P.n_chunks, B.cstat.as<uint32_t>(), B.bc.as<uint64_t>(), B.tkey.as<uint64_t>(), B.tcnt.as<unsigned long long>(),
                         (uint32_t)(cap - 1), B.ones.as<unsigned long long>(), B.status.as<DevStatus>());
    }
    {
        ScopedTimer t(c, K_GPL_COMPACT, s);
        launch_gpl_compact(s, B.tkey.as<uint64_t>(), B.tcnt.as<unsigned long long>(), cap, B.okey.as<uint64_t>(), B.ocnt.as<uint64_t>(), B.nout.as<uint32_t>());
    }
    T(hipGetLastError());
    uint32_t n_tab = 0;
    unsigned long long n_ones = 0;
    T(hipMemcpyAsync(&st, B.status.p, sizeof(st), hipMemcpyDeviceToHost, s));
    T(hipMemcpyAsync(&n_tab, B.nout.p, 4, hipMemcpyDeviceToHost, s));
    T(hipMemcpyAsync(&n_ones, B.ones.p, 8, hipMemcpyDeviceToHost, s));
    T(hipStreamSynchronize(s));
    if (!T.ok()) return P.hip_fail(c);
    if (st.err_code) { harvest_timers(c); return fail(c, AFQ_ERR_HIP, std::string(who) + ": the counting table of " + std::to_string(cap) + " slots ran full (device status " + std::to_string(st.err_code) + ")"); }
    if (n_tab > cap / 2) return fail(c, AFQ_ERR_HIP, std::string(who) + ": " + std::to_string(n_tab) + " keys in a table of " + std::to_string(cap) + " slots");
    pairs.assign((size_t)n_tab + (n_ones ? 1 : 0), {0, 0});
    {
        std::vector<uint64_t> k(n_tab), n(n_tab);
        if (n_tab) {
            T(hipMemcpyAsync(k.data(), B.okey.p, 8ull * n_tab, hipMemcpyDeviceToHost, s));
            T(hipMemcpyAsync(n.data(), B.ocnt.p, 8ull * n_tab, hipMemcpyDeviceToHost, s));
            T(hipStreamSynchronize(s));
        }
        harvest_timers(c);
        if (!T.ok()) return P.hip_fail(c);
        for (uint32_t i = 0; i < n_tab; ++i) pairs[i] = {k[i], n[i]};
        if (n_ones) pairs[n_tab] = {kSortEmptyKey, (uint64_t)n_ones};
    }
    std::sort(pairs.begin(), pairs.end());
    return 0;
}

// The pairs of gpl_count_sorted count every record the parse put into the barcode column: `expect` of them, which the entry
// point calls `what`.
static int gpl_check_total(afq_ctx* c, const char* who, const std::vector<std::pair<uint64_t, uint64_t>>& pairs, uint64_t expect, const char* what) {
    uint64_t total = 0;
    for (const auto& pr : pairs) total += pr.second;
    if (total == expect) return 0;
    return fail(c, AFQ_ERR_HIP, std::string(who) + ": the table counts " + std::to_string(total) + " of " + std::to_string(expect) + " " + what);
}

// The pairs as the histogram a single-barcode pass hands over: barcodes and counts in blocks of H; with `obins`, a block for n_bins
// position bins beside them (`atac generate-permit-list`'s, which fills it).
static int gpl_hist_out(afq_ctx* c, const char* who, const std::vector<std::pair<uint64_t, uint64_t>>& pairs, HostOuts& H, uint64_t** obc, uint64_t** ocnt,
                        uint64_t n_bins = 0, uint64_t** obins = nullptr) {
    const uint64_t n_out = pairs.size(), o1 = std::max<uint64_t>(n_out, 1);
    *obc = (uint64_t*)H.mallocd(8 * o1);
    *ocnt = (uint64_t*)H.mallocd(8 * o1);
    if (obins) *obins = n_bins ? (uint64_t*)H.mallocd(8ull * n_bins) : nullptr;
    if (!*obc || !*ocnt || (n_bins && !*obins))
        return fail(c, AFQ_ERR_OOM, std::string(who) + ": host allocation failed (" + std::to_string(16 * o1 + 8ull * n_bins) + " bytes of histogram" + (obins ? " and bins)" : ")"));
    for (uint64_t i = 0; i < n_out; ++i) { (*obc)[i] = pairs[i].first; (*ocnt)[i] = pairs[i].second; }
    return 0;
}

// `generate-permit-list` on the device (afq_gpl.hip): parse + orientation filter, counting table, compaction; the host sorts the
// distinct barcodes.  And the correction decisions of distinct observed barcodes against a retained set.
void afq_gpl_limits(uint32_t out[4]) {
    if (!out) return;
    out[0] = kGplParseTile; out[1] = kGplParseHalo; out[2] = kGplLaneAlns; out[3] = 0;
}

void afq_gpl_table_slot(uint64_t barcode, uint64_t n_kept, uint32_t bc_bytes, uint32_t* home_slot, uint32_t* capacity) {
    const uint64_t cap = gpl_table_capacity(n_kept < (1ull << 30) ? n_kept : (1ull << 30) - 1, valid_width(bc_bytes) ? bc_bytes : 8);   // (afq_gpl_hist_rad refuses 2^30 records and more)
    if (home_slot) *home_slot = sort_hash_bc(barcode) & (uint32_t)(cap - 1);
    if (capacity) *capacity = (uint32_t)cap;
}

int afq_gpl_hist_rad(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t bc_bytes,
                     uint32_t umi_bytes, uint32_t expected_ori, int bytes_on_device, uint64_t* out_n, uint64_t** out_bc, uint64_t** out_count,
                     afq_gpl_hist_stats* stats) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!bytes && n_bytes) || (!chunk_off && n_chunks) || !out_n || !out_bc || !out_count) return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    if (!valid_width(bc_bytes)) return fail(c, AFQ_ERR_INVALID_ARG, "bc_bytes must be 1, 2, 4 or 8");
    if (!valid_width(umi_bytes)) return fail(c, AFQ_ERR_INVALID_ARG, "umi_bytes must be 1, 2, 4 or 8");
    if (expected_ori > kGplOriRc) return fail(c, AFQ_ERR_INVALID_ARG, "expected_ori must be 0 (both), 1 (fw) or 2 (rc)");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    hipStream_t s = c->stream;
    // ---- chunk table
    RadPass P{"afq_gpl_hist_rad"};
    if (int rc = P.open(c, bytes, n_bytes, chunk_off, n_chunks, bytes_on_device != 0, 4 + bc_bytes + umi_bytes, 30)) return rc;
    const uint64_t n_slots = P.n_slots;
    const uint64_t s1 = std::max<uint64_t>(n_slots, 1), nc1 = std::max<uint32_t>(n_chunks, 1);
    {   // does it fit?  (input + staging, 8 bytes a record of parse output, 16 a slot of the largest table, 16 a distinct barcode)
        const uint64_t need_rec = s1 * 8, need_tab = gpl_table_capacity(n_slots, bc_bytes) * 24, need_misc = nc1 * (sizeof(SortChunk) + 16);
        if (int rc = P.fits(c, RadNeed{need_rec, need_tab + need_misc})) return rc;
    }
    auto& B = c->gpl;
    HipLatch& T = P.T;
    T(B.chunks.ensure(sizeof(SortChunk) * nc1)); T(B.bc.ensure(8 * s1)); T(B.cstat.ensure(16ull * nc1)); T(B.status.ensure(sizeof(DevStatus)));
    T(B.ones.ensure(8)); T(B.nout.ensure(4));
    if (int rc = P.stage(c, B.chunks)) return rc;
    T(hipMemsetAsync(B.status.p, 0, sizeof(DevStatus), s));
    T(hipMemsetAsync(B.ones.p, 0, 8, s));
    T(hipMemsetAsync(B.nout.p, 0, 4, s));
    if (!T.ok()) return P.hip_fail(c);
    reset_kernel_times(c);
    {
        ScopedTimer t(c, K_GPL_PARSE, s);
        launch_gpl_parse(s, GplParseArgs{P.d_bytes, (uint64_t)n_bytes, B.chunks.as<SortChunk>(), n_chunks, bc_bytes, umi_bytes, c->aln_extra, expected_ori,
                                         B.bc.as<uint64_t>(), B.cstat.as<uint32_t>(), B.status.as<DevStatus>()});
    }
    if (int rc = P.read_back(c, hc, B.status, B.cstat, 4, "gpl: parse")) return rc;
    const std::vector<uint32_t>& cstat = P.cstat;
    afq_gpl_hist_stats S{};
    for (uint32_t i = 0; i < n_chunks; ++i) {
        S.n_records += cstat[4 * i]; S.n_compatible += cstat[4 * i + 1]; S.max_ambig = std::max<uint64_t>(S.max_ambig, cstat[4 * i + 2]); S.n_long_records += cstat[4 * i + 3];
    }
    // ---- count, compact
    std::vector<std::pair<uint64_t, uint64_t>> pairs;
    if (int rc = gpl_count_sorted(c, P, S.n_compatible, bc_bytes, pairs)) return rc;
    hc.lap("gpl: count + compact + sort");
    if (int rc = gpl_check_total(c, "afq_gpl_hist_rad", pairs, S.n_compatible, "compatible records")) return rc;
    HostOuts H;
    uint64_t *obc = nullptr, *ocnt = nullptr;
    if (int rc = gpl_hist_out(c, "afq_gpl_hist_rad", pairs, H, &obc, &ocnt)) return rc;
    if (stats) *stats = S;
    H.release();
    *out_n = pairs.size(); *out_bc = obc; *out_count = ocnt;
    return 0;
}

// multi-barcode `generate-permit-list` on the device (afq_gpl_multi.hip): entry table, parse + orientation filter + routing; the
// counting table and its compaction are afq_gpl_hist_rad's, over the keys entry << 32 | b1.
void afq_gpl_multi_limits(uint32_t out[4]) {
    if (!out) return;
    out[0] = kGplParseTile; out[1] = kGplParseHalo; out[2] = kGplLaneAlns; out[3] = 0;
}

int afq_gpl_multi_hist_rad(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t b0_bytes,
                           uint32_t b1_bytes, uint32_t umi_bytes, uint32_t expected_ori, int bytes_on_device, const uint64_t* sample_observed,
                           uint64_t n_entries, uint64_t* out_n, uint32_t** out_entry, uint64_t** out_cell, uint64_t** out_count,
                           afq_gpl_multi_hist_stats* stats) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!bytes && n_bytes) || (!chunk_off && n_chunks) || (!sample_observed && n_entries) || !out_n || !out_entry || !out_cell || !out_count)
        return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    {   // widths, orientation, the entry list (afq_gpl_host.h: the CPU suite runs these checks without a device)
        std::string e;
        if (int rc = gplhost::multi_check_args(b0_bytes, b1_bytes, umi_bytes, expected_ori, sample_observed, n_entries, e)) return fail(c, rc, e);
    }
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    hipStream_t s = c->stream;
    // ---- chunk table
    RadPass P{"afq_gpl_multi_hist_rad", ", " + std::to_string(n_entries) + " routing entries"};
    if (int rc = P.open(c, bytes, n_bytes, chunk_off, n_chunks, bytes_on_device != 0, 4 + b0_bytes + b1_bytes + umi_bytes, 30)) return rc;
    const uint64_t n_slots = P.n_slots;
    const uint64_t s1 = std::max<uint64_t>(n_slots, 1), nc1 = std::max<uint32_t>(n_chunks, 1), ne1 = std::max<uint64_t>(n_entries, 1), ecap = sort_table_capacity(n_entries);
    {   // does it fit?  (input + staging, 8 bytes a record of parse output, 24 a slot of the largest counting table, 12 an entry and 12 a slot of its table)
        const uint64_t need_rec = s1 * 8, need_tab = gpl_table_capacity(n_slots, 8) * 24 + ne1 * 12 + ecap * 12, need_misc = nc1 * (sizeof(SortChunk) + 16);
        if (int rc = P.fits(c, RadNeed{need_rec, need_tab + need_misc, "of tables (" + std::to_string(n_entries) + " routing entries)"})) return rc;
    }
    auto& B = c->gpl;
    HipLatch& T = P.T;
    T(B.chunks.ensure(sizeof(SortChunk) * nc1)); T(B.bc.ensure(8 * s1)); T(B.cstat.ensure(16ull * nc1)); T(B.status.ensure(sizeof(DevStatus)));
    T(B.ones.ensure(8)); T(B.nout.ensure(4));
    T(B.obs.ensure(8 * ne1)); T(B.idx.ensure(4 * ne1)); T(B.rkey.ensure(8 * ecap)); T(B.rval.ensure(4 * ecap)); T(B.cstatus.ensure(sizeof(DevStatus)));
    if (int rc = P.stage(c, B.chunks)) return rc;
    std::vector<uint32_t> idx(n_entries);
    for (uint64_t i = 0; i < n_entries; ++i) idx[i] = (uint32_t)i;
    if (n_entries) {
        T(hipMemcpyAsync(B.obs.p, sample_observed, 8 * n_entries, hipMemcpyHostToDevice, s));
        T(hipMemcpyAsync(B.idx.p, idx.data(), 4 * n_entries, hipMemcpyHostToDevice, s));
    }
    T(hipMemsetAsync(B.rkey.p, 0xFF, 8 * ecap, s));
    T(hipMemsetAsync(B.status.p, 0, sizeof(DevStatus), s));
    T(hipMemsetAsync(B.cstatus.p, 0, sizeof(DevStatus), s));
    T(hipMemsetAsync(B.ones.p, 0, 8, s));
    T(hipMemsetAsync(B.nout.p, 0, 4, s));
    if (!T.ok()) return P.hip_fail(c);
    reset_kernel_times(c);
    {
        ScopedTimer t(c, K_GPLM_TABLE, s);
        launch_sort_table(s, B.obs.as<uint64_t>(), B.idx.as<uint32_t>(), n_entries, B.rkey.as<uint64_t>(), B.rval.as<uint32_t>(), (uint32_t)(ecap - 1), B.cstatus.as<DevStatus>());
    }
    {
        ScopedTimer t(c, K_GPLM_PARSE, s);
        launch_gpl_multi_parse(s, GplMultiParseArgs{P.d_bytes, (uint64_t)n_bytes, B.chunks.as<SortChunk>(), n_chunks, b0_bytes, b1_bytes, umi_bytes, c->aln_extra, expected_ori,
                                                    B.rkey.as<uint64_t>(), B.rval.as<uint32_t>(), (uint32_t)(ecap - 1), B.bc.as<uint64_t>(), B.cstat.as<uint32_t>(),
                                                    B.status.as<DevStatus>()});
    }
    DevStatus tst{};   // (the entry table's status comes down in the pass's sync; multi_check_args has refused what could set it)
    T(hipMemcpyAsync(&tst, B.cstatus.p, sizeof(tst), hipMemcpyDeviceToHost, s));
    if (int rc = P.read_back(c, hc, B.status, B.cstat, 4, "gpl multi: table + parse")) return rc;
    if (tst.err_code) { harvest_timers(c); return fail(c, AFQ_ERR_HIP, "afq_gpl_multi_hist_rad: entry table status " + std::to_string(tst.err_code) + " at entry " + std::to_string(tst.err_cell)); }
    const std::vector<uint32_t>& cstat = P.cstat;
    afq_gpl_multi_hist_stats S{};
    for (uint32_t i = 0; i < n_chunks; ++i) {
        S.n_records += cstat[4 * i]; S.n_routed += cstat[4 * i + 1]; S.n_unrouted += cstat[4 * i + 2]; S.n_long_records += cstat[4 * i + 3];
    }
    S.n_compatible = S.n_routed + S.n_unrouted;
    // ---- count, compact (chunk i's first cstat[4 i + 1] slots hold its keys)
    std::vector<std::pair<uint64_t, uint64_t>> pairs;
    if (int rc = gpl_count_sorted(c, P, S.n_routed, 8, pairs)) return rc;
    hc.lap("gpl multi: count + compact + sort");
    if (int rc = gpl_check_total(c, "afq_gpl_multi_hist_rad", pairs, S.n_routed, "routed records")) return rc;
    const uint64_t n_out = pairs.size(), o1 = std::max<uint64_t>(n_out, 1);
    HostOuts H;
    uint32_t* oent = (uint32_t*)H.mallocd(4 * o1);
    uint64_t* ocell = (uint64_t*)H.mallocd(8 * o1);
    uint64_t* ocnt = (uint64_t*)H.mallocd(8 * o1);
    if (!oent || !ocell || !ocnt) return fail(c, AFQ_ERR_OOM, "afq_gpl_multi_hist_rad: host allocation failed (" + std::to_string(20 * o1) + " bytes of histogram)");
    for (uint64_t i = 0; i < n_out; ++i) { oent[i] = (uint32_t)(pairs[i].first >> 32); ocell[i] = pairs[i].first & 0xFFFFFFFFull; ocnt[i] = pairs[i].second; }
    if (stats) *stats = S;
    H.release();
    *out_n = n_out; *out_entry = oent; *out_cell = ocell; *out_count = ocnt;
    return 0;
}

// `atac generate-permit-list` on the device (afq_atac_gpl.hip): one walk for the barcode column, the largest na and the position
// bins; the counting table and its compaction are afq_gpl_hist_rad's.
void afq_atac_gpl_limits(uint32_t out[4]) {
    if (!out) return;
    out[0] = kSortParseTile; out[1] = kSortParseHalo; out[2] = 0; out[3] = 0;   // ([2]: the bins are counted in global memory, no workgroup holds any)
}

int afq_atac_gpl_hist_rad(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t bc_bytes,
                          int bytes_on_device, const uint64_t* bin_base, uint32_t ref_count, uint32_t bin_size, uint64_t* out_n, uint64_t** out_bc,
                          uint64_t** out_count, uint64_t** out_bins, afq_atac_gpl_hist_stats* stats) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!bytes && n_bytes) || (!chunk_off && n_chunks) || !bin_base || !out_n || !out_bc || !out_count || !out_bins) return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    if (!valid_width(bc_bytes)) return fail(c, AFQ_ERR_INVALID_ARG, "bc_bytes must be 1, 2, 4 or 8");
    if (!bin_size) return fail(c, AFQ_ERR_INVALID_ARG, "bin_size must be at least 1");
    if (bin_base[0] != 0) return fail(c, AFQ_ERR_INVALID_ARG, "bin_base[0] must be 0");
    for (uint32_t r = 0; r < ref_count; ++r)
        if (bin_base[r + 1] < bin_base[r]) return fail(c, AFQ_ERR_INVALID_ARG, "bin_base must ascend (entry " + std::to_string(r + 1) + " is below the one in front)");
    if (bin_base[ref_count] >= (1ull << 31)) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_atac_gpl_hist_rad: 2^31 or more position bins (" + std::to_string(bin_base[ref_count]) + ")");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    hipStream_t s = c->stream;
    const uint32_t n_bins = (uint32_t)bin_base[ref_count];
    std::vector<uint32_t> bbase(std::max<uint32_t>(ref_count, 1), 0);
    for (uint32_t r = 0; r < ref_count; ++r) bbase[r] = (uint32_t)bin_base[r];
    // ---- chunk table
    RadPass P{"afq_atac_gpl_hist_rad", ", " + std::to_string(n_bins) + " bins"};
    if (int rc = P.open(c, bytes, n_bytes, chunk_off, n_chunks, bytes_on_device != 0, 4 + bc_bytes, 30)) return rc;
    const uint64_t n_slots = P.n_slots;
    const uint64_t s1 = std::max<uint64_t>(n_slots, 1), nc1 = std::max<uint32_t>(n_chunks, 1), nb1 = std::max<uint32_t>(n_bins, 1);
    {   // does it fit?  (input + staging, 8 bytes a record of parse output, 24 a slot of the largest table, 12 a bin)
        const uint64_t need_rec = s1 * 8, need_tab = gpl_table_capacity(n_slots, bc_bytes) * 24, need_misc = nc1 * (sizeof(SortChunk) + 16) + 12ull * nb1 + 4ull * bbase.size();
        if (int rc = P.fits(c, RadNeed{need_rec, need_tab + need_misc, "of tables and bins"})) return rc;
    }
    auto& B = c->gpl;
    HipLatch& T = P.T;
    T(B.chunks.ensure(sizeof(SortChunk) * nc1)); T(B.bc.ensure(8 * s1)); T(B.cstat.ensure(16ull * nc1)); T(B.status.ensure(sizeof(DevStatus)));
    T(B.ones.ensure(8)); T(B.nout.ensure(4)); T(B.bbase.ensure(4ull * bbase.size())); T(B.bins.ensure(4ull * nb1)); T(B.bins64.ensure(8ull * nb1)); T(B.bmax.ensure(4));
    if (int rc = P.stage(c, B.chunks)) return rc;
    T(hipMemcpyAsync(B.bbase.p, bbase.data(), 4ull * bbase.size(), hipMemcpyHostToDevice, s));
    T(hipMemsetAsync(B.status.p, 0, sizeof(DevStatus), s));
    T(hipMemsetAsync(B.ones.p, 0, 8, s));
    T(hipMemsetAsync(B.nout.p, 0, 4, s));
    T(hipMemsetAsync(B.bins.p, 0, 4ull * nb1, s));
    T(hipMemsetAsync(B.bmax.p, 0, 4, s));
    if (!T.ok()) return P.hip_fail(c);
    reset_kernel_times(c);
    {
        ScopedTimer t(c, K_AGPL_PARSE, s);
        launch_atac_gpl_parse(s, AtacGplParseArgs{P.d_bytes, (uint64_t)n_bytes, B.chunks.as<SortChunk>(), n_chunks, bc_bytes, B.bbase.as<uint32_t>(), ref_count, n_bins,
                                                  bin_size, B.bc.as<uint64_t>(), B.bins.as<uint32_t>(), B.cstat.as<uint32_t>(), B.status.as<DevStatus>()});
    }
    {
        ScopedTimer t(c, K_AGPL_BINS, s);
        launch_atac_gpl_bins(s, B.bins.as<uint32_t>(), n_bins, B.bins64.as<uint64_t>(), B.bmax.as<uint32_t>());
    }
    uint32_t max_bin = 0;   // (comes down in the pass's sync)
    T(hipMemcpyAsync(&max_bin, B.bmax.p, 4, hipMemcpyDeviceToHost, s));
    if (int rc = P.read_back(c, hc, B.status, B.cstat, 4, "atac gpl: parse + bins", ("a start position's bin is not below the number of bins (" + std::to_string(n_bins) + ")").c_str()))
        return rc;
    const std::vector<uint32_t>& cstat = P.cstat;
    afq_atac_gpl_hist_stats S{};
    for (uint32_t i = 0; i < n_chunks; ++i) {
        S.n_unmapped += cstat[4 * i]; S.n_records += cstat[4 * i + 1]; S.max_ambig = std::max<uint64_t>(S.max_ambig, cstat[4 * i + 2]); S.n_multimapped += cstat[4 * i + 3];
    }
    S.n_binned = S.n_records - S.n_unmapped - S.n_multimapped;
    S.max_bin = max_bin;
    if (S.n_records != n_slots)
        return fail(c, AFQ_ERR_HIP, "afq_atac_gpl_hist_rad: the parse saw " + std::to_string(S.n_records) + " of " + std::to_string(n_slots) + " records");
    // ---- count, compact
    std::vector<std::pair<uint64_t, uint64_t>> pairs;
    if (int rc = gpl_count_sorted(c, P, S.n_records, bc_bytes, pairs)) return rc;
    hc.lap("atac gpl: count + compact + sort");
    if (int rc = gpl_check_total(c, "afq_atac_gpl_hist_rad", pairs, S.n_records, "records")) return rc;
    HostOuts H;
    uint64_t *obc = nullptr, *ocnt = nullptr, *obins = nullptr;
    if (int rc = gpl_hist_out(c, "afq_atac_gpl_hist_rad", pairs, H, &obc, &ocnt, n_bins, &obins)) return rc;
    if (n_bins) {
        T(hipMemcpyAsync(obins, B.bins64.p, 8ull * n_bins, hipMemcpyDeviceToHost, s));
        T(hipStreamSynchronize(s));
        if (!T.ok()) return P.hip_fail(c);
    }
    if (stats) *stats = S;
    H.release();
    *out_n = pairs.size(); *out_bc = obc; *out_count = ocnt; *out_bins = obins;
    return 0;
}

int afq_gpl_correct(afq_ctx* c, const uint64_t* observed, const uint64_t* obs_count, uint64_t n_obs, const uint64_t* retained, const uint64_t* ret_count,
                    uint64_t n_ret, uint32_t barcode_len, uint32_t neighborhood, uint32_t resolution, uint64_t conf_num, uint64_t conf_den,
                    uint64_t pseudocount, uint8_t** out_decision, uint32_t** out_target, uint64_t** out_target_count, afq_gpl_correction_stats* stats) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if (((!observed || !obs_count) && n_obs) || ((!retained || !ret_count) && n_ret) || !out_decision || !out_target || !out_target_count)
        return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    if (barcode_len < 1 || barcode_len > 32) return fail(c, AFQ_ERR_INVALID_ARG, "barcode length must be between 1 and 32 (got " + std::to_string(barcode_len) + ")");
    if (neighborhood > kGplShift) return fail(c, AFQ_ERR_INVALID_ARG, "neighborhood must be 0 (hamming-1) or 1 (substitution-or-shift-1)");
    if (resolution > kGplFrequency) return fail(c, AFQ_ERR_INVALID_ARG, "resolution must be 0 (unique) or 1 (frequency)");
    if (resolution == kGplFrequency) {
        if (conf_den == 0 || conf_num > conf_den)
            return fail(c, AFQ_ERR_INVALID_ARG, "barcode-correction confidence must be between zero and one (got " + std::to_string(conf_num) + "/" + std::to_string(conf_den) + ")");
        if (pseudocount == 0) return fail(c, AFQ_ERR_INVALID_ARG, "frequency correction requires a non-zero pseudocount");
        if (pseudocount >= kGplMaxWeight) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_gpl_correct: a pseudocount of 2^55 or more");
    } else { conf_num = 0; conf_den = 1; pseudocount = 0; }
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    if (n_ret >= (1ull << 30)) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_gpl_correct: 2^30 or more retained barcodes (" + std::to_string(n_ret) + ")");
    if (n_obs >= (1ull << 32)) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_gpl_correct: 2^32 or more observed barcodes in one call (" + std::to_string(n_obs) + ")");
    const uint64_t fit = barcode_len < 32 ? (1ull << (2 * barcode_len)) : 0;   // (0: every u64 fits)
    for (uint64_t i = 0; i < n_ret; ++i) {
        if (i && retained[i] <= retained[i - 1]) return fail(c, AFQ_ERR_INVALID_ARG, "retained barcodes must ascend without duplicates (entry " + std::to_string(i) + ")");
        if (fit && retained[i] >= fit) return fail(c, AFQ_ERR_BAD_INPUT, "packed barcode " + std::to_string(retained[i]) + " does not fit declared length " + std::to_string(barcode_len));
        if (resolution == kGplFrequency && ret_count[i] >= kGplMaxWeight - pseudocount)
            return fail(c, AFQ_ERR_UNSUPPORTED, "afq_gpl_correct: retained barcode " + std::to_string(retained[i]) + " has an exact count + pseudocount of 2^55 or more");
    }
    for (uint64_t i = 0; i < n_obs; ++i) {
        if (i && observed[i] <= observed[i - 1]) return fail(c, AFQ_ERR_INVALID_ARG, "observed barcodes must ascend without duplicates (entry " + std::to_string(i) + ")");
        if (fit && observed[i] >= fit) return fail(c, AFQ_ERR_BAD_INPUT, "packed barcode " + std::to_string(observed[i]) + " does not fit declared length " + std::to_string(barcode_len));
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint64_t cap = sort_table_capacity(n_ret), no1 = std::max<uint64_t>(n_obs, 1), nr1 = std::max<uint64_t>(n_ret, 1);
    {
        const uint64_t need = no1 * 21 + nr1 * 28 + cap * 12;
        size_t fr = 0, tot = 0;
        HIP_TRY(c, hipMemGetInfo(&fr, &tot));
        if (need > tot)
            return fail(c, AFQ_ERR_OOM, "afq_gpl_correct: " + std::to_string(need) + " bytes for " + std::to_string(n_obs) + " observed and " + std::to_string(n_ret) +
                        " retained barcodes > " + std::to_string(tot) + " bytes of device memory");
    }
    std::vector<uint32_t> idx(n_ret);
    uint32_t ones_idx = kGplNoTarget;
    for (uint64_t i = 0; i < n_ret; ++i) { idx[i] = (uint32_t)i; if (retained[i] == kSortEmptyKey) ones_idx = (uint32_t)i; }
    auto& B = c->gpl;
    HipLatch T;
    auto hip_fail = [&]() { return T.fail(c, "afq_gpl_correct", " (" + std::to_string(n_obs) + " observed, " + std::to_string(n_ret) + " retained barcodes)"); };
    T(B.obs.ensure(8 * no1)); T(B.obscnt.ensure(8 * no1)); T(B.ret.ensure(8 * nr1)); T(B.retcnt.ensure(8 * nr1)); T(B.idx.ensure(4 * nr1));
    T(B.rkey.ensure(8 * cap)); T(B.rval.ensure(4 * cap)); T(B.dec.ensure(no1)); T(B.tgt.ensure(4 * no1)); T(B.stats.ensure(64)); T(B.tcount.ensure(8 * nr1));
    T(B.cstatus.ensure(sizeof(DevStatus)));
    if (!T.ok()) return hip_fail();
    if (n_obs) { T(hipMemcpyAsync(B.obs.p, observed, 8 * n_obs, hipMemcpyHostToDevice, s)); T(hipMemcpyAsync(B.obscnt.p, obs_count, 8 * n_obs, hipMemcpyHostToDevice, s)); }
    if (n_ret) {
        T(hipMemcpyAsync(B.ret.p, retained, 8 * n_ret, hipMemcpyHostToDevice, s)); T(hipMemcpyAsync(B.retcnt.p, ret_count, 8 * n_ret, hipMemcpyHostToDevice, s));
        T(hipMemcpyAsync(B.idx.p, idx.data(), 4 * n_ret, hipMemcpyHostToDevice, s));
    }
    T(hipMemsetAsync(B.rkey.p, 0xFF, 8 * cap, s));
    T(hipMemsetAsync(B.stats.p, 0, 64, s));
    T(hipMemsetAsync(B.tcount.p, 0, 8 * nr1, s));
    T(hipMemsetAsync(B.cstatus.p, 0, sizeof(DevStatus), s));
    if (!T.ok()) return hip_fail();
    reset_kernel_times(c);
    {
        ScopedTimer t(c, K_GPL_TABLE, s);
        launch_sort_table(s, B.ret.as<uint64_t>(), B.idx.as<uint32_t>(), n_ret, B.rkey.as<uint64_t>(), B.rval.as<uint32_t>(), (uint32_t)(cap - 1), B.cstatus.as<DevStatus>());
    }
    {
        ScopedTimer t(c, K_GPL_CORRECT, s);
        launch_gpl_correct(s, GplCorrectArgs{B.obs.as<uint64_t>(), B.obscnt.as<uint64_t>(), n_obs, B.rkey.as<uint64_t>(), B.rval.as<uint32_t>(), (uint32_t)(cap - 1), ones_idx,
                                             B.retcnt.as<uint64_t>(), barcode_len, neighborhood, resolution, conf_num, conf_den, pseudocount, B.dec.as<uint8_t>(),
                                             B.tgt.as<uint32_t>(), B.stats.as<unsigned long long>(), B.tcount.as<unsigned long long>()});
    }
    T(hipGetLastError());
    HostOuts H;
    uint8_t* odec = (uint8_t*)H.mallocd(no1);
    uint32_t* otgt = (uint32_t*)H.mallocd(4 * no1);
    uint64_t* otc = (uint64_t*)H.mallocd(8 * nr1);
    if (!odec || !otgt || !otc) { (void)hipStreamSynchronize(s); return fail(c, AFQ_ERR_OOM, "afq_gpl_correct: host allocation failed (" + std::to_string(5 * no1 + 8 * nr1) + " bytes of decisions)"); }
    DevStatus st{};
    uint64_t cs[8] = {};
    T(hipMemcpyAsync(&st, B.cstatus.p, sizeof(st), hipMemcpyDeviceToHost, s));
    T(hipMemcpyAsync(cs, B.stats.p, 64, hipMemcpyDeviceToHost, s));
    if (n_obs) { T(hipMemcpyAsync(odec, B.dec.p, n_obs, hipMemcpyDeviceToHost, s)); T(hipMemcpyAsync(otgt, B.tgt.p, 4 * n_obs, hipMemcpyDeviceToHost, s)); }
    T(hipMemcpyAsync(otc, B.tcount.p, 8 * nr1, hipMemcpyDeviceToHost, s));
    T(hipStreamSynchronize(s));   // (before any exit below: the copies write into H's blocks)
    harvest_timers(c);
    if (!T.ok()) return hip_fail();
    if (st.err_code) return fail(c, AFQ_ERR_HIP, "afq_gpl_correct: device status " + std::to_string(st.err_code) + " at retained entry " + std::to_string(st.err_cell));
    if (stats) {
        stats->exact_distinct = cs[0]; stats->exact_reads = cs[1]; stats->corrected_distinct = cs[2]; stats->corrected_reads = cs[3];
        stats->ambiguous_distinct = cs[4]; stats->ambiguous_reads = cs[5]; stats->not_found_distinct = cs[6]; stats->not_found_reads = cs[7];
    }
    H.release();
    *out_decision = odec; *out_target = otgt; *out_target_count = otc;
    return 0;
}
