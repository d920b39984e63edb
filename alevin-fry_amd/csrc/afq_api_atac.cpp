// afq_api_atac.cpp — the scATAC entry points of include/afquant.h: afq_atac_dedup, afq_atac_dedup_rad, afq_atac_sort_*.
#include <atomic>
#include <thread>

#include "afq_ctx.h"

// Shared back half of the two ATAC entry points: de-duplicate the fragments sitting in A.ref/A.start/A.flen (cell i at
// A.ptr[i], cell_cnt[i] of them when d_cnt is given, else up to A.ptr[i+1]) and hand the distinct ones out as malloc'd arrays.
static int atac_dedup_device(afq_ctx* c, uint64_t n, uint32_t n_cells, const uint32_t* d_cnt, uint64_t** out_cell_ptr, uint32_t** out_ref,
                             uint32_t** out_start, uint16_t** out_frag_len, uint16_t** out_count, HostClock& hc, unsigned long long* tally_out = nullptr) {
    auto& A = c->atac;
    hipStream_t s = c->stream;
    const uint64_t n1 = std::max<uint64_t>(n, 1);
    HipLatch T;
    T(A.scr.ensure(16 * n1)); T(A.oref.ensure(4 * n1)); T(A.ostart.ensure(4 * n1)); T(A.oflen.ensure(2 * n1));
    T(A.ocnt.ensure(2 * n1)); T(A.on.ensure(4ull * std::max<uint32_t>(n_cells, 1))); T(A.optr.ensure(8ull * (n_cells + 1)));
    T(A.flag.ensure(4)); T(A.tally.ensure(16));
    if (T.ok()) T(hipMemsetAsync(A.flag.p, 0, 4, s));
    if (T.ok()) T(hipMemsetAsync(A.tally.p, 0, 16, s));
    // (the tally starts here, not at the compaction: the dedup kernels add the runs whose 16-bit count wrapped to 0 or 1)
    unsigned long long* const d_tally = tally_out ? A.tally.as<unsigned long long>() : nullptr;
    std::vector<uint32_t> on(n_cells);
    uint32_t wide = 0;
    if (T.ok()) {
        ScopedTimer t(c, K_ATAC, s);
        launch_atac_dedup64(s, n_cells, A.ref.as<uint32_t>(), A.start.as<uint32_t>(), A.flen.as<uint16_t>(), A.ptr.as<uint64_t>(),
                            A.scr.p, A.oref.as<uint32_t>(), A.ostart.as<uint32_t>(), A.oflen.as<uint16_t>(),
                            A.ocnt.as<uint16_t>(), A.on.as<uint32_t>(), A.flag.as<uint32_t>(), d_cnt, d_tally);
        T(hipGetLastError());
    }
    if (T.ok()) {
        T(hipMemcpyAsync(&wide, A.flag.p, 4, hipMemcpyDeviceToHost, s));
        T(hipStreamSynchronize(s));
    }
    if (T.ok() && wide) {  // a reference id >= 65536: the 16-byte-record kernel (and its tally, not that of the cut keys' runs)
        T(hipMemsetAsync(A.tally.p, 0, 16, s));
        ScopedTimer t(c, K_ATAC, s);
        launch_atac_dedup(s, n_cells, A.ref.as<uint32_t>(), A.start.as<uint32_t>(), A.flen.as<uint16_t>(), A.ptr.as<uint64_t>(),
                          A.scr.p, A.oref.as<uint32_t>(), A.ostart.as<uint32_t>(), A.oflen.as<uint16_t>(),
                          A.ocnt.as<uint16_t>(), A.on.as<uint32_t>(), d_cnt, d_tally);
        T(hipGetLastError());
    }
    if (T.ok() && n_cells) T(hipMemcpyAsync(on.data(), A.on.p, 4ull * n_cells, hipMemcpyDeviceToHost, s));
    if (T.ok()) T(hipStreamSynchronize(s));
    hc.lap("atac: kernel");
    if (!T.ok()) return T.fail(c, "afq_atac_dedup");
    HostOuts H;
    uint64_t* optr = (uint64_t*)H.mallocd(8ull * (n_cells + 1));
    if (!optr) return fail(c, AFQ_ERR_OOM, "afq_atac_dedup: host allocation failed");
    optr[0] = 0;
    for (uint32_t i = 0; i < n_cells; ++i) optr[i + 1] = optr[i] + on[i];
    const uint64_t tot = optr[n_cells], tot1 = std::max<uint64_t>(tot, 1);
    uint32_t* oref = (uint32_t*)H.pinned(4 * tot1);
    uint32_t* ostart = (uint32_t*)H.pinned(4 * tot1);
    uint16_t* oflen = (uint16_t*)H.pinned(2 * tot1);
    uint16_t* ocnt = (uint16_t*)H.pinned(2 * tot1);
    if (!oref || !ostart || !oflen || !ocnt) return fail(c, AFQ_ERR_OOM, "afq_atac_dedup: host allocation failed");
    // dense runs on the device, then straight into the caller's arrays
    T(A.cref.ensure(4 * tot1)); T(A.cstart.ensure(4 * tot1)); T(A.cflen.ensure(2 * tot1)); T(A.ccnt.ensure(2 * tot1));
    if (T.ok()) T(hipMemcpyAsync(A.optr.p, optr, 8ull * (n_cells + 1), hipMemcpyHostToDevice, s));
    if (T.ok() && tot) {
        launch_atac_compact(s, n_cells, A.ptr.as<uint64_t>(), A.optr.as<uint64_t>(), A.oref.as<uint32_t>(), A.ostart.as<uint32_t>(),
                            A.oflen.as<uint16_t>(), A.ocnt.as<uint16_t>(), A.cref.as<uint32_t>(), A.cstart.as<uint32_t>(),
                            A.cflen.as<uint16_t>(), A.ccnt.as<uint16_t>(), tally_out ? A.tally.as<unsigned long long>() : nullptr);
        T(hipGetLastError());
        T(hipMemcpyAsync(oref, A.cref.p, 4 * tot, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(ostart, A.cstart.p, 4 * tot, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(oflen, A.cflen.p, 2 * tot, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(ocnt, A.ccnt.p, 2 * tot, hipMemcpyDeviceToHost, s));
    }
    if (T.ok() && tally_out) T(hipMemcpyAsync(tally_out, A.tally.p, 16, hipMemcpyDeviceToHost, s));
    if (T.ok()) T(hipStreamSynchronize(s));
    hc.lap("atac: compact + D2H");
    harvest_timers(c);
    if (!T.ok()) return T.fail(c, "afq_atac_dedup");
    H.release();
    *out_cell_ptr = optr; *out_ref = oref; *out_start = ostart; *out_frag_len = oflen; *out_count = ocnt;
    return 0;
}

int afq_atac_dedup(afq_ctx* c, const uint32_t* ref, const uint32_t* start, const uint16_t* frag_len,
                   const uint64_t* cell_ptr, uint32_t n_cells, uint64_t** out_cell_ptr, uint32_t** out_ref,
                   uint32_t** out_start, uint16_t** out_frag_len, uint16_t** out_count) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if (!cell_ptr || !out_cell_ptr || !out_ref || !out_start || !out_frag_len || !out_count)
        return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    const uint64_t n = cell_ptr[n_cells];
    if (n && (!ref || !start || !frag_len)) return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    for (uint32_t i = 0; i < n_cells; ++i)
        if (cell_ptr[i + 1] < cell_ptr[i] || cell_ptr[i + 1] - cell_ptr[i] > 0x7FFFFFFFull)
            return fail(c, AFQ_ERR_INVALID_ARG, "cell_ptr must be non-decreasing");
    HostClock hc;
    auto& A = c->atac;
    hipStream_t s = c->stream;
    const uint64_t n1 = std::max<uint64_t>(n, 1);
    HipLatch T;
    T(A.ref.ensure(4 * n1)); T(A.start.ensure(4 * n1)); T(A.flen.ensure(2 * n1)); T(A.ptr.ensure(8ull * (n_cells + 1)));
    if (T.ok() && n) {   // (the pinned staging path of afq_submit was measured here too: no faster for these arrays)
        T(hipMemcpyAsync(A.ref.p, ref, 4 * n, hipMemcpyHostToDevice, s));
        T(hipMemcpyAsync(A.start.p, start, 4 * n, hipMemcpyHostToDevice, s));
        T(hipMemcpyAsync(A.flen.p, frag_len, 2 * n, hipMemcpyHostToDevice, s));
    }
    if (T.ok()) T(hipMemcpyAsync(A.ptr.p, cell_ptr, 8ull * (n_cells + 1), hipMemcpyHostToDevice, s));
    if (hc.on) { T(hipStreamSynchronize(s)); hc.lap("atac: alloc + H2D"); }
    if (!T.ok()) return T.fail(c, "afq_atac_dedup");
    reset_kernel_times(c);
    return atac_dedup_device(c, n, n_cells, nullptr, out_cell_ptr, out_ref, out_start, out_frag_len, out_count, hc);
}

namespace {
// What the two routes of afq_atac_dedup_rad (the eight-range pipeline and the plain one) work on.
struct AtacRadJob {
    const uint8_t* d_bytes;
    size_t n_bytes;
    uint32_t n_cells, bc_bytes;
    uint64_t n_rec = 0;
    std::vector<uint64_t> cap_ptr;   // capacity offsets of the cells' fragments = prefix of nrec
    DevStatus st{};
    std::vector<uint32_t> stat;      // per cell: multi-mapped, not a mapped pair
    unsigned long long tally[2] = {0, 0};
    uint64_t* obc = nullptr;         // the cells' barcodes (the caller's; owned by afq_atac_dedup_rad until it returns 0)
    AtacParseArgs parse_args(AtacBufs& A, uint32_t c0, uint32_t c1, uint32_t* nwalk, DevStatus* dst) const {
        return AtacParseArgs{d_bytes, A.cells.as<AtacCell>() + c0, c1 - c0, bc_bytes, A.bm.as<uint64_t>(), A.ref.as<uint32_t>(), A.start.as<uint32_t>(),
                             A.flen.as<uint16_t>(), A.cnt.as<uint32_t>() + c0, A.bc.as<uint64_t>() + c0, A.stat.as<uint32_t>() + 2ull * c0,
                             A.walk.as<uint32_t>() + c0, nwalk, dst, (uint64_t)n_bytes};
    }
};
constexpr int kPipedDone = 0, kPipedRedo = 1;   // (or an AFQ_ERR_ code, all negative)
}  // namespace

// Big batches go through in eight ranges of cells: the distinct fragments of range r cross PCIe on a second stream while the
// later ranges are still parsed and sorted.  The rows are the long pole - 12 bytes a row, 1.8 GB for 2*10^8 records, 34 ms at
// the 52 GB/s the link gives (the e2e leg), against 20 ms for all the kernels - so (round 5) the ref column stays on the device
// (8 bytes a row cross, 23 ms; the host writes the column from a list of runs, below), and what matters then is how soon the
// FIRST rows can leave and how few are left when the last kernel ends: the ranges GROW (4, 8, 12, 14, 15, 16, 16, 15 % of the
// records; four equal ranges kept the link idle for the first quarter of the kernels), the opposite of the cr-like taper,
// whose rows are short.  Measured and not kept: the parse of range r+1 on a stream of its own next to the sort of range r
// (the sort's workgroups wait for CUs behind the parse's: 12.7 -> 18.3 ms of sort, 28.6 -> 30.9 ms a step).
// Returns kPipedDone (the outputs, J.obc, J.stat, J.tally and J.st.n_fallback are filled), kPipedRedo (a reference id >= 65536:
// nothing is handed out or left allocated, the plain route runs the 16-byte-record kernel) or an error code.
static int atac_dedup_piped(afq_ctx* c, AtacRadJob& J, uint64_t** out_cell_ptr, uint32_t** out_ref, uint32_t** out_start, uint16_t** out_frag_len,
                            uint16_t** out_count, HostClock& hc) {
    auto& A = c->atac;
    hipStream_t s = c->stream;
    const uint32_t n_cells = J.n_cells;
    const uint64_t n1 = std::max<uint64_t>(J.n_rec, 1), nc1 = std::max<uint32_t>(n_cells, 1);
    constexpr uint32_t kR = 8;
    static const double kGrow[kR] = {0.04, 0.12, 0.24, 0.38, 0.53, 0.69, 0.85, 1.0};
    uint32_t cut[kR + 1];
    cut[0] = 0;
    for (uint32_t r = 1; r < kR; ++r) {
        const uint64_t target = (uint64_t)((double)J.n_rec * kGrow[r - 1]);
        cut[r] = (uint32_t)(std::lower_bound(J.cap_ptr.begin(), J.cap_ptr.begin() + n_cells, target) - J.cap_ptr.begin());
        if (cut[r] < cut[r - 1]) cut[r] = cut[r - 1];
    }
    cut[kR] = n_cells;
    HipLatch T;
    T(A.scr.ensure(16 * n1)); T(A.oref.ensure(4 * n1)); T(A.ostart.ensure(4 * n1)); T(A.oflen.ensure(2 * n1)); T(A.ocnt.ensure(2 * n1));
    T(A.on.ensure(4ull * nc1)); T(A.optr.ensure(8ull * (n_cells + 1))); T(A.flag.ensure(4)); T(A.tally.ensure(16));
    T(A.cref.ensure(4 * n1)); T(A.cstart.ensure(4 * n1)); T(A.cflen.ensure(2 * n1)); T(A.ccnt.ensure(2 * n1));   // (sized for "nothing is a duplicate")
    T(A.rstat.ensure(kR * (sizeof(DevStatus) + 16))); T(A.runctr.ensure(4));
    // The ref column does not cross PCIe: a cell's rows are sorted by ref first, so the column is a few runs per cell - the
    // compaction kernel lists them (first row, length, ref: 16 bytes a run, written straight into pinned host memory) and
    // host threads write the column from the list while the other three columns (8 of the 12 bytes of a row) are on the link.
    // A list that overflows (more than 64 runs per cell on average: thousands of contigs) sends the column itself, as before.
    const long cap_hook = test_hook_long("ATAC_RUN_CAP", -1);   // (tests: force the overflow)
    // (at most 2^22 runs = 64 MiB of pinned memory whatever the number of barcodes - an unfiltered sample has a million of them; a
    //  list that does not fit, or that the host has no pinned memory for, is the overflow case: the column crosses as a copy)
    uint32_t run_cap = cap_hook >= 0 ? (uint32_t)cap_hook : (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1u << 20, 64ull * n_cells), 1u << 22);
    HostOuts out, tmp;   // the caller's columns; the run list and the pinned block, this function's own
    uint4* runs = (uint4*)tmp.pinned(16ull * std::max<uint32_t>(run_cap, 1));
    if (!runs) { run_cap = 0; runs = (uint4*)tmp.pinned(16); }
    uint32_t* oref = (uint32_t*)out.pinned(4 * n1);
    uint32_t* ostart = (uint32_t*)out.pinned(4 * n1);
    uint16_t* oflen = (uint16_t*)out.pinned(2 * n1);
    uint16_t* ocnt = (uint16_t*)out.pinned(2 * n1);
    uint64_t* optr = (uint64_t*)out.mallocd(8ull * (n_cells + 1));
    // (the per-range counts and flags land in PINNED memory: an async copy into pageable memory holds the host until the
    // stream gets there, and the ranges would be enqueued one at a time)
    uint8_t* pin = (uint8_t*)tmp.pinned(4ull * nc1 + kR * (sizeof(DevStatus) + 16));
    if (!oref || !ostart || !oflen || !ocnt || !optr || !runs || !pin) return fail(c, AFQ_ERR_OOM, "afq_atac_dedup_rad: host allocation failed");
    hipStream_t s2 = second_stream(c);
    DevStatus* d_rst = reinterpret_cast<DevStatus*>(A.rstat.p);
    uint32_t* d_rnw = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(A.rstat.p) + kR * sizeof(DevStatus));
    uint32_t* on = reinterpret_cast<uint32_t*>(pin);
    DevStatus* rst = reinterpret_cast<DevStatus*>(pin + 4ull * nc1);
    uint32_t* wide = reinterpret_cast<uint32_t*>(pin + 4ull * nc1 + kR * sizeof(DevStatus));
    volatile uint32_t* snap = wide + kR;   // the run counter as it stood after each range's compaction (the block has four words per range)
    uint32_t* pin_dev = nullptr;   // the same block as the device sees it
    T(hipHostGetDevicePointer(reinterpret_cast<void**>(&pin_dev), pin, 0));
    uint4* runs_dev = nullptr;
    T(hipHostGetDevicePointer(reinterpret_cast<void**>(&runs_dev), runs, 0));
    hipEvent_t ev[2 * kR], *const ev2 = ev + kR;   // a range's kernels are done; its run list is complete
    for (auto& x : ev) x = get_event(c);
    T(hipMemsetAsync(A.runctr.p, 0, 4, s));
    // the threads that write the ref column: thread 0 waits for a range's list (the event after its compaction), all fill
    std::atomic<int> recorded{0}, listed{0}, stop{0};
    const unsigned nfill = stage_threads();
    std::vector<std::thread> fillers;
    if (T.ok()) {
        for (unsigned t = 0; t < nfill; ++t)
            fillers.emplace_back([&, t]() {
                if (t == 0) (void)hipSetDevice(c->device);
                uint32_t lo = 0;
                for (uint32_t r = 0; r < kR; ++r) {
                    if (t == 0) {
                        while (recorded.load(std::memory_order_acquire) <= (int)r) { if (stop.load(std::memory_order_relaxed)) return; std::this_thread::sleep_for(std::chrono::microseconds(20)); }
                        if (hipEventSynchronize(ev2[r]) != hipSuccess) { (void)hipGetLastError(); stop.store(1); return; }
                        listed.store((int)r + 1, std::memory_order_release);
                    } else {
                        while (listed.load(std::memory_order_acquire) <= (int)r) { if (stop.load(std::memory_order_relaxed)) return; std::this_thread::sleep_for(std::chrono::microseconds(20)); }
                    }
                    const uint32_t hi = snap[r];
                    if (hi > run_cap) return;   // this range's column and every later one come as copies
                    for (uint32_t i = lo + t; i < hi; i += nfill) {
                        const uint4 q = runs[i];
                        std::fill_n(oref + (((uint64_t)q.y << 32) | q.x), (size_t)q.z, q.w);
                    }
                    lo = hi;
                }
            });
    }
    T(hipMemsetAsync(A.flag.p, 0, 4, s));
    T(hipMemsetAsync(A.tally.p, 0, 16, s));
    T(hipMemsetAsync(A.rstat.p, 0, kR * (sizeof(DevStatus) + 16), s));
    for (uint32_t r = 0; r < kR && T.ok(); ++r) {
        const uint32_t c0 = cut[r], nr = cut[r + 1] - c0;
        { ScopedTimer t(c, K_ATAC_PARSE, s); launch_atac_parse(s, J.parse_args(A, c0, cut[r + 1], d_rnw + r, d_rst + r)); }
        { ScopedTimer t(c, K_ATAC, s);
          launch_atac_dedup64(s, nr, A.ref.as<uint32_t>(), A.start.as<uint32_t>(), A.flen.as<uint16_t>(), A.ptr.as<uint64_t>() + c0, A.scr.p,
                              A.oref.as<uint32_t>(), A.ostart.as<uint32_t>(), A.oflen.as<uint16_t>(), A.ocnt.as<uint16_t>(), A.on.as<uint32_t>() + c0,
                              A.flag.as<uint32_t>(), A.cnt.as<uint32_t>() + c0, A.tally.as<unsigned long long>()); }
        T(hipGetLastError());
        // (the range's counts, flag and status go to the pinned block by a kernel, not as copies: see k_copy_words3)
        launch_copy_words3(s, A.on.as<uint32_t>() + c0, nr, pin_dev + c0, A.flag.as<uint32_t>(), 1, pin_dev + (wide - on) + r,
                           reinterpret_cast<const uint32_t*>(d_rst + r), (uint32_t)(sizeof(DevStatus) / 4), pin_dev + (reinterpret_cast<uint32_t*>(rst + r) - on));
        T(hipGetLastError());
        T(hipEventRecord(ev[r], s));
    }
    optr[0] = 0;
    bool redo = false;
    int bad_rc = 0;
    uint64_t n_fallback = 0;
    for (uint32_t r = 0; r < kR && T.ok() && !redo && !bad_rc; ++r) {
        const uint32_t c0 = cut[r], c1 = cut[r + 1];
        T(hipEventSynchronize(ev[r]));
        if (!T.ok()) break;
        if (wide[r]) { redo = true; break; }
        if (rst[r].err_code) { bad_rc = fail(c, AFQ_ERR_BAD_INPUT, "cell " + std::to_string(c0 + rst[r].err_cell) + ": chunk nbytes does not match its records"); break; }
        n_fallback += rst[r].n_fallback;
        for (uint32_t i = c0; i < c1; ++i) optr[i + 1] = optr[i] + on[i];
        const uint64_t o0 = optr[c0], tot_r = optr[c1] - o0;
        T(hipMemcpyAsync(A.optr.as<uint64_t>() + c0, optr + c0, 8ull * (c1 - c0 + 1), hipMemcpyHostToDevice, s2));
        if (tot_r) {
            launch_atac_compact(s2, c1 - c0, A.ptr.as<uint64_t>() + c0, A.optr.as<uint64_t>() + c0, A.oref.as<uint32_t>(), A.ostart.as<uint32_t>(),
                                A.oflen.as<uint16_t>(), A.ocnt.as<uint16_t>(), A.cref.as<uint32_t>(), A.cstart.as<uint32_t>(),
                                A.cflen.as<uint16_t>(), A.ccnt.as<uint16_t>(), A.tally.as<unsigned long long>(), runs_dev, A.runctr.as<uint32_t>(), run_cap);
            T(hipGetLastError());
        }
        launch_copy_words3(s2, A.runctr.as<uint32_t>(), 1, pin_dev + (const_cast<uint32_t*>(snap) - on) + r, nullptr, 0, nullptr, nullptr, 0, nullptr);
        T(hipGetLastError());
        T(hipEventRecord(ev2[r], s2));
        if (T.ok()) recorded.store((int)r + 1, std::memory_order_release);
        if (tot_r) {
            T(hipMemcpyAsync(ostart + o0, A.cstart.as<uint32_t>() + o0, 4 * tot_r, hipMemcpyDeviceToHost, s2));
            T(hipMemcpyAsync(oflen + o0, A.cflen.as<uint16_t>() + o0, 2 * tot_r, hipMemcpyDeviceToHost, s2));
            T(hipMemcpyAsync(ocnt + o0, A.ccnt.as<uint16_t>() + o0, 2 * tot_r, hipMemcpyDeviceToHost, s2));
        }
    }
    const bool done = T.ok() && !redo && !bad_rc;
    if (!done) stop.store(1);
    for (auto& th : fillers) th.join();
    if (done) {
        T(hipEventSynchronize(ev2[kR - 1]));   // (every range's count is on the host; the fillers stop at the first list that overflowed)
        for (uint32_t r = 0; r < kR && T.ok(); ++r)
            if (snap[r] > run_cap) {
                const uint64_t o0 = optr[cut[r]], tot_r = optr[cut[r + 1]] - o0;
                if (tot_r) T(hipMemcpyAsync(oref + o0, A.cref.as<uint32_t>() + o0, 4 * tot_r, hipMemcpyDeviceToHost, s2));
            }
        T(hipMemcpyAsync(J.tally, A.tally.p, 16, hipMemcpyDeviceToHost, s2));
        if (n_cells) T(hipMemcpyAsync(J.stat.data(), A.stat.p, 8ull * n_cells, hipMemcpyDeviceToHost, s2));
        if (n_cells) T(hipMemcpyAsync(J.obc, A.bc.p, 8ull * n_cells, hipMemcpyDeviceToHost, s2));
    }
    (void)hipStreamSynchronize(s);
    (void)hipStreamSynchronize(s2);
    for (auto x : ev) c->event_pool.push_back(x);
    tmp.free_all();
    harvest_timers(c);
    hc.lap("atac: ranges (parse, sort, compact, D2H)");
    if (bad_rc) return bad_rc;
    if (!T.ok()) return T.fail(c, "afq_atac_dedup_rad");
    if (redo) return kPipedRedo;
    J.st.n_fallback += n_fallback;
    out.release();
    *out_cell_ptr = optr; *out_ref = oref; *out_start = ostart; *out_frag_len = oflen; *out_count = ocnt;
    return kPipedDone;
}

int afq_atac_dedup_rad(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_cells, uint32_t bc_bytes,
                       int bytes_on_device, uint64_t** out_cell_ptr, uint64_t** out_bc, uint32_t** out_ref, uint32_t** out_start,
                       uint16_t** out_frag_len, uint16_t** out_count, afq_atac_stats* stats) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!bytes && n_bytes) || (!chunk_off && n_cells) || !out_cell_ptr || !out_bc || !out_ref || !out_start || !out_frag_len || !out_count)
        return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    if (!valid_width(bc_bytes)) return fail(c, AFQ_ERR_INVALID_ARG, "bc_bytes must be 1, 2, 4 or 8");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    hipStream_t s = c->stream;
    // ---- validate: chunk headers (from the host copy, or gathered off the device), capacity offsets = prefix of nrec
    std::vector<uint32_t> hdr(2ull * n_cells);
    if (int rc = fetch_chunk_headers(c, bytes, n_bytes, chunk_off, n_cells, bytes_on_device != 0, hdr.data())) return rc;
    AtacRadJob J{bytes, n_bytes, n_cells, bc_bytes};
    std::vector<AtacCell> cells(n_cells);
    J.cap_ptr.assign((size_t)n_cells + 1, 0);
    uint64_t bm_words = 0;
    for (uint32_t i = 0; i < n_cells; ++i) {
        const uint32_t nb = hdr[2 * i], nr = hdr[2 * i + 1];
        if (const ChunkFault f = check_chunk_header(chunk_off[i], nb, nr, n_bytes, 4 + bc_bytes)) return chunk_fault(c, "cell", i, f);
        cells[i] = AtacCell{chunk_off[i], J.n_rec, bm_words, nb, nr};
        J.cap_ptr[i] = J.n_rec;
        J.n_rec += nr;
        bm_words += 4ull * (((uint64_t)nb + 3 + 255) / 256);   // four ballots per group of 256 positions (counted from the dword boundary below the chunk)
    }
    J.cap_ptr[n_cells] = J.n_rec;
    // ---- upload
    auto& A = c->atac;
    const uint64_t n1 = std::max<uint64_t>(J.n_rec, 1), nc1 = std::max<uint32_t>(n_cells, 1);
    HIP_TRY(c, A.ref.ensure(4 * n1)); HIP_TRY(c, A.start.ensure(4 * n1)); HIP_TRY(c, A.flen.ensure(2 * n1)); HIP_TRY(c, A.ptr.ensure(8ull * (n_cells + 1)));
    HIP_TRY(c, A.cells.ensure(sizeof(AtacCell) * nc1)); HIP_TRY(c, A.bm.ensure(8 * std::max<uint64_t>(bm_words, 1))); HIP_TRY(c, A.cnt.ensure(4ull * nc1));
    HIP_TRY(c, A.bc.ensure(8ull * nc1)); HIP_TRY(c, A.stat.ensure(8ull * nc1)); HIP_TRY(c, A.walk.ensure(4ull * nc1)); HIP_TRY(c, A.nwalk.ensure(4));
    HIP_TRY(c, A.status.ensure(sizeof(DevStatus)));
    if (!bytes_on_device) {
        HIP_TRY(c, c->d_bytes_own.ensure(n_bytes + 16));
        if (n_bytes) { int rc2 = staged_h2d(c, (uint8_t*)c->d_bytes_own.p, bytes, n_bytes, s, host_ptr_is_pinned(bytes) && host_ptr_is_pinned(bytes + n_bytes - 1)); if (rc2) return rc2; }
        J.d_bytes = c->d_bytes_own.as<uint8_t>();
    }
    if (n_cells) HIP_TRY(c, hipMemcpyAsync(A.cells.p, cells.data(), sizeof(AtacCell) * n_cells, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(A.ptr.p, J.cap_ptr.data(), 8ull * (n_cells + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(A.nwalk.p, 0, 4, s));
    HIP_TRY(c, hipMemsetAsync(A.status.p, 0, sizeof(DevStatus), s));
    if (hc.on) { HIP_TRY(c, hipStreamSynchronize(s)); hc.lap("atac: alloc + H2D"); }
    reset_kernel_times(c);
    J.stat.assign(2ull * n_cells, 0);
    HostOuts H;
    J.obc = (uint64_t*)H.mallocd(8ull * nc1);
    if (!J.obc) return fail(c, AFQ_ERR_OOM, "afq_atac_dedup_rad: host allocation failed");
    // ---- piped (big batches) or plain
    const size_t pipe_min = (size_t)test_hook_long("ATAC_PIPE_BYTES", 128L << 20);   // (tests: pipeline small inputs too)
    int route = kPipedRedo;
    if (n_cells >= 8 && n_bytes >= pipe_min) {
        route = atac_dedup_piped(c, J, out_cell_ptr, out_ref, out_start, out_frag_len, out_count, hc);
        if (route < 0) return route;
        if (route == kPipedRedo) reset_kernel_times(c);
    }
    if (route == kPipedRedo) {
        HIP_TRY(c, hipMemsetAsync(A.nwalk.p, 0, 4, s));
        HIP_TRY(c, hipMemsetAsync(A.status.p, 0, sizeof(DevStatus), s));
        {
            ScopedTimer t(c, K_ATAC_PARSE, s);
            launch_atac_parse(s, J.parse_args(A, 0, n_cells, A.nwalk.as<uint32_t>(), A.status.as<DevStatus>()));
            HIP_TRY(c, hipGetLastError());
        }
        HipLatch T;
        T(hipMemcpyAsync(&J.st, A.status.p, sizeof(J.st), hipMemcpyDeviceToHost, s));
        if (T.ok() && n_cells) T(hipMemcpyAsync(J.stat.data(), A.stat.p, 8ull * n_cells, hipMemcpyDeviceToHost, s));
        if (T.ok() && n_cells) T(hipMemcpyAsync(J.obc, A.bc.p, 8ull * n_cells, hipMemcpyDeviceToHost, s));
        if (T.ok()) T(hipStreamSynchronize(s));   // the caller keeps ownership of `bytes`: the copy out of them is done by now, too
        if (!T.ok()) return T.fail(c, "afq_atac_dedup_rad");
        if (J.st.err_code) return fail(c, AFQ_ERR_BAD_INPUT, "cell " + std::to_string(J.st.err_cell) + ": chunk nbytes does not match its records");
        int rc = atac_dedup_device(c, J.n_rec, n_cells, A.cnt.as<uint32_t>(), out_cell_ptr, out_ref, out_start, out_frag_len, out_count, hc, J.tally);
        if (rc) return rc;
    }
    // ---- stats
    H.release();
    *out_bc = J.obc;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->n_records = J.n_rec;
        for (uint32_t i = 0; i < n_cells; ++i) { stats->n_multimapped += J.stat[2 * i]; stats->n_not_mapped_pair += J.stat[2 * i + 1]; }
        stats->n_distinct = (*out_cell_ptr)[n_cells];
        stats->n_deduplicated = J.tally[0]; stats->n_long_fragments = J.tally[1];   // (tallied by the compaction kernel)
        stats->n_fallback_cells = J.st.n_fallback;
    }
    return 0;
}

// `atac sort` on the device (afq_atac_sort.hip): table, parse + correct, partition into position bins, re-partition of the
// oversize ones, leaves, dense arrays.  The host's part is what needs the whole picture and is small: the ranks of the corrected
// barcodes, the bins' first ids, and - from the bins' counts - which segments are leaves and which are split again.
void afq_atac_sort_limits(uint32_t out[4]) {
    if (!out) return;
    out[0] = kSortBinShift; out[1] = kSortLeafCap; out[2] = kSortRepartAbove; out[3] = kSortParseTile;
}

void afq_atac_sort_leaf_limits(uint32_t out[4]) {
    if (!out) return;
    out[0] = kSortSmallLeaf; out[1] = (uint32_t)kSortSmallLeafNT; out[2] = (uint32_t)kSortLeafNT; out[3] = kSortParseHalo;
}

void afq_atac_sort_table_slot(uint64_t barcode, uint64_t n_corr, uint32_t* home_slot, uint32_t* capacity) {
    const uint64_t cap = sort_table_capacity(n_corr < (1ull << 30) ? n_corr : (1ull << 30) - 1);   // (afq_atac_sort_rad refuses 2^30 entries and more)
    if (home_slot) *home_slot = sort_hash_bc(barcode) & (uint32_t)(cap - 1);
    if (capacity) *capacity = (uint32_t)cap;
}

int afq_atac_sort_rad(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t bc_bytes,
                      int bytes_on_device, const uint64_t* observed, const uint64_t* corrected, uint64_t n_corr, const uint32_t* ref_lengths,
                      uint32_t ref_count, uint64_t* out_n, uint32_t** out_ref, uint32_t** out_start, uint16_t** out_frag_len, uint64_t** out_bc,
                      uint32_t** out_count, afq_atac_sort_stats* stats) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!bytes && n_bytes) || (!chunk_off && n_chunks) || ((!observed || !corrected) && n_corr) || (!ref_lengths && ref_count) || !out_n || !out_ref ||
        !out_start || !out_frag_len || !out_bc || !out_count)
        return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    if (!valid_width(bc_bytes)) return fail(c, AFQ_ERR_INVALID_ARG, "bc_bytes must be 1, 2, 4 or 8");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    if (n_corr >= (1ull << 30)) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_atac_sort_rad: 2^30 or more correction entries");
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    hipStream_t s = c->stream;
    // ---- host: ranks of the corrected barcodes, the all-ones key, the bins' first ids
    std::vector<uint64_t> uniq(corrected, corrected + n_corr);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    if (uniq.size() >= (1ull << 31)) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_atac_sort_rad: 2^31 or more distinct corrected barcodes");
    std::vector<uint32_t> rank(n_corr);
    uint32_t ones_rank = kSortNoRank;
    for (uint64_t i = 0; i < n_corr; ++i) {
        rank[i] = (uint32_t)(std::lower_bound(uniq.begin(), uniq.end(), corrected[i]) - uniq.begin());
        if (observed[i] == kSortEmptyKey) {
            if (ones_rank != kSortNoRank && ones_rank != rank[i]) return fail(c, AFQ_ERR_BAD_INPUT, "correction entry " + std::to_string(i) + ": an observed barcode with two different corrected barcodes");
            ones_rank = rank[i];
        }
    }
    std::vector<uint2> ref_info(std::max<uint32_t>(ref_count, 1));
    std::vector<uint32_t> bin_base((size_t)ref_count + 1, 0);
    uint64_t n_bins64 = 0;
    for (uint32_t r = 0; r < ref_count; ++r) {
        bin_base[r] = (uint32_t)n_bins64;
        ref_info[r] = make_uint2(ref_lengths[r], (uint32_t)n_bins64);
        n_bins64 += ((uint64_t)ref_lengths[r] + (1u << kSortBinShift) - 1) >> kSortBinShift;
        if (n_bins64 >= (1ull << 31)) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_atac_sort_rad: 2^31 or more position bins");
    }
    bin_base[ref_count] = (uint32_t)n_bins64;
    const uint32_t n_bins = (uint32_t)n_bins64;
    // ---- chunk table
    RadPass P{"afq_atac_sort_rad", ", " + std::to_string(n_corr) + " corrections"};
    if (int rc = P.open(c, bytes, n_bytes, chunk_off, n_chunks, bytes_on_device != 0, 4 + bc_bytes, 32, "")) return rc;
    const uint64_t n_slots = P.n_slots;
    const uint64_t cap = sort_table_capacity(n_corr);
    const uint32_t tab_mask = (uint32_t)(cap - 1);
    // ---- does it fit?  (input + staging, 12 bytes a record of parse output, two key buffers, 22 bytes a row of output, the tables)
    const uint64_t s1 = std::max<uint64_t>(n_slots, 1), nc1 = std::max<uint32_t>(n_chunks, 1), nb1 = std::max<uint32_t>(n_bins, 1);
    const uint64_t need_rec = s1 * (12 + 16 + 22), need_tab = cap * 12 + n_corr * 12 + uniq.size() * 8,
                   need_misc = nc1 * (sizeof(SortChunk) + 16) + (uint64_t)nb1 * 8 + (uint64_t)ref_count * 12;
    if (int rc = P.fits(c, RadNeed{need_rec, need_tab + need_misc})) return rc;
    auto& B = c->asort;
    HipLatch& T = P.T;
    T(B.chunks.ensure(sizeof(SortChunk) * nc1)); T(B.obs.ensure(8 * std::max<uint64_t>(n_corr, 1))); T(B.rank.ensure(4 * std::max<uint64_t>(n_corr, 1)));
    T(B.tkey.ensure(8 * cap)); T(B.tval.ensure(4 * cap)); T(B.rinfo.ensure(8ull * ref_info.size())); T(B.bbase.ensure(4ull * bin_base.size()));
    T(B.rbc.ensure(8 * std::max<uint64_t>(uniq.size(), 1))); T(B.bin.ensure(4 * s1)); T(B.key0.ensure(8 * s1)); T(B.cstat.ensure(16ull * nc1));
    T(B.status.ensure(sizeof(DevStatus))); T(B.hist.ensure(4ull * nb1)); T(B.cur.ensure(4ull * nb1)); T(B.segs.ensure(sizeof(SortSeg))); T(B.tally.ensure(8));
    if (int rc = P.stage(c, B.chunks)) return rc;
    if (n_corr) { T(hipMemcpyAsync(B.obs.p, observed, 8 * n_corr, hipMemcpyHostToDevice, s)); T(hipMemcpyAsync(B.rank.p, rank.data(), 4 * n_corr, hipMemcpyHostToDevice, s)); }
    if (ref_count) T(hipMemcpyAsync(B.rinfo.p, ref_info.data(), 8ull * ref_count, hipMemcpyHostToDevice, s));
    T(hipMemcpyAsync(B.bbase.p, bin_base.data(), 4ull * bin_base.size(), hipMemcpyHostToDevice, s));
    if (!uniq.empty()) T(hipMemcpyAsync(B.rbc.p, uniq.data(), 8 * uniq.size(), hipMemcpyHostToDevice, s));
    T(hipMemsetAsync(B.tkey.p, 0xFF, 8 * cap, s));
    T(hipMemsetAsync(B.status.p, 0, sizeof(DevStatus), s));
    T(hipMemsetAsync(B.hist.p, 0, 4ull * nb1, s));
    T(hipMemsetAsync(B.tally.p, 0, 8, s));
    if (hc.on) { T(hipStreamSynchronize(s)); hc.lap("atac sort: alloc + H2D"); }
    if (!T.ok()) return P.hip_fail(c);
    reset_kernel_times(c);
    // ---- table, parse
    {
        ScopedTimer t(c, K_ASORT_TABLE, s);
        launch_sort_table(s, B.obs.as<uint64_t>(), B.rank.as<uint32_t>(), n_corr, B.tkey.as<uint64_t>(), B.tval.as<uint32_t>(), tab_mask, B.status.as<DevStatus>());
    }
    {
        ScopedTimer t(c, K_ASORT_PARSE, s);
        launch_sort_parse(s, SortParseArgs{P.d_bytes, (uint64_t)n_bytes, B.chunks.as<SortChunk>(), n_chunks, bc_bytes, B.tkey.as<uint64_t>(), B.tval.as<uint32_t>(), tab_mask,
                                           ones_rank, B.rinfo.as<uint2>(), ref_count, B.bin.as<uint32_t>(), B.key0.as<uint64_t>(), B.cstat.as<uint32_t>(),
                                           B.status.as<DevStatus>()});
    }
    if (int rc = P.read_back(c, hc, B.status, B.cstat, 4, "atac sort: table + parse", "a start position is not below its reference's length")) return rc;
    afq_atac_sort_stats S{};
    S.n_records = n_slots;
    for (uint32_t i = 0; i < n_chunks; ++i) { S.n_unmapped += P.cstat[4 * i]; S.n_multimapped += P.cstat[4 * i + 1]; S.n_uncorrected += P.cstat[4 * i + 2]; S.n_kept += P.cstat[4 * i + 3]; }
    const uint32_t n_kept = (uint32_t)S.n_kept;   // (< 2^32: n_slots is)
    // ---- level 0: the position bins
    std::vector<SortLeaf> leaves;
    struct Big { uint32_t off, cnt, bin; };
    std::vector<Big> big;
    if (n_kept) {
        T(B.ka.ensure(8ull * n_kept));
        if (!T.ok()) return P.hip_fail(c);
        const SortSeg seg0{0, (uint32_t)n_slots, 0, 0};
        T(hipMemcpyAsync(B.segs.p, &seg0, sizeof(seg0), hipMemcpyHostToDevice, s));
        {
            ScopedTimer t(c, K_ASORT_PART, s);
            launch_sort_partition(s, B.segs.as<SortSeg>(), 1, (uint32_t)n_slots, B.key0.as<uint64_t>(), B.bin.as<uint32_t>(), n_bins, B.hist.as<uint32_t>(),
                                  B.cur.as<uint32_t>(), B.ka.as<uint64_t>());
        }
        T(hipGetLastError());
        std::vector<uint32_t> hist(n_bins);
        T(hipMemcpyAsync(hist.data(), B.hist.p, 4ull * n_bins, hipMemcpyDeviceToHost, s));
        T(hipStreamSynchronize(s));
        if (!T.ok()) return P.hip_fail(c);
        uint32_t off = 0;
        for (uint32_t b = 0; b < n_bins; ++b) {
            const uint32_t n = hist[b];
            if (!n) continue;
            if (n > kSortRepartAbove) { big.push_back(Big{off, n, b}); ++S.n_repartitioned_bins; }
            else leaves.push_back(SortLeaf{off, n, b, 0});
            off += n;
        }
        if (off != n_kept) return fail(c, AFQ_ERR_HIP, "afq_atac_sort_rad: the bins hold " + std::to_string(off) + " of " + std::to_string(n_kept) + " fragments");
    }
    hc.lap("atac sort: partition");
    // ---- oversize segments: split by the eight highest bits in which their keys differ, until they fit a leaf or are one run
    uint32_t src_is_b = 0;
    for (uint32_t level = 0; !big.empty(); ++level) {
        if (level > 64 / kSortRadixBits) return fail(c, AFQ_ERR_HIP, "afq_atac_sort_rad: a segment survived every key bit");
        const uint32_t nb_ = (uint32_t)big.size();
        std::vector<SortSeg> segs(nb_);
        std::vector<uint64_t> ao(2ull * nb_);
        uint32_t max_cnt = 0;
        for (uint32_t i = 0; i < nb_; ++i) { segs[i] = SortSeg{big[i].off, big[i].cnt, i * 256u, 0}; ao[2 * i] = ~0ull; ao[2 * i + 1] = 0; max_cnt = std::max(max_cnt, big[i].cnt); }
        T(B.segs.ensure(sizeof(SortSeg) * nb_)); T(B.andor.ensure(16ull * nb_)); T(B.hist.ensure(1024ull * nb_)); T(B.cur.ensure(1024ull * nb_)); T(B.kb.ensure(8ull * n_kept));
        if (!T.ok()) return P.hip_fail(c);
        uint64_t* src = src_is_b ? B.kb.as<uint64_t>() : B.ka.as<uint64_t>();
        uint64_t* dst = src_is_b ? B.ka.as<uint64_t>() : B.kb.as<uint64_t>();
        T(hipMemcpyAsync(B.segs.p, segs.data(), sizeof(SortSeg) * nb_, hipMemcpyHostToDevice, s));
        T(hipMemcpyAsync(B.andor.p, ao.data(), 16ull * nb_, hipMemcpyHostToDevice, s));
        { ScopedTimer t(c, K_ASORT_PART, s); launch_sort_bits(s, B.segs.as<SortSeg>(), nb_, max_cnt, src, B.andor.as<uint64_t>()); }
        T(hipGetLastError());
        T(hipMemcpyAsync(ao.data(), B.andor.p, 16ull * nb_, hipMemcpyDeviceToHost, s));
        T(hipStreamSynchronize(s));
        if (!T.ok()) return P.hip_fail(c);
        std::vector<Big> split;
        std::vector<SortSeg> ssegs;
        max_cnt = 0;
        for (uint32_t i = 0; i < nb_; ++i) {
            const uint64_t diff = ao[2 * i] ^ ao[2 * i + 1];
            if (!diff) { leaves.push_back(SortLeaf{big[i].off, big[i].cnt, big[i].bin, src_is_b | 2u}); continue; }   // one run: no sort
            const uint32_t top = 63u - (uint32_t)__builtin_clzll(diff);
            const uint32_t shift = top >= kSortRadixBits - 1 ? top - (kSortRadixBits - 1) : 0u;
            ssegs.push_back(SortSeg{big[i].off, big[i].cnt, (uint32_t)split.size() * 256u, shift});
            split.push_back(big[i]);
            max_cnt = std::max(max_cnt, big[i].cnt);
        }
        big.clear();
        if (split.empty()) break;
        const uint32_t ns = (uint32_t)split.size();
        std::vector<uint32_t> hist(256ull * ns);
        T(hipMemcpyAsync(B.segs.p, ssegs.data(), sizeof(SortSeg) * ns, hipMemcpyHostToDevice, s));
        T(hipMemsetAsync(B.hist.p, 0, 1024ull * ns, s));
        { ScopedTimer t(c, K_ASORT_PART, s); launch_sort_partition(s, B.segs.as<SortSeg>(), ns, max_cnt, src, nullptr, 256, B.hist.as<uint32_t>(), B.cur.as<uint32_t>(), dst); }
        T(hipGetLastError());
        T(hipMemcpyAsync(hist.data(), B.hist.p, 1024ull * ns, hipMemcpyDeviceToHost, s));
        T(hipStreamSynchronize(s));
        if (!T.ok()) return P.hip_fail(c);
        src_is_b ^= 1u;
        for (uint32_t i = 0; i < ns; ++i) {
            uint32_t off = split[i].off;
            for (uint32_t d = 0; d < 256; ++d) {
                const uint32_t n = hist[256ull * i + d];
                if (!n) continue;
                if (n == split[i].cnt) return fail(c, AFQ_ERR_HIP, "afq_atac_sort_rad: a re-partition level did not split its segment");
                if (n > kSortRepartAbove) big.push_back(Big{off, n, split[i].bin});
                else leaves.push_back(SortLeaf{off, n, split[i].bin, src_is_b});
                off += n;
            }
        }
    }
    hc.lap("atac sort: re-partition");
    // ---- leaves, in position order
    std::sort(leaves.begin(), leaves.end(), [](const SortLeaf& a, const SortLeaf& b) { return a.off < b.off; });
    const uint32_t n_leaves = (uint32_t)leaves.size();
    std::vector<uint32_t> ids_small, ids_big, on(n_leaves), lout((size_t)n_leaves + 1, 0);
    for (uint32_t i = 0; i < n_leaves; ++i) ((leaves[i].flags & 2u) || leaves[i].cnt <= kSortSmallLeaf ? ids_small : ids_big).push_back(i);
    uint64_t n_out = 0;
    if (n_leaves) {
        T(B.leaves.ensure(sizeof(SortLeaf) * n_leaves)); T(B.ids.ensure(4ull * n_leaves)); T(B.on.ensure(4ull * n_leaves)); T(B.lout.ensure(4ull * (n_leaves + 1)));
        if (!T.ok()) return P.hip_fail(c);
        std::vector<uint32_t> ids(ids_small);
        ids.insert(ids.end(), ids_big.begin(), ids_big.end());
        T(hipMemcpyAsync(B.leaves.p, leaves.data(), sizeof(SortLeaf) * n_leaves, hipMemcpyHostToDevice, s));
        T(hipMemcpyAsync(B.ids.p, ids.data(), 4ull * n_leaves, hipMemcpyHostToDevice, s));
        {   // (the parse's outputs are dead after level 0: the runs' keys and lengths go where they were)
            ScopedTimer t(c, K_ASORT_LEAF, s);
            launch_sort_leaves(s, B.leaves.as<SortLeaf>(), B.ids.as<uint32_t>(), (uint32_t)ids_small.size(), B.ids.as<uint32_t>() + ids_small.size(), (uint32_t)ids_big.size(),
                               B.ka.as<uint64_t>(), B.kb.as<uint64_t>(), B.key0.as<uint64_t>(), B.bin.as<uint32_t>(), B.on.as<uint32_t>());
        }
        T(hipGetLastError());
        T(hipMemcpyAsync(on.data(), B.on.p, 4ull * n_leaves, hipMemcpyDeviceToHost, s));
        T(hipStreamSynchronize(s));
        if (!T.ok()) return P.hip_fail(c);
        for (uint32_t i = 0; i < n_leaves; ++i) { n_out += on[i]; lout[i + 1] = (uint32_t)n_out; }
    }
    hc.lap("atac sort: leaves");
    const uint64_t o1 = std::max<uint64_t>(n_out, 1);
    HostOuts H;
    uint32_t* oref = (uint32_t*)H.pinned(4 * o1);
    uint32_t* ostart = (uint32_t*)H.pinned(4 * o1);
    uint16_t* oflen = (uint16_t*)H.pinned(2 * o1);
    uint64_t* obc = (uint64_t*)H.pinned(8 * o1);
    uint32_t* ocnt = (uint32_t*)H.pinned(4 * o1);
    if (!oref || !ostart || !oflen || !obc || !ocnt) return fail(c, AFQ_ERR_OOM, "afq_atac_sort_rad: host allocation failed (" + std::to_string(22 * o1) + " bytes of rows)");
    unsigned long long n_long = 0;
    if (n_out) {
        // one allocation, the columns behind one another (8-byte column first)
        T(B.out.ensure(22 * o1 + 64));
        if (!T.ok()) return P.hip_fail(c);
        uint8_t* b = B.out.as<uint8_t>();
        uint64_t* dbc = reinterpret_cast<uint64_t*>(b);
        uint32_t* dref = reinterpret_cast<uint32_t*>(b + 8 * o1);
        uint32_t* dstart = reinterpret_cast<uint32_t*>(b + 12 * o1);
        uint32_t* dcnt = reinterpret_cast<uint32_t*>(b + 16 * o1);
        uint16_t* dflen = reinterpret_cast<uint16_t*>(b + 20 * o1);
        T(hipMemcpyAsync(B.lout.p, lout.data(), 4ull * (n_leaves + 1), hipMemcpyHostToDevice, s));
        {
            ScopedTimer t(c, K_ASORT_EMIT, s);
            launch_sort_emit(s, B.leaves.as<SortLeaf>(), n_leaves, B.lout.as<uint32_t>(), B.key0.as<uint64_t>(), B.bin.as<uint32_t>(), B.bbase.as<uint32_t>(), ref_count,
                             B.rbc.as<uint64_t>(), dref, dstart, dflen, dbc, dcnt, B.tally.as<unsigned long long>());
        }
        T(hipGetLastError());
        T(hipMemcpyAsync(oref, dref, 4 * n_out, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(ostart, dstart, 4 * n_out, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(oflen, dflen, 2 * n_out, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(obc, dbc, 8 * n_out, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(ocnt, dcnt, 4 * n_out, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(&n_long, B.tally.p, 8, hipMemcpyDeviceToHost, s));
        T(hipStreamSynchronize(s));
    }
    hc.lap("atac sort: emit + D2H");
    harvest_timers(c);
    if (!T.ok()) return P.hip_fail(c);
    S.n_distinct = n_out; S.n_long_fragments = n_long;
    if (stats) *stats = S;
    H.release();
    *out_n = n_out; *out_ref = oref; *out_start = ostart; *out_frag_len = oflen; *out_bc = obc; *out_count = ocnt;
    return 0;
}
