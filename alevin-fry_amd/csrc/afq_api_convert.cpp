// afq_api_convert.cpp — afq_convert_bam_rad: BAM spans to RAD on the device.
#include "afq_ctx.h"

void afq_convert_limits(uint32_t out[4]) {
    if (!out) return;
    out[0] = kGplParseTile; out[1] = kGplParseHalo; out[2] = kConvertLaneAlns; out[3] = kConvertScanBlock;   // (the layout scan's workgroups take kCollateScanBlock, half of that)
}

// the error word of the convert kernels (record index << 8 | code) as the entry point's refusal
static int convert_fault(afq_ctx* c, unsigned long long e) {
    harvest_timers(c);
    const std::string at = "record " + std::to_string(e >> 8) + ": ";
    switch ((uint32_t)(e & 0xFF)) {
        case kConvErrRecord: return fail(c, AFQ_ERR_BAD_INPUT, at + "malformed record: block_size is too small for the record's fixed fields, name, CIGAR and sequence, or runs past the stream, or the aux fields do not end at the record's end");
        case kConvErrRef: return fail(c, AFQ_ERR_BAD_INPUT, at + "the reference id is negative or not below the BAM header's reference count");
        case kConvErrTagMissing: return fail(c, AFQ_ERR_BAD_INPUT, at + "Input record missing CR or UR tag!");
        case kConvErrTagType: return fail(c, AFQ_ERR_BAD_INPUT, at + "cannot convert non-string (Z) tag into barcode or umi string.");
        case kConvErrBase: return fail(c, AFQ_ERR_BAD_INPUT, at + "unknown nucleotide in the CR or UR string (only A, C, G, T and N are coded)");
        case kConvErrScore: return fail(c, AFQ_ERR_BAD_INPUT, at + "NO SCORE: --filter_best needs an integer AS tag on every record of a read that is written");
        default: return fail(c, AFQ_ERR_HIP, "afq_convert_bam_rad: device error word " + std::to_string(e));
    }
}

int afq_convert_bam_rad(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* span_off, uint32_t n_spans, uint32_t n_ref, uint32_t bc_bytes,
                        uint32_t umi_bytes, int filter_best, int bytes_on_device, uint8_t** out_bytes, uint64_t* out_n_bytes, uint64_t** out_chunk_off,
                        uint32_t** out_nrec, uint64_t* out_n_chunks, afq_convert_stats* stats) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!bytes && n_bytes) || (!span_off && n_spans) || !out_bytes || !out_n_bytes || !out_chunk_off || !out_nrec || !out_n_chunks)
        return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    if (!valid_width(bc_bytes) || !valid_width(umi_bytes)) return fail(c, AFQ_ERR_INVALID_ARG, "bc_bytes and umi_bytes must be 1, 2, 4 or 8");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    if ((n_spans == 0) != (n_bytes == 0)) return fail(c, AFQ_ERR_INVALID_ARG, "afq_convert_bam_rad: a record stream needs a span table, and a span table a record stream");
    for (uint32_t i = 0; i < n_spans; ++i)   // (the walks read [span_off[i], span_off[i + 1]) and nothing else)
        if ((i == 0 && span_off[0] != 0) || (i && span_off[i] <= span_off[i - 1]) || span_off[i] >= n_bytes)
            return fail(c, AFQ_ERR_INVALID_ARG, "afq_convert_bam_rad: span " + std::to_string(i) + ": the span table must begin at 0, ascend and stay below n_bytes");
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    hipStream_t s = c->stream;
    size_t fr = 0, tot = 0;
    HIP_TRY(c, hipMemGetInfo(&fr, &tot));
    const uint64_t ns1 = std::max<uint32_t>(n_spans, 1), need_in = (bytes_on_device ? 0 : (uint64_t)n_bytes + 16) + ns1 * 24;
    if (need_in > tot)
        return fail(c, AFQ_ERR_OOM, "afq_convert_bam_rad: the input does not fit the device: " + std::to_string(need_in) + " bytes of input, staging and span table > " +
                    std::to_string(tot) + " bytes of device memory");
    auto& B = c->convert;
    HipLatch T;
    uint64_t n_rec = 0, n_kept64 = 0;
    auto hip_fail = [&]() {
        return T.fail(c, "afq_convert_bam_rad", " (" + std::to_string(n_bytes) + " input bytes, " + std::to_string(n_spans) + " spans, " + std::to_string(n_rec) + " records)");
    };
    T(B.spans.ensure(8 * ns1)); T(B.scnt.ensure(8 * ns1)); T(B.sbase.ensure(8 * ns1)); T(B.err.ensure(8)); T(B.stat.ensure(8 * kConvStatCount)); T(B.status.ensure(sizeof(DevStatus)));
    if (!T.ok()) return hip_fail();
    const uint8_t* d_bytes = nullptr;
    if (int rc = stage_rad_bytes(c, T, bytes, n_bytes, bytes_on_device != 0, s, &d_bytes)) return rc;
    if (!T.ok()) return hip_fail();
    if (n_spans) T(hipMemcpyAsync(B.spans.p, span_off, 8ull * n_spans, hipMemcpyHostToDevice, s));
    T(hipMemsetAsync(B.err.p, 0xFF, 8, s));
    T(hipMemsetAsync(B.stat.p, 0, 8 * kConvStatCount, s));
    T(hipMemsetAsync(B.status.p, 0, sizeof(DevStatus), s));
    if (!T.ok()) return hip_fail();
    reset_kernel_times(c);
    ConvertArgs a{};
    a.bytes = d_bytes; a.n_bytes = n_bytes; a.span_off = B.spans.as<uint64_t>(); a.n_spans = n_spans; a.n_ref = n_ref;
    a.bc_bytes = bc_bytes; a.umi_bytes = umi_bytes; a.filter_best = filter_best != 0;
    a.span_cnt = B.scnt.as<uint32_t>(); a.span_base = B.sbase.as<uint32_t>(); a.stat = B.stat.as<uint64_t>();
    a.err = B.err.as<unsigned long long>(); a.st = B.status.as<DevStatus>();
    // ---- the count walk; the host sums the spans' counts (a few words a span) into the bases of the fill walk
    {
        ScopedTimer t(c, K_CONVERT_WALK, s);
        launch_convert_count(s, a);
    }
    T(hipGetLastError());
    std::vector<uint32_t> cnt(2ull * n_spans), base(2ull * n_spans);
    if (n_spans) T(hipMemcpyAsync(cnt.data(), B.scnt.p, 8ull * n_spans, hipMemcpyDeviceToHost, s));
    T(hipStreamSynchronize(s));   // (the caller keeps `bytes`: the copy out of them is done by now, too)
    hc.lap("convert: H2D + count walk");
    if (!T.ok()) return hip_fail();
    for (uint32_t i = 0; i < n_spans; ++i) {
        base[2ull * i] = (uint32_t)n_rec; base[2ull * i + 1] = (uint32_t)n_kept64;   // (read only below 2^32: checked next)
        n_rec += cnt[2ull * i]; n_kept64 += cnt[2ull * i + 1];
    }
    if (n_rec >= (1ull << 32)) { harvest_timers(c); return fail(c, AFQ_ERR_UNSUPPORTED, "afq_convert_bam_rad: 2^32 or more records in one call (" + std::to_string(n_rec) + "): convert the file in parts"); }
    const uint32_t n_kept = (uint32_t)n_kept64;
    afq_convert_stats S{};
    unsigned long long e = kConvNoErr;
    uint32_t n_runs = 0, n_written = 0;
    uint64_t n_chunks = 0, out_total = 0;
    const uint64_t k1 = (uint64_t)n_kept + 1;
    // does the rest fit?  A kept record: 25 bytes of offset, index, word, head flag, score; as a run of its own 36 more (first,
    // barcode, UMI, flag, na, best score), 32 of placement (sort word, length, scan, destination) and its 4 + 8 + 8 + 4 output bytes
    {
        const uint64_t need_rec = k1 * (25 + 36 + 32 + 24) + 8 * (k1 / kConvertChunkRuns + 2) * 3;
        if (need_in + need_rec > tot) {
            harvest_timers(c);
            return fail(c, AFQ_ERR_OOM, "afq_convert_bam_rad: the input does not fit the device: " + std::to_string(need_in) + " bytes of input and staging + up to " +
                        std::to_string(need_rec) + " for " + std::to_string(n_kept) + " kept records > " + std::to_string(tot) + " bytes of device memory");
        }
    }
    T(B.roff.ensure(8 * k1)); T(B.ridx.ensure(4 * k1)); T(B.word.ensure(4 * k1)); T(B.head.ensure(4 * k1)); T(B.score.ensure(4 * k1)); T(B.has.ensure(k1));
    T(B.ssum.ensure(4 * ((k1 + kConvertScanBlock - 1) / kConvertScanBlock)));   // (the runs number at most n_kept: it serves both flag scans)
    if (!T.ok()) return hip_fail();
    a.n_kept = n_kept; a.rec_off = B.roff.as<uint64_t>(); a.rec_idx = B.ridx.as<uint32_t>(); a.word = B.word.as<uint32_t>(); a.head = B.head.as<uint32_t>();
    a.score = B.score.as<int32_t>(); a.has_score = B.has.as<uint8_t>();
    // ---- the fill walk (it raises the walk's errors: only now is a record's index in the file known), the names, the run numbers
    if (n_spans) T(hipMemcpyAsync(B.sbase.p, base.data(), 8ull * n_spans, hipMemcpyHostToDevice, s));
    {
        ScopedTimer t(c, K_CONVERT_WALK, s);
        launch_convert_fill(s, a);
    }
    {
        ScopedTimer t(c, K_CONVERT_RUNS, s);
        launch_convert_heads(s, a);
        launch_convert_scan(s, a.head, k1, B.ssum.as<uint32_t>());
    }
    T(hipGetLastError());
    T(hipMemcpyAsync(&e, B.err.p, 8, hipMemcpyDeviceToHost, s));
    T(hipMemcpyAsync(&n_runs, a.head + n_kept, 4, hipMemcpyDeviceToHost, s));
    T(hipStreamSynchronize(s));
    hc.lap("convert: fill walk + names");
    if (!T.ok()) return hip_fail();
    if (e != kConvNoErr) return convert_fault(c, e);
    if (n_runs > n_kept || (n_runs == 0) != (n_kept == 0)) { harvest_timers(c); return fail(c, AFQ_ERR_HIP, "afq_convert_bam_rad: " + std::to_string(n_runs) + " runs of " + std::to_string(n_kept) + " records"); }
    if (n_kept) {
        // ---- the aux fields, the runs' best scores, the ranks of the written runs
        const uint64_t r1 = (uint64_t)n_runs + 1;
        T(B.rfirst.ensure(4 * r1)); T(B.rbc.ensure(8 * r1)); T(B.rumi.ensure(8 * r1)); T(B.rflag.ensure(4 * r1)); T(B.rna.ensure(4 * r1)); T(B.rmax.ensure(4 * r1));
        if (!T.ok()) return hip_fail();
        a.n_runs = n_runs; a.run_first = B.rfirst.as<uint32_t>(); a.run_bc = B.rbc.as<uint64_t>(); a.run_umi = B.rumi.as<uint64_t>(); a.run_flag = B.rflag.as<uint32_t>();
        a.run_na = B.rna.as<uint32_t>(); a.run_max = B.rmax.as<int32_t>();
        {
            ScopedTimer t(c, K_CONVERT_RUNS, s);
            launch_convert_aux(s, a);
            launch_convert_runs(s, a);
            launch_convert_scan(s, a.run_flag, r1, B.ssum.as<uint32_t>());
        }
        T(hipGetLastError());
        uint64_t dstat[kConvStatCount] = {};
        T(hipMemcpyAsync(&e, B.err.p, 8, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(&n_written, a.run_flag + n_runs, 4, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(dstat, B.stat.p, sizeof dstat, hipMemcpyDeviceToHost, s));
        T(hipStreamSynchronize(s));
        hc.lap("convert: aux + runs");
        if (!T.ok()) return hip_fail();
        if (e != kConvNoErr) return convert_fault(c, e);
        S.n_runs_dropped_n = dstat[kConvRunsDroppedN]; S.n_alignments_in = dstat[kConvAlnIn]; S.n_alignments_written = dstat[kConvAlnWritten]; S.n_long_runs = dstat[kConvLongRuns];
        if (n_written > n_runs || n_written + S.n_runs_dropped_n != n_runs) {   // (the placement's bounds rest on these)
            harvest_timers(c);
            return fail(c, AFQ_ERR_HIP, "afq_convert_bam_rad: " + std::to_string(n_written) + " written and " + std::to_string(S.n_runs_dropped_n) + " dropped runs of " + std::to_string(n_runs));
        }
    }
    n_chunks = ((uint64_t)n_written + kConvertChunkRuns - 1) / kConvertChunkRuns;
    const uint64_t nc1 = n_chunks + 1;
    if (n_written) {
        // ---- the layout: the scan of the runs' lengths in written order, 8 bytes in front of every 10 001st
        const uint64_t w1 = (uint64_t)n_written + 1, n_sblocks = (w1 + kCollateScanBlock - 1) / kCollateScanBlock;
        T(B.key.ensure(8 * w1)); T(B.rec.ensure(8 * w1)); T(B.bsum.ensure(8 * n_sblocks)); T(B.ex.ensure(8 * w1)); T(B.dest.ensure(8 * w1));
        if (!T.ok()) return hip_fail();
        a.n_written = n_written; a.key = B.key.as<uint64_t>(); a.rec = B.rec.as<uint2>(); a.dest = B.dest.as<uint64_t>();
        {
            ScopedTimer t(c, K_CONVERT_PLACE, s);
            launch_convert_place(s, a);
            launch_collate_scan(s, a.key, a.rec, n_written, B.bsum.as<uint64_t>(), B.ex.as<uint64_t>(), B.dest.as<uint64_t>());
        }
        T(hipGetLastError());
        uint64_t rec_bytes = 0;
        T(hipMemcpyAsync(&rec_bytes, B.ex.as<uint64_t>() + n_written, 8, hipMemcpyDeviceToHost, s));
        T(hipStreamSynchronize(s));
        if (!T.ok()) return hip_fail();
        const uint64_t H = 4 + bc_bytes + umi_bytes;
        if (rec_bytes > H * n_written + 4 * S.n_alignments_written) {   // (equal, unless a run alone is 4 GiB: the status word says so below)
            harvest_timers(c);
            return fail(c, AFQ_ERR_HIP, "afq_convert_bam_rad: the layout holds " + std::to_string(rec_bytes) + " bytes of runs, the runs " + std::to_string(H * n_written + 4 * S.n_alignments_written));
        }
        out_total = rec_bytes + 8 * n_chunks;
    }
    const uint64_t o1 = std::max<uint64_t>(out_total, 1);
    T(B.out.ensure(o1)); T(B.off.ensure(8 * nc1)); T(B.nrec.ensure(4 * nc1));
    if (!T.ok()) return hip_fail();
    a.out = B.out.as<uint8_t>();
    if (n_written) {
        {
            ScopedTimer t(c, K_CONVERT_PLACE, s);
            launch_collate_heads(s, a.key, n_written, B.ex.as<uint64_t>(), (uint32_t)n_chunks, B.off.as<uint64_t>(), B.nrec.as<uint32_t>(), a.out, a.st);
        }
        {
            ScopedTimer t(c, K_CONVERT_WRITE, s);
            launch_convert_write(s, a);
        }
        T(hipGetLastError());
    }
    HostOuts Hs;
    uint8_t* ob = (uint8_t*)Hs.mallocd(o1);
    uint64_t* ooff = (uint64_t*)Hs.mallocd(8 * nc1);
    uint32_t* onrec = (uint32_t*)Hs.mallocd(4 * nc1);
    if (!ob || !ooff || !onrec) { (void)hipStreamSynchronize(s); harvest_timers(c); return fail(c, AFQ_ERR_OOM, "afq_convert_bam_rad: host allocation failed (" + std::to_string(o1 + 12 * nc1) + " bytes of output)"); }
    DevStatus st{};
    ooff[0] = 0;
    if (n_written) {
        T(hipMemcpyAsync(&st, B.status.p, sizeof(st), hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(ob, B.out.p, out_total, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(ooff, B.off.p, 8 * nc1, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(onrec, B.nrec.p, 4 * n_chunks, hipMemcpyDeviceToHost, s));
    }
    T(hipStreamSynchronize(s));   // (before any exit below: the copies write into Hs's blocks)
    harvest_timers(c);
    hc.lap("convert: place + write + D2H");
    if (!T.ok()) return hip_fail();
    if (st.err_code == kErrCollateChunk) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_convert_bam_rad: output chunk " + std::to_string(st.err_cell) + ": an output chunk of 4 GiB or more");
    if (st.err_code) return fail(c, AFQ_ERR_HIP, "afq_convert_bam_rad: device status " + std::to_string(st.err_code) + " in the write");
    if (ooff[n_chunks] != out_total) return fail(c, AFQ_ERR_HIP, "afq_convert_bam_rad: the chunks end at " + std::to_string(ooff[n_chunks]) + " of " + std::to_string(out_total) + " output bytes");
    S.n_records = n_rec; S.n_dropped_by_flag = n_rec - n_kept; S.n_runs = n_runs; S.n_runs_written = n_written; S.n_chunks = n_chunks; S.out_bytes = out_total;
    if (stats) *stats = S;
    Hs.release();
    *out_bytes = ob; *out_n_bytes = out_total; *out_chunk_off = ooff; *out_nrec = onrec; *out_n_chunks = n_chunks;
    return 0;
}
