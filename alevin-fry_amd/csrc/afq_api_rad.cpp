// afq_api_rad.cpp — the chunk-table checks with the entry points' error texts, and the record pass (RadPass) that the
// *_rad entry points over an uncollated RAD share: chunk table, fit check, staging, status read-back.
#include <optional>

#include "afq_ctx.h"

// The checks of afq_chunk_table.h with the entry points' error texts (`noun`: what the caller's API calls a chunk).
int chunk_fault(afq_ctx* c, const char* noun, uint32_t i, ChunkFault f) {
    static const char* const kWhat[] = {"", ": chunk offset out of range", ": chunk header/size out of range", ": chunk nbytes does not match its records"};
    return fail(c, AFQ_ERR_BAD_INPUT, std::string(noun) + " " + std::to_string(i) + kWhat[f]);
}
int check_chunk_offsets(afq_ctx* c, const uint64_t* chunk_off, uint32_t n, size_t n_bytes, const char* noun) {
    const uint32_t bad = first_chunk_outside(chunk_off, n, n_bytes);
    return bad < n ? chunk_fault(c, noun, bad, kChunkOffset) : 0;
}

// The `nbytes, nrec` headers of n chunks into hdr[2 * n], from host bytes or gathered off the device (k_gather_headers; `timed`:
// under a K_GATHER bracket).  No byte is read and nothing is launched before every offset has passed stage A.
int fetch_chunk_headers(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n, bool on_device, uint32_t* hdr,
                        const char* noun, bool timed) {
    if (int rc = check_chunk_offsets(c, chunk_off, n, n_bytes, noun)) return rc;
    for (uint32_t i = 0; i < n && !on_device; ++i) std::memcpy(hdr + 2ull * i, bytes + chunk_off[i], 8);
    if (!on_device || !n) return 0;
    HIP_TRY(c, c->d_chunk_off.ensure(8ull * n));
    HIP_TRY(c, c->d_hdr.ensure(8ull * n));
    HIP_TRY(c, hipMemcpyAsync(c->d_chunk_off.p, chunk_off, 8ull * n, hipMemcpyHostToDevice, c->stream));
    std::optional<ScopedTimer> t;
    if (timed) t.emplace(c, K_GATHER);
    launch_gather_headers(c->stream, bytes, n_bytes, c->d_chunk_off.as<uint64_t>(), n, c->d_hdr.as<uint32_t>());
    t.reset();
    HIP_TRY(c, hipMemcpyAsync(hdr, c->d_hdr.p, 8ull * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

// The chunk table of a record pass (the *_rad entry points over an uncollated RAD): every header fetched and checked - `min_rec`
// is the bytes of a record without alignments -, each chunk with the slot of its first record; n_slots: the records of the call.
static int build_sort_chunks(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, bool on_device, uint32_t min_rec,
                             std::vector<SortChunk>& out, uint64_t& n_slots) {
    std::vector<uint32_t> hdr(2ull * n_chunks);
    if (int rc = fetch_chunk_headers(c, bytes, n_bytes, chunk_off, n_chunks, on_device, hdr.data(), "chunk")) return rc;
    std::vector<SortChunk> chunks(n_chunks);
    n_slots = 0;
    for (uint32_t i = 0; i < n_chunks; ++i) {
        const uint32_t nb = hdr[2 * i], nr = hdr[2 * i + 1];
        if (const ChunkFault f = check_chunk_header(chunk_off[i], nb, nr, n_bytes, min_rec)) return chunk_fault(c, "chunk", i, f);
        chunks[i] = SortChunk{chunk_off[i], n_slots, nb, nr};
        n_slots += nr;
    }
    out.swap(chunks);
    return 0;
}

// Host bytes of a record pass to the device (c->d_bytes_own, through staged_h2d); bytes that are there already stay where they
// are.  *d_bytes: where the kernels read them.  Called behind the entry point's own `ensure`s and before its copies of tables;
// an allocation that fails is left in T, for the caller to word.
int stage_rad_bytes(afq_ctx* c, HipLatch& T, const uint8_t* bytes, size_t n_bytes, bool on_device, hipStream_t s, const uint8_t** d_bytes) {
    *d_bytes = bytes;
    if (on_device) return 0;
    T(c->d_bytes_own.ensure(n_bytes + 16));
    if (!T.ok()) return 0;
    if (n_bytes)
        if (int rc = staged_h2d(c, (uint8_t*)c->d_bytes_own.p, bytes, n_bytes, s, host_ptr_is_pinned(bytes) && host_ptr_is_pinned(bytes + n_bytes - 1))) return rc;
    *d_bytes = c->d_bytes_own.as<uint8_t>();
    return 0;
}

// A non-zero status word of a record pass's table + parse / measure kernels as the entry point's refusal.  `start_range`: what
// the caller says of kErrStartRange behind "chunk k: " (`atac sort` and `atac generate-permit-list` mean different things by it);
// null where the kernels never raise it.
static int rad_status_fault(afq_ctx* c, const char* who, const DevStatus& st, const char* start_range) {
    harvest_timers(c);
    const std::string at = std::to_string(st.err_cell);
    if (st.err_code == kErrStartRange && start_range) return fail(c, AFQ_ERR_BAD_INPUT, "chunk " + at + ": " + start_range);
    switch (st.err_code) {
        case kErrCorrection: return fail(c, AFQ_ERR_BAD_INPUT, "correction entry " + at + ": an observed barcode with two different corrected barcodes");
        case kErrRecordWalk: return fail(c, AFQ_ERR_BAD_INPUT, "chunk " + at + ": the records do not tile the chunk (nbytes / nrec do not match them)");
        case kErrRefRange: return fail(c, AFQ_ERR_BAD_INPUT, "chunk " + at + ": a reference id is not below ref_count");
        default: return fail(c, AFQ_ERR_HIP, std::string(who) + ": device status " + std::to_string(st.err_code));
    }
}
int RadPass::open(afq_ctx* c, const uint8_t* bytes_, size_t n_bytes_, const uint64_t* chunk_off, uint32_t n_chunks_, bool on_device_, uint32_t min_rec, uint32_t ceiling_log2,
                  const char* tail) {
    bytes = bytes_; n_bytes = n_bytes_; n_chunks = n_chunks_; on_device = on_device_;
    if (int rc = build_sort_chunks(c, bytes, n_bytes, chunk_off, n_chunks, on_device, min_rec, chunks, n_slots)) return rc;
    if (n_slots >= (1ull << ceiling_log2))
        return fail(c, AFQ_ERR_UNSUPPORTED, std::string(who) + ": 2^" + std::to_string(ceiling_log2) + " or more records in one call (" + std::to_string(n_slots) + ")" + tail);
    return 0;
}

int RadPass::fits(afq_ctx* c, const RadNeed& need) {
    const uint64_t need_in = on_device ? 0 : n_bytes + 16;
    size_t fr = 0, tot = 0;
    HIP_TRY(c, hipMemGetInfo(&fr, &tot));
    if (need_in + need.out + need.rec + need.tab_misc + need.snappy <= tot) return 0;
    return fail(c, AFQ_ERR_OOM, std::string(who) + ": the input does not fit the device: " + std::to_string(need_in) + " bytes of input and staging + " +
                (need.has_out ? "up to " + std::to_string(need.out) + " of output + " : std::string()) + std::to_string(need.rec) + " for " + std::to_string(n_slots) +
                " records + " + std::to_string(need.tab_misc) + " " + need.tables + (need.snappy ? " + " + std::to_string(need.snappy) + " for the snappy encoder" : std::string()) +
                " > " + std::to_string(tot) + " bytes of device memory");
}

int RadPass::stage(afq_ctx* c, DevBuf& chunks_buf) {
    if (!T.ok()) return hip_fail(c);
    if (int rc = stage_rad_bytes(c, T, bytes, n_bytes, on_device, c->stream, &d_bytes)) return rc;
    if (!T.ok()) return hip_fail(c);
    if (n_chunks) T(hipMemcpyAsync(chunks_buf.p, chunks.data(), sizeof(SortChunk) * n_chunks, hipMemcpyHostToDevice, c->stream));
    return 0;
}

int RadPass::read_back(afq_ctx* c, HostClock& hc, DevBuf& status_buf, DevBuf& cstat_buf, uint32_t words_per_chunk, const char* lap, const char* start_range) {
    hipStream_t s = c->stream;
    T(hipGetLastError());
    cstat.assign((size_t)words_per_chunk * n_chunks, 0);
    T(hipMemcpyAsync(&st, status_buf.p, sizeof(st), hipMemcpyDeviceToHost, s));
    if (n_chunks) T(hipMemcpyAsync(cstat.data(), cstat_buf.p, 4ull * words_per_chunk * n_chunks, hipMemcpyDeviceToHost, s));
    T(hipStreamSynchronize(s));   // (the caller keeps `bytes` and its tables: the copies out of them are done by now, too)
    hc.lap(lap);
    if (!T.ok()) return hip_fail(c);
    if (st.err_code) return rad_status_fault(c, who, st, start_range);
    return 0;
}
