// afq_api_collate.cpp — the snappy frame encoder's and decoder's host side and the three collates with their limits.
#include <functional>

#include "afq_ctx.h"
#include "afq_gpl_host.h"
#include "afq_snappy_elem.h"
#include "afq_snappy_plan.h"

// Both collates' host step: val[i] = the index in `cells` of corrected[i]; ones_cell = the cell of the all-ones observed barcode
// (it cannot be a key of the device's table, whose free slots are all ones), kSortNoRank without one.
static int collate_cell_index(afq_ctx* c, const uint64_t* observed, const uint64_t* corrected, uint64_t n_corr, const uint64_t* cells, uint32_t n_cells,
                              std::vector<uint32_t>& val, uint32_t& ones_cell) {
    val.assign(n_corr, 0);
    ones_cell = kSortNoRank;
    std::vector<std::pair<uint64_t, uint32_t>> by_bc(n_cells);
    for (uint32_t i = 0; i < n_cells; ++i) by_bc[i] = {cells[i], i};
    std::sort(by_bc.begin(), by_bc.end());
    for (uint32_t i = 1; i < n_cells; ++i)
        if (by_bc[i].first == by_bc[i - 1].first)
            return fail(c, AFQ_ERR_BAD_INPUT, "cells " + std::to_string(by_bc[i - 1].second) + " and " + std::to_string(by_bc[i].second) + " carry one barcode (" +
                        std::to_string(by_bc[i].first) + ")");
    for (uint64_t i = 0; i < n_corr; ++i) {
        const auto it = std::lower_bound(by_bc.begin(), by_bc.end(), std::make_pair(corrected[i], 0u));
        if (it == by_bc.end() || it->first != corrected[i])
            return fail(c, AFQ_ERR_BAD_INPUT, "correction entry " + std::to_string(i) + ": observed barcode " + std::to_string(observed[i]) + " is corrected to " +
                        std::to_string(corrected[i]) + ", which is not a cell");
        val[i] = it->second;
        if (observed[i] == kSortEmptyKey) {
            if (ones_cell != kSortNoRank && ones_cell != val[i]) return fail(c, AFQ_ERR_BAD_INPUT, "correction entry " + std::to_string(i) + ": an observed barcode with two different corrected barcodes");
            ones_cell = val[i];
        }
    }
    return 0;
}

// The snappy frame encoder (afq_snappy.hip).  Device bytes it takes beside n bytes of input that are on the device already: a
// slot a chunk, 16 bytes of meta and 8 of offset a chunk, and the stream at its bound.
static uint64_t snappy_device_need(uint64_t n) {
    const uint64_t nb = snappy_blocks(n);
    return nb * kSnappySlot + nb * sizeof(SnappyMeta) + (nb + 1) * 8 + snappy_stream_bound(n);
}

// d_in: n bytes on the device (whatever c->stream holds in front of them is waited for) -> their frame stream as one malloc'd
// block.  The caller has checked that snappy_device_need(n) fits.
static int snappy_encode_device(afq_ctx* c, const char* who, const uint8_t* d_in, uint64_t n, uint8_t** out, uint64_t* out_n, afq_snappy_stats* stats) {
    static const uint8_t kId[10] = {0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59};
    afq_snappy_stats S{};
    S.n_in = n;
    const uint64_t nb = snappy_blocks(n);
    if (nb >= (1ull << 31)) return fail(c, AFQ_ERR_UNSUPPORTED, std::string(who) + ": 2^31 or more snappy frame chunks (" + std::to_string(n) + " bytes)");
    if (!nb) {
        uint8_t* ob = (uint8_t*)std::malloc(10);
        if (!ob) return fail(c, AFQ_ERR_OOM, std::string(who) + ": host allocation failed (10 bytes of snappy stream)");
        std::memcpy(ob, kId, 10);
        S.n_out = 10;
        if (stats) *stats = S;
        *out = ob; *out_n = 10;
        return 0;
    }
    auto& Z = c->snappy;
    hipStream_t s = c->stream;
    HipLatch T;
    HostClock hc;
    const std::string detail = " (snappy encoder, " + std::to_string(n) + " bytes in " + std::to_string(nb) + " frame chunks)";
    T(Z.slots.ensure(nb * kSnappySlot)); T(Z.meta.ensure(nb * sizeof(SnappyMeta))); T(Z.off.ensure((nb + 1) * 8)); T(Z.stream.ensure(snappy_stream_bound(n)));
    if (!T.ok()) return T.fail(c, who, detail);
    hc.lap("snappy: buffers");
    {
        ScopedTimer t(c, K_SNAPPY_BLOCKS, s);
        launch_snappy_blocks(s, d_in, n, nb, Z.slots.as<uint8_t>(), Z.meta.as<SnappyMeta>());
    }
    {
        ScopedTimer t(c, K_SNAPPY_PACK, s);
        launch_snappy_layout(s, Z.meta.as<SnappyMeta>(), nb, Z.off.as<uint64_t>());
        launch_snappy_pack(s, d_in, nb, Z.slots.as<uint8_t>(), Z.meta.as<SnappyMeta>(), Z.off.as<uint64_t>(), Z.stream.as<uint8_t>());
    }
    T(hipGetLastError());
    std::vector<SnappyMeta> meta(nb);
    uint64_t total = 0;
    T(hipMemcpyAsync(&total, Z.off.as<uint64_t>() + nb, 8, hipMemcpyDeviceToHost, s));
    T(hipMemcpyAsync(meta.data(), Z.meta.p, nb * sizeof(SnappyMeta), hipMemcpyDeviceToHost, s));
    T(hipStreamSynchronize(s));
    hc.lap("snappy: kernels + lengths");
    if (!T.ok()) { harvest_timers(c); return T.fail(c, who, detail); }
    if (total < 10 + 8 * nb || total > snappy_stream_bound(n)) {
        harvest_timers(c);
        return fail(c, AFQ_ERR_HIP, std::string(who) + ": a snappy stream of " + std::to_string(total) + " bytes from " + std::to_string(n) + " of input");
    }
    uint8_t* ob = (uint8_t*)std::malloc(total);
    if (!ob) { harvest_timers(c); return fail(c, AFQ_ERR_OOM, std::string(who) + ": host allocation failed (" + std::to_string(total) + " bytes of snappy stream)"); }
    hc.lap("snappy: host block");
    T(hipMemcpyAsync(ob, Z.stream.p, total, hipMemcpyDeviceToHost, s));
    T(hipStreamSynchronize(s));
    hc.lap("snappy: stream D2H");
    harvest_timers(c);
    if (!T.ok()) { std::free(ob); return T.fail(c, who, detail); }
    S.n_out = total; S.n_blocks = nb;
    for (const SnappyMeta& m : meta) {
        if (m.body & kSnappyStored) ++S.n_blocks_stored;
        S.n_literal_bytes += m.lit; S.n_copies += m.copies;
    }
    if (stats) *stats = S;
    *out = ob; *out_n = total;
    return 0;
}

void afq_snappy_limits(uint32_t out[4]) {
    if (!out) return;
    out[0] = kSnappyBlock; out[1] = kSnappyHashSlots; out[2] = kSnappyMaxCopy; out[3] = kSnappyBlocksPerWg;
}

int afq_snappy_frame_encode(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, int bytes_on_device, uint8_t** out_bytes, uint64_t* out_n_bytes, afq_snappy_stats* stats) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!bytes && n_bytes) || !out_bytes || !out_n_bytes) return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    const uint64_t need_in = bytes_on_device ? 0 : (uint64_t)n_bytes, need = snappy_device_need(n_bytes);
    {
        size_t fr = 0, tot = 0;
        HIP_TRY(c, hipMemGetInfo(&fr, &tot));
        if (need_in + need > tot)
            return fail(c, AFQ_ERR_OOM, "afq_snappy_frame_encode: the input does not fit the device: " + std::to_string(need_in) + " bytes of input + " + std::to_string(need) +
                        " of slots, stream and tables > " + std::to_string(tot) + " bytes of device memory");
    }
    const uint8_t* d_in = bytes;
    if (!bytes_on_device && n_bytes) {
        HipLatch T;
        T(c->snappy.in.ensure(n_bytes));
        if (T.ok()) T(hipMemcpyAsync(c->snappy.in.p, bytes, n_bytes, hipMemcpyHostToDevice, c->stream));
        if (!T.ok()) return T.fail(c, "afq_snappy_frame_encode", " (" + std::to_string(n_bytes) + " bytes of input)");
        d_in = c->snappy.in.as<uint8_t>();
    }
    reset_kernel_times(c);
    return snappy_encode_device(c, "afq_snappy_frame_encode", d_in, n_bytes, out_bytes, out_n_bytes, stats);
}

// ---------------------------------------------------------------------------------------------------------------- the decoder
void afq_snappy_decode_limits(uint32_t out[4]) {
    if (!out) return;
    out[0] = kSnappyDecWindow; out[1] = kSnappyDecThreads; out[2] = kSnappyDecPieceChunks; out[3] = kSnappyDecLds;
}

static const char* snappy_code_words(uint32_t code) {
    switch (code) {
        case kSnappyLiteralPastBody: return "a literal runs past the block";
        case kSnappyOffsetZero: return "a copy from offset 0";
        case kSnappyOffsetPastStart: return "a copy from in front of the chunk";
        case kSnappyOutputPastUlen: return "more bytes than declared";
        case kSnappyTagCutOff: return "an element cut off";
        case kSnappyOutputShort: return "fewer bytes than declared";
        case kSnappyLengthDisagrees: return "the block's length is not the planned one";
        default: return "";
    }
}

// The compressed bytes of a piece - at most kSnappyDecPieceChunks data chunks within kSnappyDecPieceBytes of stream - cross
// into one of two device buffers on c->stream while the launch of the piece in front reads the other on the second stream.
// A piece is sized so that staged_h2d takes it through the context's pinned staging and its filler threads (it does so from
// 64 MiB on; a full piece of compressible records is some 150 MB, one of stored chunks 128 MiB); what is shorter - a small
// stream, a stream's last piece - goes up as one plain copy, as everywhere in the library.
static constexpr uint64_t kSnappyDecPieceBytes = 128ull << 20;   // (a chunk holds less than 2^24)
int afq_snappy_frame_decode_device(afq_ctx* c, const uint8_t* stream, size_t n, uint32_t shift, int out_on_device, uint8_t** out, uint64_t* out_n, afq_snappy_stats* stats) {
    static const char* who = "afq_snappy_frame_decode_device";
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!stream && n) || !out || !out_n || shift > 3) return fail(c, AFQ_ERR_INVALID_ARG, !out || !out_n || (!stream && n) ? "null argument" : "shift is 0..3");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    std::vector<SnappyChunk> chunks;
    uint64_t total = 0;
    {
        std::string err;
        if (!snappy_frame_plan(stream, n, chunks, total, err)) return fail(c, AFQ_ERR_BAD_INPUT, err);
    }
    const uint64_t nc = chunks.size();
    if (nc >= (1ull << 31)) return fail(c, AFQ_ERR_UNSUPPORTED, std::string(who) + ": 2^31 or more snappy frame chunks");
    // the pieces: [first[k], first[k + 1]) of the chunks, their bytes [lo, hi) of the stream
    struct Piece { uint64_t c0, c1, lo, hi; };
    std::vector<Piece> pieces;
    std::vector<SnappyDecChunk> plan(nc);
    uint64_t piece_max = 0;
    for (uint64_t i = 0; i < nc;) {
        Piece P{i, i, chunks[i].in_off, chunks[i].in_off};
        while (P.c1 < nc && P.c1 - P.c0 < kSnappyDecPieceChunks && (P.c1 == P.c0 || chunks[P.c1].in_off + chunks[P.c1].in_len - P.lo <= kSnappyDecPieceBytes)) {
            const SnappyChunk& k = chunks[P.c1];
            plan[P.c1] = SnappyDecChunk{(uint64_t)k.in_off - P.lo, k.out_off, (uint32_t)k.in_len, (uint32_t)k.ulen, k.crc, k.compressed ? 1u : 0u};
            P.hi = k.in_off + k.in_len;
            ++P.c1;
        }
        piece_max = std::max(piece_max, P.hi - P.lo);
        pieces.push_back(P);
        i = P.c1;
    }
    hc.lap("sz decode: plan");
    const uint64_t n_buf = pieces.size() > 1 ? 2 : 1;
    const uint64_t need_in = n_buf * piece_max, need_plan = nc * sizeof(SnappyDecChunk) + 64, need_out = (uint64_t)shift + total + 16;
    auto& Z = c->snappy;
    {   // what the decoder has to allocate beyond what it holds from an earlier call, against what the device has free
        auto more = [](const DevBuf& b, uint64_t want) -> uint64_t { return want > b.cap ? want : 0; };
        uint64_t alloc = more(Z.dec_plan, need_plan) + more(Z.dec_out, need_out) + more(Z.dec_stat, 5 * 8);
        for (uint64_t b = 0; b < n_buf && nc; ++b) alloc += more(Z.dec_in[b], piece_max);
        size_t fr = 0, tot = 0;
        HIP_TRY(c, hipMemGetInfo(&fr, &tot));
        uint64_t room = fr;
        if (const long hook = test_hook_long("SNAPPY_DEC_ROOM_BYTES", -1); hook >= 0) room = std::min<uint64_t>(room, (uint64_t)hook);
        if (alloc > room)
            return fail(c, AFQ_ERR_OOM, std::string(who) + ": the stream does not fit the device: " + std::to_string(need_in) + " bytes of compressed pieces + " +
                        std::to_string(need_plan) + " of plan + " + std::to_string(need_out) + " of decoded bytes, " + std::to_string(alloc) + " of them still to allocate > " +
                        std::to_string(room) + " bytes free of " + std::to_string(tot) + " of device memory");
    }
    const std::string detail = " (snappy decoder, " + std::to_string(n) + " bytes in " + std::to_string(nc) + " data chunks, " + std::to_string(total) + " decoded)";
    HipLatch T;
    T(Z.dec_out.ensure(need_out)); T(Z.dec_plan.ensure(need_plan)); T(Z.dec_stat.ensure(5 * 8));
    for (uint64_t b = 0; b < n_buf && nc; ++b) T(Z.dec_in[b].ensure(piece_max));
    if (!T.ok()) return T.fail(c, who, detail);
    hipStream_t up = c->stream, ks = second_stream(c);
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr}, ev_plan = nullptr;
    for (int b = 0; b < 2; ++b) { T(hipEventCreateWithFlags(&ev_up[b], hipEventDisableTiming)); T(hipEventCreateWithFlags(&ev_done[b], hipEventDisableTiming)); }
    T(hipEventCreateWithFlags(&ev_plan, hipEventDisableTiming));
    auto drop_events = [&] {
        for (int b = 0; b < 2; ++b) { if (ev_up[b]) (void)hipEventDestroy(ev_up[b]); if (ev_done[b]) (void)hipEventDestroy(ev_done[b]); }
        if (ev_plan) (void)hipEventDestroy(ev_plan);
    };
    uint64_t h_stat[5] = {~0ull, 0, 0, 0, 0};   // the status word, then chunks, stored chunks, literal bytes, copy elements
    int rc = 0;
    if (T.ok()) {
        reset_kernel_times(c);
        T(hipMemcpyAsync(Z.dec_stat.p, h_stat, sizeof h_stat, hipMemcpyHostToDevice, up));
        if (nc) T(hipMemcpyAsync(Z.dec_plan.p, plan.data(), nc * sizeof(SnappyDecChunk), hipMemcpyHostToDevice, up));
        if (shift) T(hipMemsetAsync(Z.dec_out.p, 0, 4, up));   // what stands around the decoded bytes is zero, as around a batch that submit_host landed
        T(hipMemsetAsync(Z.dec_out.as<uint8_t>() + shift + total, 0, 16, up));
        T(hipEventRecord(ev_plan, up));
        T(hipStreamWaitEvent(ks, ev_plan, 0));
        uint8_t* d_dst = Z.dec_out.as<uint8_t>() + shift;
        for (size_t k = 0; k < pieces.size() && T.ok() && !rc; ++k) {
            const Piece& P = pieces[k];
            const int b = (int)(k & 1);
            if (k >= 2) T(hipStreamWaitEvent(up, ev_done[b], 0));   // the launch that read this buffer last
            const uint8_t* src = stream + P.lo;
            const size_t len = (size_t)(P.hi - P.lo);
            if (len) rc = staged_h2d(c, Z.dec_in[b].as<uint8_t>(), src, len, up, host_ptr_is_pinned(src) && host_ptr_is_pinned(src + len - 1));
            if (rc) break;
            T(hipEventRecord(ev_up[b], up));
            T(hipStreamWaitEvent(ks, ev_up[b], 0));
            {
                ScopedTimer t(c, K_SNAPPY_DECODE, ks);
                launch_snappy_decode(ks, Z.dec_in[b].as<uint8_t>(), Z.dec_plan.as<SnappyDecChunk>() + P.c0, (uint32_t)(P.c1 - P.c0), P.c0, d_dst, Z.dec_stat.as<uint64_t>(),
                                     Z.dec_stat.as<uint64_t>() + 1);
            }
            T(hipGetLastError());
            T(hipEventRecord(ev_done[b], ks));
        }
        T(hipMemcpyAsync(h_stat, Z.dec_stat.p, sizeof h_stat, hipMemcpyDeviceToHost, ks));
        T(hipStreamSynchronize(up));
        T(hipStreamSynchronize(ks));
        harvest_timers(c);
    }
    drop_events();
    hc.lap("sz decode: upload + kernels");
    if (rc) return rc;
    if (!T.ok()) return T.fail(c, who, detail);
    if (h_stat[0] != ~0ull) {
        const uint32_t code = (uint32_t)(h_stat[0] & 0xff);
        const std::string at = "chunk " + std::to_string(h_stat[0] >> 8);
        if (code == kSnappyCrcMismatch) return fail(c, AFQ_ERR_BAD_INPUT, "snappy CRC mismatch (" + at + ")");
        return fail(c, AFQ_ERR_BAD_INPUT, "corrupt snappy block (" + at + ": " + snappy_code_words(code) + ")");
    }
    if (h_stat[1] != nc) return fail(c, AFQ_ERR_HIP, std::string(who) + ": " + std::to_string(h_stat[1]) + " of " + std::to_string(nc) + " chunks decoded" + detail);
    if (out_on_device) *out = Z.dec_out.as<uint8_t>();
    else {
        uint8_t* ob = (uint8_t*)std::malloc(total ? total : 1);
        if (!ob) return fail(c, AFQ_ERR_OOM, std::string(who) + ": host allocation failed (" + std::to_string(total) + " decoded bytes)");
        if (total) {
            T(hipMemcpyAsync(ob, Z.dec_out.as<uint8_t>() + shift, total, hipMemcpyDeviceToHost, ks));
            T(hipStreamSynchronize(ks));
        }
        if (!T.ok()) { std::free(ob); return T.fail(c, who, detail); }
        hc.lap("sz decode: bytes D2H");
        *out = ob;
    }
    *out_n = total;
    if (stats) {
        afq_snappy_stats S{};
        S.n_in = n; S.n_out = total; S.n_blocks = h_stat[1]; S.n_blocks_stored = h_stat[2]; S.n_literal_bytes = h_stat[3]; S.n_copies = h_stat[4];
        *stats = S;
    }
    return 0;
}

// The chunk table of a collated record stream on the device.  The hop counts every chunk and writes those that the buffers hold:
// a first guess of a chunk per 4 KiB, and a second launch with room for all where the stream has more.
int afq_collated_chunk_table(afq_ctx* c, const uint8_t* d_bytes, uint64_t n, uint64_t first_chunk, uint32_t rec_hdr_bytes, uint64_t** out_off, uint32_t** out_nbytes,
                             uint32_t** out_nrec, uint64_t** out_first_bc, uint64_t* out_n_chunks) {
    static const char* who = "afq_collated_chunk_table";
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!d_bytes && n) || !out_off || !out_nbytes || !out_nrec || !out_first_bc || !out_n_chunks) return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    auto& Z = c->snappy;
    hipStream_t s = c->stream;
    uint64_t cap = std::max<uint64_t>(4096, n / 4096), h_stat[2] = {0, 0};
    reset_kernel_times(c);
    for (int pass = 0; pass < 2; ++pass) {
        HipLatch T;
        T(Z.ct_off.ensure(cap * 8)); T(Z.ct_nb.ensure(cap * 4)); T(Z.ct_nr.ensure(cap * 4)); T(Z.ct_bc.ensure(cap * 8)); T(Z.ct_stat.ensure(16));
        if (T.ok()) {
            ScopedTimer t(c, K_CHUNK_TABLE, s);
            launch_collated_chunk_table(s, d_bytes, n, first_chunk, rec_hdr_bytes, cap, Z.ct_off.as<uint64_t>(), Z.ct_nb.as<uint32_t>(), Z.ct_nr.as<uint32_t>(),
                                        Z.ct_bc.as<uint64_t>(), Z.ct_stat.as<uint64_t>());
        }
        T(hipGetLastError());
        T(hipMemcpyAsync(h_stat, Z.ct_stat.p, 16, hipMemcpyDeviceToHost, s));
        T(hipStreamSynchronize(s));
        harvest_timers(c);
        if (!T.ok()) return T.fail(c, who, " (" + std::to_string(n) + " bytes, room for " + std::to_string(cap) + " chunks)");
        if (h_stat[1] != kChunkTableOk || h_stat[0] <= cap) break;
        cap = h_stat[0];
    }
    hc.lap("chunk table: hop");
    switch (h_stat[1]) {   // the host hop's sentences (afq_quantify)
        case kChunkTableOk: break;
        case kChunkTableTrailing: return fail(c, AFQ_ERR_BAD_INPUT, "trailing bytes after the last chunk");
        case kChunkTableCorrupt: return fail(c, AFQ_ERR_BAD_INPUT, "corrupt chunk header");
        case kChunkTableNoRecord: return fail(c, AFQ_ERR_BAD_INPUT, "chunk " + std::to_string(h_stat[0]) + " holds no record");
        default: return fail(c, AFQ_ERR_HIP, std::string(who) + ": unknown status " + std::to_string(h_stat[1]));
    }
    const uint64_t nc = h_stat[0];
    if (nc > cap) return fail(c, AFQ_ERR_HIP, std::string(who) + ": " + std::to_string(nc) + " chunks on the second hop, " + std::to_string(cap) + " on the first");
    uint64_t* o_off = (uint64_t*)std::malloc(std::max<uint64_t>(1, nc) * 8);
    uint32_t* o_nb = (uint32_t*)std::malloc(std::max<uint64_t>(1, nc) * 4);
    uint32_t* o_nr = (uint32_t*)std::malloc(std::max<uint64_t>(1, nc) * 4);
    uint64_t* o_bc = (uint64_t*)std::malloc(std::max<uint64_t>(1, nc) * 8);
    auto drop = [&] { std::free(o_off); std::free(o_nb); std::free(o_nr); std::free(o_bc); };
    if (!o_off || !o_nb || !o_nr || !o_bc) { drop(); return fail(c, AFQ_ERR_OOM, std::string(who) + ": host allocation failed (" + std::to_string(nc) + " chunks)"); }
    if (nc) {
        HipLatch T;
        T(hipMemcpyAsync(o_off, Z.ct_off.p, nc * 8, hipMemcpyDeviceToHost, s)); T(hipMemcpyAsync(o_nb, Z.ct_nb.p, nc * 4, hipMemcpyDeviceToHost, s));
        T(hipMemcpyAsync(o_nr, Z.ct_nr.p, nc * 4, hipMemcpyDeviceToHost, s)); T(hipMemcpyAsync(o_bc, Z.ct_bc.p, nc * 8, hipMemcpyDeviceToHost, s));
        T(hipStreamSynchronize(s));
        if (!T.ok()) { drop(); return T.fail(c, who, " (" + std::to_string(nc) + " chunks)"); }
    }
    hc.lap("chunk table: D2H");
    *out_off = o_off; *out_nbytes = o_nb; *out_nrec = o_nr; *out_first_bc = o_bc; *out_n_chunks = nc;
    return 0;
}

void afq_set_collate_compress(afq_ctx* c, int on) {
    if (c) c->collate_compress = on != 0;
}

// Both collates' placement: stable LSD passes over the bytes of the cell word that n_cells (the dropped records' word) occupies.
// The sorted words end in `src`; `dst` is the buffer the last pass read, free again.
static void collate_radix_place(hipStream_t s, uint64_t*& src, uint64_t*& dst, uint32_t n, uint32_t n_cells, uint32_t* hist) {
    for (uint32_t shift = 32; shift < 64 && (n_cells >> (shift - 32)) != 0; shift += 8) {
        launch_collate_radix_pass(s, src, dst, n, shift, hist);
        std::swap(src, dst);
    }
}

// What afq_collate_rad and afq_collate_multi_rad share from the chunk table to the return: collate_plan in front of the entry's
// uploads, collate_finish behind its measure launch.  The entry fills the first block, the plain data the two differ in, and keeps
// what is its own: the index step, the uploads (the sample table's sit among the cell table's, and the order of the stream's
// operations is the entry's), the args struct, the table and measure launches in their brackets, and the sum of its chunk_stat words.
namespace {
struct CollateRun {
    RadPass P;                                         // the entry's name, the chunk table, the latch (", N cells" behind the records)
    int k_sort, k_scan, k_write;                       // timer ids: placement, length scan + heads, write walk
    const char* lap_measure; const char* lap_write;    // HostClock labels
    uint32_t head_bytes;                               // a record without alignments
    uint64_t extra_tab_bytes;                          // device bytes of tables beside the cell table, the correction entries and the cells
    // collate_plan's
    uint64_t cap = 0, need_out = 0;
    uint32_t n = 0, n_cells = 0;
};
struct CollateDown { DevBuf &status, &out, &off, &nrec; DevBuf* ocell; };   // collate_copy_down's device side
}  // namespace

// The chunk table, the sizes, the fit check and the buffers both entries use (R.P.T holds the first failure of an `ensure`: the
// pass's stage looks at it behind the entry's own).
static int collate_plan(afq_ctx* c, CollateRun& R, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, bool on_device, uint64_t n_corr,
                        uint32_t n_cells) {
    RadPass& P = R.P;
    if (int rc = P.open(c, bytes, n_bytes, chunk_off, n_chunks, on_device, R.head_bytes, 32)) return rc;
    R.n = (uint32_t)P.n_slots; R.n_cells = n_cells;
    R.cap = sort_table_capacity(n_corr);
    const uint64_t s1 = std::max<uint64_t>(P.n_slots, 1), nc1 = std::max<uint32_t>(n_chunks, 1), ncell1 = (uint64_t)n_cells + 1, ncorr1 = std::max<uint64_t>(n_corr, 1), cap = R.cap;
    const uint64_t n_rblocks = (s1 + kCollateRadixBlock - 1) / kCollateRadixBlock, n_sblocks = (s1 + kCollateScanBlock - 1) / kCollateScanBlock;
    // does it fit?  (input + staging, the output - never longer than the input's records + the cells' headers -, 32 bytes a record
    // of slots, sort words and offsets, the digit counts, the tables)
    R.need_out = (uint64_t)n_bytes + 8 * ncell1;
    const uint64_t need_rec = s1 * 32 + 8 + n_rblocks * 1024 + n_sblocks * 8, need_tab = cap * 12 + n_corr * 12 + R.extra_tab_bytes + ncell1 * 20,
                   need_misc = nc1 * (sizeof(SortChunk) + 32);
    const uint64_t need_sz = c->collate_compress ? snappy_device_need(R.need_out) : 0;   // (the encoder's slots, tables and stream beside the output)
    if (int rc = P.fits(c, RadNeed{need_rec, need_tab + need_misc, "of tables", true, R.need_out, need_sz})) return rc;
    auto& B = c->collate;
    HipLatch& T = P.T;
    T(B.chunks.ensure(sizeof(SortChunk) * nc1)); T(B.obs.ensure(8 * ncorr1)); T(B.val.ensure(4 * ncorr1)); T(B.tkey.ensure(8 * cap)); T(B.tval.ensure(4 * cap));
    T(B.cells.ensure(8 * ncell1)); T(B.rec.ensure(8 * s1)); T(B.ka.ensure(8 * s1)); T(B.kb.ensure(8 * s1)); T(B.hist.ensure(1024 * n_rblocks)); T(B.bsum.ensure(8 * n_sblocks));
    T(B.ex.ensure(8 * (s1 + 1))); T(B.cstat.ensure(32ull * nc1)); T(B.status.ensure(sizeof(DevStatus))); T(B.off.ensure(8 * ncell1)); T(B.nrec.ensure(4 * ncell1));
    return 0;
}

// The three collates' copy down, behind the write walk: out_total bytes in n_out chunks - the cells of the RNA collates, the
// non-empty ones of `atac collate`, which hands out the chunks' cells in a column of their own (D.ocell, out_cell).  The host
// blocks (no chunk bytes under collate_compress), the write's status and the arrays down, the closing checks, the snappy encoder.
// cell_text(cell) words a cell for the 4 GiB-chunk refusal.
static int collate_copy_down(afq_ctx* c, RadPass& P, HostClock& hc, const char* lap, CollateDown D, uint64_t out_total, uint32_t n_out,
                             const std::function<std::string(uint32_t)>& cell_text, uint8_t** out_bytes, uint64_t* out_n_bytes, uint64_t** out_chunk_off, uint32_t** out_nrec,
                             uint32_t** out_cell = nullptr) {
    HipLatch& T = P.T;
    hipStream_t s = c->stream;
    const std::string who = P.who;
    const uint64_t o1 = std::max<uint64_t>(out_total, 1), nout1 = (uint64_t)n_out + 1;
    T(hipGetLastError());
    HostOuts H;
    const bool sz = c->collate_compress;   // the chunk bytes go down as a snappy frame stream, encoded behind the checks below
    uint8_t* ob = sz ? nullptr : (uint8_t*)H.mallocd(o1);
    uint64_t* ooff = (uint64_t*)H.mallocd(8 * nout1);
    uint32_t* onrec = (uint32_t*)H.mallocd(4 * nout1);
    uint32_t* ocell = D.ocell ? (uint32_t*)H.mallocd(4 * nout1) : nullptr;
    if ((!sz && !ob) || !ooff || !onrec || (D.ocell && !ocell)) {
        (void)hipStreamSynchronize(s); harvest_timers(c);
        return fail(c, AFQ_ERR_OOM, who + ": host allocation failed (" + std::to_string(o1 + (D.ocell ? 16 : 12) * nout1) + " bytes of output)");
    }
    DevStatus st{};
    T(hipMemcpyAsync(&st, D.status.p, sizeof(st), hipMemcpyDeviceToHost, s));
    if (out_total && !sz) T(hipMemcpyAsync(ob, D.out.p, out_total, hipMemcpyDeviceToHost, s));
    T(hipMemcpyAsync(ooff, D.off.p, 8 * nout1, hipMemcpyDeviceToHost, s));
    if (n_out) T(hipMemcpyAsync(onrec, D.nrec.p, 4ull * n_out, hipMemcpyDeviceToHost, s));
    if (n_out && D.ocell) T(hipMemcpyAsync(ocell, D.ocell->p, 4ull * n_out, hipMemcpyDeviceToHost, s));
    T(hipStreamSynchronize(s));   // (before any exit below: the copies write into H's blocks)
    harvest_timers(c);
    hc.lap(lap);
    if (!T.ok()) return P.hip_fail(c);
    if (st.err_code == kErrCollateChunk)
        return fail(c, AFQ_ERR_UNSUPPORTED, who + ": cell " + std::to_string(st.err_cell) + " (" + cell_text(st.err_cell) + "): an output chunk of 4 GiB or more");
    if (st.err_code) return fail(c, AFQ_ERR_HIP, who + ": device status " + std::to_string(st.err_code) + " in the write");
    if (ooff[n_out] != out_total) return fail(c, AFQ_ERR_HIP, who + ": the chunks end at " + std::to_string(ooff[n_out]) + " of " + std::to_string(out_total) + " output bytes");
    uint64_t out_n = out_total;
    if (sz) {
        if (int rc = snappy_encode_device(c, P.who, D.out.as<uint8_t>(), out_total, &ob, &out_n, nullptr)) return rc;
        hc.lap("snappy encode + D2H");
    }
    H.release();
    *out_bytes = ob; *out_n_bytes = out_n; *out_chunk_off = ooff; *out_nrec = onrec;
    if (out_cell) *out_cell = ocell;
    return 0;
}

// Behind the entry's measure launch: status and chunk_stat readback (R.P.cstat: [n_chunks][8], the entry's to sum), radix placement,
// length scan, chunk heads, the entry's write walk (launch_write(dest, out)), the copy down.
static int collate_finish(afq_ctx* c, CollateRun& R, HostClock& hc, const std::function<void(const uint64_t*, uint8_t*)>& launch_write,
                          const std::function<std::string(uint32_t)>& cell_text, uint8_t** out_bytes, uint64_t* out_n_bytes, uint64_t** out_chunk_off, uint32_t** out_nrec) {
    auto& B = c->collate;
    RadPass& P = R.P;
    HipLatch& T = P.T;
    hipStream_t s = c->stream;
    const std::string who = P.who;
    const uint32_t n = R.n, n_cells = R.n_cells;
    if (int rc = P.read_back(c, hc, B.status, B.cstat, 8, R.lap_measure)) return rc;
    // ---- placement: stable LSD passes over the bytes of the cell word that n_cells (the dropped records' word) occupies
    uint64_t* src = B.ka.as<uint64_t>();
    uint64_t* dst = B.kb.as<uint64_t>();
    {
        ScopedTimer t(c, R.k_sort, s);
        collate_radix_place(s, src, dst, n, n_cells, B.hist.as<uint32_t>());
    }
    uint64_t kept_bytes = 0;
    {
        ScopedTimer t(c, R.k_scan, s);
        launch_collate_scan(s, src, B.rec.as<uint2>(), n, B.bsum.as<uint64_t>(), B.ex.as<uint64_t>(), dst);   // (dst: the buffer the last pass read is free)
    }
    T(hipGetLastError());
    T(hipMemcpyAsync(&kept_bytes, B.ex.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s));
    T(hipStreamSynchronize(s));
    if (!T.ok()) return P.hip_fail(c);
    const uint64_t out_total = 8ull * n_cells + kept_bytes, o1 = std::max<uint64_t>(out_total, 1);
    if (out_total > R.need_out) { harvest_timers(c); return fail(c, AFQ_ERR_HIP, who + ": " + std::to_string(out_total) + " bytes of output from " + std::to_string(P.n_bytes) + " of input"); }
    T(B.out.ensure(o1));
    if (!T.ok()) return P.hip_fail(c);
    {
        ScopedTimer t(c, R.k_scan, s);
        launch_collate_heads(s, src, n, B.ex.as<uint64_t>(), n_cells, B.off.as<uint64_t>(), B.nrec.as<uint32_t>(), B.out.as<uint8_t>(), B.status.as<DevStatus>());
    }
    {
        ScopedTimer t(c, R.k_write, s);
        launch_write(dst, B.out.as<uint8_t>());
    }
    return collate_copy_down(c, P, hc, R.lap_write, CollateDown{B.status, B.out, B.off, B.nrec, nullptr}, out_total, n_cells, cell_text, out_bytes, out_n_bytes, out_chunk_off,
                             out_nrec);
}

// `collate` on the device (afq_collate.hip): correction table, measure walk, radix placement, length scan, chunk heads, write walk.
void afq_collate_limits(uint32_t out[4]) {
    if (!out) return;
    out[0] = kGplParseTile; out[1] = kGplParseHalo; out[2] = kGplLaneAlns; out[3] = kCollateRadixBlock;
}

int afq_collate_rad(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t bc_bytes, uint32_t umi_bytes,
                    uint32_t expected_ori, int bytes_on_device, const uint64_t* observed, const uint64_t* corrected, uint64_t n_corr, const uint64_t* cells,
                    uint64_t n_cells64, uint8_t** out_bytes, uint64_t* out_n_bytes, uint64_t** out_chunk_off, uint32_t** out_nrec, afq_collate_stats* stats) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!bytes && n_bytes) || (!chunk_off && n_chunks) || ((!observed || !corrected) && n_corr) || (!cells && n_cells64) || !out_bytes || !out_n_bytes ||
        !out_chunk_off || !out_nrec)
        return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    if (!valid_width(bc_bytes)) return fail(c, AFQ_ERR_INVALID_ARG, "bc_bytes must be 1, 2, 4 or 8");
    if (!valid_width(umi_bytes)) return fail(c, AFQ_ERR_INVALID_ARG, "umi_bytes must be 1, 2, 4 or 8");
    if (expected_ori > kGplOriRc) return fail(c, AFQ_ERR_INVALID_ARG, "expected_ori must be 0 (both), 1 (fw) or 2 (rc)");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    if (n_corr >= (1ull << 30)) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_collate_rad: 2^30 or more correction entries");
    if (n_cells64 > 0xFFFFFFFEull) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_collate_rad: more than 2^32 - 2 cells (" + std::to_string(n_cells64) + ")");
    const uint32_t n_cells = (uint32_t)n_cells64;
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    hipStream_t s = c->stream;
    // ---- host: corrected barcode -> its index in `cells`; the all-ones key
    std::vector<uint32_t> val;
    uint32_t ones_cell = kSortNoRank;
    if (int rc = collate_cell_index(c, observed, corrected, n_corr, cells, n_cells, val, ones_cell)) return rc;
    // ---- chunk table, sizes, fit check, buffers
    CollateRun R{{"afq_collate_rad", ", " + std::to_string(n_cells) + " cells"}, K_COLLATE_SORT, K_COLLATE_SCAN, K_COLLATE_WRITE, "collate: table + measure", "collate: place + write + D2H", 4 + bc_bytes + umi_bytes, 0};
    if (int rc = collate_plan(c, R, bytes, n_bytes, chunk_off, n_chunks, bytes_on_device != 0, n_corr, n_cells)) return rc;
    const uint64_t cap = R.cap;
    const uint32_t tab_mask = (uint32_t)(cap - 1);
    auto& B = c->collate;
    RadPass& P = R.P;
    HipLatch& T = P.T;
    if (int rc = P.stage(c, B.chunks)) return rc;
    if (n_corr) { T(hipMemcpyAsync(B.obs.p, observed, 8 * n_corr, hipMemcpyHostToDevice, s)); T(hipMemcpyAsync(B.val.p, val.data(), 4 * n_corr, hipMemcpyHostToDevice, s)); }
    if (n_cells) T(hipMemcpyAsync(B.cells.p, cells, 8ull * n_cells, hipMemcpyHostToDevice, s));
    T(hipMemsetAsync(B.tkey.p, 0xFF, 8 * cap, s));
    T(hipMemsetAsync(B.status.p, 0, sizeof(DevStatus), s));
    T(hipMemsetAsync(B.ex.p, 0, 8, s));   // (ex[0]; with no record at all it is also ex[n])
    if (!T.ok()) return P.hip_fail(c);
    reset_kernel_times(c);
    CollateArgs a{P.d_bytes, (uint64_t)n_bytes, B.chunks.as<SortChunk>(), n_chunks, bc_bytes, umi_bytes, c->aln_extra, expected_ori, B.tkey.as<uint64_t>(),
                  B.tval.as<uint32_t>(), tab_mask, ones_cell, n_cells, B.rec.as<uint2>(), B.ka.as<uint64_t>(), B.cstat.as<uint32_t>(), B.cells.as<uint64_t>(),
                  nullptr, nullptr, B.status.as<DevStatus>()};
    {
        ScopedTimer t(c, K_COLLATE_TABLE, s);
        launch_sort_table(s, B.obs.as<uint64_t>(), B.val.as<uint32_t>(), n_corr, B.tkey.as<uint64_t>(), B.tval.as<uint32_t>(), tab_mask, B.status.as<DevStatus>());
    }
    {
        ScopedTimer t(c, K_COLLATE_MEASURE, s);
        launch_collate_measure(s, a);
    }
    if (int rc = collate_finish(c, R, hc, [&](const uint64_t* dest, uint8_t* out) { a.dest = dest; a.out = out; launch_collate_write(s, a); },
                                [&](uint32_t cell) { return "barcode " + std::to_string(cells[cell]); }, out_bytes, out_n_bytes, out_chunk_off, out_nrec))
        return rc;
    afq_collate_stats S{};
    for (uint32_t i = 0; i < n_chunks; ++i) {
        const uint32_t* q = P.cstat.data() + 8ull * i;
        S.n_records += q[0]; S.n_compatible += q[1]; S.n_uncorrected += q[2]; S.n_kept += q[3]; S.n_alignments_in += q[4]; S.n_alignments_kept += q[5]; S.n_long_records += q[6];
    }
    S.out_bytes = (*out_chunk_off)[n_cells];   // (uncompressed, also under afq_set_collate_compress)
    if (stats) *stats = S;
    return 0;
}

// multi-barcode `collate` on the device (k_collate_walk over CollateMultiArgs, afq_collate.hip): sample table, cell table, measure
// walk, then collate's radix placement, length scan and chunk heads, write walk.
void afq_collate_multi_limits(uint32_t out[4]) { afq_collate_limits(out); }   // (one walk: one set of limits)

int afq_collate_multi_rad(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t b0_bytes, uint32_t b1_bytes,
                          uint32_t umi_bytes, uint32_t expected_ori, int bytes_on_device, const uint64_t* sample_observed, const uint32_t* sample_index,
                          uint64_t n_sample_entries, const uint32_t* corr_sample, const uint64_t* corr_observed, const uint64_t* corr_corrected, uint64_t n_corr,
                          const uint32_t* cell_sample, const uint64_t* cell_bc, uint64_t n_cells64, const uint32_t* sample_b0_out, uint64_t n_samples,
                          uint8_t** out_bytes, uint64_t* out_n_bytes, uint64_t** out_chunk_off, uint32_t** out_nrec, afq_collate_multi_stats* stats) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!bytes && n_bytes) || (!chunk_off && n_chunks) || !out_bytes || !out_n_bytes || !out_chunk_off || !out_nrec) return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    // ---- host: widths, orientation, the three inputs; (sample, corrected barcode) -> its index among the cells (afq_gpl_host.h: the CPU suite runs this without a device)
    std::vector<uint32_t> val;
    {
        std::string e;
        if (int rc = gplhost::collate_multi_index(b0_bytes, b1_bytes, umi_bytes, expected_ori, sample_observed, sample_index, n_sample_entries, corr_sample, corr_observed,
                                                  corr_corrected, n_corr, cell_sample, cell_bc, n_cells64, sample_b0_out, n_samples, val, e))
            return fail(c, rc, e);
    }
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    const uint32_t n_cells = (uint32_t)n_cells64;
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    hipStream_t s = c->stream;
    std::vector<uint64_t> ckey(n_corr), chead(n_cells);
    for (uint64_t i = 0; i < n_corr; ++i) ckey[i] = (uint64_t)corr_sample[i] << 32 | corr_observed[i];
    for (uint32_t j = 0; j < n_cells; ++j) chead[j] = (uint64_t)sample_b0_out[cell_sample[j]] << 32 | cell_bc[j];
    // ---- chunk table, sizes, fit check, buffers (afq_collate_rad's, with the sample entries and their table beside the cell table)
    const uint64_t scap = sort_table_capacity(n_sample_entries), nse1 = std::max<uint64_t>(n_sample_entries, 1);
    CollateRun R{{"afq_collate_multi_rad", ", " + std::to_string(n_cells) + " cells"}, K_COLLATEM_SORT, K_COLLATEM_SCAN, K_COLLATEM_WRITE, "collate multi: tables + measure", "collate multi: place + write + D2H",
                 4 + b0_bytes + b1_bytes + umi_bytes, scap * 12 + n_sample_entries * 12};
    if (int rc = collate_plan(c, R, bytes, n_bytes, chunk_off, n_chunks, bytes_on_device != 0, n_corr, n_cells)) return rc;
    const uint64_t cap = R.cap;
    const uint32_t tab_mask = (uint32_t)(cap - 1), stab_mask = (uint32_t)(scap - 1);
    auto& B = c->collate;
    RadPass& P = R.P;
    HipLatch& T = P.T;
    T(B.sobs.ensure(8 * nse1)); T(B.sidx.ensure(4 * nse1)); T(B.skey.ensure(8 * scap)); T(B.sval.ensure(4 * scap));
    if (int rc = P.stage(c, B.chunks)) return rc;
    if (n_corr) { T(hipMemcpyAsync(B.obs.p, ckey.data(), 8 * n_corr, hipMemcpyHostToDevice, s)); T(hipMemcpyAsync(B.val.p, val.data(), 4 * n_corr, hipMemcpyHostToDevice, s)); }
    if (n_sample_entries) {
        T(hipMemcpyAsync(B.sobs.p, sample_observed, 8 * n_sample_entries, hipMemcpyHostToDevice, s));
        T(hipMemcpyAsync(B.sidx.p, sample_index, 4 * n_sample_entries, hipMemcpyHostToDevice, s));
    }
    if (n_cells) T(hipMemcpyAsync(B.cells.p, chead.data(), 8ull * n_cells, hipMemcpyHostToDevice, s));
    T(hipMemsetAsync(B.tkey.p, 0xFF, 8 * cap, s));
    T(hipMemsetAsync(B.skey.p, 0xFF, 8 * scap, s));
    T(hipMemsetAsync(B.status.p, 0, sizeof(DevStatus), s));
    T(hipMemsetAsync(B.ex.p, 0, 8, s));   // (ex[0]; with no record at all it is also ex[n])
    if (!T.ok()) return P.hip_fail(c);
    reset_kernel_times(c);
    CollateMultiArgs a{P.d_bytes, (uint64_t)n_bytes, B.chunks.as<SortChunk>(), n_chunks, b0_bytes, b1_bytes, umi_bytes, c->aln_extra, expected_ori,
                       B.skey.as<uint64_t>(), B.sval.as<uint32_t>(), stab_mask, B.tkey.as<uint64_t>(), B.tval.as<uint32_t>(), tab_mask, n_cells,
                       B.rec.as<uint2>(), B.ka.as<uint64_t>(), B.cstat.as<uint32_t>(), B.cells.as<uint64_t>(), nullptr, nullptr, B.status.as<DevStatus>()};
    {
        ScopedTimer t(c, K_COLLATEM_TABLE, s);
        launch_sort_table(s, B.sobs.as<uint64_t>(), B.sidx.as<uint32_t>(), n_sample_entries, B.skey.as<uint64_t>(), B.sval.as<uint32_t>(), stab_mask, B.status.as<DevStatus>());
        launch_sort_table(s, B.obs.as<uint64_t>(), B.val.as<uint32_t>(), n_corr, B.tkey.as<uint64_t>(), B.tval.as<uint32_t>(), tab_mask, B.status.as<DevStatus>());
    }
    {
        ScopedTimer t(c, K_COLLATEM_MEASURE, s);
        launch_collate_multi_measure(s, a);
    }
    if (int rc = collate_finish(c, R, hc, [&](const uint64_t* dest, uint8_t* out) { a.dest = dest; a.out = out; launch_collate_multi_write(s, a); },
                                [&](uint32_t cell) { return "sample " + std::to_string(cell_sample[cell]) + ", barcode " + std::to_string(cell_bc[cell]); }, out_bytes,
                                out_n_bytes, out_chunk_off, out_nrec))
        return rc;
    afq_collate_multi_stats S{};
    for (uint32_t i = 0; i < n_chunks; ++i) {
        const uint32_t* q = P.cstat.data() + 8ull * i;
        S.n_records += q[0]; S.n_compatible += q[1]; S.n_unrouted += q[2]; S.n_uncorrected += q[3]; S.n_kept += q[4]; S.n_alignments_in += q[5]; S.n_alignments_kept += q[6];
        S.n_long_records += q[7];
    }
    S.out_bytes = (*out_chunk_off)[n_cells];   // (uncompressed, also under afq_set_collate_compress)
    if (stats) *stats = S;
    return 0;
}

// `atac collate` on the device (afq_atac_collate.hip): correction table, measure walk, radix placement, cell runs + their scan, chunk
// heads, write walk.
void afq_atac_collate_limits(uint32_t out[4]) {
    if (!out) return;
    out[0] = kSortParseTile; out[1] = kSortParseHalo; out[2] = 11; out[3] = kCollateRadixBlock;
}

int afq_atac_collate_rad(afq_ctx* c, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off, uint32_t n_chunks, uint32_t bc_bytes, int bytes_on_device,
                         const uint64_t* observed, const uint64_t* corrected, uint64_t n_corr, const uint64_t* cells, uint64_t n_cells64, uint8_t** out_bytes,
                         uint64_t* out_n_bytes, uint64_t* out_n_chunks, uint64_t** out_chunk_off, uint32_t** out_nrec, uint32_t** out_cell,
                         afq_atac_collate_stats* stats) {
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!bytes && n_bytes) || (!chunk_off && n_chunks) || ((!observed || !corrected) && n_corr) || (!cells && n_cells64) || !out_bytes || !out_n_bytes ||
        !out_n_chunks || !out_chunk_off || !out_nrec || !out_cell)
        return fail(c, AFQ_ERR_INVALID_ARG, "null argument");
    if (!valid_width(bc_bytes)) return fail(c, AFQ_ERR_INVALID_ARG, "bc_bytes must be 1, 2, 4 or 8");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    if (n_corr >= (1ull << 30)) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_atac_collate_rad: 2^30 or more correction entries");
    if (n_cells64 > 0xFFFFFFFEull) return fail(c, AFQ_ERR_UNSUPPORTED, "afq_atac_collate_rad: more than 2^32 - 2 cells (" + std::to_string(n_cells64) + ")");
    const uint32_t n_cells = (uint32_t)n_cells64;
    const uint32_t R = 4 + bc_bytes + 11;
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    hipStream_t s = c->stream;
    // ---- host: corrected barcode -> its index in `cells`; the all-ones key
    std::vector<uint32_t> val;
    uint32_t ones_cell = kSortNoRank;
    if (int rc = collate_cell_index(c, observed, corrected, n_corr, cells, n_cells, val, ones_cell)) return rc;
    // ---- chunk table
    RadPass P{"afq_atac_collate_rad", ", " + std::to_string(n_cells) + " cells"};
    if (int rc = P.open(c, bytes, n_bytes, chunk_off, n_chunks, bytes_on_device != 0, 4 + bc_bytes, 32)) return rc;
    const uint64_t n_slots = P.n_slots;
    const uint32_t n = (uint32_t)n_slots;
    const uint64_t cap = sort_table_capacity(n_corr);
    const uint32_t tab_mask = (uint32_t)(cap - 1);
    const uint64_t s1 = std::max<uint64_t>(n_slots, 1), nc1 = std::max<uint32_t>(n_chunks, 1), ncell1 = (uint64_t)n_cells + 1, ncorr1 = std::max<uint64_t>(n_corr, 1);
    const uint64_t n_rblocks = (s1 + kCollateRadixBlock - 1) / kCollateRadixBlock;
    const uint64_t max_out = std::min<uint64_t>(n_cells, n_slots);   // chunks the output can have
    // does it fit?  (input + staging, the output - a kept record is never longer than it was, + the heads -, 20 bytes a record of
    // cells and sort words + the destination that reuses a sort buffer, the digit counts, the tables)
    const uint64_t need_out = (uint64_t)n_bytes + 8 * max_out + 8, need_rec = s1 * 20 + n_rblocks * 1024, need_tab = cap * 12 + n_corr * 12 + ncell1 * 16 + (max_out + 1) * 16,
                   need_misc = nc1 * (sizeof(SortChunk) + 32);
    const uint64_t need_sz = c->collate_compress ? snappy_device_need(need_out) : 0;   // (the encoder's slots, tables and stream beside the output)
    if (int rc = P.fits(c, RadNeed{need_rec, need_tab + need_misc, "of tables", true, need_out, need_sz})) return rc;
    auto& B = c->acollate;
    HipLatch& T = P.T;
    T(B.chunks.ensure(sizeof(SortChunk) * nc1)); T(B.obs.ensure(8 * ncorr1)); T(B.val.ensure(4 * ncorr1)); T(B.tkey.ensure(8 * cap)); T(B.tval.ensure(4 * cap));
    T(B.cells.ensure(8 * ncell1)); T(B.cellof.ensure(4 * s1)); T(B.ka.ensure(8 * s1)); T(B.kb.ensure(8 * s1)); T(B.hist.ensure(1024 * n_rblocks));
    T(B.first.ensure(4 * ncell1)); T(B.rank.ensure(4 * ncell1)); T(B.cstat.ensure(32ull * nc1)); T(B.status.ensure(sizeof(DevStatus)));
    if (int rc = P.stage(c, B.chunks)) return rc;
    if (n_corr) { T(hipMemcpyAsync(B.obs.p, observed, 8 * n_corr, hipMemcpyHostToDevice, s)); T(hipMemcpyAsync(B.val.p, val.data(), 4 * n_corr, hipMemcpyHostToDevice, s)); }
    if (n_cells) T(hipMemcpyAsync(B.cells.p, cells, 8ull * n_cells, hipMemcpyHostToDevice, s));
    T(hipMemsetAsync(B.tkey.p, 0xFF, 8 * cap, s));
    T(hipMemsetAsync(B.status.p, 0, sizeof(DevStatus), s));
    if (!T.ok()) return P.hip_fail(c);
    reset_kernel_times(c);
    AtacCollateArgs a{P.d_bytes, (uint64_t)n_bytes, B.chunks.as<SortChunk>(), n_chunks, bc_bytes, B.tkey.as<uint64_t>(), B.tval.as<uint32_t>(), tab_mask, ones_cell,
                      n_cells, B.cellof.as<uint32_t>(), B.ka.as<uint64_t>(), B.cstat.as<uint32_t>(), B.cells.as<uint64_t>(), nullptr, nullptr, B.status.as<DevStatus>()};
    {
        ScopedTimer t(c, K_ACOLLATE_TABLE, s);
        launch_sort_table(s, B.obs.as<uint64_t>(), B.val.as<uint32_t>(), n_corr, B.tkey.as<uint64_t>(), B.tval.as<uint32_t>(), tab_mask, B.status.as<DevStatus>());
    }
    {
        ScopedTimer t(c, K_ACOLLATE_MEASURE, s);
        launch_atac_collate_measure(s, a);
    }
    if (int rc = P.read_back(c, hc, B.status, B.cstat, 8, "atac collate: table + measure")) return rc;
    afq_atac_collate_stats S{};
    for (uint32_t i = 0; i < n_chunks; ++i) {
        const uint32_t* q = P.cstat.data() + 8ull * i;
        S.n_records += q[0]; S.n_unmapped += q[1]; S.n_multimapped += q[2]; S.n_uncorrected += q[3]; S.n_kept += q[4];
    }
    // ---- placement: stable LSD passes over the bytes of the cell word that n_cells (the dropped records' word) occupies, then the
    // cells' runs and the scan that numbers the non-empty ones
    uint64_t* src = B.ka.as<uint64_t>();
    uint64_t* dst = B.kb.as<uint64_t>();
    {
        ScopedTimer t(c, K_ACOLLATE_PLACE, s);
        collate_radix_place(s, src, dst, n, n_cells, B.hist.as<uint32_t>());
        launch_atac_collate_runs(s, src, n, n_cells, B.first.as<uint32_t>(), B.rank.as<uint32_t>());
        launch_collate_excl_scan_u32(s, B.rank.as<uint32_t>(), ncell1);
    }
    T(hipGetLastError());
    uint32_t n_out = 0, n_kept_dev = 0;
    T(hipMemcpyAsync(&n_out, B.rank.as<uint32_t>() + n_cells, 4, hipMemcpyDeviceToHost, s));
    T(hipMemcpyAsync(&n_kept_dev, B.first.as<uint32_t>() + n_cells, 4, hipMemcpyDeviceToHost, s));
    T(hipStreamSynchronize(s));
    if (!T.ok()) return P.hip_fail(c);
    if (n_kept_dev != S.n_kept || n_out > max_out || (n_out == 0) != (S.n_kept == 0)) {   // (the write's bounds rest on these)
        harvest_timers(c);
        return fail(c, AFQ_ERR_HIP, "afq_atac_collate_rad: the placement holds " + std::to_string(n_kept_dev) + " records in " + std::to_string(n_out) + " cells, the measure kept " +
                    std::to_string(S.n_kept));
    }
    const uint64_t out_total = (uint64_t)R * S.n_kept + 8ull * n_out, nout1 = (uint64_t)n_out + 1;
    T(B.out.ensure(std::max<uint64_t>(out_total, 1))); T(B.off.ensure(8 * nout1)); T(B.nrec.ensure(4 * nout1)); T(B.ocell.ensure(4 * nout1));
    if (!T.ok()) return P.hip_fail(c);
    a.dest = dst; a.out = B.out.as<uint8_t>();   // (dst: the buffer the last pass read is free)
    {
        ScopedTimer t(c, K_ACOLLATE_PLACE, s);
        launch_atac_collate_heads(s, src, n, n_cells, R, B.first.as<uint32_t>(), B.rank.as<uint32_t>(), B.off.as<uint64_t>(), B.nrec.as<uint32_t>(), B.ocell.as<uint32_t>(),
                                  dst, a.out, B.status.as<DevStatus>());
    }
    {
        ScopedTimer t(c, K_ACOLLATE_WRITE, s);
        if (S.n_kept) launch_atac_collate_write(s, a);
    }
    if (int rc = collate_copy_down(c, P, hc, "atac collate: place + write + D2H", CollateDown{B.status, B.out, B.off, B.nrec, &B.ocell}, out_total, n_out,
                                   [&](uint32_t cell) { return "barcode " + std::to_string(cells[cell]); }, out_bytes, out_n_bytes, out_chunk_off, out_nrec, out_cell))
        return rc;
    S.n_cells_out = n_out; S.n_cells_empty = (uint64_t)n_cells - n_out; S.out_bytes = out_total;
    if (stats) *stats = S;
    *out_n_chunks = n_out;
    return 0;
}
