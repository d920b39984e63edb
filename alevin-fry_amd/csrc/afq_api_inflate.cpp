// afq_api_inflate.cpp — the BGZF inflater's host side (afq_inflate.hip): the plan, the pieces, the refusals' sentences.
#include "afq_bgzf_plan.h"
#include "afq_ctx.h"
#include "afq_inflate_elem.h"

void afq_inflate_limits(uint32_t out[4]) {
    if (!out) return;
    out[0] = kInflateThreads; out[1] = kInflatePieceBlocks; out[2] = kInflateLds; out[3] = kInflateBlocksPerWg;
}

// The compressed bytes of a piece - at most kInflatePieceBlocks whole BGZF blocks, header and trailer with them - cross into one
// of two device buffers on c->stream while the launch of the piece in front reads the other on the second stream, as the pieces
// of afq_snappy_frame_decode_device do (a full piece of level-6 records is some 80 MB and goes through the pinned staging).
int afq_bgzf_inflate_device(afq_ctx* c, const uint8_t* file, size_t n, uint32_t shift, int out_on_device, uint8_t** out, uint64_t* out_n, afq_inflate_stats* stats) {
    static const char* who = "afq_bgzf_inflate_device";
    if (!c) return AFQ_ERR_INVALID_ARG;
    if ((!file && n) || !out || !out_n || shift > 15) return fail(c, AFQ_ERR_INVALID_ARG, !out || !out_n || (!file && n) ? "null argument" : "shift is 0..15");
    if (c->pending) return fail(c, AFQ_ERR_STATE, "a quant batch is pending on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HostClock hc;
    std::vector<BgzfBlock> blocks;
    uint64_t total = 0;
    {
        std::string err;
        if (!bgzf_plan(file, n, blocks, total, err)) return fail(c, AFQ_ERR_BAD_INPUT, err);
    }
    const uint64_t nb = blocks.size();
    if (nb >= (1ull << 31)) return fail(c, AFQ_ERR_UNSUPPORTED, std::string(who) + ": 2^31 or more BGZF blocks");
    // the pieces: [b0, b1) of the blocks, their payloads within bytes [lo, hi) of the file
    struct Piece { uint64_t b0, b1, lo, hi; };
    std::vector<Piece> pieces;
    std::vector<BgzfDecBlock> plan(nb);
    uint64_t piece_max = 0;
    for (uint64_t i = 0; i < nb;) {
        Piece P{i, i, blocks[i].data_off, blocks[i].data_off};
        while (P.b1 < nb && P.b1 - P.b0 < kInflatePieceBlocks) {
            const BgzfBlock& k = blocks[P.b1];
            plan[P.b1] = BgzfDecBlock{(uint64_t)k.data_off - P.lo, k.out_off, (uint32_t)k.data_len, k.isize, k.crc, 0u};
            P.hi = k.data_off + k.data_len;
            ++P.b1;
        }
        piece_max = std::max(piece_max, P.hi - P.lo);
        pieces.push_back(P);
        i = P.b1;
    }
    hc.lap("inflate: plan");
    constexpr uint64_t kStatWords = 9;   // the status word, the short block's word, then blocks, empty blocks, stored, fixed, dynamic, literals, copies
    const uint64_t n_buf = pieces.size() > 1 ? 2 : 1;
    const uint64_t need_in = n_buf * piece_max, need_plan = nb * sizeof(BgzfDecBlock) + 64, need_out = (uint64_t)shift + total + 16;
    auto& Z = c->inflate;
    {   // what the inflater has to allocate beyond what it holds from an earlier call, against what the device has free
        auto more = [](const DevBuf& b, uint64_t want) -> uint64_t { return want > b.cap ? want : 0; };
        uint64_t alloc = more(Z.plan, need_plan) + more(Z.out, need_out) + more(Z.stat, kStatWords * 8);
        for (uint64_t b = 0; b < n_buf && nb; ++b) alloc += more(Z.in[b], piece_max);
        size_t fr = 0, tot = 0;
        HIP_TRY(c, hipMemGetInfo(&fr, &tot));
        uint64_t room = fr;
        if (const long hook = test_hook_long("INFLATE_ROOM_BYTES", -1); hook >= 0) room = std::min<uint64_t>(room, (uint64_t)hook);
        if (alloc > room)
            return fail(c, AFQ_ERR_OOM, std::string(who) + ": the file does not fit the device: " + std::to_string(need_in) + " bytes of compressed pieces + " +
                        std::to_string(need_plan) + " of plan + " + std::to_string(kStatWords * 8) + " of status and tallies + " + std::to_string(need_out) +
                        " of inflated bytes, " + std::to_string(alloc) + " of them still to allocate > " + std::to_string(room) + " bytes free of " + std::to_string(tot) +
                        " of device memory");
    }
    const std::string detail = " (BGZF inflater, " + std::to_string(n) + " bytes in " + std::to_string(nb) + " blocks, " + std::to_string(total) + " inflated)";
    HipLatch T;
    T(Z.out.ensure(need_out)); T(Z.plan.ensure(need_plan)); T(Z.stat.ensure(kStatWords * 8));
    for (uint64_t b = 0; b < n_buf && nb; ++b) T(Z.in[b].ensure(piece_max));
    if (!T.ok()) return T.fail(c, who, detail);
    hipStream_t up = c->stream, ks = second_stream(c);
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr}, ev_plan = nullptr;
    for (int b = 0; b < 2; ++b) { T(hipEventCreateWithFlags(&ev_up[b], hipEventDisableTiming)); T(hipEventCreateWithFlags(&ev_done[b], hipEventDisableTiming)); }
    T(hipEventCreateWithFlags(&ev_plan, hipEventDisableTiming));
    auto drop_events = [&] {
        for (int b = 0; b < 2; ++b) { if (ev_up[b]) (void)hipEventDestroy(ev_up[b]); if (ev_done[b]) (void)hipEventDestroy(ev_done[b]); }
        if (ev_plan) (void)hipEventDestroy(ev_plan);
    };
    uint64_t h_stat[kStatWords] = {~0ull, ~0ull, 0, 0, 0, 0, 0, 0, 0};
    int rc = 0;
    if (T.ok()) {
        reset_kernel_times(c);
        T(hipMemcpyAsync(Z.stat.p, h_stat, sizeof h_stat, hipMemcpyHostToDevice, up));
        if (nb) T(hipMemcpyAsync(Z.plan.p, plan.data(), nb * sizeof(BgzfDecBlock), hipMemcpyHostToDevice, up));
        if (shift) T(hipMemsetAsync(Z.out.p, 0, 16, up));   // what stands around the inflated bytes is zero
        T(hipMemsetAsync(Z.out.as<uint8_t>() + shift + total, 0, 16, up));
        T(hipEventRecord(ev_plan, up));
        T(hipStreamWaitEvent(ks, ev_plan, 0));
        uint8_t* d_dst = Z.out.as<uint8_t>() + shift;
        for (size_t k = 0; k < pieces.size() && T.ok() && !rc; ++k) {
            const Piece& P = pieces[k];
            const int b = (int)(k & 1);
            if (k >= 2) T(hipStreamWaitEvent(up, ev_done[b], 0));   // the launch that read this buffer last
            const uint8_t* src = file + P.lo;
            const size_t len = (size_t)(P.hi - P.lo);
            if (len) rc = staged_h2d(c, Z.in[b].as<uint8_t>(), src, len, up, host_ptr_is_pinned(src) && host_ptr_is_pinned(src + len - 1));
            if (rc) break;
            T(hipEventRecord(ev_up[b], up));
            T(hipStreamWaitEvent(ks, ev_up[b], 0));
            {
                ScopedTimer t(c, K_BGZF_INFLATE, ks);
                launch_bgzf_inflate(ks, Z.in[b].as<uint8_t>(), Z.plan.as<BgzfDecBlock>() + P.b0, (uint32_t)(P.b1 - P.b0), P.b0, d_dst, Z.stat.as<uint64_t>(), Z.stat.as<uint64_t>() + 2);
            }
            T(hipGetLastError());
            T(hipEventRecord(ev_done[b], ks));
        }
        T(hipMemcpyAsync(h_stat, Z.stat.p, sizeof h_stat, hipMemcpyDeviceToHost, ks));
        T(hipStreamSynchronize(up));
        T(hipStreamSynchronize(ks));
        harvest_timers(c);
    }
    drop_events();
    hc.lap("inflate: upload + kernels");
    if (rc) return rc;
    if (!T.ok()) return T.fail(c, who, detail);
    if (h_stat[0] != ~0ull) {   // the host door's words (bgzf_inflate of afq_host.cpp) where they do not depend on zlib
        const uint32_t code = (uint32_t)(h_stat[0] & 0xff);
        const uint64_t bad = h_stat[0] >> 8;
        const std::string at = "BGZF block " + std::to_string(bad) + ": ";
        if (code == kInflateCrcMismatch) return fail(c, AFQ_ERR_BAD_INPUT, at + "bad CRC32");
        if (code == kInflateOutputShort && (h_stat[1] >> 32) == bad)
            return fail(c, AFQ_ERR_BAD_INPUT, at + "ISIZE says " + std::to_string(blocks[bad].isize) + " bytes, the deflate stream holds " + std::to_string(h_stat[1] & 0xffffffffull));
        return fail(c, AFQ_ERR_BAD_INPUT, at + "the deflate stream is corrupt or longer than ISIZE (" + inflate_code_words(code) + ")");
    }
    if (h_stat[2] != nb) return fail(c, AFQ_ERR_HIP, std::string(who) + ": " + std::to_string(h_stat[2]) + " of " + std::to_string(nb) + " blocks inflated" + detail);
    if (out_on_device) *out = Z.out.as<uint8_t>();
    else {
        uint8_t* ob = (uint8_t*)std::malloc(total ? total : 1);
        if (!ob) return fail(c, AFQ_ERR_OOM, std::string(who) + ": host allocation failed (" + std::to_string(total) + " inflated bytes)");
        if (total) {
            T(hipMemcpyAsync(ob, Z.out.as<uint8_t>() + shift, total, hipMemcpyDeviceToHost, ks));
            T(hipStreamSynchronize(ks));
        }
        if (!T.ok()) { std::free(ob); return T.fail(c, who, detail); }
        hc.lap("inflate: bytes D2H");
        *out = ob;
    }
    *out_n = total;
    if (stats) {
        afq_inflate_stats S{};
        S.n_in = n; S.n_out = total; S.n_blocks = h_stat[2]; S.n_blocks_empty = h_stat[3]; S.n_stored = h_stat[4]; S.n_fixed = h_stat[5]; S.n_dynamic = h_stat[6];
        S.n_literals = h_stat[7]; S.n_copies = h_stat[8];
        *stats = S;
    }
    return 0;
}

int afq_bgzf_resident_to_host(afq_ctx* c, uint32_t shift, uint64_t from, uint8_t* dst, uint64_t n) {
    static const char* who = "afq_bgzf_inflate_device";
    if (!c || (!dst && n) || (uint64_t)shift + from + n > c->inflate.out.cap) return fail(c, AFQ_ERR_INVALID_ARG, "the bytes asked for are not resident");
    if (!n) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    HipLatch T;
    T(hipMemcpyAsync(dst, c->inflate.out.as<uint8_t>() + shift + from, n, hipMemcpyDeviceToHost, c->stream));
    T(hipStreamSynchronize(c->stream));
    if (!T.ok()) return T.fail(c, who, " (" + std::to_string(n) + " inflated bytes back to the host)");
    return 0;
}
