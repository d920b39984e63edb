// afq_convert.hip — the device half of `convert` (bam2rad, src/convert.rs:167-594 of the reference): the alignment records of a
// BAM, as they stand in the inflated stream behind the BAM header, become the records of a mapper RAD, `na, b, u, na x u32`.
//
// A BAM record is `block_size:u32` and block_size bytes: refID, pos, l_read_name:u8, mapq, bin, n_cigar_op:u16, flag:u16, l_seq:u32,
// next_refID, next_pos, tlen (32 bytes), the name, the CIGAR, the packed sequence, the qualities, then the aux fields up to the
// record's end (SAM/BAM specification, section 4.2).  The phases, each a kernel or a scan, in stream order:
//   - walk (k_convert_walk, twice: count, then fill): a wave owns a host-made span of records and stages it through LDS a tile at a
//     time; a tile begins at a record start, the starts inside it are found by hopping block_size in LDS (wave-uniform), then a lane
//     takes a record: the fixed fields, the size check (the fixed fields, name, CIGAR and sequence fit block_size; the hop checked
//     that block_size fits the span), the flag filter (0x4, 0x800), the refID check.  Nothing behind these checks reads outside a
//     record, and no record lies outside the stream.  The count walk leaves (records, kept) per span; the host sums them, and the
//     fill walk writes every kept record's offset, file index and alignment word at its rank: compaction by scan, input order kept.
//   - heads (k_convert_heads): a lane per kept record compares its name with its predecessor's - the length first, then the bytes,
//     out of global memory; the predecessor is the kept record in front, however many dropped records or spans lie between.
//     The exclusive scan of the head flags (launch_convert_scan: blocked, 4 096 words a workgroup) numbers the runs.
//   - aux (k_convert_aux): a lane per kept record that needs it - a run's head for CR / UR, every record under -f for AS - hops the
//     aux fields by their sizes (A c C s S i I f, Z and H to their NUL, B arrays by subtype and count); the fields must end exactly
//     at the record's end.  The head's CR and UR are coded two bits a base (A0 C1 G2 T3, first base most significant, one N as A);
//     two N in either drop the run.
//   - runs (k_convert_runs): a lane per run: under -f the best AS and the number of records that reach it.
//     The exclusive scan of the written flags ranks the written runs.
//   - place (k_convert_place): written run of rank w: the sort word  (w / 10 001) << 32 | w  and its length.  launch_collate_scan and
//     launch_collate_heads (afq_collate.hip) lay the runs out from these as they lay out a cell's records: 8 bytes of chunk header in
//     front of every 10 001st run.  The scan IS the layout: no allocation atomics, the output is a function of the input alone.
//   - write (k_convert_write): a lane per written run stores na, b, u and the words of the records that reach the best AS.
// A run of more than kConvertLaneAlns records is a LONG run: in runs and in write the whole wave takes it, 64 records a trip.
// Errors go into one word, record index << 8 | code, by atomicMin: the first record in error is named, whatever the schedule.
#include <hip/hip_runtime.h>

#include <climits>

#include "afq_common.h"
#include "afq_kernels.h"
#include "afq_prims.h"
#include "afq_rad_walk.h"

namespace afq {

namespace {

constexpr int kWalkNT = 256;
constexpr uint32_t kWalkWaves = kWalkNT / 64;
static_assert(kGplParseHalo >= kConvertRecFixed, "the halo holds the fixed fields of a record that starts on the tile's last byte");
static_assert(kConvertTileRecs <= 65536 && kGplParseTile <= 65536, "a record start fits the uint16 slot");

__device__ __forceinline__ void conv_err(const ConvertArgs& a, uint32_t rec, uint32_t code) { atomicMin(a.err, ((unsigned long long)rec << 8) | code); }

// where the aux fields of the record at `o` begin and end (the walk checked: begin <= end <= the stream's end)
__device__ __forceinline__ void conv_aux_range(const ConvertArgs& a, uint64_t o, uint64_t& begin, uint64_t& end) {
    const uint32_t bs = gpl_ld_u32(a.bytes, a.n_bytes, o), l_name = a.bytes[o + 12];
    const uint32_t n_cig = gpl_ld_u32(a.bytes, a.n_bytes, o + 16) & 0xFFFFu, l_seq = gpl_ld_u32(a.bytes, a.n_bytes, o + 20);
    begin = o + kConvertRecFixed + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + l_seq;
    end = o + 4ull + bs;
}

template <bool FILL>
__global__ __launch_bounds__(kWalkNT) void k_convert_walk(ConvertArgs a) {
    __shared__ uint32_t s_tile[kWalkWaves][kRadWalkTileWords];
    __shared__ uint16_t s_start[kWalkWaves][kConvertTileRecs];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t span = blockIdx.x * kWalkWaves + wave;
    if (span >= a.n_spans) return;   // (no workgroup barrier below: the waves of a block run spans of different lengths)
    const uint64_t s0 = a.span_off[span], s1 = span + 1 < a.n_spans ? a.span_off[span + 1] : a.n_bytes;   // the host checked: ascending, <= n_bytes
    const uint64_t nb = s1 - s0;
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t base_rec = 0, base_kept = 0;
    if constexpr (FILL) { base_rec = a.span_base[2ull * span]; base_kept = a.span_base[2ull * span + 1]; }
    uint32_t* tile = s_tile[wave];
    uint16_t* starts = s_start[wave];
    uint64_t p = 0;                    // wave-uniform
    uint32_t seen = 0, kept = 0;       // uniform
    bool stop = false;                 // uniform: a record in error ends the span's walk (both walks at the same record)
    while (p < nb && !stop) {
        // stage [p, p + tile + halo) of the span, as aligned dwords
        const uint32_t len = nb - p < kGplParseTile + kGplParseHalo ? (uint32_t)(nb - p) : kGplParseTile + kGplParseHalo;
        const uint64_t g = s0 + p;
        const uint32_t al = (uint32_t)((reinterpret_cast<uintptr_t>(a.bytes) + g) & 3u);
        const uint32_t nw = (al + len + 3) >> 2;
        for (uint32_t i = lane; i < nw; i += 64) tile[i] = gpl_ld_dword_in(a.bytes, a.n_bytes, (int64_t)g - al + 4ll * i);
        gpl_wave_lds_sync();
        // hop the block_size chain: record starts q (relative to p) below the tile's end
        uint64_t q = 0;
        uint32_t nr = 0;
        while (q < kGplParseTile && q < nb - p) {
            const uint64_t left = nb - p - q;
            const uint32_t bs = left >= 4 ? gpl_lds32(tile, al + (uint32_t)q) : 0u;
            if (left < 4 || bs < kConvertRecFixed - 4 || bs > left - 4) { stop = true; break; }   // no room for block_size, for the fixed fields, or past the span
            if (lane == 0) starts[nr] = (uint16_t)q;
            ++nr;
            q += 4ull + bs;   // (<= nb - p)
        }
        const bool hop_bad = stop;
        gpl_wave_lds_sync();
        for (uint32_t r0 = 0; r0 < nr; r0 += 64) {
            const uint32_t r = r0 + lane;
            uint32_t code = 0, word = 0, ro = 0;
            bool keep = false;
            if (r < nr) {   // (the record's 36 fixed bytes lie inside the span and inside tile + halo: bs >= 32 fits `left`)
                ro = starts[r];
                const uint32_t o = al + ro;
                const uint32_t bs = gpl_lds32(tile, o), refid = gpl_lds32(tile, o + 4), l_name = gpl_lds32(tile, o + 12) & 0xFFu;
                const uint32_t cf = gpl_lds32(tile, o + 16), n_cig = cf & 0xFFFFu, flag = cf >> 16, l_seq = gpl_lds32(tile, o + 20);
                const uint64_t need = (kConvertRecFixed - 4) + (uint64_t)l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + l_seq;
                if (need > bs) code = kConvErrRecord;
                else if (!(flag & 0x804u)) {   // unmapped and supplementary records do not exist for what follows (convert.rs:434)
                    if (refid >= a.n_ref) code = kConvErrRef;   // (a negative refID is a large unsigned one)
                    else { keep = true; word = refid | ((flag & 0x10u) ? 0u : 0x80000000u); }
                }
            }
            const uint64_t m = __ballot(keep);
            if constexpr (FILL) {
                if (keep) {   // (k < n_kept: the count walk counted the same records)
                    const uint64_t k = (uint64_t)base_kept + kept + (uint32_t)__popcll(m & lt);
                    a.rec_off[k] = s0 + p + ro; a.rec_idx[k] = base_rec + seen + r; a.word[k] = word;
                }
                if (code) conv_err(a, base_rec + seen + r, code);
            }
            kept += (uint32_t)__popcll(m);
            if (__ballot(code != 0)) stop = true;
        }
        seen += nr;
        if constexpr (FILL) { if (hop_bad && lane == 0) conv_err(a, base_rec + seen, kConvErrRecord); }
        p += q;
        gpl_wave_lds_sync();   // (the next trip overwrites the tile)
    }
    if constexpr (!FILL) { if (lane == 0) { a.span_cnt[2ull * span] = seen; a.span_cnt[2ull * span + 1] = kept; } }
}

__global__ __launch_bounds__(256) void k_convert_heads(ConvertArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > a.n_kept) return;
    if (k == a.n_kept) { a.head[k] = 0; return; }
    uint32_t h = 1;
    if (k) {
        const uint64_t o1 = a.rec_off[k], o0 = a.rec_off[k - 1];
        const uint32_t l1 = a.bytes[o1 + 12], l0 = a.bytes[o0 + 12];
        if (l1 == l0) {   // the length first, then the bytes (l_read_name of them: inside both records, the walk checked)
            h = 0;
            for (uint32_t i = 0; i < l1 && !h; i += 4) {
                uint32_t x = gpl_ld_u32(a.bytes, a.n_bytes, o1 + kConvertRecFixed + i) ^ gpl_ld_u32(a.bytes, a.n_bytes, o0 + kConvertRecFixed + i);
                if (l1 - i < 4) x &= (1u << (8 * (l1 - i))) - 1u;
                h = x != 0;
            }
        }
    }
    a.head[k] = h;
}

// a Z string of len bases at `at`, two bits a base, first base most significant; base i stands at bit 2 (len - 1 - i) mod 64, as
// cb_string_to_u64's shift does in a release build (convert.rs:75-89)
__device__ __forceinline__ void conv_code(const uint8_t* b, uint64_t at, uint32_t len, uint64_t& v, uint32_t& n_n, bool& bad) {
    v = 0; n_n = 0; bad = false;
    for (uint32_t i = 0; i < len; ++i) {
        const uint8_t ch = b[at + i];
        uint64_t c = 0;
        if (ch == 'C') c = 1; else if (ch == 'G') c = 2; else if (ch == 'T') c = 3; else if (ch == 'N') ++n_n; else if (ch != 'A') bad = true;
        v |= c << ((2u * (len - 1 - i)) & 63u);
    }
}

__global__ __launch_bounds__(256) void k_convert_aux(ConvertArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n_kept) return;
    const uint32_t h1 = a.head[k + 1], run = h1 - 1;
    const bool is_head = h1 != a.head[k];
    if (is_head) a.run_first[run] = (uint32_t)k;
    if (k == 0) a.run_first[a.n_runs] = a.n_kept;
    if (!is_head && !a.filter_best) return;   // nothing of this record's aux is asked for
    const uint8_t* b = a.bytes;
    uint64_t g, end;
    conv_aux_range(a, a.rec_off[k], g, end);
    bool bad = false, have_cr = false, cr_z = false, have_ur = false, ur_z = false, have_as = false, as_int = false;
    uint64_t cr_at = 0, ur_at = 0;
    uint32_t cr_len = 0, ur_len = 0;
    int32_t score = 0;
    while (g < end && !bad) {
        if (end - g < 3) { bad = true; break; }
        const uint8_t t0 = b[g], t1 = b[g + 1], ty = b[g + 2];
        g += 3;
        const uint64_t v0 = g;   // the value
        uint32_t sz = 0, zlen = 0;
        switch (ty) {
            case 'A': case 'c': case 'C': sz = 1; break;
            case 's': case 'S': sz = 2; break;
            case 'i': case 'I': case 'f': sz = 4; break;
            case 'Z': case 'H': {
                while (g < end && b[g]) ++g;
                if (g == end) bad = true; else { zlen = (uint32_t)(g - v0); ++g; }
                break;
            }
            case 'B': {
                if (end - g < 5) { bad = true; break; }
                const uint8_t sub = b[g];
                const uint64_t cnt = gpl_ld_u32(b, a.n_bytes, g + 1);
                const uint32_t es = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
                if (!es || cnt * es > end - g - 5) bad = true; else g += 5 + cnt * es;
                break;
            }
            default: bad = true;
        }
        if (bad) break;
        if (sz) { if (end - g < sz) { bad = true; break; } g += sz; }
        if (is_head && t0 == 'C' && t1 == 'R' && !have_cr) { have_cr = true; cr_z = ty == 'Z'; cr_at = v0; cr_len = zlen; }
        else if (is_head && t0 == 'U' && t1 == 'R' && !have_ur) { have_ur = true; ur_z = ty == 'Z'; ur_at = v0; ur_len = zlen; }
        else if (a.filter_best && t0 == 'A' && t1 == 'S' && !have_as) {   // get_score, convert.rs:146-165: an I above 2^31 - 1 wraps
            have_as = true; as_int = true;
            switch (ty) {
                case 'c': score = (int8_t)b[v0]; break;
                case 'C': score = b[v0]; break;
                case 's': score = (int16_t)(b[v0] | b[v0 + 1] << 8); break;
                case 'S': score = b[v0] | b[v0 + 1] << 8; break;
                case 'i': case 'I': score = (int32_t)gpl_ld_u32(b, a.n_bytes, v0); break;
                default: as_int = false;
            }
        }
    }
    const uint32_t ri = a.rec_idx[k];
    if (bad) {   // (the runs kernel is enqueued behind this one before the host reads the error word: leave nothing of the record unwritten)
        conv_err(a, ri, kConvErrRecord);
        if (a.filter_best) { a.score[k] = 0; a.has_score[k] = 0; }
        if (is_head) { a.run_bc[run] = 0; a.run_umi[run] = 0; a.run_flag[run] = 1; }
        return;
    }
    if (a.filter_best) { a.score[k] = score; a.has_score[k] = have_as && as_int; }
    if (!is_head) return;
    bool drop = true;
    uint64_t bc = 0, umi = 0;
    if (!have_cr || !have_ur) conv_err(a, ri, kConvErrTagMissing);
    else if (!cr_z || !ur_z) conv_err(a, ri, kConvErrTagType);
    else {
        uint32_t n0, n1;
        bool bad0, bad1;
        conv_code(b, cr_at, cr_len, bc, n0, bad0);
        conv_code(b, ur_at, ur_len, umi, n1, bad1);
        drop = n0 >= 2 || n1 >= 2;   // (convert.rs:525-532: before the bases are looked at)
        if (!drop && (bad0 || bad1)) conv_err(a, ri, kConvErrBase);
    }
    a.run_bc[run] = bc; a.run_umi[run] = umi; a.run_flag[run] = drop;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d); return v; }

__global__ __launch_bounds__(256) void k_convert_runs(ConvertArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool live = r < a.n_runs;
    uint32_t s = 0, n = 0, na = 0, missing = ~0u;   // missing: the first record of the run without an integer AS
    int32_t mx = INT_MIN;
    bool drop = true, is_long = false;
    if (live) {
        s = a.run_first[r]; n = a.run_first[r + 1] - s; drop = a.run_flag[r] != 0;
        if (!drop) {
            if (!a.filter_best) na = n;
            else if (n <= kConvertLaneAlns) {
                for (uint32_t j = s; j < s + n; ++j) { if (!a.has_score[j]) { if (missing == ~0u) missing = j; } else mx = max(mx, a.score[j]); }
                for (uint32_t j = s; j < s + n; ++j) na += a.has_score[j] && a.score[j] == mx;
            } else is_long = true;
        }
    }
    uint64_t pend = __ballot(is_long);
    while (pend) {   // (uniform: every lane of the wave is here)
        const int src = __ffsll((long long)pend) - 1;
        pend &= pend - 1;
        const uint32_t ls = __shfl(s, src), ln = __shfl(n, src);
        int32_t wmx = INT_MIN;
        uint32_t wmiss = ~0u, cnt = 0;
        for (uint32_t j = ls + lane; j < ls + ln; j += 64) { if (!a.has_score[j]) wmiss = min(wmiss, j); else wmx = max(wmx, a.score[j]); }
        for (int d = 32; d; d >>= 1) { wmx = max(wmx, __shfl_xor(wmx, d)); wmiss = min(wmiss, __shfl_xor(wmiss, d)); }
        for (uint32_t j = ls + lane; j < ls + ln; j += 64) cnt += a.has_score[j] && a.score[j] == wmx;
        cnt = wave_sum(cnt);
        if ((int)lane == src) { mx = wmx; missing = wmiss; na = cnt; }
    }
    if (live) {
        if (missing != ~0u) conv_err(a, a.rec_idx[missing], kConvErrScore);
        a.run_na[r] = na; a.run_max[r] = mx; a.run_flag[r] = !drop;
        if (r == 0) a.run_flag[a.n_runs] = 0;
    }
    const bool wr = live && !drop;
    const uint32_t c0 = wave_sum(live && drop), c1 = wave_sum(wr ? n : 0u), c2 = wave_sum(wr ? na : 0u), c3 = wave_sum(wr && n > kConvertLaneAlns);
    if (lane == 0) {
        if (c0) atomicAdd((unsigned long long*)&a.stat[kConvRunsDroppedN], c0);
        if (c1) atomicAdd((unsigned long long*)&a.stat[kConvAlnIn], c1);
        if (c2) atomicAdd((unsigned long long*)&a.stat[kConvAlnWritten], c2);
        if (c3) atomicAdd((unsigned long long*)&a.stat[kConvLongRuns], c3);
    }
}

__global__ __launch_bounds__(256) void k_convert_place(ConvertArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_runs) return;
    const uint32_t w = a.run_flag[r];   // (scanned: the written runs in front)
    if (a.run_flag[r + 1] == w) return;
    const uint32_t H = 4 + a.bc_bytes + a.umi_bytes, na = a.run_na[r], chunk = w / kConvertChunkRuns;
    uint32_t len = 0;
    if (na > (0xFFFFFFFFu - H) / 4) set_err(a.st, kErrCollateChunk, chunk);   // the run alone is 4 GiB or more
    else len = H + 4 * na;
    a.key[w] = ((uint64_t)chunk << 32) | w;
    a.rec[w] = make_uint2((uint32_t)r, len);
}

__global__ __launch_bounds__(256) void k_convert_write(ConvertArgs a) {
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lt = (1ull << lane) - 1ull;
    const uint32_t H = 4 + a.bc_bytes + a.umi_bytes;
    const bool live = w < a.n_written, fb = a.filter_best != 0;
    uint32_t s = 0, n = 0;
    int32_t mx = 0;
    uint64_t d = 0;
    if (live) {
        const uint32_t r = a.rec[w].x;
        s = a.run_first[r]; n = a.run_first[r + 1] - s; mx = a.run_max[r]; d = a.dest[w];
        ByteOut o{a.out + d, 0, 0};
        o.put(a.run_na[r], 4);
        o.put_field(a.run_bc[r], a.bc_bytes);
        o.put_field(a.run_umi[r], a.umi_bytes);
        if (n <= kConvertLaneAlns)
            for (uint32_t j = s; j < s + n; ++j)
                if (!fb || a.score[j] == mx) o.put(a.word[j], 4);
        o.flush();
    }
    uint64_t pend = __ballot(live && n > kConvertLaneAlns);
    while (pend) {   // (uniform)
        const int src = __ffsll((long long)pend) - 1;
        pend &= pend - 1;
        const uint32_t ls = __shfl(s, src), ln = __shfl(n, src);
        const int32_t lmx = __shfl(mx, src);
        const uint64_t ld = ((uint64_t)__shfl((uint32_t)(d >> 32), src) << 32) | __shfl((uint32_t)d, src);
        uint32_t base = 0;   // words written in front of this trip
        for (uint32_t j0 = 0; j0 < ln; j0 += 64) {
            const uint32_t j = ls + j0 + lane;
            const bool h = j0 + lane < ln && (!fb || a.score[j] == lmx);
            const uint64_t m = __ballot(h);
            if (h) {   // (base + rank < na: runs counted the same records)
                ByteOut o{a.out + ld + H + 4ull * (base + (uint32_t)__popcll(m & lt)), 0, 0};
                o.put(a.word[j], 4);
                o.flush();
            }
            base += (uint32_t)__popcll(m);
        }
    }
}

// ---- the exclusive scan of n words in place (head flags, written flags), by many workgroups: a workgroup's sum of its kConvertScanBlock
// words, the one-workgroup scan of those sums (launch_collate_excl_scan_u32: one word per 4 096), then every position's prefix
__global__ __launch_bounds__(256) void k_convert_scan_sum(const uint32_t* __restrict__ v, uint64_t n, uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t s[256 / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * kConvertScanBlock + (uint64_t)threadIdx.x * kConvertScanItems;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kConvertScanItems; ++j)
        if (i0 + j < n) mine += v[i0 + j];
    uint32_t tot;
    (void)block_excl_scan<256>(mine, s, tot);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void k_convert_scan_apply(uint32_t* __restrict__ v, uint64_t n, const uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t s[256 / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * kConvertScanBlock + (uint64_t)threadIdx.x * kConvertScanItems;
    uint32_t x[kConvertScanItems], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kConvertScanItems; ++j) { x[j] = i0 + j < n ? v[i0 + j] : 0u; mine += x[j]; }
    uint32_t tot;
    uint32_t ex = block_sum[blockIdx.x] + block_excl_scan<256>(mine, s, tot);
#pragma unroll
    for (uint32_t j = 0; j < kConvertScanItems; ++j) { if (i0 + j < n) v[i0 + j] = ex; ex += x[j]; }
}

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + 255) / 256); }

}  // namespace

void launch_convert_count(hipStream_t s, const ConvertArgs& a) {
    if (a.n_spans) AFQ_LAUNCH(k_convert_walk<false>, (a.n_spans + kWalkWaves - 1) / kWalkWaves, kWalkNT, s, a);
}
void launch_convert_fill(hipStream_t s, const ConvertArgs& a) {
    if (a.n_spans) AFQ_LAUNCH(k_convert_walk<true>, (a.n_spans + kWalkWaves - 1) / kWalkWaves, kWalkNT, s, a);
}
void launch_convert_heads(hipStream_t s, const ConvertArgs& a) { AFQ_LAUNCH(k_convert_heads, blocks_of((uint64_t)a.n_kept + 1), 256, s, a); }
void launch_convert_scan(hipStream_t s, uint32_t* v, uint64_t n, uint32_t* block_sum) {
    if (!n) return;
    const uint32_t nb = (uint32_t)((n + kConvertScanBlock - 1) / kConvertScanBlock);
    AFQ_LAUNCH(k_convert_scan_sum, nb, 256, s, v, n, block_sum);
    launch_collate_excl_scan_u32(s, block_sum, nb);
    AFQ_LAUNCH(k_convert_scan_apply, nb, 256, s, v, n, block_sum);
}
void launch_convert_aux(hipStream_t s, const ConvertArgs& a) {
    if (a.n_kept) AFQ_LAUNCH(k_convert_aux, blocks_of(a.n_kept), 256, s, a);
}
void launch_convert_runs(hipStream_t s, const ConvertArgs& a) {
    if (a.n_runs) AFQ_LAUNCH(k_convert_runs, blocks_of(a.n_runs), 256, s, a);
}
void launch_convert_place(hipStream_t s, const ConvertArgs& a) {
    if (a.n_runs) AFQ_LAUNCH(k_convert_place, blocks_of(a.n_runs), 256, s, a);
}
void launch_convert_write(hipStream_t s, const ConvertArgs& a) {
    if (a.n_written) AFQ_LAUNCH(k_convert_write, blocks_of(a.n_written), 256, s, a);
}

}  // namespace afq
