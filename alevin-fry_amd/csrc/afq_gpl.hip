// afq_gpl.hip — the device half of `generate-permit-list` (src/cellfilter.rs, src/barcode_correction.rs of the reference): the
// barcode histogram of an UNCOLLATED single-barcode RNA RAD, and the correction decision of every distinct observed barcode.
//
// Histogram.  k_gpl_parse walks a mapper chunk as k_sort_parse does (afq_atac_sort.hip): a wave owns a chunk and stages it
// through LDS a tile at a time, a tile BEGINS at a record start, the record starts inside it are found by hopping the na
// fields in LDS (wave-uniform), then a lane per record reads its barcode and decides whether the record is compatible with
// the expected orientation.  The compatible records put their barcode into the chunk's own slots, filled from the front by
// ballot; the chunk's kept count (chunk_stat[1]) marks the rest of its slots empty - no barcode value can, the all-ones
// 8-byte barcode being a legal one.  k_gpl_count then counts the kept barcodes in an open-addressing table in HBM: keys
// claimed by 64-bit CAS at agent scope, counts by 64-bit atomicAdd, the all-ones barcode (the table's free mark) in a counter
// of its own.  k_gpl_compact gathers the taken slots (one cursor add per workgroup); the host sorts the pairs by barcode, so nothing depends on which lane
// won which slot.
//
// Correction.  k_gpl_correct takes a lane per distinct observed barcode and restates CorrectionIndex::resolve for retained
// sources whose canonical target is the source itself (GPL's case): a table of the retained barcodes gives a barcode's index
// in the sorted retained list, and with it its exact count.
#include <hip/hip_runtime.h>

#include "afq_common.h"
#include "afq_kernels.h"
#include "afq_prims.h"
#include "afq_rad_walk.h"

namespace afq {

namespace {

constexpr int kGplParseNT = 256;
constexpr uint32_t kGplWaves = kGplParseNT / 64;
constexpr uint32_t kGplTileWords = (3 + kGplParseTile + kGplParseHalo + 3) / 4 + 1;   // (+ the dword an unaligned 4-byte read of the last bytes also touches)
static_assert(kGplParseHalo >= (4 + 8 + 8) + (4 + 8) * kGplLaneAlns, "the halo holds the widest head and kGplLaneAlns of the widest alignments");
constexpr uint32_t kGplTileRecs = kGplParseTile / 6 + 1;   // the shortest record: na = 0, a 1-byte barcode, a 1-byte UMI

// Which record takes which route to its orientation test (cellfilter.rs:1698-1771):
//   - expected_ori == both: no alignment word is read; every record is compatible, na == 0 included.
//   - na == 0 under fw / rc: not compatible; nothing to read.
//   - na <= kGplLaneAlns: the record's own lane reads the words from LDS.  The halo is sized so that the whole list of such
//     a record is staged even when the record starts on the tile's last byte with the widest fields (static_assert below).
//   - na > kGplLaneAlns, however large (nothing bounds na) and wherever the list ends: a LONG record.  After the lanes' pass
//     the wave takes the long records of the batch one by one and its 64 lanes stride the record's alignment words in
//     global memory, stopping at the first trip with a fitting word.  The hop has checked that the list lies inside the
//     chunk, and the host that the chunk lies inside the buffer, before any of it is read.
__global__ __launch_bounds__(kGplParseNT) void k_gpl_parse(GplParseArgs a) {
    __shared__ uint32_t s_tile[kGplWaves][kGplTileWords];
    __shared__ uint16_t s_start[kGplWaves][kGplTileRecs];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t chunk = blockIdx.x * kGplWaves + wave;
    if (chunk >= a.n_chunks) return;   // (no workgroup barrier below: the waves of a block run chunks of different lengths)
    const SortChunk c = a.chunks[chunk];
    const uint32_t nb = c.nbytes, H = 4 + a.bc_bytes + a.umi_bytes, A = 4 + a.aln_extra;   // the host checked 8 <= nb and chunk_off + nb <= n_bytes
    uint32_t* tile = s_tile[wave];
    uint16_t* starts = s_start[wave];
    uint32_t p = 8, seen = 0, kept = 0, n_long = 0;   // wave-uniform
    uint32_t max_na = 0;                              // per lane: the largest na among ITS compatible records
    bool bad = false;                                 // uniform: the records do not tile the chunk
    while (p < nb && !bad) {
        // stage [p, p + tile + halo) of the chunk, as aligned dwords
        const uint32_t span = nb - p < kGplParseTile + kGplParseHalo ? nb - p : kGplParseTile + kGplParseHalo;
        const uint64_t g = c.chunk_off + p;
        const uint32_t al = (uint32_t)((reinterpret_cast<uintptr_t>(a.bytes) + g) & 3u);
        const uint32_t nw = (al + span + 3) >> 2;
        for (uint32_t i = lane; i < nw; i += 64) tile[i] = gpl_ld_dword_in(a.bytes, a.n_bytes, (int64_t)g - al + 4ll * i);
        gpl_wave_lds_sync();
        // hop the na chain: record starts q (relative to p) below the tile's end
        uint32_t q = 0, nr = 0;
        while (q < kGplParseTile && p + q < nb) {
            if (nb - (p + q) < H) { bad = true; break; }             // a head that runs past the chunk
            const uint32_t na = gpl_lds32(tile, al + q);
            if (na > (nb - (p + q) - H) / A) { bad = true; break; }   // alignments that run past the chunk
            if (lane == 0) starts[nr] = (uint16_t)q;
            ++nr;
            q += H + A * na;   // (<= nb - p: no wrap)
        }
        if (bad) break;
        if (seen + nr > c.nrec) { bad = true; break; }               // more records than the header says
        gpl_wave_lds_sync();
        for (uint32_t r0 = 0; r0 < nr; r0 += 64) {
            const uint32_t r = r0 + lane;
            bool keep = false, is_long = false;
            uint32_t na = 0, ro = 0;
            uint64_t bc = 0;
            if (r < nr) {
                ro = starts[r];
                const uint32_t o = al + ro;
                na = gpl_lds32(tile, o);
                bc = gpl_lds32(tile, o + 4);
                if (a.bc_bytes == 8) bc |= (uint64_t)gpl_lds32(tile, o + 8) << 32;
                else if (a.bc_bytes < 4) bc &= (1u << (8 * a.bc_bytes)) - 1u;
                if (a.expected_ori == kGplOriBoth) keep = true;
                else if (na == 0) keep = false;
                else if (na <= kGplLaneAlns) {   // (ro + H + A * na <= span: the record lies inside the chunk, and the halo holds it)
                    for (uint32_t j = 0; j < na && !keep; ++j) keep = gpl_word_fits(gpl_lds32(tile, o + H + A * j), a.expected_ori);
                } else is_long = true;
            }
            uint64_t pend = __ballot(is_long);
            n_long += (uint32_t)__popcll(pend);
            while (pend) {   // (uniform: every lane of the wave is here)
                const int src = __ffsll((long long)pend) - 1;
                pend &= pend - 1;
                const uint32_t lna = __shfl(na, src), lro = __shfl(ro, src);
                const uint64_t first = c.chunk_off + p + lro + H;   // the record's first alignment word
                bool hit = false;
                for (uint32_t j0 = 0; j0 < lna && !hit; j0 += 64) {
                    const uint32_t j = j0 + lane;
                    const bool h = j < lna && gpl_word_fits(gpl_ld_u32(a.bytes, a.n_bytes, first + (uint64_t)A * j), a.expected_ori);
                    hit = __ballot(h) != 0;
                }
                if ((int)lane == src) keep = hit;
            }
            const uint64_t m = __ballot(keep);
            if (keep) {   // (seen + nr <= nrec, so the slot is one of the chunk's)
                a.o_bc[c.out_off + kept + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = bc;
                max_na = na > max_na ? na : max_na;
            }
            kept += (uint32_t)__popcll(m);
        }
        seen += nr;
        p += q;
        gpl_wave_lds_sync();   // (the next trip overwrites the tile)
    }
    if (!bad && (p != nb || seen != c.nrec)) bad = true;
    for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(max_na, d); max_na = o > max_na ? o : max_na; }
    if (bad) { kept = 0; max_na = 0; if (lane == 0) set_err(a.st, kErrRecordWalk, chunk); }
    if (lane == 0) {
        uint32_t* s = a.chunk_stat + 4ull * chunk;
        s[0] = seen; s[1] = kept; s[2] = max_na; s[3] = n_long;
    }
}

// ---- counting table: a wave per chunk takes the chunk's kept barcodes
__global__ __launch_bounds__(256) void k_gpl_count(const SortChunk* __restrict__ chunks, uint32_t n_chunks, const uint32_t* __restrict__ chunk_stat,
                                                  const uint64_t* __restrict__ bcs, uint64_t* __restrict__ tab_key,
                                                  unsigned long long* __restrict__ tab_cnt, uint32_t mask, unsigned long long* __restrict__ ones,
                                                  DevStatus* __restrict__ st) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    const uint64_t base = chunks[chunk].out_off;
    const uint32_t kept = chunk_stat[4ull * chunk + 1];
    uint32_t n_ones = 0;
    for (uint32_t i = lane; i < kept; i += 64) {
        const uint64_t k = bcs[base + i];
        if (k == kSortEmptyKey) { ++n_ones; continue; }
        uint32_t slot = sort_hash_bc(k) & mask;
        bool done = false;
        for (uint32_t probe = 0; probe <= mask; ++probe) {
            unsigned long long prev = tab_key[slot];   // (a plain look first: most keys are in already)
            if (prev != k) {
                if (prev != kSortEmptyKey) { slot = (slot + 1) & mask; continue; }
                prev = atomicCAS(reinterpret_cast<unsigned long long*>(tab_key + slot), (unsigned long long)kSortEmptyKey, (unsigned long long)k);
                if (prev != kSortEmptyKey && prev != k) { slot = (slot + 1) & mask; continue; }
            }
            atomicAdd(tab_cnt + slot, 1ull);
            done = true;
            break;
        }
        if (!done) set_err(st, kErrInternal, chunk);   // at most half the slots are taken: a probe never runs through them all
    }
    for (int d = 32; d; d >>= 1) n_ones += __shfl_xor(n_ones, d);
    if (lane == 0 && n_ones) atomicAdd(ones, (unsigned long long)n_ones);
}

// the taken slots, gathered: a workgroup takes kGplCompactItems x 256 slots, scans its hits and draws its output range with ONE add
// to the cursor (a table sized for 10^8 records holds 10^6 keys: a cursor add per wave with a hit would be 10^6 adds to one address)
constexpr uint32_t kGplCompactItems = 16;
__global__ __launch_bounds__(256) void k_gpl_compact(const uint64_t* __restrict__ tab_key, const unsigned long long* __restrict__ tab_cnt, uint64_t cap,
                                                    uint64_t* __restrict__ o_key, uint64_t* __restrict__ o_cnt, uint32_t* __restrict__ n_out) {
    __shared__ uint32_t s_ws[256 / 64];
    __shared__ uint32_t s_base;
    const uint64_t first = (uint64_t)blockIdx.x * (256 * kGplCompactItems) + threadIdx.x;
    uint64_t k[kGplCompactItems];
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kGplCompactItems; ++j) {
        const uint64_t i = first + 256ull * j;
        k[j] = i < cap ? tab_key[i] : kSortEmptyKey;
        mine += k[j] != kSortEmptyKey;
    }
    uint32_t tot;
    const uint32_t ex = block_excl_scan<256>(mine, s_ws, tot);
    if (!tot) return;   // (uniform)
    if (threadIdx.x == 0) s_base = atomicAdd(n_out, tot);   // (at most cap / 2 < 2^31 keys)
    __syncthreads();
    uint32_t o = s_base + ex;
#pragma unroll
    for (uint32_t j = 0; j < kGplCompactItems; ++j)
        if (k[j] != kSortEmptyKey) { o_key[o] = k[j]; o_cnt[o] = tab_cnt[first + 256ull * j]; ++o; }
}

// ---- correction
__device__ __forceinline__ uint64_t gpl_base_mask(uint32_t n) { return n >= 32 ? ~0ull : (1ull << (2 * n)) - 1ull; }

__device__ __forceinline__ uint32_t gpl_find(const GplCorrectArgs& a, uint64_t k) {
    if (k == kSortEmptyKey) return a.ones_idx;
    uint32_t slot = sort_hash_bc(k) & a.tab_mask;
    for (uint32_t probe = 0; probe <= a.tab_mask; ++probe) {   // (at most half the slots are taken: an empty one ends the probe)
        const uint64_t kk = a.tab_key[slot];
        if (kk == k) return a.tab_val[slot];
        if (kk == kSortEmptyKey) return kGplNoTarget;
        slot = (slot + 1) & a.tab_mask;
    }
    return kGplNoTarget;
}

// The inverse shift candidates of x at one boundary, numbered t = 0..19 (for_each_inverse_shift_candidate): t < 4 is the
// inverse of `insertion` with free terminal base t; t >= 4 is the inverse of `deletion` with (lower, upper) = ((t-4) & 3,
// (t-4) >> 2), which exists only where lower | upper is x's base at the boundary.
__device__ __forceinline__ bool gpl_shift_cand(uint64_t x, uint32_t boundary, uint32_t t, uint64_t& out) {
    const uint64_t lower_mask = gpl_base_mask(boundary), low_wo = gpl_base_mask(boundary - 1);
    if (t < 4) { out = (x & ~lower_mask) | ((x & low_wo) << 2) | t; return true; }
    const uint64_t lo = (t - 4) & 3u, up = (t - 4) >> 2;
    if ((lo | up) != ((x >> (2 * boundary)) & 3ull)) return false;
    out = (x & ~gpl_base_mask(boundary + 1)) | ((x >> 2) & low_wo) | (lo << (2 * (boundary - 1))) | (up << (2 * boundary));
    return true;
}
__device__ __forceinline__ bool gpl_is_substitution(uint64_t s, uint64_t x) {   // s and x differ in exactly one base
    const uint64_t d = s ^ x, b = (d | (d >> 1)) & 0x5555555555555555ull;
    return b != 0 && (b & (b - 1)) == 0;
}

// Running state of one observed barcode's candidate walk.  Unique needs the first target and whether a second one turned up;
// Frequency the sum of the weights and the greatest (weight, target).  Targets are the sources themselves, so two candidates
// share a target exactly when they are the same source.
struct GplWalk { uint32_t first; bool ambiguous; uint64_t total, best_w; uint32_t best; };

__device__ __forceinline__ void gpl_take(const GplCorrectArgs& a, GplWalk& w, uint32_t idx) {
    if (w.first == kGplNoTarget) w.first = idx; else if (w.first != idx) w.ambiguous = true;
    const uint64_t wt = a.ret_count[idx] + a.pseudocount;   // (< 2^55: the host checked; at most 499 candidates, so total < 2^64)
    w.total += wt;
    if (w.best == kGplNoTarget || wt > w.best_w || (wt == w.best_w && idx > w.best)) { w.best_w = wt; w.best = idx; }
}

__global__ __launch_bounds__(256) void k_gpl_correct(GplCorrectArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t dec = kGplNotFound, tgt = kGplNoTarget;
    uint64_t cnt = 0;
    const bool live = i < a.n_obs;
    if (live) {
        const uint64_t x = a.observed[i];
        cnt = a.obs_count[i];
        tgt = gpl_find(a, x);
        if (tgt != kGplNoTarget) dec = kGplExact;
        else {
            GplWalk w{kGplNoTarget, false, 0, 0, kGplNoTarget};
            for (uint32_t pos = 0; pos < a.barcode_len; ++pos) {   // for_each_substitution: 3 L distinct candidates, none equal to x
                const uint32_t sh = 2 * pos;
                const uint64_t cleared = x & ~(3ull << sh), base = (x >> sh) & 3ull;
                for (uint64_t rep = 0; rep < 4; ++rep) {
                    if (rep == base) continue;
                    const uint32_t idx = gpl_find(a, cleared | (rep << sh));
                    if (idx != kGplNoTarget) gpl_take(a, w, idx);
                }
            }
            if (a.neighborhood == kGplShift) {
                for (uint32_t b = 1; b < a.barcode_len; ++b)
                    for (uint32_t t = 0; t < 20; ++t) {
                        uint64_t s;
                        if (!gpl_shift_cand(x, b, t, s)) continue;
                        const uint32_t idx = gpl_find(a, s);
                        if (idx == kGplNoTarget) continue;
                        // a source weighs once however many constructions lead to it: skip one the substitutions reached, or
                        // an earlier shift candidate (the walk is repeated up to here; only a retained candidate pays it)
                        bool dup = gpl_is_substitution(s, x);
                        for (uint32_t b2 = 1; b2 <= b && !dup; ++b2)
                            for (uint32_t t2 = 0; t2 < (b2 < b ? 20u : t) && !dup; ++t2) {
                                uint64_t s2;
                                dup = gpl_shift_cand(x, b2, t2, s2) && s2 == s;
                            }
                        if (!dup) gpl_take(a, w, idx);
                    }
            }
            if (w.first == kGplNoTarget) dec = kGplNotFound;
            else if (a.resolution == kGplUnique) {
                if (w.ambiguous) dec = kGplAmbiguous; else { dec = kGplCorrected; tgt = w.first; }
            } else {
                // winner / total >= num / den  <=>  winner * den >= num * total: two 64 x 64 -> 128-bit products, compared exactly
                const uint64_t lh = __umul64hi(w.best_w, a.conf_den), ll = w.best_w * a.conf_den;
                const uint64_t rh = __umul64hi(a.conf_num, w.total), rl = a.conf_num * w.total;
                if (lh > rh || (lh == rh && ll >= rl)) { dec = kGplCorrected; tgt = w.best; } else dec = kGplAmbiguous;
            }
        }
        a.o_decision[i] = (uint8_t)dec;
        a.o_target[i] = tgt;
        if (tgt != kGplNoTarget && cnt) atomicAdd(a.target_count + tgt, (unsigned long long)cnt);
    }
    // the eight CorrectionStats counters: distinct and reads per decision, summed over the wave first
    for (uint32_t d = 0; d < 4; ++d) {
        const bool mine = live && dec == d;
        const uint64_t m = __ballot(mine);
        if (!m) continue;   // (uniform)
        uint64_t reads = mine ? cnt : 0;
        for (int s = 32; s; s >>= 1) reads += __shfl_xor(reads, s);
        if ((threadIdx.x & 63u) == 0) {
            atomicAdd(a.stats + 2 * d, (unsigned long long)__popcll(m));
            if (reads) atomicAdd(a.stats + 2 * d + 1, (unsigned long long)reads);
        }
    }
}

}  // namespace

void launch_gpl_parse(hipStream_t s, const GplParseArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH(k_gpl_parse, (a.n_chunks + kGplWaves - 1) / kGplWaves, kGplParseNT, s, a);
}

void launch_gpl_count(hipStream_t s, const SortChunk* chunks, uint32_t n_chunks, const uint32_t* chunk_stat, const uint64_t* bcs, uint64_t* tab_key,
                      unsigned long long* tab_cnt, uint32_t mask, unsigned long long* ones, DevStatus* st) {
    if (!n_chunks) return;
    AFQ_LAUNCH(k_gpl_count, (n_chunks + 3) / 4, 256, s, chunks, n_chunks, chunk_stat, bcs, tab_key, tab_cnt, mask, ones, st);
}

void launch_gpl_compact(hipStream_t s, const uint64_t* tab_key, const unsigned long long* tab_cnt, uint64_t cap, uint64_t* o_key, uint64_t* o_cnt,
                        uint32_t* n_out) {
    AFQ_LAUNCH(k_gpl_compact, (uint32_t)((cap + 256 * kGplCompactItems - 1) / (256 * kGplCompactItems)), 256, s, tab_key, tab_cnt, cap, o_key, o_cnt, n_out);
}

void launch_gpl_correct(hipStream_t s, const GplCorrectArgs& a) {
    if (!a.n_obs) return;
    AFQ_LAUNCH(k_gpl_correct, (uint32_t)((a.n_obs + 255) / 256), 256, s, a);
}

}  // namespace afq
