// afq_collate.hip — the device half of `collate` (src/collate.rs of the reference): the records of an UNCOLLATED single-barcode
// RNA RAD, filtered by orientation, barcode-corrected, and written as one chunk per cell in a given cell order.
//
// The input is walked twice, as k_gpl_parse walks it (afq_gpl.hip): a wave owns a chunk and stages it through LDS a tile at a
// time, a tile begins at a record start, the record starts are found by hopping the na fields (wave-uniform), then a lane takes
// a record.  Both walks are ONE kernel template, so that they cannot disagree about where a record lies:
//   - measure: the lane counts the record's fitting alignment words (nk), probes the correction table with its barcode and writes
//     (cell, H + A nk) into the record's own slot - the chunk table's prefix + the record's index, so the slots are in input
//     order by construction - and the sort word  cell << 32 | slot.  A dropped record carries the cell n_cells and no bytes.
//   - placement: a stable LSD radix sort of the sort words over the cell bits (8-bit digits; per-workgroup digit counts, one scan,
//     rank-preserving scatter), then an exclusive 64-bit scan of the record lengths in sorted order.  The scan IS the layout:
//     dest[slot] = 8 (cell + 1) + scan.  No allocation atomics, so the output is a function of the input alone.
//   - heads: a lane per cell finds its run in the sorted words by binary search: chunk offset, nrec, the (nbytes, nrec) header.
//   - write: the second walk; the lane of a kept record writes nk, the corrected barcode, the UMI and the fitting alignments with
//     their position bytes at dest[slot].
// A record with more than kGplLaneAlns alignments is handled by the whole wave out of global memory in both walks.
//
// Multi-barcode `collate` (do_collate_multi_bc_fast, src/collate.rs:1415-1920 of the reference) is the same template over another
// args type: the records are `na, b0, b1, umi, alignments`, routed to a sample by b0, corrected to a cell of that sample by b1, and
// written with b0 = the sample's ordinal and b1 = the corrected cell barcode.  Five sites of the walk differ, each behind an
// `if constexpr` on the args type: the head size, the lookup, the counter n_unrouted, the head's barcode fields as written, and the
// order of the chunk_stat words.  Its lookup has two levels:
//   - the sample table: observed b0 -> sample index (a few thousand entries at most; it stays in cache).  The lane starts this
//     probe beside the read of na, before the alignment words are counted, as k_gpl_multi_parse does;
//   - the cell table: sample << 32 | b1 -> the index of the corrected barcode among the cells.  It depends on the first probe's
//     result.  b1 has at most 4 bytes and a sample index is below 2^31, so no key is the all-ones free mark (single-barcode keys
//     can be all-ones: that barcode travels beside the table as ones_cell).
// Both tables are launch_sort_table's; placement, the length scan and the chunk heads below serve both.
//
// Stores.  Two records that are neighbours in the output share an aligned dword and different waves write them.  ByteOut stores
// only the bytes it was given: byte / short stores up to the first dword boundary and after the last, dwords between; it never
// reads the output.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "afq_common.h"
#include "afq_kernels.h"
#include "afq_prims.h"
#include "afq_rad_walk.h"

namespace afq {

namespace {

constexpr int kWalkNT = 256;
constexpr uint32_t kWalkWaves = kWalkNT / 64;
static_assert(kGplParseHalo >= (4 + 8 + 8) + (4 + 8) * kGplLaneAlns, "the halo holds the widest head and kGplLaneAlns of the widest alignments");
static_assert(kGplParseHalo >= (4 + 4 + 4 + 8) + (4 + 8) * kGplLaneAlns, "the halo holds the widest head (na, b0, b1, umi) and kGplLaneAlns of the widest alignments");
static_assert(kRadWalkTileRecs >= kGplParseTile / (4 + 1 + 1 + 1) + 1, "a start slot for every record of a tile of the shortest records");

__device__ __forceinline__ uint32_t collate_find(const CollateArgs& a, uint64_t k) {
    if (k == kSortEmptyKey) return a.ones_cell;
    return sort_table_find(a.tab_key, a.tab_val, a.tab_mask, k);
}
__device__ __forceinline__ uint32_t collate_head_bytes(const CollateArgs& a) { return 4 + a.bc_bytes + a.umi_bytes; }
__device__ __forceinline__ uint32_t collate_head_bytes(const CollateMultiArgs& a) { return 4 + a.b0_bytes + a.b1_bytes + a.umi_bytes; }

template <bool WRITE, class Args>
__global__ __launch_bounds__(kWalkNT) void k_collate_walk(Args a) {
    constexpr bool M = std::is_same_v<Args, CollateMultiArgs>;
    __shared__ uint32_t s_tile[kWalkWaves][kRadWalkTileWords];
    __shared__ uint16_t s_start[kWalkWaves][kRadWalkTileRecs];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t chunk = blockIdx.x * kWalkWaves + wave;
    if (chunk >= a.n_chunks) return;   // (no workgroup barrier below: the waves of a block run chunks of different lengths)
    const SortChunk c = a.chunks[chunk];
    const uint32_t nb = c.nbytes, H = collate_head_bytes(a), A = 4 + a.aln_extra;   // the host checked 8 <= nb and chunk_off + nb <= n_bytes
    [[maybe_unused]] uint32_t m0 = 0, m1 = 0;   // multi: the masks of b0 and b1
    if constexpr (M) { m0 = a.b0_bytes < 4 ? (1u << (8 * a.b0_bytes)) - 1u : ~0u; m1 = a.b1_bytes < 4 ? (1u << (8 * a.b1_bytes)) - 1u : ~0u; }
    const bool both = a.expected_ori == kGplOriBoth;
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t* tile = s_tile[wave];
    uint16_t* starts = s_start[wave];
    uint32_t p = 8, seen = 0;                                          // wave-uniform
    uint32_t n_compat = 0, n_uncorr = 0, n_kept = 0, aln_in = 0, aln_kept = 0, n_long = 0;   // per lane (a chunk is below 4 GiB: no sum wraps)
    [[maybe_unused]] uint32_t n_unrouted = 0;   // multi: compatible, but b0 names no sample
    bool bad = false;                                                  // uniform: the records do not tile the chunk
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
            const bool live = r < nr;
            const uint64_t slot = c.out_off + seen + r;   // (seen + nr <= nrec, so a live lane's slot is one of the chunk's; below 2^32: the host checked)
            uint32_t na = 0, ro = 0, o = 0;
            if (live) { ro = starts[r]; o = al + ro; na = gpl_lds32(tile, o); }
            const bool is_long = live && na > kGplLaneAlns;   // its list may end behind the halo: the wave takes it, out of global memory
            if constexpr (!WRITE) {
                uint32_t nfit = 0;
                [[maybe_unused]] uint32_t sample = kSortNoRank;
                if (live) {
                    if constexpr (M) sample = sort_table_find(a.stab_key, a.stab_val, a.stab_mask, gpl_lds32(tile, o + 4) & m0);   // (its loads fly while the alignment words are read)
                    aln_in += na;
                    n_long += is_long;
                    if (both) nfit = na;
                    else if (!is_long)   // (ro + H + A * na <= span: the record lies inside the chunk, and the halo holds it)
                        for (uint32_t j = 0; j < na; ++j) nfit += gpl_word_fits(gpl_lds32(tile, o + H + A * j), a.expected_ori);
                }
                uint64_t pend = both ? 0ull : __ballot(is_long);
                while (pend) {   // (uniform: every lane of the wave is here)
                    const int src = __ffsll((long long)pend) - 1;
                    pend &= pend - 1;
                    const uint32_t lna = __shfl(na, src), lro = __shfl(ro, src);
                    const uint64_t first = c.chunk_off + p + lro + H;   // the record's first alignment word; the hop checked that the list lies inside the chunk
                    uint32_t cnt = 0;
                    for (uint32_t j0 = 0; j0 < lna; j0 += 64) {
                        const uint32_t j = j0 + lane;
                        const bool h = j < lna && gpl_word_fits(gpl_ld_u32(a.bytes, a.n_bytes, first + (uint64_t)A * j), a.expected_ori);
                        cnt += (uint32_t)__popcll(__ballot(h));
                    }
                    if ((int)lane == src) nfit = cnt;
                }
                if (live) {
                    uint32_t cell = a.n_cells, len = 0;
                    if (both || nfit) {   // compatible (na == 0 only under `both`)
                        ++n_compat;
                        if constexpr (M) {
                            if (sample == kSortNoRank) ++n_unrouted;
                            else {
                                const uint32_t b1 = gpl_lds32(tile, o + 4 + a.b0_bytes) & m1;
                                const uint32_t f = sort_table_find(a.ctab_key, a.ctab_val, a.ctab_mask, (uint64_t)sample << 32 | b1);
                                if (f == kSortNoRank) ++n_uncorr;
                                else { cell = f; len = H + A * nfit; ++n_kept; aln_kept += nfit; }   // (len <= the record's own length < 2^32)
                            }
                        } else {
                            uint64_t bc = gpl_lds32(tile, o + 4);
                            if (a.bc_bytes == 8) bc |= (uint64_t)gpl_lds32(tile, o + 8) << 32;
                            else if (a.bc_bytes < 4) bc &= (1u << (8 * a.bc_bytes)) - 1u;
                            const uint32_t f = collate_find(a, bc);
                            if (f == kSortNoRank) ++n_uncorr;
                            else { cell = f; len = H + A * nfit; ++n_kept; aln_kept += nfit; }   // (len <= the record's own length < 2^32)
                        }
                    }
                    a.rec[slot] = make_uint2(cell, len);
                    a.key[slot] = ((uint64_t)cell << 32) | slot;
                }
            } else {
                uint32_t cell = a.n_cells, nk = 0;
                uint64_t d = 0;
                if (live) {
                    const uint2 rc = a.rec[slot];
                    cell = rc.x;
                    if (cell != a.n_cells) { nk = (rc.y - H) / A; d = a.dest[slot]; }
                }
                const bool kept = cell != a.n_cells;
                if (kept) {   // the head, and the alignments of a record whose list the halo holds
                    ByteOut w{a.out + d, 0, 0};
                    uint64_t umi;
                    if constexpr (M) {   // (each side as it stood as a kernel of its own, the order of load and first put included: the multi write walk's code moves otherwise)
                        const uint64_t ch = a.cell_head[cell];   // the sample's ordinal << 32 | the corrected cell barcode
                        w.put(nk, 4);
                        w.put((uint32_t)(ch >> 32), a.b0_bytes);
                        w.put((uint32_t)ch, a.b1_bytes);
                        umi = gpl_lds32(tile, o + 4 + a.b0_bytes + a.b1_bytes);
                        if (a.umi_bytes == 8) umi |= (uint64_t)gpl_lds32(tile, o + 8 + a.b0_bytes + a.b1_bytes) << 32;
                    } else {
                        w.put(nk, 4);
                        w.put_field(a.cells[cell], a.bc_bytes);
                        umi = gpl_lds32(tile, o + 4 + a.bc_bytes);
                        if (a.umi_bytes == 8) umi |= (uint64_t)gpl_lds32(tile, o + 8 + a.bc_bytes) << 32;
                    }
                    w.put_field(umi, a.umi_bytes);
                    if (!is_long)
                        for (uint32_t j = 0; j < na; ++j) {
                            const uint32_t ao = o + H + A * j, word = gpl_lds32(tile, ao);
                            if (both || gpl_word_fits(word, a.expected_ori)) { w.put(word, 4); put_extra_lds(w, tile, ao + 4, a.aln_extra); }
                        }
                    w.flush();
                }
                uint64_t pend = __ballot(is_long && kept);
                while (pend) {   // (uniform)
                    const int src = __ffsll((long long)pend) - 1;
                    pend &= pend - 1;
                    const uint32_t lna = __shfl(na, src), lro = __shfl(ro, src);
                    const uint64_t ld = ((uint64_t)__shfl((uint32_t)(d >> 32), src) << 32) | __shfl((uint32_t)d, src);
                    const uint64_t first = c.chunk_off + p + lro + H;
                    uint32_t base = 0;   // fitting alignments in front of this trip
                    for (uint32_t j0 = 0; j0 < lna; j0 += 64) {
                        const uint32_t j = j0 + lane;
                        const uint64_t ga = first + (uint64_t)A * j;
                        const uint32_t word = j < lna ? gpl_ld_u32(a.bytes, a.n_bytes, ga) : 0u;
                        const bool h = j < lna && (both || gpl_word_fits(word, a.expected_ori));
                        const uint64_t m = __ballot(h);
                        if (h) {   // (base + rank < nk: measure counted the same words)
                            ByteOut w{a.out + ld + H + (uint64_t)A * (base + (uint32_t)__popcll(m & lt)), 0, 0};
                            w.put(word, 4);
                            put_extra_glb(w, a.bytes, a.n_bytes, ga + 4, a.aln_extra);
                            w.flush();
                        }
                        base += (uint32_t)__popcll(m);
                    }
                }
            }
        }
        seen += nr;
        p += q;
        gpl_wave_lds_sync();   // (the next trip overwrites the tile)
    }
    if (!bad && (p != nb || seen != c.nrec)) bad = true;
    if (bad && lane == 0) set_err(a.st, kErrRecordWalk, chunk);
    if constexpr (!WRITE) {
        for (int d = 32; d; d >>= 1) {
            n_compat += __shfl_xor(n_compat, d);
            if constexpr (M) n_unrouted += __shfl_xor(n_unrouted, d);
            n_uncorr += __shfl_xor(n_uncorr, d); n_kept += __shfl_xor(n_kept, d);
            aln_in += __shfl_xor(aln_in, d); aln_kept += __shfl_xor(aln_kept, d); n_long += __shfl_xor(n_long, d);
        }
        if (lane == 0) {
            uint32_t* s = a.chunk_stat + 8ull * chunk;
            if constexpr (M) { s[0] = seen; s[1] = n_compat; s[2] = n_unrouted; s[3] = n_uncorr; s[4] = n_kept; s[5] = aln_in; s[6] = aln_kept; s[7] = n_long; }
            else { s[0] = seen; s[1] = n_compat; s[2] = n_uncorr; s[3] = n_kept; s[4] = aln_in; s[5] = aln_kept; s[6] = n_long; s[7] = 0; }
        }
    }
}

// ---- placement
// exclusive scan of one value per thread over the workgroup, any unsigned width (Hillis-Steele in LDS)
template <typename T>
__device__ __forceinline__ T collate_block_scan(T v, T* s, T& total) {
    const uint32_t t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kCollateRadixNT; d <<= 1) {
        const T x = t >= d ? s[t - d] : (T)0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    total = s[kCollateRadixNT - 1];
    const T r = s[t] - v;
    __syncthreads();
    return r;
}

// in-place exclusive scan of n values by ONE workgroup (the digit counts of a radix pass; the workgroups' length sums): 4 096
// values a trip, a thread's sixteen in registers; 32-bit values take the shuffle scan of afq_prims.h (two barriers a trip)
constexpr uint32_t kScan1Items = 16;
template <typename T>
__global__ __launch_bounds__(kCollateRadixNT) void k_collate_scan1(T* v, uint64_t n) {
    __shared__ T s[sizeof(T) == 4 ? kCollateRadixNT / 64 : kCollateRadixNT];
    T carry = 0;
    for (uint64_t b0 = 0; b0 < n; b0 += (uint64_t)kCollateRadixNT * kScan1Items) {   // (uniform)
        const uint64_t i0 = b0 + (uint64_t)threadIdx.x * kScan1Items;
        T x[kScan1Items], mine = 0;
#pragma unroll
        for (uint32_t j = 0; j < kScan1Items; ++j) { x[j] = i0 + j < n ? v[i0 + j] : (T)0; mine += x[j]; }
        T tot, ex;
        if constexpr (sizeof(T) == 4) ex = block_excl_scan<(int)kCollateRadixNT>(mine, s, tot);
        else ex = collate_block_scan<T>(mine, s, tot);
        ex += carry;
#pragma unroll
        for (uint32_t j = 0; j < kScan1Items; ++j) { if (i0 + j < n) v[i0 + j] = ex; ex += x[j]; }
        carry += tot;
    }
}

__global__ __launch_bounds__(kCollateRadixNT) void k_collate_radix_hist(const uint64_t* __restrict__ keys, uint32_t n, uint32_t shift, uint32_t* __restrict__ hist,
                                                                       uint32_t n_blocks) {
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i0 = (uint64_t)blockIdx.x * kCollateRadixBlock + threadIdx.x;
#pragma unroll
    for (uint32_t j = 0; j < kCollateRadixItems; ++j) {
        const uint64_t i = i0 + (uint64_t)j * kCollateRadixNT;
        if (i < n) atomicAdd(&s_h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * n_blocks + blockIdx.x] = s_h[threadIdx.x];
}

// keys of the workgroup go out in their input order within each digit: round by round, and inside a round by (wave, lane)
__global__ __launch_bounds__(kCollateRadixNT) void k_collate_radix_scatter(const uint64_t* __restrict__ keys, uint64_t* __restrict__ dst, uint32_t n, uint32_t shift,
                                                                          const uint32_t* __restrict__ hist, uint32_t n_blocks) {
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_wc[kCollateRadixNT / 64][256];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    s_base[t] = hist[(uint64_t)t * n_blocks + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < kCollateRadixNT / 64; ++w) s_wc[w][t] = 0;
    __syncthreads();
    const uint64_t i0 = (uint64_t)blockIdx.x * kCollateRadixBlock + t;
    for (uint32_t j = 0; j < kCollateRadixItems; ++j) {
        const uint64_t i = i0 + (uint64_t)j * kCollateRadixNT;
        const bool live = i < n;
        const uint64_t k = live ? keys[i] : 0ull;
        const uint32_t dg = (uint32_t)(k >> shift) & 255u;
        uint64_t peers = __ballot(live);   // the live lanes of the wave with this lane's digit
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const bool bit = (dg >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (live && rank == 0) s_wc[wave][dg] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (live) {
            uint32_t pos = s_base[dg] + rank;
            for (uint32_t w = 0; w < wave; ++w) pos += s_wc[w][dg];
            dst[pos] = k;   // (pos < n: the counts are this pass's own)
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (uint32_t w = 0; w < kCollateRadixNT / 64; ++w) { add += s_wc[w][t]; s_wc[w][t] = 0; }
        s_base[t] += add;
        __syncthreads();
    }
}

// the record lengths in sorted order: a workgroup's sum, then (after the one-workgroup scan of the sums) every position's prefix
__global__ __launch_bounds__(kCollateRadixNT) void k_collate_len_sum(const uint64_t* __restrict__ sorted, const uint2* __restrict__ rec, uint32_t n,
                                                                    uint64_t* __restrict__ block_sum) {
    __shared__ uint64_t s[kCollateRadixNT];
    const uint64_t i0 = (uint64_t)blockIdx.x * kCollateScanBlock + (uint64_t)threadIdx.x * kCollateScanItems;
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kCollateScanItems; ++j)
        if (i0 + j < n) mine += rec[(uint32_t)sorted[i0 + j]].y;
    uint64_t tot;
    (void)collate_block_scan<uint64_t>(mine, s, tot);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(kCollateRadixNT) void k_collate_dest(const uint64_t* __restrict__ sorted, const uint2* __restrict__ rec, uint32_t n,
                                                                 const uint64_t* __restrict__ block_sum, uint64_t* __restrict__ ex, uint64_t* __restrict__ dest) {
    __shared__ uint64_t s[kCollateRadixNT];
    const uint64_t i0 = (uint64_t)blockIdx.x * kCollateScanBlock + (uint64_t)threadIdx.x * kCollateScanItems;
    uint64_t key[kCollateScanItems];
    uint32_t len[kCollateScanItems];
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kCollateScanItems; ++j) {
        key[j] = 0; len[j] = 0;
        if (i0 + j < n) { key[j] = sorted[i0 + j]; len[j] = rec[(uint32_t)key[j]].y; }
        mine += len[j];
    }
    uint64_t tot;
    uint64_t e = block_sum[blockIdx.x] + collate_block_scan<uint64_t>(mine, s, tot);
#pragma unroll
    for (uint32_t j = 0; j < kCollateScanItems; ++j) {
        if (i0 + j < n) {
            ex[i0 + j] = e;
            dest[(uint32_t)key[j]] = 8ull * ((key[j] >> 32) + 1ull) + e;   // (a dropped record's is never read)
            if (i0 + j + 1 == n) ex[n] = e + len[j];
        }
        e += len[j];
    }
}

__device__ __forceinline__ uint32_t collate_lower_bound(const uint64_t* a, uint32_t n, uint64_t x) {   // first i with a[i] >= x
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
__global__ __launch_bounds__(256) void k_collate_heads(const uint64_t* __restrict__ sorted, uint32_t n, const uint64_t* __restrict__ ex, uint32_t n_cells,
                                                      uint64_t* __restrict__ off, uint32_t* __restrict__ nrec, uint8_t* __restrict__ out, DevStatus* __restrict__ st) {
    const uint64_t cidx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (cidx > n_cells) return;
    const uint32_t lo = collate_lower_bound(sorted, n, cidx << 32);
    const uint64_t o = 8ull * cidx + ex[lo];
    off[cidx] = o;   // (cidx == n_cells: the dropped records carry no bytes, so this is the end of the last chunk)
    if (cidx == n_cells) return;
    const uint32_t hi = collate_lower_bound(sorted, n, (cidx + 1) << 32);
    const uint64_t nbytes = 8ull + (ex[hi] - ex[lo]);
    nrec[cidx] = hi - lo;
    if (nbytes >= (1ull << 32)) { set_err(st, kErrCollateChunk, (uint32_t)cidx); return; }
    ByteOut w{out + o, 0, 0};
    w.put((uint32_t)nbytes, 4);
    w.put(hi - lo, 4);
    w.flush();
}

}  // namespace

void launch_collate_measure(hipStream_t s, const CollateArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH((k_collate_walk<false, CollateArgs>), (a.n_chunks + kWalkWaves - 1) / kWalkWaves, kWalkNT, s, a);
}
void launch_collate_write(hipStream_t s, const CollateArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH((k_collate_walk<true, CollateArgs>), (a.n_chunks + kWalkWaves - 1) / kWalkWaves, kWalkNT, s, a);
}
void launch_collate_multi_measure(hipStream_t s, const CollateMultiArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH((k_collate_walk<false, CollateMultiArgs>), (a.n_chunks + kWalkWaves - 1) / kWalkWaves, kWalkNT, s, a);
}
void launch_collate_multi_write(hipStream_t s, const CollateMultiArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH((k_collate_walk<true, CollateMultiArgs>), (a.n_chunks + kWalkWaves - 1) / kWalkWaves, kWalkNT, s, a);
}

void launch_collate_radix_pass(hipStream_t s, const uint64_t* src, uint64_t* dst, uint32_t n, uint32_t shift, uint32_t* hist) {
    if (!n) return;
    const uint32_t nb = (uint32_t)(((uint64_t)n + kCollateRadixBlock - 1) / kCollateRadixBlock);
    AFQ_LAUNCH(k_collate_radix_hist, nb, kCollateRadixNT, s, src, n, shift, hist, nb);
    AFQ_LAUNCH(k_collate_scan1<uint32_t>, 1, kCollateRadixNT, s, hist, 256ull * nb);
    AFQ_LAUNCH(k_collate_radix_scatter, nb, kCollateRadixNT, s, src, dst, n, shift, hist, nb);
}

void launch_collate_excl_scan_u32(hipStream_t s, uint32_t* v, uint64_t n) {
    if (!n) return;
    AFQ_LAUNCH(k_collate_scan1<uint32_t>, 1, kCollateRadixNT, s, v, n);
}

void launch_collate_scan(hipStream_t s, const uint64_t* sorted, const uint2* rec, uint32_t n, uint64_t* block_sum, uint64_t* ex, uint64_t* dest) {
    if (!n) return;   // (the caller zeroes ex[0])
    const uint32_t nb = (uint32_t)(((uint64_t)n + kCollateScanBlock - 1) / kCollateScanBlock);
    AFQ_LAUNCH(k_collate_len_sum, nb, kCollateRadixNT, s, sorted, rec, n, block_sum);
    AFQ_LAUNCH(k_collate_scan1<uint64_t>, 1, kCollateRadixNT, s, block_sum, (uint64_t)nb);
    AFQ_LAUNCH(k_collate_dest, nb, kCollateRadixNT, s, sorted, rec, n, block_sum, ex, dest);
}

void launch_collate_heads(hipStream_t s, const uint64_t* sorted, uint32_t n, const uint64_t* ex, uint32_t n_cells, uint64_t* off, uint32_t* nrec, uint8_t* out,
                          DevStatus* st) {
    AFQ_LAUNCH(k_collate_heads, (uint32_t)(((uint64_t)n_cells + 1 + 255) / 256), 256, s, sorted, n, ex, n_cells, off, nrec, out, st);
}

}  // namespace afq
