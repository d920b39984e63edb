// afq_collate_multi.hip — the device half of multi-barcode `collate` (do_collate_multi_bc_fast, src/collate.rs:1415-1920 of the
// reference): the records `na, b0, b1, umi, alignments` of an UNCOLLATED two-barcode RNA RAD, filtered by orientation, routed to
// a sample by b0, corrected to a cell of that sample by b1, and written as one chunk per cell in a given cell order with b0 = the
// sample's ordinal and b1 = the corrected cell barcode.
//
// The two walks are k_collate_walk's (afq_collate.hip), as ONE kernel template over another head, so that measure and write
// cannot disagree about where a record lies: a wave per chunk, tile and halo in LDS, the na hop, a lane per record, the whole wave
// for a record with more than kGplLaneAlns alignments.  What differs is the lookup, which has two levels:
//   - the sample table: observed b0 -> sample index (a few thousand entries at most; it stays in cache).  The lane starts this
//     probe beside the read of na, before the alignment words are counted, as k_gpl_multi_parse does;
//   - the cell table: sample << 32 | b1 -> the index of the corrected barcode among the cells.  It depends on the first probe's
//     result.  b1 has at most 4 bytes and a sample index is below 2^31, so no key is the all-ones free mark.
// Both tables are launch_sort_table's.  Measure writes (cell, len) and the sort word cell << 32 | slot into the record's own slot;
// placement, the length scan and the chunk heads are collate's kernels unchanged (launch_collate_radix_pass, launch_collate_scan,
// launch_collate_heads), so the layout is the scan and the output a function of the input alone.  Write stores through ByteOut,
// which never reads the output: neighbouring records share dwords across waves.
#include <hip/hip_runtime.h>

#include "afq_common.h"
#include "afq_kernels.h"
#include "afq_prims.h"
#include "afq_rad_walk.h"

namespace afq {

namespace {

constexpr int kWalkNT = 256;
constexpr uint32_t kWalkWaves = kWalkNT / 64;
static_assert(kGplParseHalo >= (4 + 4 + 4 + 8) + (4 + 8) * kGplLaneAlns, "the halo holds the widest head (na, b0, b1, umi) and kGplLaneAlns of the widest alignments");
static_assert(kRadWalkTileRecs >= kGplParseTile / (4 + 1 + 1 + 1) + 1, "a start slot for every record of a tile of the shortest records");

__device__ __forceinline__ uint32_t multi_find(const uint64_t* __restrict__ tab_key, const uint32_t* __restrict__ tab_val, uint32_t mask, uint64_t k) {
    uint32_t slot = sort_hash_bc(k) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {   // (at most half the slots are taken: an empty one ends the probe)
        const uint64_t kk = tab_key[slot];
        if (kk == k) return tab_val[slot];
        if (kk == kSortEmptyKey) return kSortNoRank;
        slot = (slot + 1) & mask;
    }
    return kSortNoRank;
}

template <bool WRITE>
__global__ __launch_bounds__(kWalkNT) void k_collate_multi_walk(CollateMultiArgs a) {
    __shared__ uint32_t s_tile[kWalkWaves][kRadWalkTileWords];
    __shared__ uint16_t s_start[kWalkWaves][kRadWalkTileRecs];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t chunk = blockIdx.x * kWalkWaves + wave;
    if (chunk >= a.n_chunks) return;   // (no workgroup barrier below: the waves of a block run chunks of different lengths)
    const SortChunk c = a.chunks[chunk];
    const uint32_t nb = c.nbytes, H = 4 + a.b0_bytes + a.b1_bytes + a.umi_bytes, A = 4 + a.aln_extra;   // the host checked 8 <= nb and chunk_off + nb <= n_bytes
    const uint32_t m0 = a.b0_bytes < 4 ? (1u << (8 * a.b0_bytes)) - 1u : ~0u, m1 = a.b1_bytes < 4 ? (1u << (8 * a.b1_bytes)) - 1u : ~0u;
    const bool both = a.expected_ori == kGplOriBoth;
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t* tile = s_tile[wave];
    uint16_t* starts = s_start[wave];
    uint32_t p = 8, seen = 0;                                          // wave-uniform
    uint32_t n_compat = 0, n_unrouted = 0, n_uncorr = 0, n_kept = 0, aln_in = 0, aln_kept = 0, n_long = 0;   // per lane (a chunk is below 4 GiB: no sum wraps)
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
                uint32_t nfit = 0, sample = kSortNoRank;
                if (live) {
                    sample = multi_find(a.stab_key, a.stab_val, a.stab_mask, gpl_lds32(tile, o + 4) & m0);   // (its loads fly while the alignment words are read)
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
                        if (sample == kSortNoRank) ++n_unrouted;
                        else {
                            const uint32_t b1 = gpl_lds32(tile, o + 4 + a.b0_bytes) & m1;
                            const uint32_t f = multi_find(a.ctab_key, a.ctab_val, a.ctab_mask, (uint64_t)sample << 32 | b1);
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
                    const uint64_t ch = a.cell_head[cell];   // the sample's ordinal << 32 | the corrected cell barcode
                    w.put(nk, 4);
                    w.put((uint32_t)(ch >> 32), a.b0_bytes);
                    w.put((uint32_t)ch, a.b1_bytes);
                    uint64_t umi = gpl_lds32(tile, o + 4 + a.b0_bytes + a.b1_bytes);
                    if (a.umi_bytes == 8) umi |= (uint64_t)gpl_lds32(tile, o + 8 + a.b0_bytes + a.b1_bytes) << 32;
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
            n_compat += __shfl_xor(n_compat, d); n_unrouted += __shfl_xor(n_unrouted, d); n_uncorr += __shfl_xor(n_uncorr, d); n_kept += __shfl_xor(n_kept, d);
            aln_in += __shfl_xor(aln_in, d); aln_kept += __shfl_xor(aln_kept, d); n_long += __shfl_xor(n_long, d);
        }
        if (lane == 0) {
            uint32_t* s = a.chunk_stat + 8ull * chunk;
            s[0] = seen; s[1] = n_compat; s[2] = n_unrouted; s[3] = n_uncorr; s[4] = n_kept; s[5] = aln_in; s[6] = aln_kept; s[7] = n_long;
        }
    }
}

}  // namespace

void launch_collate_multi_measure(hipStream_t s, const CollateMultiArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH(k_collate_multi_walk<false>, (a.n_chunks + kWalkWaves - 1) / kWalkWaves, kWalkNT, s, a);
}
void launch_collate_multi_write(hipStream_t s, const CollateMultiArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH(k_collate_multi_walk<true>, (a.n_chunks + kWalkWaves - 1) / kWalkWaves, kWalkNT, s, a);
}

}  // namespace afq
