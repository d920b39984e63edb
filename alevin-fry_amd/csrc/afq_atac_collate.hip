// afq_atac_collate.hip — the device half of `atac collate` (src/atac/collate.rs of the reference): the records of an UNCOLLATED
// scATAC RAD that have exactly one alignment and a barcode of the correction map, barcode-corrected, written as one chunk per cell
// that received a record, in a given cell order.  A cell that receives nothing has no chunk.
//
// The input is walked twice, as k_sort_parse walks it (afq_atac_sort.hip): a wave owns a chunk and stages it through LDS a tile at
// a time, a tile begins at a record start, the record starts are found by hopping the na fields (wave-uniform), then a lane takes
// a record.  A record with na > 1 is hopped over however long it is: the hop leaves the tile, and the next tile begins behind it.
// Both walks are ONE kernel template, so that they cannot disagree about where a record lies:
//   - measure: the lane of a record with na == 1 probes the correction table and writes the record's cell and the sort word
//     cell << 32 | slot  into the record's own slot - the chunk table's prefix + the record's index, so the slots are in input
//     order by construction.  A dropped record carries the cell n_cells.
//   - placement: collate's stable LSD radix passes over the cell bits (afq_collate.hip) give (cell, input order).  Every kept
//     record has R = 4 + bc_bytes + 11 bytes, so the sorted position IS the layout: a lane per cell finds its run by binary search,
//     the non-empty cells are numbered by an exclusive scan of their flags, and the record at sorted position i of the j-th
//     non-empty cell lies at  R i + 8 (j + 1).  No allocation atomics, so the output is a function of the input alone.
//   - write: the second walk; the lane of a kept record writes na = 1, the corrected barcode and the 11 alignment bytes as read.
//
// Stores.  R is 16, 17, 19 or 23: two records that are neighbours in the output share an aligned dword and different waves write
// them.  ByteOut (afq_rad_walk.h) stores only the bytes it was given and never reads the output.
#include <hip/hip_runtime.h>

#include "afq_common.h"
#include "afq_kernels.h"
#include "afq_prims.h"
#include "afq_rad_walk.h"

namespace afq {

namespace {

constexpr int kWalkNT = 256;
constexpr uint32_t kWalkWaves = kWalkNT / 64;
constexpr uint32_t kAln = 11;   // ref u32, type u8, start_pos u32, frag_len u16
constexpr uint32_t kTileWords = (3 + kSortParseTile + kSortParseHalo + 3) / 4 + 1;   // (+ the dword an unaligned 4-byte read of the last bytes also touches)
constexpr uint32_t kTileRecs = kSortParseTile / 5 + 1;   // the shortest record is na = 0 with a 1-byte barcode
static_assert(kSortParseHalo >= 4 + 8 + kAln + 1, "the halo holds the widest head, one alignment and the byte a 4-byte read of its last three also takes");

__device__ __forceinline__ uint32_t acollate_find(const AtacCollateArgs& a, uint64_t k) {
    if (k == kSortEmptyKey) return a.ones_cell;
    uint32_t slot = sort_hash_bc(k) & a.tab_mask;
    for (uint32_t probe = 0; probe <= a.tab_mask; ++probe) {   // (at most half the slots are taken: an empty one ends the probe)
        const uint64_t kk = a.tab_key[slot];
        if (kk == k) return a.tab_val[slot];
        if (kk == kSortEmptyKey) return kSortNoRank;
        slot = (slot + 1) & a.tab_mask;
    }
    return kSortNoRank;
}

template <bool WRITE>
__global__ __launch_bounds__(kWalkNT) void k_atac_collate_walk(AtacCollateArgs a) {
    __shared__ uint32_t s_tile[kWalkWaves][kTileWords];
    __shared__ uint16_t s_start[kWalkWaves][kTileRecs];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t chunk = blockIdx.x * kWalkWaves + wave;
    if (chunk >= a.n_chunks) return;   // (no workgroup barrier below: the waves of a block run chunks of different lengths)
    const SortChunk c = a.chunks[chunk];
    const uint32_t nb = c.nbytes, H = 4 + a.bc_bytes;   // the host checked 8 <= nb and chunk_off + nb <= n_bytes
    uint32_t* tile = s_tile[wave];
    uint16_t* starts = s_start[wave];
    uint32_t p = 8, seen = 0;                              // wave-uniform
    uint32_t n0 = 0, multi = 0, uncorr = 0, kept = 0;      // per lane (a chunk is below 4 GiB: no sum wraps)
    bool bad = false;                                      // uniform: the records do not tile the chunk
    while (p < nb && !bad) {
        // stage [p, p + tile + halo) of the chunk, as aligned dwords
        const uint32_t span = nb - p < kSortParseTile + kSortParseHalo ? nb - p : kSortParseTile + kSortParseHalo;
        const uint64_t g = c.chunk_off + p;
        const uint32_t al = (uint32_t)((reinterpret_cast<uintptr_t>(a.bytes) + g) & 3u);
        const uint32_t nw = (al + span + 3) >> 2;
        for (uint32_t i = lane; i < nw; i += 64) tile[i] = gpl_ld_dword_in(a.bytes, a.n_bytes, (int64_t)g - al + 4ll * i);
        gpl_wave_lds_sync();
        // hop the na chain: record starts q (relative to p) below the tile's end
        uint32_t q = 0, nr = 0;
        while (q < kSortParseTile && p + q < nb) {
            if (nb - (p + q) < H) { bad = true; break; }                 // a head that runs past the chunk
            const uint32_t na = gpl_lds32(tile, al + q);
            if (na > (nb - (p + q) - H) / kAln) { bad = true; break; }   // alignments that run past the chunk
            if (lane == 0) starts[nr] = (uint16_t)q;
            ++nr;
            q += H + kAln * na;   // (<= nb - p: no wrap; a long record carries q past the tile, and the next tile begins behind it)
        }
        if (bad) break;
        if (seen + nr > c.nrec) { bad = true; break; }                   // more records than the header says
        gpl_wave_lds_sync();
        for (uint32_t r0 = 0; r0 < nr; r0 += 64) {
            const uint32_t r = r0 + lane;
            if (r >= nr) continue;
            const uint64_t slot = c.out_off + seen + r;   // (seen + nr <= nrec, so the slot is one of the chunk's; below 2^32: the host checked)
            const uint32_t o = al + starts[r];
            if constexpr (!WRITE) {
                const uint32_t na = gpl_lds32(tile, o);
                uint32_t cell = a.n_cells;
                if (na == 0) ++n0;
                else if (na > 1) ++multi;
                else {
                    uint64_t bc = gpl_lds32(tile, o + 4);
                    if (a.bc_bytes == 8) bc |= (uint64_t)gpl_lds32(tile, o + 8) << 32;
                    else if (a.bc_bytes < 4) bc &= (1u << (8 * a.bc_bytes)) - 1u;
                    const uint32_t f = acollate_find(a, bc);
                    if (f == kSortNoRank) ++uncorr;
                    else { cell = f; ++kept; }
                }
                a.cell_of[slot] = cell;
                a.key[slot] = ((uint64_t)cell << 32) | slot;
            } else {
                const uint32_t cell = a.cell_of[slot];
                if (cell != a.n_cells) {   // (na == 1: the hop checked that the alignment lies inside the chunk; it lies inside the halo)
                    ByteOut w{a.out + a.dest[slot], 0, 0};
                    w.put(1u, 4);
                    w.put_field(a.cells[cell], a.bc_bytes);
                    w.put(gpl_lds32(tile, o + H), 4);
                    w.put(gpl_lds32(tile, o + H + 4), 4);
                    w.put(gpl_lds32(tile, o + H + 8), 3);
                    w.flush();
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
            n0 += __shfl_xor(n0, d); multi += __shfl_xor(multi, d); uncorr += __shfl_xor(uncorr, d); kept += __shfl_xor(kept, d);
        }
        if (lane == 0) {
            uint32_t* s = a.chunk_stat + 8ull * chunk;
            s[0] = seen; s[1] = n0; s[2] = multi; s[3] = uncorr; s[4] = kept; s[5] = 0; s[6] = 0; s[7] = 0;
        }
    }
}

// ---- placement
__device__ __forceinline__ uint32_t acollate_lower_bound(const uint64_t* a, uint32_t n, uint64_t x) {   // first i with a[i] >= x
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

__global__ __launch_bounds__(256) void k_atac_collate_runs(const uint64_t* __restrict__ sorted, uint32_t n, uint32_t n_cells, uint32_t* __restrict__ first,
                                                          uint32_t* __restrict__ flag) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > n_cells) return;
    const uint32_t lo = acollate_lower_bound(sorted, n, c << 32);
    first[c] = lo;   // (c == n_cells: where the dropped records begin = the number of kept ones)
    flag[c] = c < n_cells && lo < n && (sorted[lo] >> 32) == c;
}

__global__ __launch_bounds__(256) void k_atac_collate_heads(const uint32_t* __restrict__ first, const uint32_t* __restrict__ rank, uint32_t n_cells, uint32_t rec_bytes,
                                                           uint64_t* __restrict__ off, uint32_t* __restrict__ nrec, uint32_t* __restrict__ cell,
                                                           uint8_t* __restrict__ out, DevStatus* __restrict__ st) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > n_cells) return;
    const uint32_t j = rank[c];
    if (c == n_cells) { off[j] = (uint64_t)rec_bytes * first[c] + 8ull * j; return; }   // the end of the last chunk
    if (rank[c + 1] == j) return;                                                       // an empty cell: no chunk
    const uint32_t cnt = first[c + 1] - first[c];   // (the runs of the cells are adjacent)
    const uint64_t o = (uint64_t)rec_bytes * first[c] + 8ull * j, nbytes = 8ull + (uint64_t)rec_bytes * cnt;
    off[j] = o; nrec[j] = cnt; cell[j] = (uint32_t)c;
    if (nbytes >= (1ull << 32)) { set_err(st, kErrCollateChunk, (uint32_t)c); return; }
    ByteOut w{out + o, 0, 0};
    w.put((uint32_t)nbytes, 4);
    w.put(cnt, 4);
    w.flush();
}

__global__ __launch_bounds__(256) void k_atac_collate_dest(const uint64_t* __restrict__ sorted, uint32_t n, uint32_t n_cells, uint32_t rec_bytes,
                                                          const uint32_t* __restrict__ rank, uint64_t* __restrict__ dest) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = sorted[i];
    const uint32_t c = (uint32_t)(k >> 32);
    if (c >= n_cells) return;   // (a dropped record's is never read)
    dest[(uint32_t)k] = (uint64_t)rec_bytes * i + 8ull * (rank[c] + 1ull);
}

}  // namespace

void launch_atac_collate_measure(hipStream_t s, const AtacCollateArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH(k_atac_collate_walk<false>, (a.n_chunks + kWalkWaves - 1) / kWalkWaves, kWalkNT, s, a);
}
void launch_atac_collate_write(hipStream_t s, const AtacCollateArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH(k_atac_collate_walk<true>, (a.n_chunks + kWalkWaves - 1) / kWalkWaves, kWalkNT, s, a);
}

void launch_atac_collate_runs(hipStream_t s, const uint64_t* sorted, uint32_t n, uint32_t n_cells, uint32_t* first, uint32_t* flag) {
    AFQ_LAUNCH(k_atac_collate_runs, (uint32_t)(((uint64_t)n_cells + 1 + 255) / 256), 256, s, sorted, n, n_cells, first, flag);
}

void launch_atac_collate_heads(hipStream_t s, const uint64_t* sorted, uint32_t n, uint32_t n_cells, uint32_t rec_bytes, const uint32_t* first, const uint32_t* rank,
                               uint64_t* off, uint32_t* nrec, uint32_t* cell, uint64_t* dest, uint8_t* out, DevStatus* st) {
    AFQ_LAUNCH(k_atac_collate_heads, (uint32_t)(((uint64_t)n_cells + 1 + 255) / 256), 256, s, first, rank, n_cells, rec_bytes, off, nrec, cell, out, st);
    if (n) AFQ_LAUNCH(k_atac_collate_dest, (uint32_t)(((uint64_t)n + 255) / 256), 256, s, sorted, n, n_cells, rec_bytes, rank, dest);
}

}  // namespace afq
