// afq_atac_gpl.hip — the device half of `atac generate-permit-list` (update_barcode_hist_unfiltered, src/atac/cellfilter.rs:68-103
// of the reference): ONE walk of an uncollated scATAC RAD that yields the barcode of every record, the largest na, and the
// position-bin histogram of the records with exactly one alignment.
//
// The walk is k_sort_parse's (afq_atac_sort.hip): a wave owns a chunk and stages it through LDS a tile at a time, a tile BEGINS
// at a record start, the record starts inside it are found by hopping the na fields in LDS (wave-uniform), then a lane per
// record.  Unlike the sort parse EVERY record is kept - a record without an alignment still counts its barcode - so the head is
// read for every record and record r of a trip goes to slot out_off + seen + r: no ballot, no empty mark.  The barcode column
// then goes through the counting table of afq_gpl.hip (k_gpl_count / k_gpl_compact) as it stands.
//
// Bins.  A record with one alignment adds 1 to  bin_base[ref] + start_pos / bin_size.  The reference tests no position against
// its reference's length, so a position past the reference's bins counts in the next reference's; only an index past ALL bins
// (where the reference panics) is an error here.  The counters are u32 words in HBM that every workgroup shares, bumped with
// one global atomic a record, as level 0 of the sort's partition counts its bins (k_sort_hist): a genome has ~31 000 bins, a
// mapper's chunk holds reads in sequencing order, so the 64 records of a trip fall into 64 unrelated bins, and a workgroup's four
// chunks put fewer than one record into each counter of an LDS-private histogram (124 KB: one workgroup a CU instead of seven),
// whose flush would then cost what the records' own atomics cost (with the measured time).  A call holds fewer than
// 2^30 records, so a u32 counter cannot wrap; k_atac_gpl_bins widens them.
#include <hip/hip_runtime.h>

#include "afq_common.h"
#include "afq_kernels.h"
#include "afq_prims.h"
#include "afq_rad_walk.h"

namespace afq {

namespace {

constexpr int kAtacGplNT = 256;
constexpr uint32_t kAtacGplWaves = kAtacGplNT / 64;
constexpr uint32_t kAtacGplTileWords = (3 + kSortParseTile + kSortParseHalo + 3) / 4 + 1;   // (+ the dword an unaligned 4-byte read of the last bytes also touches)
constexpr uint32_t kAtacGplTileRecs = kSortParseTile / 5 + 1;   // the shortest record is na = 0 with a 1-byte barcode
static_assert(kSortParseHalo >= 4 + 8 + 9, "the halo holds the widest head and the ref, type and start_pos of one alignment");

__global__ __launch_bounds__(kAtacGplNT) void k_atac_gpl_parse(AtacGplParseArgs a) {
    __shared__ uint32_t s_tile[kAtacGplWaves][kAtacGplTileWords];
    __shared__ uint16_t s_start[kAtacGplWaves][kAtacGplTileRecs];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t chunk = blockIdx.x * kAtacGplWaves + wave;
    if (chunk >= a.n_chunks) return;   // (no workgroup barrier below: the waves of a block run chunks of different lengths)
    const SortChunk c = a.chunks[chunk];
    const uint32_t nb = c.nbytes, H = 4 + a.bc_bytes;   // the host checked 8 <= nb and chunk_off + nb <= n_bytes
    uint32_t* tile = s_tile[wave];
    uint16_t* starts = s_start[wave];
    uint32_t p = 8, seen = 0;                    // wave-uniform
    uint32_t n0 = 0, multi = 0, max_na = 0;      // per lane
    uint32_t err = 0;                            // per lane: a field out of range
    bool bad = false;                            // uniform: the records do not tile the chunk
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
            if (nb - (p + q) < H) { bad = true; break; }             // a head that runs past the chunk
            const uint32_t na = gpl_lds32(tile, al + q);
            if (na > (nb - (p + q) - H) / 11u) { bad = true; break; }   // alignments that run past the chunk
            if (lane == 0) starts[nr] = (uint16_t)q;
            ++nr;
            q += H + 11u * na;   // (<= nb - p: no wrap)
        }
        if (bad) break;
        if (seen + nr > c.nrec) { bad = true; break; }               // more records than the header says
        gpl_wave_lds_sync();
        for (uint32_t r = lane; r < nr; r += 64) {
            const uint32_t o = al + starts[r];
            const uint32_t na = gpl_lds32(tile, o);
            uint64_t bc = gpl_lds32(tile, o + 4);   // (the hop checked that the head lies inside the chunk; it lies inside the halo)
            if (a.bc_bytes == 8) bc |= (uint64_t)gpl_lds32(tile, o + 8) << 32;
            else if (a.bc_bytes < 4) bc &= (1u << (8 * a.bc_bytes)) - 1u;
            a.o_bc[c.out_off + seen + r] = bc;      // (seen + nr <= nrec, so the slot is one of the chunk's)
            max_na = na > max_na ? na : max_na;
            if (na == 0) ++n0;
            else if (na > 1) ++multi;
            else {   // (the hop checked that the alignment's 11 bytes lie inside the chunk; ref and start_pos lie inside the halo)
                const uint32_t ref = gpl_lds32(tile, o + H), start = gpl_lds32(tile, o + H + 5);
                if (ref >= a.ref_count) err = kErrRefRange;   // (the smaller code of the two: it stays)
                else {
                    const uint64_t bin = (uint64_t)a.bin_base[ref] + start / a.bin_size;
                    if (bin >= a.n_bins) err = err ? err : kErrStartRange;
                    else atomicAdd(a.bins + bin, 1u);
                }
            }
        }
        seen += nr;
        p += q;
        gpl_wave_lds_sync();   // (the next trip overwrites the tile)
    }
    if (!bad && (p != nb || seen != c.nrec)) bad = true;
    uint32_t e = bad ? kErrRecordWalk : err;
    for (int d = 32; d; d >>= 1) {
        const uint32_t o = __shfl_xor(e, d);
        if (e == 0 || (o != 0 && o < e)) e = o;   // (any lane's error; the smallest code, so that the message does not depend on the lane)
        n0 += __shfl_xor(n0, d); multi += __shfl_xor(multi, d);
        const uint32_t m = __shfl_xor(max_na, d);
        max_na = m > max_na ? m : max_na;
    }
    if (e && lane == 0) set_err(a.st, e, chunk);
    if (lane == 0) {   // ([1] is what k_gpl_count takes from a chunk's slots: all of them, none of a refused chunk)
        uint32_t* s = a.chunk_stat + 4ull * chunk;
        s[0] = n0; s[1] = e ? 0u : seen; s[2] = max_na; s[3] = multi;
    }
}

// the largest counter, and the counters widened to u64
__global__ __launch_bounds__(256) void k_atac_gpl_bins(const uint32_t* __restrict__ bins, uint32_t n_bins, uint64_t* __restrict__ o_bins,
                                                      uint32_t* __restrict__ o_max) {
    uint32_t m = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_bins; i += gridDim.x * 256) {
        const uint32_t v = bins[i];
        o_bins[i] = v;
        m = v > m ? v : m;
    }
    for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(m, d); m = o > m ? o : m; }
    if ((threadIdx.x & 63u) == 0 && m) atomicMax(o_max, m);
}

}  // namespace

void launch_atac_gpl_parse(hipStream_t s, const AtacGplParseArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH(k_atac_gpl_parse, (a.n_chunks + kAtacGplWaves - 1) / kAtacGplWaves, kAtacGplNT, s, a);
}

void launch_atac_gpl_bins(hipStream_t s, const uint32_t* bins, uint32_t n_bins, uint64_t* o_bins, uint32_t* o_max) {
    if (!n_bins) return;
    const uint32_t grid = (n_bins + 255) / 256;
    AFQ_LAUNCH(k_atac_gpl_bins, grid < 1024 ? grid : 1024, 256, s, bins, n_bins, o_bins, o_max);
}

}  // namespace afq
