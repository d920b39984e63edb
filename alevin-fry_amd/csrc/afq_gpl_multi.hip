// afq_gpl_multi.hip — the device half of multi-barcode `generate-permit-list` (do_generate_permit_list_multi_bc, src/cellfilter.rs
// of the reference): the (routing entry, cell barcode) histogram of an UNCOLLATED two-barcode RNA RAD.
//
// k_gpl_multi_parse walks a mapper chunk exactly as k_gpl_parse does (rad_walk_chunk, afq_rad_walk.h, restates that walk as a
// template: a wave per chunk, tile and halo in LDS, the na hop, the lane route and the whole-wave route to the orientation test).  A record is `na, b0, b1, umi,
// alignments`; a record's lane looks b0 up in the table of routing entries (open addressing in global memory,
// built by k_sort_table_insert / k_sort_table_verify of afq_atac_sort.hip: a few thousand entries, it stays in cache).  A hit at
// entry e puts the key e << 32 | b1 into the chunk's own slots, filled from the front by ballot; a miss counts as unrouted.  The
// device knows nothing of samples, rotations, aliases or deferral: the host derives them from the entry index.  An entry index is
// below 2^31, so no key is all-ones and the counting table's free mark (k_gpl_count, afq_gpl.hip) never meets a key; counting and
// compaction are k_gpl_count / k_gpl_compact unchanged, and the host sorts the pairs.
#include <hip/hip_runtime.h>

#include "afq_common.h"
#include "afq_kernels.h"
#include "afq_prims.h"
#include "afq_rad_walk.h"

namespace afq {

namespace {

constexpr int kGplMultiNT = 256;
constexpr uint32_t kGplMultiWaves = kGplMultiNT / 64;
static_assert(kGplParseHalo >= (4 + 4 + 4 + 8) + (4 + 8) * kGplLaneAlns, "the halo holds the widest head (na, b0, b1, umi) and kGplLaneAlns of the widest alignments");
static_assert(kRadWalkTileRecs >= kGplParseTile / (4 + 1 + 1 + 1) + 1, "a start slot for every record of a tile of the shortest records");

struct GplMultiHead { uint32_t entry, b1; };   // what a lane keeps of its record's head: b0's index among the entries (kGplNoTarget: none), b1

static_assert(kGplNoTarget == kSortNoRank, "sort_table_find's no-entry mark is this pass's");

__global__ __launch_bounds__(kGplMultiNT) void k_gpl_multi_parse(GplMultiParseArgs a) {
    __shared__ uint32_t s_tile[kGplMultiWaves][kRadWalkTileWords];
    __shared__ uint16_t s_start[kGplMultiWaves][kRadWalkTileRecs];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t chunk = blockIdx.x * kGplMultiWaves + wave;
    if (chunk >= a.n_chunks) return;   // (no workgroup barrier below: the waves of a block run chunks of different lengths)
    const SortChunk c = a.chunks[chunk];
    const uint32_t* tile = s_tile[wave];
    const uint32_t m0 = a.b0_bytes < 4 ? (1u << (8 * a.b0_bytes)) - 1u : ~0u, m1 = a.b1_bytes < 4 ? (1u << (8 * a.b1_bytes)) - 1u : ~0u;
    uint32_t seen = 0, routed = 0, unrouted = 0, n_long = 0;   // wave-uniform
    const bool ok = rad_walk_chunk(a.bytes, a.n_bytes, c, 4 + a.b0_bytes + a.b1_bytes + a.umi_bytes, 4 + a.aln_extra, a.expected_ori, s_tile[wave], s_start[wave], lane,
                                   seen, n_long,
                                   [&](uint32_t o) {   // (the probe starts before the orientation test: its loads fly while the alignment words are read)
        return GplMultiHead{sort_table_find(a.tab_key, a.tab_val, a.tab_mask, gpl_lds32(tile, o + 4) & m0), gpl_lds32(tile, o + 4 + a.b0_bytes) & m1};
    },
                                   [&](const GplMultiHead& h, uint32_t, bool keep) {
        const bool route = keep && h.entry != kGplNoTarget;
        const uint64_t mk = __ballot(keep), mr = __ballot(route);
        if (route)   // (routed <= seen + the batch <= nrec: the slot is one of the chunk's)
            a.o_key[c.out_off + routed + (uint32_t)__popcll(mr & ((1ull << lane) - 1ull))] = (uint64_t)h.entry << 32 | h.b1;
        routed += (uint32_t)__popcll(mr);
        unrouted += (uint32_t)__popcll(mk & ~mr);
    });
    if (!ok) { routed = 0; unrouted = 0; if (lane == 0) set_err(a.st, kErrRecordWalk, chunk); }
    if (lane == 0) {
        uint32_t* s = a.chunk_stat + 4ull * chunk;
        s[0] = seen; s[1] = routed; s[2] = unrouted; s[3] = n_long;
    }
}

}  // namespace

void launch_gpl_multi_parse(hipStream_t s, const GplMultiParseArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH(k_gpl_multi_parse, (a.n_chunks + kGplMultiWaves - 1) / kGplMultiWaves, kGplMultiNT, s, a);
}

}  // namespace afq
