// afq_kernels.h — host-callable launchers of the gfx950 kernels in afq_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "afq_common.h"
#include "afq_inflate_elem.h"

// the scattering decoder's tile: slabs per wave (four waves a tile) and the keys its LDS stage holds (measurement builds override them)
#ifndef AFQ_DTILE_SLABS
#define AFQ_DTILE_SLABS 4
#endif
#ifndef AFQ_DTILE_KEYS
#define AFQ_DTILE_KEYS 1536
#endif

namespace afq {

// The decoder a range takes.  run_range picks it once per range; the launchers switch on it, and who places the keys in their
// bucket slabs (k_scatter, or the scattering decoder with its spill counts and k_fix_slabs' recount) follows from it.
enum class DecodeRoute : uint32_t {
    Walk,          // k_decode alone, the sequential walk: chunks the caller placed at offsets that are no multiple of 4
    Keys,          // k_decode_keys: walk-free, a lane per dword (records of two or more alignments on average)
    Par,           // k_decode_par: walk-free, a lane per record; the general decoder of ranges with parsimony cells
    RecsPug,       // k_decode_recs, the instance that also emits the parsimony reads (short records)
    RecsScatter,   // k_decode_recs, the scattering instances (short records, no parsimony cell)
};
// walk_free: the (widened) chunks are dword aligned; has_pug: the range has parsimony cells; short_records: it averages fewer than two
// alignment words per record (or AFQ_TEST_DECODE says so).  Every walk-free route ends in k_decode's fix-up mode.
__host__ inline DecodeRoute decode_route(bool walk_free, bool has_pug, bool short_records) {
    if (!walk_free) return DecodeRoute::Walk;
    if (has_pug) return short_records ? DecodeRoute::RecsPug : DecodeRoute::Par;
    return short_records ? DecodeRoute::RecsScatter : DecodeRoute::Keys;
}

struct DecodeArgs {
    const uint8_t* bytes;
    size_t n_bytes;
    const CellMeta* meta;
    uint32_t n_cells;
    const uint32_t* t2g;
    uint32_t ref_count;
    uint32_t num_genes;
    uint64_t* keys0;
    uint32_t* cell_nkeys;
    uint64_t* bc_out;
    DevStatus* st;
    DecodeRoute route;
    // the walk-free routes: per-cell proof terms (k_decode's fix-up mode checks them) and the slab tables; unused on DecodeRoute::Walk
    const CellChk* chk;
    const uint32_t* slab_prefix;  // [n_cells+1] 1 KiB slabs per cell, prefix
    uint32_t* slab_cell;          // [n_slabs] device-filled: cell of each slab
    uint64_t* cell_bc;            // [n_cells] device-filled: barcode words of each cell's first record
    uint32_t n_slabs;
    PugOut pug;                   // PUG cells: per-read outputs (null pointers when the batch has none)
    uint32_t trivial;             // the batch has cells in `trivial` mode
    uint32_t* fix_list;           // [n_cells] cells whose walk-free proof failed (filled by k_verify_cells)
    // DecodeRoute::RecsScatter only (k_decode_recs with a bin count).  It places the keys of multi-bucket
    // cells straight into their bucket slabs (keys1, cursor) - keys0 then holds single-bucket cells' keys and the keys that found
    // their slab full - and the fix-up decode re-decodes every cell whose proof failed into keys0 for k_fix_slabs
    uint2* dtile;                 // [n_dtiles] device-filled (k_slab_setup): tile -> (cell, tile index inside the cell)
    uint32_t n_dtiles_lo;         // tiles of the kDecodeSplitBins instance (cells of <= kDecodeSplitBins or > kLdsBins buckets) ...
    uint32_t n_dtiles_hi;         // ... then those of the kLdsBins instance (kDecodeSplitBins < buckets <= kLdsBins)
    uint64_t* keys1;
    uint32_t* cursor;
    uint32_t* slab_ovf;
    uint32_t* spill;              // [n_cells] keys that found their slab full (kept at the front of the cell's keys0 region)
};
constexpr uint32_t kDecodeTileSlabsHost = 4 * AFQ_DTILE_SLABS;   // 1 KiB slabs per scattering-decoder tile (4 waves)
constexpr uint32_t kLdsBins = 2048;          // buckets per cell the LDS paths (k_scatter, the scattering decoder) can hold
#ifndef AFQ_DECODE_SPLIT_BINS
#define AFQ_DECODE_SPLIT_BINS 1024
#endif
constexpr uint32_t kDecodeSplitBins = AFQ_DECODE_SPLIT_BINS;   // cells of more buckets than this (and at most kLdsBins) take the kLdsBins instance (measurement builds: 512)
__host__ __device__ inline bool decode_tile_hi(uint32_t lg_nb) { return (1u << lg_nb) > kDecodeSplitBins && (1u << lg_nb) <= kLdsBins; }

struct ResolveArgs {
    const CellMeta* meta;
    const uint32_t* bucket_cell;
    const uint32_t* multi_cells;
    const uint2* tile_desc;   // per scatter tile: (cell, tile index inside the cell)
    const uint32_t* cell_nkeys;
    uint32_t* cursor;      // per-bucket: count -> exclusive offset -> end offset
    uint64_t* keys0;
    uint64_t* keys1;
    uint32_t* cell_ncols;  // per-cell length of the resolved-column list (multi-bucket cells)
    uint32_t* nnz;
    OverflowEnt* ovf_list;
    uint32_t* div_list;    // [n_buckets] buckets the hash kernel hands to the sort path (count: DevStatus::n_divert)
    uint32_t* lab;         // EM modes: label area, 2 words per key slot (null otherwise)
    uint32_t* lab_cnt;     // EM modes: per cell (label words, ambiguous molecules)
    DevStatus* st;
    uint32_t n_buckets;
    uint32_t n_multi;
    uint32_t n_tiles;
    const uint32_t* hist_cells;  // cells counted by k_cell_hist: multi-bucket cells + PUG cells
    uint32_t n_hist;
    uint32_t usa;
    uint32_t num_rows;
    uint32_t prefer_ambig;       // --sa-model prefer-ambig in USA mode (cr-like, cr-like-em)
    uint32_t max_lg_nb;          // largest lg_nb of the batch's multi-bucket cells (picks the scatter instance)
    uint32_t* slab_ovf;          // fixed-slab placement: per cell, set when one of its buckets outgrew its slab (the cell is then placed exactly)
    uint32_t sort_only;          // reads of the range average two or more alignments: buckets are resolved by sorting, not through the UMI table
    uint32_t trivial;            // the batch resolves `trivial`: its buckets (but those of tiny cells) are the sort path's
    uint32_t divert_all;         // tests (AFQ_TEST_RESOLVE_DIVERT=all): every bucket through the divert list to the sort path
    uint32_t fix_recount;        // the scattering decoder placed the keys: k_fix_slabs gathers an overflowed cell's keys into keys0
                                 // (flag 1) or counts a re-decoded one's buckets afresh (flag 2) before placing it
    const uint32_t* spill;       // ... with the spilled keys' count per cell (DecodeArgs::spill)
};

// one launch that clears / fills a range's small buffers (k_range_init): dst <- zeros (src_off == ~0) or arena[src_off ...)
struct RangeInitOp { void* dst; uint64_t src_off; uint64_t bytes; };
constexpr uint32_t kRangeInitOps = 32;
struct RangeInitOps { RangeInitOp op[kRangeInitOps]; uint32_t n; };
void launch_range_init(hipStream_t s, const RangeInitOps& ops, const uint8_t* arena);
constexpr uint32_t kPackHdrWords = 16;   // k_pack_small: words in front of the per-cell arrays
void launch_copy_words3(hipStream_t s, const uint32_t* a, uint32_t na, uint32_t* da, const uint32_t* b, uint32_t nb, uint32_t* db,
                        const uint32_t* c, uint32_t nc, uint32_t* dc);
void launch_pack_small(hipStream_t s, const DevStatus* st, const uint32_t* em_flag, const uint32_t* alt, const uint32_t* nnz, const uint32_t* em_nnz,
                       const uint64_t* bc, const uint32_t* n_mono, uint32_t n, uint32_t* out);
void launch_gather_headers(hipStream_t s, const uint8_t* bytes, size_t n_bytes, const uint64_t* chunk_off,
                           uint32_t n_cells, uint32_t* hdr);
int launch_decode(hipStream_t s, const DecodeArgs& a, uint32_t bw, uint32_t uw);
// chunks with 1/2-byte barcode or UMI fields rewritten with 4-byte ones (meta: the widened chunks; src_off: where each cell's chunk sits in src)

void launch_widen(hipStream_t s, const uint8_t* src, size_t n_src, const uint64_t* src_off, const CellMeta* meta, uint32_t n_cells,
                  uint32_t bw, uint32_t uw, uint32_t ebw, uint32_t euw, uint8_t* dst, DevStatus* st, uint32_t bsplit = 0);
// records with an e-byte position behind every alignment word rewritten without them (and with k_widen's 4-byte fields);
// meta: the stripped chunks
void launch_strip_aln(hipStream_t s, const uint8_t* src, size_t n_src, const uint64_t* src_off, const CellMeta* meta, uint32_t n_cells,
                      uint32_t bw, uint32_t uw, uint32_t ebw, uint32_t euw, uint32_t e, uint8_t* dst, DevStatus* st);
bool decode_par_supported(uint32_t bw, uint32_t uw);
int launch_decode_par(hipStream_t s, const DecodeArgs& a, uint32_t bw, uint32_t uw);
void launch_fix_slabs(hipStream_t s, const ResolveArgs& a);
void launch_scatter(hipStream_t s, const ResolveArgs& a);
uint64_t em_scratch_words(uint32_t nU, uint32_t W, uint32_t M, bool usa);
void launch_em(hipStream_t s, const ResolveArgs& a, uint32_t n_cells, const uint64_t* em_off, uint32_t* scratch,
               uint32_t* out_nnz, void* em_hdr /* 16 B per cell */, const uint32_t* em_order /* cells, largest first */,
               uint32_t num_alphas, uint32_t init_uniform, bool rounds = true /* false: the set-up only (the classes, for -d / -b) */);
// the EM in order-free fixed-point arithmetic (afq_em2.hip; the default): per-cell scratch words, launcher, and whether the
// output space fits the set-up kernel's bitmap (otherwise the canonical kernels above run)
uint64_t em2_scratch_words(uint32_t nU, uint32_t W, uint32_t M, bool usa);
bool em2_supported(uint32_t num_alphas);
// plan_cap_words != 0: the per-cell offsets are made on the device (k_em2_plan) from the counts the range's kernels left, packed
// into a scratch buffer of that many words; tiers[7] != 0 afterwards = it did not fit and nothing ran.  Returns the status of
// the set-up kernel's launch, the one whose LDS grows with num_alphas (64 KiB of bitmap and ranks at em2_supported's bound)
hipError_t launch_em2(hipStream_t s, const ResolveArgs& a, uint32_t n_cells, uint64_t* em_off, uint32_t* scratch, uint32_t* out_nnz,
                const uint32_t* em_order, uint32_t* tiers /* 8 + 5 * n_cells words */, uint32_t num_alphas, uint32_t init_uniform,
                uint64_t plan_cap_words = 0);
// -d: sizes (cls_ptr == null) or fills the per-cell gene-level classes; see k_eqc_dump
void launch_eqc_dump(hipStream_t s, const ResolveArgs& a, uint32_t n_cells, const uint64_t* em_off, const uint32_t* scratch,
                     const void* em_hdr, uint32_t num_alphas, uint32_t* n_cls, uint32_t* n_words, const uint64_t* cls_ptr,
                     const uint64_t* word_ptr, uint32_t* o_len, uint32_t* o_count, uint32_t* o_labels);
// -b: bootstrap mean / variance per support entry of every cell, from the dumped classes; see k_boot
uint64_t boot_scratch_words(uint64_t K, uint64_t W, uint32_t B, bool summary_stat);
void launch_boot(hipStream_t s, uint32_t n_cells, const uint64_t* cls_ptr, const uint64_t* word_ptr, const uint32_t* len,
                 const uint32_t* cnt, const uint32_t* lab, const uint64_t* scr_off, uint32_t* scratch, uint32_t B, uint32_t summary_stat,
                 uint64_t seed, uint64_t first_cell_index, uint32_t* n_support, uint32_t* o_col, float* o_mean, float* o_var);
// `alevin-fry infer`: one EM per cell over its row of the equivalence-class count matrix (k_boot<true>); outputs per cell at
// word_ptr[cell] * (usa ? 3 : 1): the support's columns and abundances, n_support of them
uint64_t infer_scratch_words(uint64_t K, uint64_t W, bool usa);
void launch_infer(hipStream_t s, uint32_t n_cells, const uint64_t* cls_ptr, const uint64_t* word_ptr, const uint32_t* len,
                  const uint32_t* cnt, const uint32_t* lab, const uint64_t* scr_off, uint32_t* scratch, uint32_t usa, uint32_t num_alphas,
                  uint32_t* n_support, uint32_t* o_col, float* o_alpha);
void launch_boot_compact(hipStream_t s, uint32_t n_cells, const uint64_t* word_ptr, const uint64_t* sup_ptr, const uint32_t* i_col,
                         const float* i_mean, const float* i_var, uint32_t* o_col, float* o_mean, float* o_var);
void launch_compact_em(hipStream_t s, uint32_t n_cells, const uint64_t* em_off, const uint32_t* scratch, const uint32_t* nnz,
                       const uint64_t* cell_ptr, uint32_t* gene, float* val);
void launch_atac_dedup(hipStream_t s, uint32_t n_cells, const uint32_t* ref, const uint32_t* start, const uint16_t* flen,
                       const uint64_t* cell_ptr, void* scratch /* 16 B per fragment */, uint32_t* o_ref, uint32_t* o_start,
                       uint16_t* o_flen, uint16_t* o_cnt, uint32_t* o_n, const uint32_t* cell_cnt = nullptr,
                       unsigned long long* tally = nullptr);
void launch_atac_dedup64(hipStream_t s, uint32_t n_cells, const uint32_t* ref, const uint32_t* start, const uint16_t* flen,
                         const uint64_t* cell_ptr, void* scratch, uint32_t* o_ref, uint32_t* o_start, uint16_t* o_flen,
                         uint16_t* o_cnt, uint32_t* o_n, uint32_t* flag, const uint32_t* cell_cnt = nullptr,
                         unsigned long long* tally = nullptr);
// (tally: tally[0] += the runs of 65536 and more records whose 16-bit count reads 0 or 1 - launch_atac_compact, which tallies
//  "seen more than once" from the stored counts, cannot see them; zeroed by the caller before the dedup kernel it keeps)
// ATAC records straight from collated-RAD chunks (afq_atac.hip)
struct AtacCell { uint64_t chunk_off; uint64_t out_off; uint64_t bm_off; uint32_t nbytes; uint32_t nrec; };
struct AtacParseArgs {
    const uint8_t* bytes; const AtacCell* cells; uint32_t n_cells; uint32_t bc_bytes;
    uint64_t* bitmap; uint32_t* o_ref; uint32_t* o_start; uint16_t* o_flen; uint32_t* cell_cnt; uint64_t* cell_bc;
    uint32_t* cell_stat;   // [n_cells][2]: records with > 1 alignment, records that are not one properly mapped pair
    uint32_t* walk_list; uint32_t* n_walk; DevStatus* st;
    uint64_t n_bytes;      // size of the input buffer (aligned dword reads stop there)
};
void launch_atac_parse(hipStream_t s, const AtacParseArgs& a);
void launch_atac_compact(hipStream_t s, uint32_t n_cells, const uint64_t* cell_ptr, const uint64_t* out_ptr, const uint32_t* i_ref,
                         const uint32_t* i_start, const uint16_t* i_flen, const uint16_t* i_cnt, uint32_t* o_ref, uint32_t* o_start,
                         uint16_t* o_flen, uint16_t* o_cnt, unsigned long long* tally = nullptr, uint4* runs = nullptr, uint32_t* run_ctr = nullptr,
                         uint32_t run_cap = 0);
// `atac sort`: the fragments of an UNCOLLATED scATAC RAD in one global (ref, start, frag_len, barcode) order (afq_atac_sort.hip)
constexpr uint32_t kSortBinShift = 17;        // a position bin is 2^17 bases of one reference
constexpr uint32_t kSortLeafCap = 16384;      // keys one workgroup sorts in a single LDS tile
constexpr uint32_t kSortRepartAbove = kSortLeafCap;   // a segment with more keys is partitioned again by its next key bits
constexpr uint32_t kSortParseTile = 4096;     // bytes of a chunk a wave stages in LDS per trip
constexpr uint32_t kSortRadixBits = 8;        // digit width of a re-partition level
constexpr uint32_t kSortSmallLeaf = 2048;     // leaves up to this size are sorted by a workgroup of kSortSmallLeafNT threads
constexpr int kSortSmallLeafNT = 256, kSortLeafNT = 1024;   // threads of the two leaf instances: a leaf's run heads are compacted a slice of that many at a time
constexpr uint32_t kSortParseHalo = 24;       // bytes staged behind a parse tile: a record that starts inside the tile has its head (4 + 8) and ONE alignment (11) staged with it
constexpr uint32_t kSortNoBin = 0xFFFFFFFFu;  // an output slot of the parse that holds no fragment
constexpr uint32_t kSortNoRank = 0xFFFFFFFFu;
constexpr uint64_t kSortEmptyKey = ~0ull;     // free slot of the correction table (the all-ones barcode travels as SortParseArgs::ones_rank)
// the correction table: home slot = sort_hash_bc(barcode) & (capacity - 1), capacity = sort_table_capacity(entries): at most half the slots are taken
#if defined(__HIPCC__)
#define AFQ_SORT_HD __host__ __device__
#else
#define AFQ_SORT_HD
#endif
AFQ_SORT_HD inline uint32_t sort_hash_bc(uint64_t x) {
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return (uint32_t)x;
}
#undef AFQ_SORT_HD
inline uint64_t sort_table_capacity(uint64_t n_corr) {   // the smallest power of two >= max(2, 2 n_corr)
    uint64_t cap = 2;
    while (cap < 2 * n_corr) cap <<= 1;
    return cap;
}
struct SortChunk { uint64_t chunk_off; uint64_t out_off; uint32_t nbytes; uint32_t nrec; };
struct SortParseArgs {
    const uint8_t* bytes; uint64_t n_bytes; const SortChunk* chunks; uint32_t n_chunks; uint32_t bc_bytes;
    const uint64_t* tab_key; const uint32_t* tab_val; uint32_t tab_mask; uint32_t ones_rank;
    const uint2* ref_info;   // [ref_count] (length, first bin)
    uint32_t ref_count;
    uint32_t* o_bin; uint64_t* o_key;   // a slot per record of the chunk table: the kept ones first, kSortNoBin behind them
    uint32_t* chunk_stat;    // [n_chunks][4]: na == 0, na > 1, barcode not in the map, kept
    DevStatus* st;
};
struct SortSeg { uint32_t off, cnt, hist_base, shift; };    // a run of keys to partition: digit = (key >> shift) & 255, counted at hist[hist_base + digit]
struct SortLeaf { uint32_t off, cnt, bin, flags; };         // flags: bit 0 = the keys sit in the second buffer, bit 1 = all keys are equal
void launch_sort_table(hipStream_t s, const uint64_t* observed, const uint32_t* rank, uint64_t n, uint64_t* tab_key, uint32_t* tab_val, uint32_t tab_mask, DevStatus* st);
void launch_sort_parse(hipStream_t s, const SortParseArgs& a);
// level 0 (bins != nullptr): one segment, the digit of slot i is bins[i] (n_sub bins); above: 256 digits of the keys
void launch_sort_partition(hipStream_t s, const SortSeg* segs, uint32_t n_seg, uint32_t max_cnt, const uint64_t* keys, const uint32_t* bins, uint32_t n_sub,
                           uint32_t* hist, uint32_t* cursor, uint64_t* dst);
void launch_sort_bits(hipStream_t s, const SortSeg* segs, uint32_t n_seg, uint32_t max_cnt, const uint64_t* keys, uint64_t* and_or);
void launch_sort_leaves(hipStream_t s, const SortLeaf* leaves, const uint32_t* ids_small, uint32_t n_small, const uint32_t* ids_big, uint32_t n_big,
                        uint64_t* buf_a, uint64_t* buf_b, uint64_t* o_key, uint32_t* o_cnt, uint32_t* o_n);
void launch_sort_emit(hipStream_t s, const SortLeaf* leaves, uint32_t n_leaves, const uint32_t* leaf_out, const uint64_t* i_key, const uint32_t* i_cnt,
                      const uint32_t* bin_base, uint32_t ref_count, const uint64_t* rank_bc, uint32_t* o_ref, uint32_t* o_start, uint16_t* o_flen,
                      uint64_t* o_bc, uint32_t* o_cnt, unsigned long long* n_long);
// `generate-permit-list`: the barcode histogram of an uncollated RNA RAD and the correction decisions (afq_gpl.hip)
constexpr uint32_t kGplParseTile = 4096;      // bytes of a chunk a wave stages in LDS per trip
constexpr uint32_t kGplParseHalo = 256;       // bytes staged behind a tile: the head (at most 4 + 8 + 8) of a record that starts on the tile's last byte, and its first alignments
constexpr uint32_t kGplLaneAlns = 16;         // a record with more alignments than this has them tested by the whole wave, out of global memory
constexpr uint32_t kGplOriBoth = 0, kGplOriFw = 1, kGplOriRc = 2;                                   // afq_gpl_hist_rad's expected_ori
constexpr uint32_t kGplHamming = 0, kGplShift = 1;                                                  // afq_gpl_correct's neighborhood
constexpr uint32_t kGplUnique = 0, kGplFrequency = 1;                                               // ... resolution
constexpr uint32_t kGplExact = 0, kGplCorrected = 1, kGplAmbiguous = 2, kGplNotFound = 3;           // ... decisions
constexpr uint32_t kGplNoTarget = 0xFFFFFFFFu;
constexpr uint64_t kGplMaxWeight = 1ull << 55;   // exact count + pseudocount stays below this: 499 candidates' weights then sum below 2^64
// the counting table: home slot = sort_hash_bc(barcode) & (capacity - 1); at most half the slots are taken
inline uint64_t gpl_table_capacity(uint64_t n_kept, uint32_t bc_bytes) {   // the smallest power of two >= max(2, 2 min(n_kept, 2^(8 bc_bytes)))
    const uint64_t n = bc_bytes < 8 && n_kept > (1ull << (8 * bc_bytes)) ? (1ull << (8 * bc_bytes)) : n_kept;
    return sort_table_capacity(n);
}
struct GplParseArgs {
    const uint8_t* bytes; uint64_t n_bytes; const SortChunk* chunks; uint32_t n_chunks;
    uint32_t bc_bytes, umi_bytes, aln_extra, expected_ori;
    uint64_t* o_bc;          // a slot per record of the chunk table: a chunk's compatible records first (chunk_stat[1] of them)
    uint32_t* chunk_stat;    // [n_chunks][4]: records seen, compatible, largest na among the compatible, long records
    DevStatus* st;
};
struct GplCorrectArgs {
    const uint64_t* observed; const uint64_t* obs_count; uint64_t n_obs;
    const uint64_t* tab_key; const uint32_t* tab_val; uint32_t tab_mask; uint32_t ones_idx;   // retained barcode -> its index
    const uint64_t* ret_count;   // [n_retained] exact counts
    uint32_t barcode_len, neighborhood, resolution;
    uint64_t conf_num, conf_den, pseudocount;
    uint8_t* o_decision; uint32_t* o_target;
    unsigned long long* stats;          // [8]: (distinct, reads) of exact, corrected, ambiguous, not found
    unsigned long long* target_count;   // [n_retained]
};
void launch_gpl_parse(hipStream_t s, const GplParseArgs& a);
void launch_gpl_count(hipStream_t s, const SortChunk* chunks, uint32_t n_chunks, const uint32_t* chunk_stat, const uint64_t* bcs, uint64_t* tab_key,
                      unsigned long long* tab_cnt, uint32_t mask, unsigned long long* ones, DevStatus* st);
void launch_gpl_compact(hipStream_t s, const uint64_t* tab_key, const unsigned long long* tab_cnt, uint64_t cap, uint64_t* o_key, uint64_t* o_cnt,
                        uint32_t* n_out);
void launch_gpl_correct(hipStream_t s, const GplCorrectArgs& a);
// multi-barcode `generate-permit-list`: the (routing entry, cell barcode) pairs of an uncollated two-barcode RNA RAD
// (afq_gpl_multi.hip).  The walk and its limits are the GPL parse's; the entry table is launch_sort_table's (no entry is all-ones:
// a sample barcode has at most 4 bytes); the keys go through launch_gpl_count / launch_gpl_compact.
struct GplMultiParseArgs {
    const uint8_t* bytes; uint64_t n_bytes; const SortChunk* chunks; uint32_t n_chunks;
    uint32_t b0_bytes, b1_bytes, umi_bytes, aln_extra, expected_ori;
    const uint64_t* tab_key; const uint32_t* tab_val; uint32_t tab_mask;   // sample barcode -> its index in the entry list
    uint64_t* o_key;         // a slot per record of the chunk table: entry << 32 | b1 of a chunk's routed records first (chunk_stat[1] of them)
    uint32_t* chunk_stat;    // [n_chunks][4]: records seen, routed, compatible but unrouted, long records
    DevStatus* st;
};
void launch_gpl_multi_parse(hipStream_t s, const GplMultiParseArgs& a);
// `atac generate-permit-list`: the barcode of every record of an uncollated scATAC RAD, the largest na and the position-bin
// histogram of the records with one alignment (afq_atac_gpl.hip).  The walk and its limits are k_sort_parse's (kSortParseTile,
// kSortParseHalo); the barcode column goes through launch_gpl_count / launch_gpl_compact.
struct AtacGplParseArgs {
    const uint8_t* bytes; uint64_t n_bytes; const SortChunk* chunks; uint32_t n_chunks; uint32_t bc_bytes;
    const uint32_t* bin_base;   // [ref_count] first bin of a reference
    uint32_t ref_count, n_bins, bin_size;
    uint64_t* o_bc;             // a slot per record of the chunk table, in input order
    uint32_t* bins;             // [n_bins] counters, zeroed by the caller
    uint32_t* chunk_stat;       // [n_chunks][4]: na == 0, records (0 for a refused chunk), largest na, na > 1
    DevStatus* st;              // kErrRecordWalk, kErrRefRange, kErrStartRange (here: a bin index not below n_bins); err_cell: the chunk
};
void launch_atac_gpl_parse(hipStream_t s, const AtacGplParseArgs& a);
void launch_atac_gpl_bins(hipStream_t s, const uint32_t* bins, uint32_t n_bins, uint64_t* o_bins, uint32_t* o_max);   // o_bins[i] = bins[i]; *o_max (zeroed by the caller) = the largest
// `collate`: the records of an uncollated RNA RAD, barcode-corrected, one output chunk per cell (afq_collate.hip).  The walk and
// its limits are the GPL parse's (kGplParseTile, kGplParseHalo, kGplLaneAlns).
constexpr uint32_t kCollateRadixNT = 256, kCollateRadixItems = 32, kCollateScanItems = 8;
constexpr uint32_t kCollateRadixBlock = kCollateRadixNT * kCollateRadixItems;   // keys a workgroup of a radix pass takes (256 digit counts each: the fewer workgroups, the shorter the one-workgroup scan of the counts)
constexpr uint32_t kCollateScanBlock = kCollateRadixNT * kCollateScanItems;     // sorted positions a workgroup of the length scan takes (they sit in registers)
constexpr uint32_t kErrCollateChunk = 12;   // collate: an output chunk of 4 GiB or more (err_cell: the cell's index)
struct CollateArgs {
    const uint8_t* bytes; uint64_t n_bytes; const SortChunk* chunks; uint32_t n_chunks;
    uint32_t bc_bytes, umi_bytes, aln_extra, expected_ori;
    const uint64_t* tab_key; const uint32_t* tab_val; uint32_t tab_mask; uint32_t ones_cell;   // observed barcode -> index of its corrected barcode in `cells`
    uint32_t n_cells;        // (also the cell word of a record that is dropped: it sorts behind every cell)
    uint2* rec;              // a slot per record of the chunk table, in input order: (cell, bytes of the record as written)
    uint64_t* key;           // measure: cell << 32 | slot of every slot
    uint32_t* chunk_stat;    // measure: [n_chunks][8]: records, compatible, not in the map, kept, alignments in, alignments kept, long records, 0
    const uint64_t* cells;   // write: [n_cells] the corrected barcodes
    const uint64_t* dest;    // write: [slot] byte offset of the record in `out`
    uint8_t* out;
    DevStatus* st;
};
void launch_collate_measure(hipStream_t s, const CollateArgs& a);
void launch_collate_write(hipStream_t s, const CollateArgs& a);
// one stable LSD pass over n keys: digit = (key >> shift) & 255; hist holds 256 x ceil(n / kCollateRadixBlock) words (digit-major)
void launch_collate_radix_pass(hipStream_t s, const uint64_t* src, uint64_t* dst, uint32_t n, uint32_t shift, uint32_t* hist);
// ex[i] = bytes of the records in front of sorted position i (ex[n]: all of them); dest[slot] = 8 (cell + 1) + ex[i]
// (block_sum: ceil(n / kCollateScanBlock) words)
void launch_collate_scan(hipStream_t s, const uint64_t* sorted, const uint2* rec, uint32_t n, uint64_t* block_sum, uint64_t* ex, uint64_t* dest);
// chunk c: off[c] (off[n_cells]: the end), nrec[c], and its (nbytes, nrec) header into out
void launch_collate_heads(hipStream_t s, const uint64_t* sorted, uint32_t n, const uint64_t* ex, uint32_t n_cells, uint64_t* off, uint32_t* nrec, uint8_t* out,
                          DevStatus* st);
// in-place exclusive scan of n words by one workgroup (the radix passes' digit counts; `atac collate`'s non-empty-cell flags)
void launch_collate_excl_scan_u32(hipStream_t s, uint32_t* v, uint64_t n);
// multi-barcode `collate`: the records `na, b0, b1, umi, alignments` of an uncollated two-barcode RNA RAD, routed to a sample by b0 and
// corrected to a cell of that sample by b1, one output chunk per cell (k_collate_walk over these args, afq_collate.hip).  The walk and its limits are collate's;
// both tables are launch_sort_table's (no key is all-ones: b0 and b1 have at most 4 bytes and a sample index is below 2^31); placement,
// length scan and heads are launch_collate_radix_pass / launch_collate_scan / launch_collate_heads.
struct CollateMultiArgs {
    const uint8_t* bytes; uint64_t n_bytes; const SortChunk* chunks; uint32_t n_chunks;
    uint32_t b0_bytes, b1_bytes, umi_bytes, aln_extra, expected_ori;
    const uint64_t* stab_key; const uint32_t* stab_val; uint32_t stab_mask;   // observed b0 -> sample index
    const uint64_t* ctab_key; const uint32_t* ctab_val; uint32_t ctab_mask;   // sample index << 32 | observed b1 -> index of the corrected barcode among the cells
    uint32_t n_cells;        // (also the cell word of a record that is dropped: it sorts behind every cell)
    uint2* rec;              // a slot per record of the chunk table, in input order: (cell, bytes of the record as written)
    uint64_t* key;           // measure: cell << 32 | slot of every slot
    uint32_t* chunk_stat;    // measure: [n_chunks][8]: records, compatible, unrouted, routed but not in the sample's map, kept, alignments in, alignments kept, long records
    const uint64_t* cell_head;   // write: [n_cells] the value written into b0 << 32 | the corrected cell barcode
    const uint64_t* dest;    // write: [slot] byte offset of the record in `out`
    uint8_t* out;
    DevStatus* st;
};
void launch_collate_multi_measure(hipStream_t s, const CollateMultiArgs& a);
void launch_collate_multi_write(hipStream_t s, const CollateMultiArgs& a);
// `atac collate`: the records of an UNCOLLATED scATAC RAD with exactly one alignment and a barcode of the correction map, barcode-
// corrected, one output chunk per cell THAT RECEIVED A RECORD (afq_atac_collate.hip).  The walk is k_sort_parse's (kSortParseTile,
// kSortParseHalo), the placement collate's radix passes; a kept record is R = 4 + bc_bytes + 11 bytes, so the layout needs no length scan.
struct AtacCollateArgs {
    const uint8_t* bytes; uint64_t n_bytes; const SortChunk* chunks; uint32_t n_chunks; uint32_t bc_bytes;
    const uint64_t* tab_key; const uint32_t* tab_val; uint32_t tab_mask; uint32_t ones_cell;   // observed barcode -> index of its corrected barcode in `cells`
    uint32_t n_cells;        // (also the cell word of a record that is dropped: it sorts behind every cell)
    uint32_t* cell_of;       // a slot per record of the chunk table, in input order: the record's cell, n_cells if it is dropped
    uint64_t* key;           // measure: cell << 32 | slot of every slot
    uint32_t* chunk_stat;    // measure: [n_chunks][8]: records, na == 0, na > 1, not in the map, kept, 0, 0, 0
    const uint64_t* cells;   // write: [n_cells] the corrected barcodes
    const uint64_t* dest;    // write: [slot] byte offset of the record in `out`
    uint8_t* out;
    DevStatus* st;
};
void launch_atac_collate_measure(hipStream_t s, const AtacCollateArgs& a);
void launch_atac_collate_write(hipStream_t s, const AtacCollateArgs& a);
// sorted: the n sort words in (cell, slot) order.  Cell c's run [lo, hi): first[c] = lo (first[n_cells]: the number of kept records),
// flag[c] = (hi > lo), flag[n_cells] = 0
void launch_atac_collate_runs(hipStream_t s, const uint64_t* sorted, uint32_t n, uint32_t n_cells, uint32_t* first, uint32_t* flag);
// rank: the exclusive scan of flag (rank[n_cells] = n_out).  Output chunk j = rank[c] of a non-empty cell c: off[j] = R first[c] + 8 j,
// nrec[j], cell[j] = c, and its (nbytes, nrec) header into out; dest[slot] = R i + 8 (rank[cell] + 1) for sorted position i
void launch_atac_collate_heads(hipStream_t s, const uint64_t* sorted, uint32_t n, uint32_t n_cells, uint32_t rec_bytes, const uint32_t* first, const uint32_t* rank,
                               uint64_t* off, uint32_t* nrec, uint32_t* cell, uint64_t* dest, uint8_t* out, DevStatus* st);
// `convert`: the alignment records of a BAM (the inflated stream behind its header) as the chunks of a mapper RAD (afq_convert.hip;
// bam2rad, src/convert.rs:167-594 of the reference).  A wave walks a host-made span of records (tiles of kGplParseTile bytes and
// kGplParseHalo behind them, as the RAD walks); the kept records are compacted, cut into runs of one read name, their aux fields
// scanned, and the runs laid out by launch_collate_scan over the sort words  chunk << 32 | written rank, chunk = rank / 10 001.
constexpr uint32_t kConvertLaneAlns = 16;           // a run with more records than this is read and written by the whole wave
constexpr uint32_t kConvertChunkRuns = 10001;       // written runs of an output chunk (convert.rs:473 tests before :551 counts)
constexpr uint32_t kConvertRecFixed = 36;           // block_size and the fixed fields of a BAM record
constexpr uint32_t kConvertTileRecs = kGplParseTile / kConvertRecFixed + 1;
constexpr uint32_t kConvertScanItems = 16, kConvertScanBlock = 256 * kConvertScanItems;   // words a workgroup of the flag scans takes
// the error word: record index << 8 | code, the smallest wins (atomicMin), so the record named does not depend on the schedule
constexpr uint32_t kConvErrRecord = 1;     // block_size too small for the record's own fields, or past the span's end; aux that does not tile the record
constexpr uint32_t kConvErrRef = 2;        // a kept record's refID is not in [0, n_ref)
constexpr uint32_t kConvErrTagMissing = 3; // a run head without CR or UR
constexpr uint32_t kConvErrTagType = 4;    // a run head whose CR or UR is not of type Z
constexpr uint32_t kConvErrBase = 5;       // a base outside ACGTN in the barcode or UMI of a run that is written
constexpr uint32_t kConvErrScore = 6;      // -f: a record of a written run without an integer AS
constexpr uint64_t kConvNoErr = ~0ull;
enum ConvertStat { kConvRunsDroppedN = 0, kConvAlnIn, kConvAlnWritten, kConvLongRuns, kConvStatCount };
struct ConvertArgs {
    const uint8_t* bytes; uint64_t n_bytes; const uint64_t* span_off; uint32_t n_spans; uint32_t n_ref;
    uint32_t bc_bytes, umi_bytes, filter_best;
    uint32_t* span_cnt;          // count walk: [n_spans][2] records, kept records
    const uint32_t* span_base;   // fill walk: [n_spans][2] records, kept records in front of the span
    uint32_t n_kept;
    uint64_t* rec_off;           // [n_kept] where the kept record's block_size stands
    uint32_t* rec_idx;           // [n_kept] its index among the records of the file (for the error word)
    uint32_t* word;              // [n_kept] refID | 0x80000000 when flag 0x10 is clear
    uint32_t* head;              // [n_kept + 1] heads: 1 where the name differs from the predecessor's, [n_kept] = 0; scanned in place:
                                 //              runs in front of record k, so k's run is head[k + 1] - 1 and head[n_kept] = n_runs
    int32_t* score;              // [n_kept] -f: AS, and has_score: was there an integer one
    uint8_t* has_score;
    uint32_t n_runs;
    uint32_t* run_first;         // [n_runs + 1] the run's first kept record ([n_runs] = n_kept)
    uint64_t* run_bc; uint64_t* run_umi;   // [n_runs] the head's CR and UR, two bits a base
    uint32_t* run_flag;          // [n_runs + 1] aux: 1 where the run is dropped for two N; runs: 1 where it is written ([n_runs] = 0); scanned in place
    uint32_t* run_na; int32_t* run_max;    // [n_runs] alignments written, -f: the best AS
    uint64_t* stat;              // [kConvStatCount]
    uint64_t* key; uint2* rec;   // [n_written] place: chunk << 32 | rank; (run, bytes of the run as written)
    const uint64_t* dest;        // [n_written] write: byte offset of the run in out
    uint32_t n_written;
    uint8_t* out;
    unsigned long long* err;     // the error word
    DevStatus* st;               // kErrCollateChunk from place and the heads
};
void launch_convert_count(hipStream_t s, const ConvertArgs& a);
void launch_convert_fill(hipStream_t s, const ConvertArgs& a);
void launch_convert_heads(hipStream_t s, const ConvertArgs& a);   // head[] (unscanned)
// in-place exclusive scan of n words by ceil(n / kConvertScanBlock) workgroups (block_sum: that many words)
void launch_convert_scan(hipStream_t s, uint32_t* v, uint64_t n, uint32_t* block_sum);
void launch_convert_aux(hipStream_t s, const ConvertArgs& a);     // behind the scan of head[]: run_first, run_bc, run_umi, run_flag, score
void launch_convert_runs(hipStream_t s, const ConvertArgs& a);    // run_na, run_max, run_flag := written, stat
void launch_convert_place(hipStream_t s, const ConvertArgs& a);   // behind the scan of run_flag[]: key, rec
void launch_convert_write(hipStream_t s, const ConvertArgs& a);
// the snappy frame encoder (afq_snappy.hip): bytes on the device -> stream identifier + one data chunk per kSnappyBlock bytes
constexpr uint32_t kSnappyBlock = 65536;          // bytes of input per frame chunk (the format's limit)
constexpr uint32_t kSnappyHashBits = 11, kSnappyHashSlots = 1u << kSnappyHashBits;   // last-position table of a chunk, in LDS
constexpr uint32_t kSnappyMaxCopy = 64;           // longest single copy element
constexpr uint32_t kSnappyBlocksPerWg = 1;        // a workgroup is one wave and takes one chunk
constexpr uint32_t kSnappySlot = (32 + kSnappyBlock + kSnappyBlock / 6 + 15) & ~15u;   // where a chunk's raw block is first written: snappy's own worst case
constexpr uint32_t kSnappyStored = 0x80000000u;
struct SnappyMeta { uint32_t body, crc, lit, copies; };   // bytes of the chunk's body (| kSnappyStored: the input's own bytes, type 0x01), masked CRC-32C, literal bytes and copy elements of a raw block
inline uint64_t snappy_blocks(uint64_t n) { return (n + kSnappyBlock - 1) / kSnappyBlock; }
inline uint64_t snappy_stream_bound(uint64_t n) { return 10 + n + 8 * snappy_blocks(n); }
void launch_snappy_blocks(hipStream_t s, const uint8_t* in, uint64_t n, uint64_t n_blocks, uint8_t* slots, SnappyMeta* meta);
void launch_snappy_layout(hipStream_t s, const SnappyMeta* meta, uint64_t n_blocks, uint64_t* off);   // off[i]: where chunk i's header stands, off[n_blocks]: the stream's length
void launch_snappy_pack(hipStream_t s, const uint8_t* in, uint64_t n_blocks, const uint8_t* slots, const SnappyMeta* meta, const uint64_t* off, uint8_t* out);

// the snappy frame decoder (afq_snappy.hip): a frame stream on the device and the host's plan of it -> its bytes on the device
constexpr uint32_t kSnappyDecThreads = 64;         // a workgroup is one wave and takes one data chunk
constexpr uint32_t kSnappyDecWindow = 8192;        // bytes of a chunk's body staged in LDS per trip to memory
constexpr uint32_t kSnappyDecPieceChunks = 4096;   // data chunks of one launch at the most (a piece of the stream; afq_snappy_frame_decode_device)
constexpr uint32_t kSnappyDecLds = (kSnappyBlock + 16) + (kSnappyDecWindow + 32) + 1024;   // staged output, window, CRC table: two workgroups share a CU's 160 KiB
struct SnappyDecChunk { uint64_t in_off, out_off; uint32_t in_len, ulen, crc, compressed; };   // in_off from the launch's `in`, out_off from its `dst`
// status: min over the refused chunks of (first_index + chunk) << 8 | SnappyDecodeCode (afq_snappy_elem.h); stats[4]: chunks,
// stored chunks, literal bytes, copy elements - of the chunks that decoded
void launch_snappy_decode(hipStream_t s, const uint8_t* in, const SnappyDecChunk* plan, uint32_t n_chunks, uint64_t first_index, uint8_t* dst, uint64_t* status, uint64_t* stats);

// the BGZF inflater (afq_inflate.hip): the blocks of a BGZF file on the device and the host's plan of them -> their bytes on the device
constexpr uint32_t kInflateThreads = 64;          // a workgroup is one wave and takes one BGZF block
constexpr uint32_t kInflateBlocksPerWg = 1;
constexpr uint32_t kInflateWindow = 8192;         // bytes of a block's payload staged in LDS per trip to memory
constexpr uint32_t kInflatePieceBlocks = 4096;    // BGZF blocks of one launch at the most (a piece of the file; afq_bgzf_inflate_device)
constexpr uint32_t kInflateLds = (kInflateMaxOut + 16) + (kInflateWindow + 32) + 1024 + (uint32_t)sizeof(InflateTables);   // staged output, window, CRC table, decode tables: two workgroups share a CU's 160 KiB
struct BgzfDecBlock { uint64_t in_off, out_off; uint32_t in_len, isize, crc, pad; };   // in_off from the launch's `in`, out_off from its `dst`
// status[0]: min over the refused blocks of (first_index + block) << 8 | InflateCode (afq_inflate_elem.h); status[1]: min over the
// blocks that ended short of ISIZE of (first_index + block) << 32 | bytes produced; stats[7]: blocks, blocks of ISIZE 0, stored,
// fixed and dynamic deflate blocks, literals, copies - of the blocks that decoded
void launch_bgzf_inflate(hipStream_t s, const uint8_t* in, const BgzfDecBlock* plan, uint32_t n_blocks, uint64_t first_index, uint8_t* dst, uint64_t* status, uint64_t* stats);

// the chunk table of a collated record stream on the device (afq_snappy.hip, k_collated_chunk_table): one wave hops the headers
constexpr uint32_t kChunkTableTile = 16384, kChunkTableShort = 1024, kChunkTableHalo = 24;   // bytes of the stream staged per trip; a header at the tile's last byte and the 8 bytes at + 12 lie in the halo
constexpr uint32_t kChunkTableWords = (3 + kChunkTableTile + kChunkTableHalo + 3) / 4 + 1;
enum ChunkTableCode : uint32_t { kChunkTableOk = 0, kChunkTableTrailing, kChunkTableCorrupt, kChunkTableNoRecord };
// stat[0]: chunks hopped (entries are written for the first `cap`), stat[1]: ChunkTableCode - on a refusal stat[0] is the chunk it is about.
// rec_hdr: bytes of a record's head (a chunk must hold one record at least), 0: no such check
void launch_collated_chunk_table(hipStream_t s, const uint8_t* bytes, uint64_t n, uint64_t first_chunk, uint32_t rec_hdr, uint64_t cap, uint64_t* off, uint32_t* nbytes,
                                 uint32_t* nrec, uint64_t* first_bc, uint64_t* stat);
void warm_code_object();
void launch_resolve(hipStream_t s, const ResolveArgs& a);
void launch_resolve_big(hipStream_t s, const ResolveArgs& a);
void launch_cell_hist(hipStream_t s, const ResolveArgs& a);
void launch_compact(hipStream_t s, const CellMeta* meta, uint32_t n_cells, const uint64_t* keys0, const uint64_t* keys1,
                    const uint32_t* nnz, const uint64_t* cell_ptr, uint32_t* gene, float* val, uint64_t cap = ~0ull);
void launch_fill_tables(hipStream_t s, const CellMeta* meta, uint32_t n_cells, uint32_t* bucket_cell, uint2* tile_desc);   // bucket -> cell and tile -> (cell, tile) from the cells' plans
struct PackSmallArgs { const DevStatus* st; const uint32_t* em_flag; const uint32_t* alt; const uint32_t* em_nnz; const uint64_t* bc; const uint32_t* n_mono; uint32_t* out; };   // what k_pack_small packs (out: pinned host memory as the device sees it)
void launch_row_ptr(hipStream_t s, const uint32_t* nnz, uint32_t n, uint64_t* cell_ptr, const PackSmallArgs& pk);   // row lengths -> row offsets (+ total at [n]); pk.out != nullptr: and k_pack_small's work in the same launch

// ---- parsimony (afq_pug.hip) ----
struct PugCellArgs {
    const uint8_t* bytes;
    const CellMeta* meta;
    const uint32_t* pug_cells;
    const uint32_t* cell_nkeys;   // reads the decode emitted per cell
    PugOut rd;
    uint64_t scr_stride;          // words of scratch per WORKGROUP (sized for the largest cell of the batch, reused cell after cell)
    uint32_t* scratch;
    uint32_t* work_counter;       // next entry of pug_cells to take (persistent workgroups)
    uint32_t n_pug;
    uint32_t* epool;              // edge pool (u32 words) + multi-word adjacency rows
    unsigned long long* epool_cursor;
    unsigned long long epool_cap;
    const uint32_t* t2g;
    uint64_t* keys0;
    uint32_t* cell_ncols;
    uint32_t* lab;
    uint32_t* lab_cnt;
    uint32_t* alt;                // [n_cells] set to 1 when a component took the cr-like fallback
    DevStatus* st;
    uint32_t ref_count, num_genes, usa, num_rows, em, exact_umi, large_thresh, hw, umi_pairs, gene_level;
    uint32_t umi32;               // the record's UMI field is 4 bytes: UMI and record offset share one sort word
    uint32_t force_global_route;  // tests: neighbour search through the global-memory hash table for every cell
    const uint32_t* n_pug_dev;    // when set: the length of pug_cells lives on the device (cells the phase kernels of afq_pug2.hip handed over)
};

void launch_pug(hipStream_t s, const PugCellArgs& a, uint32_t n_blocks);

// ---- parsimony as phase kernels over UMI partitions (afq_pug2.hip) ----
struct P2Cell {
    uint64_t rd_base;     // the cell's first read slot: rd_h / rd_u / s_h / s_u / v_off / v_flag / lidx share the indexing
    uint64_t chunk_off;   // the cell's chunk in the input bytes (= meta[cell].chunk_off)
    uint32_t cell;        // index into meta[]
    uint32_t R;           // reads
    uint32_t lgP;         // log2 of the partition count (partition = low lgP bits of the UMI)
    uint32_t part_base;   // first partition of the cell in the per-partition arrays
    uint32_t n_ref;       // alignment words of the cell (= meta[cell].n_ref: sizes the column list and the label area)
    uint32_t tile0;       // the cell's first tile (its tiles are consecutive)
    uint64_t key_off;     // = meta[cell].key_off
};
constexpr uint32_t kP2MaxComp = 4096;   // 64 mask words, one per lane: the workgroup cover of k_p2_cover (afq_pug_common.h)
constexpr uint32_t kGDescWords = 20;    // per cell: what the graph phase hands the cover kernels (P2Args.gdesc)
// The range-wide graph build (afq_pugflat.hip): one block per range, filled on the device.  Offsets are u32 words into the pool.
struct PfDev {
    unsigned long long par, cnt, rk, umi, rc, tl, loff, tcell, lh;   // per vertex that has an edge [T]: root, component size -> first slot, position | size class, UMI, reads, slot inside the cell, label offset, its cell, label key
    unsigned long long prv, midoff, mrec, tied, slow, cmv;    // two-vertex components (two slots each), first record slot per listed component (+ the end), 32-byte records, the covers' set-aside lists
    uint32_t T, NP, NC, S;
    uint32_t n_old, pad[3];                        // cells routed to the per-cell graph kernel (old_list)
};
struct PfTile {   // per tile (k_pf_tiles): what the workgroups that take a tile's roots and components need of it, in one 64-byte load
    uint32_t j, live;               // its cell; 0: the cell is not the flat kernels' (handed back, or routed to the per-cell kernel)
    uint32_t tb, te;                // its vertices' dense numbers
    uint32_t comp_base, n_tiny;     // the cell's run of the component list, its 3..8 components
    uint32_t p0, n_pr;              // the tile's slice of the pair list (range-wide entries)
    uint32_t a0, na, b0, nb;        // ... of the cell's 3..8 list and of its 9..64 list (entries counted from the cell's first)
    uint32_t s_ti, s_mi;            // first record slots of the two slices
    uint32_t pad[2];
};
static_assert(sizeof(PfTile) == 64, "PfTile");
struct P2Args {
    const uint8_t* bytes; const CellMeta* meta; const P2Cell* cells; const uint2* tiles; const uint32_t* order;
    const uint64_t* rd_h; const uint64_t* rd_u;        // the decode's reads: label key, umi << 32 | record offset
    uint64_t* s_h; uint64_t* s_u;                      // reads grouped by partition, then the vertices (key; umi << 32 | word)
    uint32_t* v_off; uint8_t* v_flag; uint32_t* lidx;  // vertex: smallest record offset, has-an-edge flag, id among the touched
    uint32_t* pcnt; uint32_t* poff; uint32_t* pcur; uint32_t* pnv; uint32_t* pcell; uint32_t* pn3;   // per partition
    uint64_t* pairs; uint32_t* pnp;                    // vertex pairs with an edge: a partition's pairs sit at its own slots; per partition: how many
    uint64_t* cstage; uint32_t* pncls;                 // two-gene classes of lone vertices (em), staged the same way
    uint32_t* gcnt;                                    // per cell [4]: columns, label words, classes, error
    uint32_t* fb; uint32_t* fb_list; uint32_t* fb_count;   // cells handed to the one-workgroup kernel
    uint32_t* pool; unsigned long long* pool_cur; unsigned long long pool_cap;
    uint32_t* work_counter;
    uint32_t* work_counter2; uint32_t* gdesc;          // the cover kernel's cell counter; per cell [16]: what the graph kernel hands it (k_p2_graph -> k_p2_cover)
    const uint32_t* cell_nkeys; const uint32_t* t2g; uint64_t* keys0; uint32_t* cell_ncols; uint32_t* lab; uint32_t* lab_cnt;
    DevStatus* st;
    uint32_t* alt;                                     // [cells of the range] set to 1 when a component took the winner-take-all fallback
    uint32_t n_cells, n_tiles, n_parts, part_cap;
    uint32_t ref_count, num_genes, usa, num_rows, em, exact_umi, large_thresh, hw, umi_pairs;
    uint32_t tile;       // reads per tile of k_p2_hist / k_p2_scatter: 2048, 4096 or 8192
    uint32_t max_comp;   // vertices of the largest component the phase kernels cover themselves (kP2MaxComp; tests: AFQ_TEST_P2_MAX_COMP)
    uint32_t n_big;   // the first n_big cells of `order` (largest first: 15 000 reads or more) get a 1024-thread workgroup each in k_p2_graph / k_p2_cover / k_p2_tied
    uint32_t defer_min;   // a cell sets the tied components of its covers aside (k_p2_tied) when its listed components hold more vertices than this; 0xFFFFFFFF: than the graph kernel's LDS class table takes (tests: 0 = every cell)
    // the range-wide graph build: six per-tile quantities and their scans (tq: nta entries each; bq: per block of 1024 tiles, nba each),
    // per cell: routed to the per-cell graph kernel; the range's block; the list of routed cells
    uint32_t* tq; uint32_t* bq; uint32_t nta, nba; uint32_t* route; PfDev* pfd; uint32_t* old_list;
    PfTile* ptile;
    uint32_t* pcpre; uint32_t* pbq; uint32_t npa;      // the scan of the lone vertices' staged class counts over the partitions (npa entries, blocks of 1024)
    uint32_t graph_flat;  // the graph phase as range-wide kernels (afq_pugflat.hip); 0: the per-cell kernel for every cell (tests: AFQ_TEST_P2_GRAPH=cell)
    uint32_t lone_coop;   // k_pl_lone: a lone vertex whose label has 5..64 refs is resolved by its whole wave; 2: those of 5..8 refs by their own lane (the L8 instance)
};
#ifndef AFQ_P2_PART_TARGET
#define AFQ_P2_PART_TARGET 144
#endif
constexpr uint32_t kP2PartTarget = AFQ_P2_PART_TARGET;   // planned mean reads per partition (the partition count is a power of two: 72..144).  It was 160 until round 5: of a
                                          // sample's 11 000 cells the one or two whose mean sat just under 160 had a partition over the capacity below (245-260 reads in
                                          // the largest of 1024 partitions) and were handed back - and k_pug_cell costs 0.4-3 ms per launch whatever it is given
constexpr uint32_t kP2PartCap = 256;      // reads one partition may hold (one wave sorts it in registers)
constexpr uint32_t kP2TileHost = 4096;   // reads per histogram / scatter tile (P2Args.tile; k_p2_scatter<512>: 8 reads per thread)
void launch_p2_split(hipStream_t s, const P2Args& a);
void launch_p2_part(hipStream_t s, const P2Args& a);
void launch_p2_search(hipStream_t s, const P2Args& a);
void launch_p2_check(hipStream_t s, const P2Args& a);   // (afq_pugflat.hip; launch_p2_search ends with it)
void launch_p2_lone(hipStream_t s, const P2Args& a);
void launch_p2_graph(hipStream_t s, const P2Args& a, uint64_t n_reads);
void launch_pf_build(hipStream_t s, const P2Args& a, uint64_t n_reads);
void launch_pf_cover(hipStream_t s, const P2Args& a);
void launch_pf_resume(hipStream_t s, const P2Args& a);
uint32_t pug_max_blocks();
uint64_t pug_scratch_words(uint32_t nrec, uint32_t n_ref, bool gene_level);

#ifndef AFQ_SCATTER_TILE
#define AFQ_SCATTER_TILE 2048
#endif
constexpr uint32_t kScatterTileHost = AFQ_SCATTER_TILE;  // keys per histogram/scatter tile (measurement builds: 4096)

}  // namespace afq
