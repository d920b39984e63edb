// afq_atac_sort.hip — `alevin-fry atac sort` (src/atac/sort.rs of the reference): every fragment of an UNCOLLATED scATAC RAD,
// barcode-corrected, in one global (ref, start, frag_len, corrected barcode) order with multiplicities.
//
// The mapper's chunks mix barcodes, so the walk-free proof of afq_atac.hip (every record of a chunk carries one barcode) has
// nothing to stand on: the na chain of a chunk is walked.  A wave owns a chunk and stages it through LDS a tile at a time; a
// tile BEGINS at a record start, the record starts inside it are found by hopping the na fields in LDS (wave-uniform, every
// lane reads the same word), and then a lane per record loads its fields, probes the correction table and makes the key.
// Nothing is counted with atomics on the way: a chunk owns nrec output slots (the prefix of the chunk table), the kept
// records fill them from the front by ballot, the rest is marked empty.
//
// Order.  A kept fragment goes to position bin  ref_bin_base[ref] + (start >> 17); bins ascend with (ref, start).  Inside a
// bin the rest of the order is ONE 64-bit key,  (start & 0x1FFFF) << 47 | frag_len << 31 | rank,  where rank is the position
// of the corrected barcode among the sorted distinct corrected barcodes (made by the host): any u32 reference id works, and
// the 64-bit LDS sort of k_atac_dedup64 serves.  Partition = histogram of the bins, scan, scatter bin-major; a segment above
// the leaf cap is partitioned again by the eight highest key bits in which its keys DIFFER (k_sort_bits finds them, so every
// level splits and eight levels spend the key), a segment of equal keys is one run and is not sorted.  A workgroup per
// leaf sorts and run-length-counts it; k_sort_emit writes the dense arrays in leaf order, which is the global order.
#include <hip/hip_runtime.h>

#include "afq_common.h"
#include "afq_kernels.h"
#include "afq_prims.h"

namespace afq {

namespace {

// ---- correction table: open addressing, 64-bit keys claimed by CAS (several workgroups share a slot word: agent scope)
__global__ __launch_bounds__(256) void k_sort_table_insert(const uint64_t* __restrict__ observed, const uint32_t* __restrict__ rank, uint64_t n,
                                                          uint64_t* __restrict__ tab_key, uint32_t* __restrict__ tab_val, uint32_t mask) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = observed[i];
    if (k == kSortEmptyKey) return;   // (the host carries this one)
    uint32_t slot = sort_hash_bc(k) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long*>(tab_key + slot), (unsigned long long)kSortEmptyKey, (unsigned long long)k);
        if (prev == kSortEmptyKey) { tab_val[slot] = rank[i]; return; }
        if (prev == k) return;        // the key is in (k_sort_table_verify compares the values)
        slot = (slot + 1) & mask;
    }
}
// every entry finds its key again with its own value: two entries of one observed barcode that disagree are refused
__global__ __launch_bounds__(256) void k_sort_table_verify(const uint64_t* __restrict__ observed, const uint32_t* __restrict__ rank, uint64_t n,
                                                          const uint64_t* __restrict__ tab_key, const uint32_t* __restrict__ tab_val, uint32_t mask,
                                                          DevStatus* __restrict__ st) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = observed[i];
    if (k == kSortEmptyKey) return;
    uint32_t slot = sort_hash_bc(k) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const uint64_t kk = tab_key[slot];
        if (kk == k) { if (tab_val[slot] != rank[i]) set_err(st, kErrCorrection, (uint32_t)i); return; }
        if (kk == kSortEmptyKey) break;
        slot = (slot + 1) & mask;
    }
    set_err(st, kErrInternal, (uint32_t)i);   // an inserted key is always found
}

__device__ __forceinline__ uint32_t table_find(const SortParseArgs& a, uint64_t k) {
    if (k == kSortEmptyKey) return a.ones_rank;
    uint32_t slot = sort_hash_bc(k) & a.tab_mask;
    for (uint32_t probe = 0; probe <= a.tab_mask; ++probe) {   // (at most half the slots are taken: an empty one ends the probe)
        const uint64_t kk = a.tab_key[slot];
        if (kk == k) return a.tab_val[slot];
        if (kk == kSortEmptyKey) return kSortNoRank;
        slot = (slot + 1) & a.tab_mask;
    }
    return kSortNoRank;
}

// ---- parse + correct
constexpr int kSortParseNT = 256;
constexpr uint32_t kParseWaves = kSortParseNT / 64;
constexpr uint32_t kHalo = kSortParseHalo;
constexpr uint32_t kTileWords = (3 + kSortParseTile + kHalo + 3) / 4 + 1;   // (+ the dword an unaligned 4-byte read of the last bytes also touches)
constexpr uint32_t kTileRecs = kSortParseTile / 5 + 1;   // the shortest record is na = 0 with a 1-byte barcode

// dword at byte offset `off` (a multiple of 4 in ADDRESS terms, possibly outside [0, n)) of the input buffer: what lies
// outside the buffer reads as 0 and is never fetched
__device__ __forceinline__ uint32_t ld_dword_in(const uint8_t* bytes, uint64_t n, int64_t off) {
    if (off >= 0 && (uint64_t)off + 4 <= n) return *reinterpret_cast<const uint32_t*>(bytes + off);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (off + k >= 0 && (uint64_t)(off + k) < n) v |= (uint32_t)bytes[off + k] << (8 * k);
    return v;
}
__device__ __forceinline__ uint32_t lds32(const uint32_t* t, uint32_t off) {   // 4 bytes at byte offset off of the tile
    const uint32_t w = off >> 2, sh = off & 3u;
    const uint32_t lo = t[w];
    return sh ? __builtin_amdgcn_alignbyte(t[w + 1], lo, sh) : lo;
}
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kSortParseNT) void k_sort_parse(SortParseArgs a) {
    __shared__ uint32_t s_tile[kParseWaves][kTileWords];
    __shared__ uint16_t s_start[kParseWaves][kTileRecs];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t chunk = blockIdx.x * kParseWaves + wave;
    if (chunk >= a.n_chunks) return;   // (no workgroup barrier below: the waves of a block run chunks of different lengths)
    const SortChunk c = a.chunks[chunk];
    const uint32_t nb = c.nbytes, H = 4 + a.bc_bytes;   // the host checked 8 <= nb and chunk_off + nb <= n_bytes
    uint32_t* tile = s_tile[wave];
    uint16_t* starts = s_start[wave];
    uint32_t p = 8, seen = 0, kept = 0;          // wave-uniform
    uint32_t n0 = 0, multi = 0, uncorr = 0;      // per lane
    uint32_t err = 0;                            // per lane: a field out of range
    bool bad = false;                            // uniform: the records do not tile the chunk
    while (p < nb && !bad) {
        // stage [p, p + tile + halo) of the chunk, as aligned dwords
        const uint32_t span = nb - p < kSortParseTile + kHalo ? nb - p : kSortParseTile + kHalo;
        const uint64_t g = c.chunk_off + p;
        const uint32_t al = (uint32_t)((reinterpret_cast<uintptr_t>(a.bytes) + g) & 3u);
        const uint32_t nw = (al + span + 3) >> 2;
        for (uint32_t i = lane; i < nw; i += 64) tile[i] = ld_dword_in(a.bytes, a.n_bytes, (int64_t)g - al + 4ll * i);
        wave_lds_sync();
        // hop the na chain: record starts q (relative to p) below the tile's end
        uint32_t q = 0, nr = 0;
        while (q < kSortParseTile && p + q < nb) {
            if (nb - (p + q) < H) { bad = true; break; }             // a head that runs past the chunk
            const uint32_t na = lds32(tile, al + q);
            if (na > (nb - (p + q) - H) / 11u) { bad = true; break; }   // alignments that run past the chunk
            if (lane == 0) starts[nr] = (uint16_t)q;
            ++nr;
            q += H + 11u * na;
        }
        if (bad) break;
        if (seen + nr > c.nrec) { bad = true; break; }               // more records than the header says
        wave_lds_sync();
        for (uint32_t r0 = 0; r0 < nr; r0 += 64) {
            const uint32_t r = r0 + lane;
            bool keep = false;
            uint32_t bin = 0;
            uint64_t key = 0;
            if (r < nr) {
                const uint32_t o = al + starts[r];
                const uint32_t na = lds32(tile, o);
                if (na == 0) ++n0;
                else if (na > 1) ++multi;
                else {   // (the hop checked that the alignment's 11 bytes lie inside the chunk; they lie inside the halo)
                    uint64_t bc = lds32(tile, o + 4);
                    if (a.bc_bytes == 8) bc |= (uint64_t)lds32(tile, o + 8) << 32;
                    else if (a.bc_bytes < 4) bc &= (1u << (8 * a.bc_bytes)) - 1u;
                    const uint32_t ref = lds32(tile, o + H), start = lds32(tile, o + H + 5), flen = lds32(tile, o + H + 9) & 0xFFFFu;
                    if (ref >= a.ref_count) err = kErrRefRange;
                    else {
                        const uint2 ri = a.ref_info[ref];
                        if (start >= ri.x) err = kErrStartRange;
                        else {
                            const uint32_t rank = table_find(a, bc);
                            if (rank == kSortNoRank) ++uncorr;
                            else {
                                keep = true;
                                bin = ri.y + (start >> kSortBinShift);
                                key = ((uint64_t)(start & ((1u << kSortBinShift) - 1u)) << 47) | ((uint64_t)flen << 31) | rank;
                            }
                        }
                    }
                }
            }
            const uint64_t m = __ballot(keep);
            if (keep) {   // (seen + nr <= nrec, so the slot is one of the chunk's)
                const uint64_t slot = c.out_off + kept + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                a.o_bin[slot] = bin; a.o_key[slot] = key;
            }
            kept += (uint32_t)__popcll(m);
        }
        seen += nr;
        p += q;
        wave_lds_sync();   // (the next trip overwrites the tile)
    }
    if (!bad && (p != nb || seen != c.nrec)) bad = true;
    uint32_t e = bad ? kErrRecordWalk : err;
    for (int d = 32; d; d >>= 1) {
        const uint32_t o = __shfl_xor(e, d);
        if (e == 0 || (o != 0 && o < e)) e = o;   // (any lane's error; the smallest code, so that the message does not depend on the lane)
        n0 += __shfl_xor(n0, d); multi += __shfl_xor(multi, d); uncorr += __shfl_xor(uncorr, d);
    }
    if (e) { kept = 0; if (lane == 0) set_err(a.st, e, chunk); }
    for (uint32_t i = kept + lane; i < c.nrec; i += 64) a.o_bin[c.out_off + i] = kSortNoBin;
    if (lane == 0) {
        uint32_t* s = a.chunk_stat + 4ull * chunk;
        s[0] = n0; s[1] = multi; s[2] = uncorr; s[3] = kept;
    }
}

// ---- partition: histogram, scan, scatter.  Level 0 counts the position bins with global atomics (tens of thousands of
// counters that every workgroup shares); a re-partition level has 256 digits per segment and counts them in LDS first.
constexpr int kPartNT = 256;
constexpr uint32_t kPartItems = 16;   // keys per thread and trip of the grid

__global__ __launch_bounds__(kPartNT) void k_sort_hist(const SortSeg* __restrict__ segs, uint32_t bps, const uint64_t* __restrict__ keys,
                                                      const uint32_t* __restrict__ bins, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[256];
    const SortSeg sg = segs[blockIdx.x / bps];
    const uint32_t b = blockIdx.x % bps;
    if (bins) {
        for (uint64_t i = (uint64_t)b * kPartNT + threadIdx.x; i < sg.cnt; i += (uint64_t)bps * kPartNT) {
            const uint32_t d = bins[sg.off + i];
            if (d != kSortNoBin) atomicAdd(hist + sg.hist_base + d, 1u);
        }
        return;
    }
    s_h[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)b * kPartNT + threadIdx.x; i < sg.cnt; i += (uint64_t)bps * kPartNT)
        atomicAdd(&s_h[(uint32_t)(keys[sg.off + i] >> sg.shift) & 255u], 1u);
    __syncthreads();
    if (s_h[threadIdx.x]) atomicAdd(hist + sg.hist_base + threadIdx.x, s_h[threadIdx.x]);
}

// a workgroup per segment: cursor[d] = the segment's offset + the counts in front of digit d
__global__ __launch_bounds__(1024) void k_sort_scan(const SortSeg* __restrict__ segs, uint32_t n_sub, const uint32_t* __restrict__ hist,
                                                   uint32_t* __restrict__ cursor) {
    __shared__ uint32_t s_ws[1024 / 64];
    const SortSeg sg = segs[blockIdx.x];
    uint32_t carry = sg.off;
    for (uint32_t base = 0; base < n_sub; base += 1024) {
        const uint32_t d = base + threadIdx.x;
        const uint32_t v = d < n_sub ? hist[sg.hist_base + d] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan<1024>(v, s_ws, tot);
        if (d < n_sub) cursor[sg.hist_base + d] = carry + ex;
        carry += tot;
    }
}

// (the order inside a digit is whatever the atomics give: the leaf sort, or the next level, settles it)
__global__ __launch_bounds__(kPartNT) void k_sort_scatter(const SortSeg* __restrict__ segs, uint32_t bps, const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ bins, uint32_t* __restrict__ cursor, uint64_t* __restrict__ dst) {
    const SortSeg sg = segs[blockIdx.x / bps];
    const uint32_t b = blockIdx.x % bps;
    for (uint64_t i = (uint64_t)b * kPartNT + threadIdx.x; i < sg.cnt; i += (uint64_t)bps * kPartNT) {
        const uint64_t k = keys[sg.off + i];
        const uint32_t d = bins ? bins[sg.off + i] : (uint32_t)(k >> sg.shift) & 255u;
        if (d == kSortNoBin) continue;
        dst[atomicAdd(cursor + sg.hist_base + d, 1u)] = k;
    }
}

// AND and OR of a segment's keys: the bits in which they differ are and ^ or
__global__ __launch_bounds__(kPartNT) void k_sort_bits(const SortSeg* __restrict__ segs, uint32_t bps, const uint64_t* __restrict__ keys,
                                                      uint64_t* __restrict__ and_or) {
    const uint32_t si = blockIdx.x / bps, b = blockIdx.x % bps;
    const SortSeg sg = segs[si];
    uint64_t x = ~0ull, y = 0;
    for (uint64_t i = (uint64_t)b * kPartNT + threadIdx.x; i < sg.cnt; i += (uint64_t)bps * kPartNT) { const uint64_t k = keys[sg.off + i]; x &= k; y |= k; }
    for (int d = 32; d; d >>= 1) { x &= __shfl_xor(x, d); y |= __shfl_xor(y, d); }
    if ((threadIdx.x & 63u) == 0) {
        atomicAnd(reinterpret_cast<unsigned long long*>(and_or + 2ull * si), (unsigned long long)x);
        atomicOr(reinterpret_cast<unsigned long long*>(and_or + 2ull * si + 1), (unsigned long long)y);
    }
}

// ---- leaves: sort, run heads, run lengths (u32: a fragment seen 70 000 times counts 70 000)
template <int NT, uint32_t TILE>
__global__ __launch_bounds__(NT) void k_sort_leaf(const SortLeaf* __restrict__ leaves, const uint32_t* __restrict__ ids, uint64_t* __restrict__ buf_a,
                                                 uint64_t* __restrict__ buf_b, uint64_t* __restrict__ o_key, uint32_t* __restrict__ o_cnt,
                                                 uint32_t* __restrict__ o_n) {
    __shared__ uint32_t s_ws[NT / 64];
    __shared__ __attribute__((aligned(16))) uint64_t s_tile[TILE];
    const uint32_t li = ids[blockIdx.x];
    const SortLeaf lf = leaves[li];
    uint64_t* f = ((lf.flags & 1u) ? buf_b : buf_a) + lf.off;
    const uint32_t n = lf.cnt;
    if (lf.flags & 2u) {   // one run
        if (threadIdx.x == 0) { o_key[lf.off] = f[0]; o_cnt[lf.off] = n; o_n[li] = 1; }
        return;
    }
    tiled_bitonic_sort_by<NT, TILE>(f, n, [](uint64_t a, uint64_t b) { return a > b; }, s_tile);
    // run heads, compacted: the key, and for now the head's position
    uint32_t nh = 0;
    for (uint32_t base = 0; base < n; base += NT) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t h = (i < n) && (i == 0 || f[i] != f[i - 1]);
        uint32_t tot;
        const uint32_t ex = block_excl_scan<NT>(h, s_ws, tot);
        if (h) { o_key[lf.off + nh + ex] = f[i]; o_cnt[lf.off + nh + ex] = i; }
        nh += tot;
    }
    __syncthreads();
    // position -> run length = the next head's position - this one's (read both, then write: a slice of NT heads at a time)
    for (uint32_t base = 0; base < nh; base += NT) {
        const uint32_t j = base + threadIdx.x;
        uint32_t len = 0;
        if (j < nh) len = (j + 1 < nh ? o_cnt[lf.off + j + 1] : n) - o_cnt[lf.off + j];
        __syncthreads();
        if (j < nh) o_cnt[lf.off + j] = len;
    }
    if (threadIdx.x == 0) o_n[li] = nh;
}

// ---- the leaves' runs -> dense arrays in leaf order (= bin order, = the global order)
__global__ __launch_bounds__(256) void k_sort_emit(const SortLeaf* __restrict__ leaves, const uint32_t* __restrict__ leaf_out,
                                                  const uint64_t* __restrict__ i_key, const uint32_t* __restrict__ i_cnt,
                                                  const uint32_t* __restrict__ bin_base, uint32_t ref_count, const uint64_t* __restrict__ rank_bc,
                                                  uint32_t* __restrict__ o_ref, uint32_t* __restrict__ o_start, uint16_t* __restrict__ o_flen,
                                                  uint64_t* __restrict__ o_bc, uint32_t* __restrict__ o_cnt, unsigned long long* __restrict__ n_long) {
    const SortLeaf lf = leaves[blockIdx.x];
    const uint32_t dst = leaf_out[blockIdx.x], n = leaf_out[blockIdx.x + 1] - dst;
    // the reference of the bin: the last one whose first bin is not above it (a reference without bins shares its base with the next)
    uint32_t lo = 0, hi = ref_count;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (bin_base[mid] <= lf.bin) lo = mid; else hi = mid; }
    const uint32_t ref = lo, start_hi = (lf.bin - bin_base[ref]) << kSortBinShift;
    uint32_t lng = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const uint64_t k = i_key[lf.off + i];
        const uint32_t fl = (uint32_t)(k >> 31) & 0xFFFFu;
        o_ref[dst + i] = ref;
        o_start[dst + i] = start_hi | (uint32_t)(k >> 47);
        o_flen[dst + i] = (uint16_t)fl;
        o_bc[dst + i] = rank_bc[(uint32_t)k & 0x7FFFFFFFu];
        o_cnt[dst + i] = i_cnt[lf.off + i];
        lng += fl >= 2000u;   // rows the writer withholds (sort.rs:75)
    }
    for (int d = 32; d; d >>= 1) lng += __shfl_xor(lng, d);
    if ((threadIdx.x & 63u) == 0 && lng) atomicAdd(n_long, (unsigned long long)lng);
}

uint32_t blocks_per_seg(uint32_t max_cnt) {
    const uint64_t b = ((uint64_t)max_cnt + kPartNT * kPartItems - 1) / (kPartNT * kPartItems);
    return (uint32_t)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}

}  // namespace

void launch_sort_table(hipStream_t s, const uint64_t* observed, const uint32_t* rank, uint64_t n, uint64_t* tab_key, uint32_t* tab_val,
                       uint32_t tab_mask, DevStatus* st) {
    if (!n) return;
    const uint32_t grid = (uint32_t)((n + 255) / 256);
    AFQ_LAUNCH(k_sort_table_insert, grid, 256, s, observed, rank, n, tab_key, tab_val, tab_mask);
    AFQ_LAUNCH(k_sort_table_verify, grid, 256, s, observed, rank, n, tab_key, tab_val, tab_mask, st);
}

void launch_sort_parse(hipStream_t s, const SortParseArgs& a) {
    if (!a.n_chunks) return;
    AFQ_LAUNCH(k_sort_parse, (a.n_chunks + kParseWaves - 1) / kParseWaves, kSortParseNT, s, a);
}

void launch_sort_partition(hipStream_t s, const SortSeg* segs, uint32_t n_seg, uint32_t max_cnt, const uint64_t* keys, const uint32_t* bins,
                           uint32_t n_sub, uint32_t* hist, uint32_t* cursor, uint64_t* dst) {
    if (!n_seg || !max_cnt) return;
    const uint32_t bps = blocks_per_seg(max_cnt);
    AFQ_LAUNCH(k_sort_hist, n_seg * bps, kPartNT, s, segs, bps, keys, bins, hist);
    AFQ_LAUNCH(k_sort_scan, n_seg, 1024, s, segs, n_sub, hist, cursor);
    AFQ_LAUNCH(k_sort_scatter, n_seg * bps, kPartNT, s, segs, bps, keys, bins, cursor, dst);
}

void launch_sort_bits(hipStream_t s, const SortSeg* segs, uint32_t n_seg, uint32_t max_cnt, const uint64_t* keys, uint64_t* and_or) {
    if (!n_seg || !max_cnt) return;
    const uint32_t bps = blocks_per_seg(max_cnt);
    AFQ_LAUNCH(k_sort_bits, n_seg * bps, kPartNT, s, segs, bps, keys, and_or);
}

void launch_sort_leaves(hipStream_t s, const SortLeaf* leaves, const uint32_t* ids_small, uint32_t n_small, const uint32_t* ids_big, uint32_t n_big,
                        uint64_t* buf_a, uint64_t* buf_b, uint64_t* o_key, uint32_t* o_cnt, uint32_t* o_n) {
    if (n_small) AFQ_LAUNCH((k_sort_leaf<kSortSmallLeafNT, kSortSmallLeaf>), n_small, kSortSmallLeafNT, s, leaves, ids_small, buf_a, buf_b, o_key, o_cnt, o_n);
    if (n_big) AFQ_LAUNCH((k_sort_leaf<kSortLeafNT, kSortLeafCap>), n_big, kSortLeafNT, s, leaves, ids_big, buf_a, buf_b, o_key, o_cnt, o_n);
}

void launch_sort_emit(hipStream_t s, const SortLeaf* leaves, uint32_t n_leaves, const uint32_t* leaf_out, const uint64_t* i_key, const uint32_t* i_cnt,
                      const uint32_t* bin_base, uint32_t ref_count, const uint64_t* rank_bc, uint32_t* o_ref, uint32_t* o_start, uint16_t* o_flen,
                      uint64_t* o_bc, uint32_t* o_cnt, unsigned long long* n_long) {
    if (!n_leaves) return;
    AFQ_LAUNCH(k_sort_emit, n_leaves, 256, s, leaves, leaf_out, i_key, i_cnt, bin_base, ref_count, rank_bc, o_ref, o_start, o_flen, o_bc, o_cnt, n_long);
}

}  // namespace afq
