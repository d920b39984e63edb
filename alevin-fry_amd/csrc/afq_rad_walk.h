// afq_rad_walk.h — what the wave-per-chunk walks of an uncollated RNA RAD share (k_gpl_parse, afq_gpl.hip; k_gpl_multi_parse,
// afq_gpl_multi.hip; the collate walks, single- and multi-barcode, afq_collate.hip; the scATAC collate walks, afq_atac_collate.hip): checked loads of the input
// buffer, unaligned reads of the LDS tile, the wave's LDS fence, the orientation test, sort_table_find (the probe of a
// launch_sort_table table), rad_walk_chunk (the whole GPL walk as a template over what is read of a record's head), and ByteOut,
// the byte stream the collate write walks store through.
#pragma once
#include <hip/hip_runtime.h>

#include "afq_kernels.h"

namespace afq {

// dword at byte offset `off` (a multiple of 4 in ADDRESS terms, possibly outside [0, n)) of the input buffer: what lies
// outside the buffer reads as 0 and is never fetched
__device__ __forceinline__ uint32_t gpl_ld_dword_in(const uint8_t* bytes, uint64_t n, int64_t off) {
    if (off >= 0 && (uint64_t)off + 4 <= n) return *reinterpret_cast<const uint32_t*>(bytes + off);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (off + k >= 0 && (uint64_t)(off + k) < n) v |= (uint32_t)bytes[off + k] << (8 * k);
    return v;
}
// 4 bytes at ANY byte offset g of the buffer (g + 4 <= n: the caller checked), as two aligned dwords
__device__ __forceinline__ uint32_t gpl_ld_u32(const uint8_t* bytes, uint64_t n, uint64_t g) {
    const uint32_t sh = (uint32_t)((reinterpret_cast<uintptr_t>(bytes) + g) & 3u);
    const int64_t base = (int64_t)g - sh;
    const uint32_t lo = gpl_ld_dword_in(bytes, n, base);
    if (!sh) return lo;
    return __builtin_amdgcn_alignbyte(gpl_ld_dword_in(bytes, n, base + 4), lo, sh);
}
__device__ __forceinline__ uint32_t gpl_lds32(const uint32_t* t, uint32_t off) {   // 4 bytes at byte offset off of the tile
    const uint32_t w = off >> 2, sh = off & 3u;
    const uint32_t lo = t[w];
    return sh ? __builtin_amdgcn_alignbyte(t[w + 1], lo, sh) : lo;
}
__device__ __forceinline__ void gpl_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// does alignment word w speak for the expected orientation?  (bit 31 set: the read maps forward)
__device__ __forceinline__ bool gpl_word_fits(uint32_t w, uint32_t ori) { return ori == kGplOriFw ? (w >> 31) != 0 : (w >> 31) == 0; }
// the open-addressing probe of a launch_sort_table table: key's value, or kSortNoRank when the table has no such key (the key is
// not the all-ones free mark: a caller whose keys can be all-ones carries that one beside the table)
__device__ __forceinline__ uint32_t sort_table_find(const uint64_t* __restrict__ tab_key, const uint32_t* __restrict__ tab_val, uint32_t mask, uint64_t key) {
    uint32_t slot = sort_hash_bc(key) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {   // (at most half the slots are taken: an empty one ends the probe)
        const uint64_t kk = tab_key[slot];
        if (kk == key) return tab_val[slot];
        if (kk == kSortEmptyKey) return kSortNoRank;
        slot = (slot + 1) & mask;
    }
    return kSortNoRank;
}

// The walk of one mapper chunk by one wave, as k_gpl_parse (afq_gpl.hip) does it, for kernels that want other fields of the head
// (k_gpl_multi_parse, afq_gpl_multi.hip).  k_gpl_parse keeps its own text of the walk: run through this template it compiled to the
// same registers and LDS but measured 15 % slower (4.61 -> 5.29 ms at 5 x 10^7 records, the two builds alternating in one run; the
// instructions differ only in the exec-mask bookkeeping around the hop loop), and nothing in this change may slow the single-barcode
// pass.  The chunk is staged
// through LDS a tile at a time, a tile BEGINS at a record start, the record starts inside it are found by hopping the na fields in
// LDS (wave-uniform), then a lane per record decides whether the record is compatible with the expected orientation.
// Which record takes which route to that test (cellfilter.rs:1698-1771):
//   - expected_ori == both: no alignment word is read; every record is compatible, na == 0 included.
//   - na == 0 under fw / rc: not compatible; nothing to read.
//   - na <= kGplLaneAlns: the record's own lane reads the words from LDS.  The halo is sized so that the whole list of such
//     a record is staged even when the record starts on the tile's last byte with the widest fields (the callers' static_assert).
//   - na > kGplLaneAlns, however large (nothing bounds na) and wherever the list ends: a LONG record.  After the lanes' pass
//     the wave takes the long records of the batch one by one and its 64 lanes stride the record's alignment words in
//     global memory, stopping at the first trip with a fitting word.  The hop has checked that the list lies inside the
//     chunk, and the host that the chunk lies inside the buffer, before any of it is read.
// H is the bytes of a record's head (na and the fields behind it), A those of an alignment.  The host checked 8 <= nbytes and
// chunk_off + nbytes <= n_bytes.  `tile` holds kRadWalkTileWords dwords and `starts` kRadWalkTileRecs entries, both the wave's own.
// load_head(o) reads what the caller wants of the head of the lane's record, at byte offset o of the tile; it runs beside the read
// of na, BEFORE the orientation test, so that its loads are in flight while the alignment words are read (the walk is bound by
// the latency of a batch's dependent reads, not by bytes).  per_batch(head, na, keep) runs once per batch of up to 64 records WITH
// EVERY LANE OF THE WAVE IN IT (it may ballot): keep says whether the lane has a record and that record is compatible; a lane
// without a record gets a value-initialised head.  `seen` and `n_long` count the records and the long ones (wave-uniform).
// Returns false when the records do not tile the chunk or do not number nrec; whatever per_batch did by then is the caller's to
// discard.
constexpr uint32_t kRadWalkTileWords = (3 + kGplParseTile + kGplParseHalo + 3) / 4 + 1;   // (+ the dword an unaligned 4-byte read of the last bytes also touches)
constexpr uint32_t kRadWalkTileRecs = kGplParseTile / 6 + 1;   // the shortest record: na = 0 and two bytes of fields
template <class LoadHead, class PerBatch>
__device__ __forceinline__ bool rad_walk_chunk(const uint8_t* bytes, uint64_t n_bytes, const SortChunk& c, uint32_t H, uint32_t A, uint32_t expected_ori,
                                               uint32_t* tile, uint16_t* starts, uint32_t lane, uint32_t& seen, uint32_t& n_long, LoadHead&& load_head,
                                               PerBatch&& per_batch) {
    const uint32_t nb = c.nbytes;
    uint32_t p = 8;      // wave-uniform
    bool bad = false;    // uniform: the records do not tile the chunk
    while (p < nb && !bad) {
        // stage [p, p + tile + halo) of the chunk, as aligned dwords
        const uint32_t span = nb - p < kGplParseTile + kGplParseHalo ? nb - p : kGplParseTile + kGplParseHalo;
        const uint64_t g = c.chunk_off + p;
        const uint32_t al = (uint32_t)((reinterpret_cast<uintptr_t>(bytes) + g) & 3u);
        const uint32_t nw = (al + span + 3) >> 2;
        for (uint32_t i = lane; i < nw; i += 64) tile[i] = gpl_ld_dword_in(bytes, n_bytes, (int64_t)g - al + 4ll * i);
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
            decltype(load_head(0u)) head{};
            if (r < nr) {
                ro = starts[r];
                const uint32_t o = al + ro;
                na = gpl_lds32(tile, o);
                head = load_head(o);
                if (expected_ori == kGplOriBoth) keep = true;
                else if (na == 0) keep = false;
                else if (na <= kGplLaneAlns) {   // (ro + H + A * na <= span: the record lies inside the chunk, and the halo holds it)
                    for (uint32_t j = 0; j < na && !keep; ++j) keep = gpl_word_fits(gpl_lds32(tile, o + H + A * j), expected_ori);
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
                    const bool h = j < lna && gpl_word_fits(gpl_ld_u32(bytes, n_bytes, first + (uint64_t)A * j), expected_ori);
                    hit = __ballot(h) != 0;
                }
                if ((int)lane == src) keep = hit;
            }
            per_batch(head, na, keep);   // (seen + nr <= nrec: a batch never holds more records than the chunk has slots left)
        }
        seen += nr;
        p += q;
        gpl_wave_lds_sync();   // (the next trip overwrites the tile)
    }
    if (!bad && (p != nb || seen != c.nrec)) bad = true;
    return !bad;
}

// A little-endian byte stream to an address of any alignment.  At most 7 bytes wait in acc; whatever is stored is stored with
// the widest naturally aligned store that holds only bytes of this stream.
struct ByteOut {
    uint8_t* p; uint64_t acc; uint32_t n;
    __device__ __forceinline__ void step() {   // store 1, 2 or 4 of the waiting bytes (n >= 1; 4 only when n >= 4)
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
        if (!mis && n >= 4) { *reinterpret_cast<uint32_t*>(p) = (uint32_t)acc; p += 4; acc >>= 32; n -= 4; }
        else if (!(mis & 1u) && n >= 2) { *reinterpret_cast<uint16_t*>(p) = (uint16_t)acc; p += 2; acc >>= 16; n -= 2; }
        else { *p = (uint8_t)acc; p += 1; acc >>= 8; n -= 1; }
    }
    __device__ __forceinline__ void put(uint32_t v, uint32_t nb) {   // the low nb (1..4) bytes of v
        if (nb < 4) v &= (1u << (8 * nb)) - 1u;
        acc |= (uint64_t)v << (8 * n);
        n += nb;
        while (n >= 4) step();
    }
    __device__ __forceinline__ void put_field(uint64_t v, uint32_t width) {   // width 1, 2, 4 or 8
        put((uint32_t)v, width < 4 ? width : 4);
        if (width == 8) put((uint32_t)(v >> 32), 4);
    }
    __device__ __forceinline__ void flush() { while (n) step(); }
};
// the position bytes (e of them: 0, 1, 2, 4 or 8) behind an alignment word, into the stream: from the tile, from global memory
__device__ __forceinline__ void put_extra_lds(ByteOut& w, const uint32_t* tile, uint32_t off, uint32_t e) {
    if (!e) return;
    w.put(gpl_lds32(tile, off), e < 4 ? e : 4);
    if (e == 8) w.put(gpl_lds32(tile, off + 4), 4);
}
__device__ __forceinline__ void put_extra_glb(ByteOut& w, const uint8_t* bytes, uint64_t n, uint64_t g, uint32_t e) {
    if (!e) return;
    w.put(gpl_ld_u32(bytes, n, g), e < 4 ? e : 4);   // (bytes past the buffer read as 0 and are cut off by put)
    if (e == 8) w.put(gpl_ld_u32(bytes, n, g + 4), 4);
}

}  // namespace afq
