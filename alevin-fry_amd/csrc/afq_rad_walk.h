// afq_rad_walk.h — what the wave-per-chunk walks of an uncollated RNA RAD share (k_gpl_parse, afq_gpl.hip; the collate walks,
// afq_collate.hip; the scATAC collate walks, afq_atac_collate.hip): checked loads of the input buffer, unaligned reads of the LDS
// tile, the wave's LDS fence, the orientation test, and ByteOut, the byte stream both collate write walks store through.
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

}  // namespace afq
