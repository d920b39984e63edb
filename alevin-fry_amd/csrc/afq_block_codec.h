// afq_block_codec.h — what the block decoders and the snappy encoder share on the device (afq_snappy.hip, afq_inflate.hip): the
// CRC of a block by one wave - a lane takes a contiguous slice bytewise through a 1 KiB table in LDS, the slices combine by the
// linearity of the CRC register,  state(A||B) = state(A) x^(8 |B|) ^ state0(B)  modulo the polynomial - with the polynomial as a
// template parameter (CRC-32C for the snappy frame format, gzip's CRC-32 for BGZF); the LDS window a body is read through; and
// the write-out of a block staged in LDS at its destination's residue.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace afq {

constexpr uint32_t kCrc32cPoly = 0x82F63B78u;   // CRC-32C (Castagnoli), reflected
constexpr uint32_t kCrc32Poly = 0xEDB88320u;    // CRC-32 of gzip and zlib, reflected

// a b modulo the polynomial; bit 31 is x^0 (the register's bit order)
template <uint32_t Poly>
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ Poly : b >> 1;
    }
    return p;
}
// x^(8 n): what n zero bytes do to the register
template <uint32_t Poly>
__host__ __device__ constexpr uint32_t gf_pow_x8(uint32_t n) {
    uint32_t r = 0x80000000u, b = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1u) r = gf_mul<Poly>(r, b);
        b = gf_mul<Poly>(b, b);
    }
    return r;
}

__device__ __forceinline__ uint32_t ld4(const uint8_t* p) {
    uint32_t w;
    __builtin_memcpy(&w, p, 4);
    return w;
}
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the bytewise CRC table, 256 words, filled by one wave
template <uint32_t Poly>
__device__ __forceinline__ void crc_table_fill(uint32_t* s_tab, uint32_t lane) {
    for (uint32_t i = lane; i < 256; i += 64) {
        uint32_t c = i;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ Poly : c >> 1;
        s_tab[i] = c;
    }
}
// The CRC of src[0, n) by one wave: lane l takes the slice [l sl, (l + 1) sl) (sl a multiple of 4, 64 sl >= n), the slices
// combine by the linearity of the register.  full_shift: [k] = x^(8 k sl) for a block of exactly 64 sl bytes (the shifts are
// constants then), or null: square-and-multiply.
template <uint32_t Poly>
__device__ __forceinline__ uint32_t wave_crc(const uint8_t* src, uint32_t n, uint32_t sl, const uint32_t* full_shift, const uint32_t* s_tab, uint32_t lane) {
    const uint32_t b = min(n, lane * sl), e = min(n, b + sl);
    uint32_t st = lane == 0 ? 0xFFFFFFFFu : 0u;
    uint32_t p = b;
    for (; p + 4 <= e; p += 4) {
        st ^= ld4(src + p);
#pragma unroll
        for (int k = 0; k < 4; ++k) st = s_tab[st & 255u] ^ (st >> 8);
    }
    for (; p < e; ++p) st = s_tab[(st ^ src[p]) & 255u] ^ (st >> 8);
    st = gf_mul<Poly>(st, full_shift ? full_shift[63 - lane] : gf_pow_x8<Poly>(n - e));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) st ^= __shfl_xor(st, d);
    return ~st;
}
// the slice of a block of n <= 65536 bytes staged in LDS: whole words, and an odd number of them from slice to slice, so that
// the lanes' reads spread over the banks
__device__ __forceinline__ uint32_t crc_slice_lds(uint32_t n) {
    uint32_t sl = ((n + 63) / 64 + 3) & ~3u;
    if (!(sl & 4u)) sl += 4;
    return sl;
}

// g[0, n) into the window s_in, at the residue of its address: 16-byte loads between a bytewise head and tail, none of them
// outside the n bytes.  Returns where g[0] stands.  The window holds n + 16 bytes at least; `threads` is the workgroup's size.
__device__ __forceinline__ const uint8_t* window_fill(uint4* s_in, const uint8_t* g, uint32_t n, uint32_t lane, uint32_t threads) {
    __syncthreads();   // the reads of what the window held
    uint8_t* sw = (uint8_t*)s_in + ((uintptr_t)g & 15);
    const uint32_t head = min(n, (uint32_t)((16 - ((uintptr_t)g & 15)) & 15));
    if (lane < head) sw[lane] = g[lane];
    const uint32_t nvec = (n - head) / 16;
    for (uint32_t k = lane; k < nvec; k += threads) *(uint4*)(sw + head + 16 * k) = *(const uint4*)(g + head + 16ull * k);
    const uint32_t done = head + 16 * nvec;
    if (lane < n - done) sw[done + lane] = g[done + lane];
    __syncthreads();
    return sw;
}

// so[0, n), staged in LDS at d's residue ((uintptr_t)so & 15 == (uintptr_t)d & 15), to d: 16-byte stores between a bytewise
// head and tail, so that both sides of a 16-byte move are aligned
__device__ __forceinline__ void staged_write_out(uint8_t* d, const uint8_t* so, uint32_t n, uint32_t lane, uint32_t threads) {
    const uint32_t head = min(n, (uint32_t)((16 - ((uintptr_t)d & 15)) & 15));
    if (lane < head) d[lane] = so[lane];
    const uint32_t nvec = (n - head) / 16;
    for (uint32_t k = lane; k < nvec; k += threads) *(uint4*)(d + head + 16 * k) = *(const uint4*)(so + head + 16 * k);
    const uint32_t done = head + 16 * nvec;
    if (lane < n - done) d[done + lane] = so[done + lane];
}

}  // namespace afq
