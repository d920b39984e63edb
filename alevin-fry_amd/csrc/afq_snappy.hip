// afq_snappy.hip — a snappy frame stream from bytes that sit on the device (what the reference's `collate -c` writes through
// snap::write::FrameEncoder, collate.rs:523-554): stream identifier, then one data chunk per kSnappyBlock bytes of input, each
// `type, len24, masked CRC-32C of the uncompressed bytes, body`, the body a raw snappy block (type 0x00) or the bytes themselves
// (type 0x01) wherever the raw block would not be shorter than they are.
//
// Three kernels, no allocation atomic, so the stream is a function of the input alone:
//   - k_snappy_blocks: ONE WAVE per frame chunk (a workgroup is one wave and takes one chunk).  CRC first: a lane takes a
//     contiguous slice (1 KiB of a full chunk), bytewise through a 1 KiB table in LDS; the slices combine by the linearity of the
//     CRC register,  state(A||B) = state(A) x^(8 |B|) ^ state0(B)  modulo the polynomial - constants for the slices of a full
//     chunk, square-and-multiply for the ragged last one.  Then the block: a table of last positions in LDS (the CRC table's
//     memory, cleared), keyed by a hash of 4 bytes.  A step: lane l hashes the 4 bytes at pos + l, reads its candidate, compares
//     the candidate's 4 bytes; a ballot picks the first lane that matched; the wave extends that match 64 bytes a compare; the
//     pending literal and the copy (elements of at most 64; the 1-byte-offset form for 4..11 bytes from less than 2048 back, the
//     2-byte-offset form otherwise) go into the chunk's slot; the lanes stepped over enter their positions.  Two lanes of a step
//     that share a slot: atomicMax, the later position wins whatever the order of the LDS operations.  The table is cleared per
//     chunk and holds positions relative to the chunk, entered only behind the reads of the step, so a candidate lies in the chunk
//     and in front of its lane's position by construction (and is tested for it).  No load passes the chunk's end, so none passes
//     the input's: 4-byte loads stop at n - 4, the extension compares bytes below n.  As soon as the block would reach the
//     chunk's own length it is abandoned: the chunk is stored (type 0x01) and the pack kernel takes the input's bytes.
//   - k_snappy_layout: one workgroup scans 8 + body bytes over the chunks, 10 in front: where every chunk header stands.
//   - k_snappy_pack: a workgroup per chunk writes the header and copies the body (slot or input) to its place - any residue of
//     the destination, 16-byte stores between a bytewise head and tail.
#include <hip/hip_runtime.h>

#include "afq_common.h"
#include "afq_kernels.h"
#include "afq_prims.h"

namespace afq {

namespace {

constexpr uint32_t kCrcPoly = 0x82F63B78u;     // CRC-32C, reflected
constexpr uint32_t kSliceFull = kSnappyBlock / 64;
static_assert(kSnappyBlock <= 65536 && kSliceFull % 4 == 0, "a frame chunk holds at most 65536 bytes; a full chunk's slices are whole words");
static_assert(kSnappySlot >= 32 + kSnappyBlock + kSnappyBlock / 6 && kSnappySlot % 16 == 0, "a slot holds snappy's worst case");

// a b modulo the polynomial; bit 31 is x^0 (the register's bit order)
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// x^(8 n): what n zero bytes do to the register
__host__ __device__ constexpr uint32_t gf_pow_x8(uint32_t n) {
    uint32_t r = 0x80000000u, b = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1u) r = gf_mul(r, b);
        b = gf_mul(b, b);
    }
    return r;
}
struct ShiftTab { uint32_t v[64]; };
constexpr ShiftTab make_shift_tab() {
    ShiftTab t{};
    for (uint32_t k = 0; k < 64; ++k) t.v[k] = gf_pow_x8(k * kSliceFull);
    return t;
}
__constant__ ShiftTab c_shift = make_shift_tab();   // [k]: k full slices behind a lane's

__device__ __forceinline__ uint32_t ld4(const uint8_t* p) {
    uint32_t w;
    __builtin_memcpy(&w, p, 4);
    return w;
}

__device__ __forceinline__ uint32_t literal_size(uint32_t len) { return len == 0 ? 0 : len + (len <= 60 ? 1 : len <= 256 ? 2 : 3); }

// the wave writes a literal of len > 0 bytes at dst; returns its size
__device__ __forceinline__ uint32_t emit_literal(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t lane) {
    const uint32_t m = len - 1;
    uint32_t h;
    if (m < 60) {
        h = 1;
        if (lane == 0) dst[0] = (uint8_t)(m << 2);
    } else if (m < 256) {
        h = 2;
        if (lane == 0) { dst[0] = 60u << 2; dst[1] = (uint8_t)m; }
    } else {
        h = 3;
        if (lane == 0) { dst[0] = 61u << 2; dst[1] = (uint8_t)m; dst[2] = (uint8_t)(m >> 8); }
    }
    for (uint32_t i = lane; i < len; i += 64) dst[h + i] = src[i];
    return h + len;
}

// a copy of len >= 4 from off back as elements of at most kSnappyMaxCopy: k64 of 64, one of 60 where that leaves 5..7, the rest
struct CopyPlan { uint32_t k64, has60, last, size, elems; };
__device__ __forceinline__ CopyPlan plan_copy(uint32_t off, uint32_t len) {
    CopyPlan c;
    c.k64 = len < 68 ? 0 : (len - 68) / 64 + 1;
    uint32_t r = len - 64 * c.k64;   // 4..67
    c.has60 = r > 64;
    if (c.has60) r -= 60;
    c.last = r;                      // 4..64
    const uint32_t last_size = (r <= 11 && off < 2048) ? 2 : 3;
    c.size = 3 * (c.k64 + c.has60) + last_size;
    c.elems = c.k64 + c.has60 + 1;
    return c;
}
__device__ __forceinline__ void emit_copy(uint8_t* dst, uint32_t off, const CopyPlan& c, uint32_t lane) {
    const uint8_t lo = (uint8_t)off, hi = (uint8_t)(off >> 8);
    for (uint32_t k = lane; k < c.k64; k += 64) {
        uint8_t* d = dst + 3 * k;
        d[0] = (uint8_t)(((kSnappyMaxCopy - 1) << 2) | 2); d[1] = lo; d[2] = hi;
    }
    if (lane == 0) {
        uint8_t* d = dst + 3 * c.k64;
        if (c.has60) { d[0] = (uint8_t)((59u << 2) | 2); d[1] = lo; d[2] = hi; d += 3; }
        if (c.last <= 11 && off < 2048) { d[0] = (uint8_t)(1u | ((c.last - 4) << 2) | ((off >> 8) << 5)); d[1] = lo; }
        else { d[0] = (uint8_t)(((c.last - 1) << 2) | 2); d[1] = lo; d[2] = hi; }
    }
}

__global__ __launch_bounds__(64) void k_snappy_blocks(const uint8_t* __restrict__ in, uint64_t n_total, uint8_t* __restrict__ slots, SnappyMeta* __restrict__ meta) {
    __shared__ uint32_t s_tab[kSnappyHashSlots];
    const uint32_t lane = threadIdx.x;
    const uint64_t blk = blockIdx.x;
    const uint64_t at = blk * kSnappyBlock;
    const uint8_t* src = in + at;
    const uint64_t left = n_total - at;
    const uint32_t n = left < kSnappyBlock ? (uint32_t)left : kSnappyBlock;   // 1..kSnappyBlock
    // ---- CRC-32C of the chunk
    for (uint32_t i = lane; i < 256; i += 64) {
        uint32_t c = i;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        s_tab[i] = c;
    }
    __syncthreads();
    uint32_t masked_crc;
    {
        const bool full = n == kSnappyBlock;
        const uint32_t sl = full ? kSliceFull : (((n + 63) / 64 + 3) & ~3u);
        const uint32_t b = min(n, lane * sl), e = min(n, b + sl);
        uint32_t st = lane == 0 ? 0xFFFFFFFFu : 0u;
        uint32_t p = b;
        for (; p + 4 <= e; p += 4) {
            st ^= ld4(src + p);
#pragma unroll
            for (int k = 0; k < 4; ++k) st = s_tab[st & 255u] ^ (st >> 8);
        }
        for (; p < e; ++p) st = s_tab[(st ^ src[p]) & 255u] ^ (st >> 8);
        st = gf_mul(st, full ? c_shift.v[63 - lane] : gf_pow_x8(n - e));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) st ^= __shfl_xor(st, d);
        const uint32_t crc = ~st;
        masked_crc = ((crc >> 15) | (crc << 17)) + 0xa282ead8u;
    }
    // ---- the raw block
    __syncthreads();
    for (uint32_t i = lane; i < kSnappyHashSlots; i += 64) s_tab[i] = 0;   // 0: no position; else position + 1
    __syncthreads();
    uint8_t* dst = slots + blk * kSnappySlot;
    uint32_t op;   // the length's uvarint
    if (n < 128) {
        op = 1;
        if (lane == 0) dst[0] = (uint8_t)n;
    } else if (n < 16384) {
        op = 2;
        if (lane == 0) { dst[0] = (uint8_t)(n | 0x80u); dst[1] = (uint8_t)(n >> 7); }
    } else {
        op = 3;
        if (lane == 0) { dst[0] = (uint8_t)(n | 0x80u); dst[1] = (uint8_t)((n >> 7) | 0x80u); dst[2] = (uint8_t)(n >> 14); }
    }
    const uint32_t lim = n >= 4 ? n - 3 : 0;   // positions below lim have 4 bytes inside the chunk
    uint32_t pos = 0, lit = 0, n_lit = 0, n_cp = 0;
    bool stored = false;
    uint32_t v = lane < lim ? ld4(src + lane) : 0;
    while (pos < lim) {
        const uint32_t p = pos + lane;
        const bool valid = p < lim;
        const uint32_t vn = p + 64 < lim ? ld4(src + p + 64) : 0;   // the next step's, should this one find nothing
        const uint32_t h = (v * 0x1e35a7bdu) >> (32 - kSnappyHashBits);
        const uint32_t cand = valid ? s_tab[h] : 0;
        const bool ok = cand != 0 && cand - 1 < p && ld4(src + (cand - 1)) == v;
        const uint64_t m = __ballot(ok);
        if (!m) {
            if (valid) atomicMax(&s_tab[h], p + 1);
            pos += 64;
            v = vn;
            continue;
        }
        const uint32_t f = (uint32_t)__ffsll((unsigned long long)m) - 1;
        const uint32_t mp = pos + f;
        const uint32_t off = mp - ((uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(cand, (int)f)) - 1);
        uint32_t len = 4;
        for (;;) {
            const uint32_t q = mp + len + lane;
            const bool eq = q < n && src[q] == src[q - off];
            const uint64_t ne = __ballot(!eq);
            if (ne) { len += (uint32_t)__ffsll((unsigned long long)ne) - 1; break; }
            len += 64;
        }
        const uint32_t ll = mp - lit;
        const CopyPlan cp = plan_copy(off, len);
        if (op + literal_size(ll) + cp.size >= n) { stored = true; break; }
        if (ll) op += emit_literal(dst + op, src + lit, ll, lane);
        emit_copy(dst + op, off, cp, lane);
        op += cp.size;
        n_lit += ll; n_cp += cp.elems;
        if (valid && p < mp + len) atomicMax(&s_tab[h], p + 1);   // the lanes stepped over
        pos = mp + len;
        lit = pos;
        v = pos + lane < lim ? ld4(src + pos + lane) : 0;
    }
    if (!stored) {
        const uint32_t ll = n - lit;
        if (op + literal_size(ll) >= n) stored = true;
        else if (ll) { op += emit_literal(dst + op, src + lit, ll, lane); n_lit += ll; }
    }
    if (lane == 0) meta[blk] = stored ? SnappyMeta{n | kSnappyStored, masked_crc, 0, 0} : SnappyMeta{op, masked_crc, n_lit, n_cp};
}

__global__ __launch_bounds__(1024) void k_snappy_layout(const SnappyMeta* __restrict__ meta, uint64_t n_blocks, uint64_t* __restrict__ off) {
    __shared__ uint32_t ws[16];
    uint64_t base = 10;
    for (uint64_t t0 = 0; t0 < n_blocks; t0 += 1024) {   // (1024 chunks: below 2^27 bytes)
        const uint64_t i = t0 + threadIdx.x;
        const uint32_t v = i < n_blocks ? 8 + (meta[i].body & ~kSnappyStored) : 0;
        uint32_t tot;
        const uint32_t ex = block_excl_scan<1024>(v, ws, tot);
        if (i < n_blocks) off[i] = base + ex;
        base += tot;
    }
    if (threadIdx.x == 0) off[n_blocks] = base;
}

constexpr int kPackNT = 256;
__global__ __launch_bounds__(kPackNT) void k_snappy_pack(const uint8_t* __restrict__ in, const uint8_t* __restrict__ slots, const SnappyMeta* __restrict__ meta,
                                                         const uint64_t* __restrict__ off, uint8_t* __restrict__ out) {
    const uint64_t blk = blockIdx.x;
    const uint32_t t = threadIdx.x;
    const SnappyMeta m = meta[blk];
    const bool stored = (m.body & kSnappyStored) != 0;
    const uint32_t len = m.body & ~kSnappyStored;
    uint8_t* d = out + off[blk];
    if (blk == 0 && t >= 16 && t < 26) {
        const uint8_t id[10] = {0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59};
        out[t - 16] = id[t - 16];
    }
    if (t < 8) {
        const uint32_t l4 = len + 4;
        const uint64_t hdr = (uint64_t)(stored ? 1u : 0u) | (uint64_t)l4 << 8 | (uint64_t)m.crc << 32;
        d[t] = (uint8_t)(hdr >> (8 * t));
    }
    d += 8;
    const uint8_t* s = stored ? in + blk * kSnappyBlock : slots + blk * kSnappySlot;
    const uint32_t head = min(len, (uint32_t)((16 - ((uintptr_t)d & 15)) & 15));
    if (t < head) d[t] = s[t];
    const uint32_t nvec = (len - head) / 16;
    for (uint32_t k = t; k < nvec; k += kPackNT) {
        uint4 w;
        __builtin_memcpy(&w, s + head + 16ull * k, 16);
        *(uint4*)(d + head + 16ull * k) = w;
    }
    const uint32_t done = head + 16 * nvec;
    if (t < len - done) d[done + t] = s[done + t];
}

}  // namespace

void launch_snappy_blocks(hipStream_t s, const uint8_t* in, uint64_t n, uint64_t n_blocks, uint8_t* slots, SnappyMeta* meta) {
    if (n_blocks) AFQ_LAUNCH(k_snappy_blocks, (uint32_t)n_blocks, 64, s, in, n, slots, meta);
}
void launch_snappy_layout(hipStream_t s, const SnappyMeta* meta, uint64_t n_blocks, uint64_t* off) {
    if (n_blocks) AFQ_LAUNCH(k_snappy_layout, 1, 1024, s, meta, n_blocks, off);
}
void launch_snappy_pack(hipStream_t s, const uint8_t* in, uint64_t n_blocks, const uint8_t* slots, const SnappyMeta* meta, const uint64_t* off, uint8_t* out) {
    if (n_blocks) AFQ_LAUNCH(k_snappy_pack, (uint32_t)n_blocks, kPackNT, s, in, slots, meta, off, out);
}

}  // namespace afq
