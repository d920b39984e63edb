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
// And the way back, k_snappy_decode (below, with its own account): a planned frame stream on the device -> its bytes.
#include <hip/hip_runtime.h>

#include "afq_block_codec.h"
#include "afq_common.h"
#include "afq_kernels.h"
#include "afq_prims.h"
#include "afq_rad_walk.h"
#include "afq_snappy_elem.h"

namespace afq {

namespace {

constexpr uint32_t kSliceFull = kSnappyBlock / 64;
static_assert(kSnappyBlock <= 65536 && kSliceFull % 4 == 0, "a frame chunk holds at most 65536 bytes; a full chunk's slices are whole words");
static_assert(kSnappySlot >= 32 + kSnappyBlock + kSnappyBlock / 6 && kSnappySlot % 16 == 0, "a slot holds snappy's worst case");

struct ShiftTab { uint32_t v[64]; };
constexpr ShiftTab make_shift_tab() {
    ShiftTab t{};
    for (uint32_t k = 0; k < 64; ++k) t.v[k] = gf_pow_x8<kCrc32cPoly>(k * kSliceFull);
    return t;
}
__constant__ ShiftTab c_shift = make_shift_tab();   // [k]: k full slices behind a lane's

// The masked CRC-32C of src[0, n) by one wave (wave_crc of afq_block_codec.h).  full: n = kSnappyBlock and sl = kSliceFull, the
// shifts are constants.
__device__ __forceinline__ uint32_t wave_masked_crc(const uint8_t* src, uint32_t n, uint32_t sl, bool full, const uint32_t* s_tab, uint32_t lane) {
    const uint32_t crc = wave_crc<kCrc32cPoly>(src, n, sl, full ? c_shift.v : nullptr, s_tab, lane);
    return ((crc >> 15) | (crc << 17)) + 0xa282ead8u;
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
    crc_table_fill<kCrc32cPoly>(s_tab, lane);
    __syncthreads();
    const bool full = n == kSnappyBlock;
    const uint32_t masked_crc = wave_masked_crc(src, n, full ? kSliceFull : (((n + 63) / 64 + 3) & ~3u), full, s_tab, lane);
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

// ---------------------------------------------------------------------------------------------------------------- the decoder
// k_snappy_decode: ONE WAVE per data chunk of a planned frame stream (the plan is the host's walk over the chunk headers,
// afq_snappy_plan.h).  The chunk's output is built in LDS and its body is read through an LDS window, so no element waits for
// global memory: a copy element reads LDS, never bytes this kernel has written to memory.  The element loop is the wave's: the
// 8 bytes at the element go from the window into scalar registers in one trip, the parser runs on them (afq_snappy_elem.h -
// nothing moves that the parser has not validated against in_len and ulen), the lanes move the element's bytes while the next
// element's 8 bytes are on their way.  Then the masked CRC-32C of the staged bytes by slices (the encoder's code), and the write-out to
// any residue of the destination, 16-byte stores between a bytewise head and tail: the output is staged at the destination's
// own residue, so both sides of a 16-byte move are aligned.  A chunk that is refused writes nothing and enters
// `index << 8 | code` into the status word by atomicMin: the lowest bad chunk is named whatever the schedule.
__global__ __launch_bounds__(kSnappyDecThreads) void k_snappy_decode(const uint8_t* __restrict__ in, const SnappyDecChunk* __restrict__ plan, uint64_t first_index,
                                                                     uint8_t* __restrict__ dst, unsigned long long* __restrict__ status, unsigned long long* __restrict__ stats) {
    __shared__ uint4 s_out[(kSnappyBlock + 16) / 16];
    __shared__ uint4 s_in[(kSnappyDecWindow + 32) / 16];   // (+ the residue of the body's address, + the words load8 touches behind the window)
    __shared__ uint32_t s_tab[256];
    static_assert(sizeof(s_out) + sizeof(s_in) + sizeof(s_tab) == kSnappyDecLds, "afq_snappy_decode_limits reports the workgroup's LDS");
    const uint32_t lane = threadIdx.x;
    const SnappyDecChunk c = plan[blockIdx.x];
    const uint8_t* body = in + c.in_off;
    uint8_t* d = dst + c.out_off;
    const uint32_t in_len = uni(c.in_len), ulen = uni(c.ulen);
    uint8_t* so = (uint8_t*)s_out + ((uintptr_t)d & 15);   // so[i] is output byte i
    crc_table_fill<kCrc32cPoly>(s_tab, lane);
    uint32_t code = kSnappyOk, n_lit = 0, n_cp = 0;
    // the window holds body[wbase, wend) at sw
    uint32_t wbase = 0, wend = 0;
    const uint8_t* sw = (const uint8_t*)s_in;
    auto stage = [&](uint32_t at) {   // at < in_len
        const uint32_t n = min(kSnappyDecWindow, in_len - at);
        sw = window_fill(s_in, body + at, n, lane, kSnappyDecThreads);
        wbase = at; wend = at + n;
    };
    // 8 bytes of the body from p on in one trip (aligned words of the window; what lies behind wend is not looked at)
    auto load8 = [&](uint32_t p) -> uint64_t {
        const uint32_t o = (uint32_t)(sw - (const uint8_t*)s_in) + (p - wbase);
        const uint32_t* t = (const uint32_t*)s_in;
        const uint32_t x = o >> 2, sh = o & 3u;
        const uint32_t w0 = t[x], w1 = t[x + 1], w2 = t[x + 2];
        const uint32_t lo = sh ? __builtin_amdgcn_alignbyte(w1, w0, sh) : w0, hi = sh ? __builtin_amdgcn_alignbyte(w2, w1, sh) : w1;
        return (uint64_t)uni(lo) | (uint64_t)uni(hi) << 32;   // into scalar registers: the parser then runs on the scalar unit
    };
    if (ulen > kSnappyBlock) code = kSnappyLengthDisagrees;
    else if (!c.compressed) {
        if (in_len != ulen) code = kSnappyLengthDisagrees;
        else
            for (uint32_t at = 0; at < in_len; at += kSnappyDecWindow) {
                stage(at);
                for (uint32_t i = lane; i < wend - wbase; i += kSnappyDecThreads) so[at + i] = sw[i];
            }
    } else {
        uint32_t p = 0, w = 0;
        uint64_t declared = 0, hdr = 0;   // hdr: the 8 bytes at p; the parser asks for at most 5 of them, all below in_len
        if (in_len) {
            stage(0);
            hdr = load8(0);
            p = uni(snappy_elem_length([&](uint32_t i) -> uint32_t { return (uint32_t)(hdr >> (8 * i)) & 255u; }, in_len, declared));
        }
        if (!p || declared != ulen) code = kSnappyLengthDisagrees;
        bool have = false;   // hdr holds the bytes at p
        while (!code && p < in_len) {
            if (!have) {
                const uint32_t need = min(kSnappyElemMaxHeader, in_len - p);
                if (p < wbase || p + need > wend) stage(p);
                hdr = load8(p);
            }
            const SnappyElem e = snappy_elem_parse([&](uint32_t i) -> uint32_t { return (uint32_t)(hdr >> (8 * (i - p))) & 255u; }, in_len, p, w, ulen);
            code = uni(e.code);
            if (code) break;
            const uint32_t len = uni(e.len), next = uni(e.next), is_copy = uni(e.copy);
            // the next element's header, read while this element's bytes move (the window's bytes do not change under a restage)
            have = false;
            uint64_t nhdr = 0;
            if (next < in_len) {
                const uint32_t need = min(kSnappyElemMaxHeader, in_len - next);
                if (next >= wbase && next + need <= wend) { nhdr = load8(next); have = true; }
            }
            if (!is_copy) {
                const uint32_t src0 = uni(e.src);
                for (uint32_t done = 0; done < len;) {   // [src0, src0 + len) lies in the body, [w, w + len) below ulen
                    const uint32_t src = src0 + done;
                    if (src < wbase || src >= wend) stage(src);
                    const uint32_t k = min(len - done, wend - src);
                    for (uint32_t i = lane; i < k; i += kSnappyDecThreads) so[w + done + i] = sw[src - wbase + i];
                    done += k;
                }
                n_lit += len;
            } else {
                const uint32_t off = uni(e.off);   // 1 <= off <= w, len <= 64, w + len <= ulen
                if (lane < len) {
                    // off < len: the run-length case, lane i reads i mod off.  lane and off are below 64: (lane + 0.5) / off is
                    // at least 1 / 128 from an integer, far more than the reciprocal's error, so the quotient is exact
                    const uint32_t i = off < len ? lane - off * (uint32_t)(((float)lane + 0.5f) * __builtin_amdgcn_rcpf((float)off)) : lane;
                    const uint8_t v = so[w - off + i];
                    so[w + lane] = v;
                }
                ++n_cp;
            }
            w += len;
            p = next;
            hdr = nhdr;
            gpl_wave_lds_sync();   // one wave: its LDS operations complete in order; this keeps the compiler to that order
        }
        if (!code && w != ulen) code = kSnappyOutputShort;
    }
    __syncthreads();
    if (!code) {
        if (wave_masked_crc(so, ulen, crc_slice_lds(ulen), false, s_tab, lane) != c.crc) code = kSnappyCrcMismatch;
    }
    if (code) {
        if (lane == 0) atomicMin(status, (unsigned long long)(first_index + blockIdx.x) << 8 | code);
        return;
    }
    staged_write_out(d, so, ulen, lane, kSnappyDecThreads);
    if (lane < 4) atomicAdd(&stats[lane], (unsigned long long)(lane == 0 ? 1u : lane == 1 ? (c.compressed ? 0u : 1u) : lane == 2 ? n_lit : n_cp));
}

// ---------------------------------------------------------------------------------------------------------------- the chunk table
// k_collated_chunk_table: the chunk table of a collated record stream that lies on the device (the decoder's output), as the
// host's hop over the `nbytes, nrec` headers finds it.  The hop is serial by nature - a header says where the next one stands -
// so ONE WAVE makes it, through LDS tiles: a tile is staged with aligned, bounded loads (what lies outside the buffer reads as
// 0 and is never fetched), the headers inside it are hopped in LDS, wave-uniform; a chunk that ends behind the tile costs one
// jump to its end, and the tile behind a jump is a short one (kChunkTableShort: a large cell costs a header's worth of loads,
// not a tile's), the whole tile again once headers keep falling into it.  Lane 0 writes offset, nbytes, nrec and the 8 bytes at chunk + 12 (the first record's barcode field) for
// the chunks below `cap`; the hop counts on past it, so that the host can come back with room for all.  It ends at the first
// refusal - the host hop's, in its order - and says which and at which chunk.
__global__ __launch_bounds__(64) void k_collated_chunk_table(const uint8_t* __restrict__ bytes, uint64_t n, uint64_t first_chunk, uint32_t rec_hdr, uint64_t cap,
                                                             uint64_t* __restrict__ off, uint32_t* __restrict__ nbytes, uint32_t* __restrict__ nrec,
                                                             uint64_t* __restrict__ first_bc, uint64_t* __restrict__ stat) {
    __shared__ uint32_t tile[kChunkTableWords];
    const uint32_t lane = threadIdx.x;
    uint64_t p = first_chunk, k = 0;
    uint32_t code = kChunkTableOk;
    uint32_t span = kChunkTableTile;   // bytes of this trip's tile: all of it while headers keep falling into it, a short one behind a jump
    while (p < n && !code) {
        const uint32_t al = (uint32_t)((reinterpret_cast<uintptr_t>(bytes) + p) & 3u);
        const uint32_t words = (3 + span + kChunkTableHalo + 3) / 4 + 1;
        const int64_t base = (int64_t)p - al;
        if (base >= 0 && (uint64_t)base + 4ull * words <= n) {   // the tile lies inside the buffer: loads without a test each, many in flight
#pragma unroll 8
            for (uint32_t i = lane; i < words; i += 64) tile[i] = *reinterpret_cast<const uint32_t*>(bytes + base + 4ull * i);
        } else
            for (uint32_t i = lane; i < words; i += 64) tile[i] = gpl_ld_dword_in(bytes, n, base + 4ll * i);
        gpl_wave_lds_sync();
        uint32_t q = 0;   // the header at p + q: its 8 bytes and the 8 at + 12 lie in the tile or its halo
        bool jumped = false;
        while (q < span && p + q < n) {
            const uint64_t a = p + q;
            if (n - a < 8) { code = kChunkTableTrailing; break; }
            const uint32_t nb = uni(gpl_lds32(tile, al + q)), nr = uni(gpl_lds32(tile, al + q + 4));
            if (nb < 8 || nb > n - a) { code = kChunkTableCorrupt; break; }
            if (rec_hdr && (nr == 0 || nb < 8 + rec_hdr)) { code = kChunkTableNoRecord; break; }
            if (lane == 0 && k < cap) {
                off[k] = a; nbytes[k] = nb; nrec[k] = nr;
                first_bc[k] = (uint64_t)gpl_lds32(tile, al + q + 12) | (uint64_t)gpl_lds32(tile, al + q + 16) << 32;
            }
            ++k;
            if (nb >= span - q) { p = a + nb; jumped = true; break; }   // the next header is not in this tile
            q += nb;
        }
        if (!jumped) p += q;
        span = jumped ? kChunkTableShort : kChunkTableTile;
        gpl_wave_lds_sync();   // (the next trip overwrites the tile)
    }
    if (lane == 0) { stat[0] = k; stat[1] = code; }   // (a refusal: k is the index of the chunk it is about)
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

void launch_snappy_decode(hipStream_t s, const uint8_t* in, const SnappyDecChunk* plan, uint32_t n_chunks, uint64_t first_index, uint8_t* dst, uint64_t* status, uint64_t* stats) {
    if (n_chunks) AFQ_LAUNCH(k_snappy_decode, n_chunks, kSnappyDecThreads, s, in, plan, first_index, dst, (unsigned long long*)status, (unsigned long long*)stats);
}
void launch_collated_chunk_table(hipStream_t s, const uint8_t* bytes, uint64_t n, uint64_t first_chunk, uint32_t rec_hdr, uint64_t cap, uint64_t* off, uint32_t* nbytes,
                                 uint32_t* nrec, uint64_t* first_bc, uint64_t* stat) {
    AFQ_LAUNCH(k_collated_chunk_table, 1, 64, s, bytes, n, first_chunk, rec_hdr, cap, off, nbytes, nrec, first_bc, stat);
}

}  // namespace afq
